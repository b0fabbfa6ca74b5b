"""Binary cross-entropy and BPR over sampled negatives (csrc/k_sampled_loss.hip, sampled_dv.h), on per-row lists
(ops.SampledCEFn) and on one shared list (ops.SharedCEFn), against the fp64 restatement of tests/_sampled_loss_ref.py evaluated on the
rounded inputs.

(1) parity of the loss and the three gradients, atomic and ordered table gradient; (2) log-Q; (3) form="softmax" is the call without
the argument, bit for bit; (4) determinism; (5) a row does not depend on the batch; (6) the models; (7) lazy Adam; (8) the driver."""
import functools
import math
import pickle

import numpy as np
import pytest
import torch

from tests import _sampled_loss_ref as SL
from tests._util import LOSS_TOL, flags_from, grad_ok, make_problem, to_dev

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f32": torch.float32}
FORMS = ["bce", "bpr"]
I_ = 300


def ops():
    from easydgl_amd import ops as _ops
    return _ops


def _f64(t):
    return t.detach().double().cpu().numpy()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _base(R, C, dt, I, seed):
    """rows / table with logits of O(1) (scale C^-0.25); about a quarter of the rows with label 0 and — R >= 7 — one label past I."""
    rng = np.random.default_rng(seed)
    s = C ** -0.25
    rows = torch.tensor(rng.standard_normal((R, C)) * s, dtype=DT[dt]).cuda()
    master = torch.tensor(rng.standard_normal((I, C)) * s, dtype=torch.float32).cuda()
    bias = torch.tensor(rng.standard_normal(I - 1) * 0.3, dtype=torch.float32).cuda()
    lab = rng.integers(1, I, size=R)
    if R >= 3:
        lab[2::4] = 0
    if R >= 7:
        lab[5] = I + 3                                       # outside the table: weight 0
    logq = np.concatenate([[0.0], np.log(rng.uniform(0.002, 0.2, size=I - 1))])
    return rng, rows, master, bias, lab, torch.tensor(logq, dtype=torch.float32).cuda()


def _refs(rows, table_c, bias, lab, lists, logq=None):
    return {f: SL.reference(_f64(rows), _f64(table_c), _f64(bias), lab, lists, None if logq is None else _f64(logq), f) for f in FORMS}


@functools.lru_cache(maxsize=None)
def _cand_problem(R, C, N, dt, I=I_, q=False):
    """Per-row lists drawn by the device sampler, then — N >= 5 — given an empty slot, an accidental hit, item 0, a repeated id, an id
    past I, and one weighted row whose every slot is dead.  Returns device tensors and the fp64 restatement of both forms (once)."""
    rng, rows, master, bias, lab, logq = _base(R, C, dt, I, 1000 * C + 10 * N + R)
    labels = torch.tensor(lab, dtype=torch.int64).cuda()
    c = ops().sample_negatives(None, labels, N, 1, I, seed=11, step=3).cpu().numpy().astype(np.int64)
    assert int((c < 0).sum()) == 0
    if N >= 5:
        c[1::5, 0] = -1                                      # empty
        c[0::3, 1] = lab[0::3]                               # accidental hit
        c[0::2, 2] = 0                                       # item 0: the zero row with bias -1000
        c[:, 3] = c[:, 4]                                    # a repeated id
        c[0, N - 1] = I + 5                                  # at or past I
        dead = 1 if R < 7 else 4
        assert 1 <= lab[dead] < I
        c[dead] = np.resize([-1, lab[dead], I + 1], N)       # every slot dead
    cand = torch.tensor(c, dtype=torch.int32).cuda()
    table_c = master.to(DT[dt])
    return rows, master, bias, table_c, labels, cand, (logq if q else None), _refs(rows, table_c, bias, lab, c, logq if q else None)


@functools.lru_cache(maxsize=None)
def _shared_problem(R, C, S, dt, I=I_, q=False):
    """One list drawn by the device sampler, then — S >= 5 — given an empty slot, item 0, an id past I, a repeated id and the label of
    a weighted row."""
    rng, rows, master, bias, lab, logq = _base(R, C, dt, I, 1000 * C + 10 * S + R + 7)
    labels = torch.tensor(lab, dtype=torch.int64).cuda()
    one = torch.zeros(1, dtype=torch.int64).cuda()
    sh = ops().sample_negatives(None, one, S, 1, I, seed=11, step=3).reshape(-1).cpu().numpy().astype(np.int64)
    assert (sh >= 1).all() and (sh < I).all()
    if S >= 5:
        sh[0] = -1
        sh[1] = 0
        sh[2] = I + 5
        sh[3] = sh[4]
        sh[S - 1] = lab[0]                                   # an accidental hit for row 0
    shared = torch.tensor(sh, dtype=torch.int32).cuda()
    table_c = master.to(DT[dt])
    return rows, master, bias, table_c, labels, shared, (logq if q else None), _refs(rows, table_c, bias, lab, sh, logq if q else None)


def _run(p, form, det, fn=None, with_form=True):
    rows, master, bias, table_c, labels, lists, logq = p[:7]
    r = rows.clone().requires_grad_(True)
    m = master.clone().requires_grad_(True)
    b = bias.clone().requires_grad_(True)
    fn = fn or (ops().SharedCEFn if lists.dim() == 1 else ops().SampledCEFn)
    args = (r, m, b, table_c, labels, lists, det)
    if with_form:
        args += (None, logq, form)
    loss = fn.apply(*args)
    loss.backward()
    return loss.detach(), r.grad, m.grad, b.grad


def _check_parity(p, form, tag):
    """As test_gpu_sampled_ce._check_parity holds the softmax form: LOSS_TOL on the loss, grad_ok / GRAD_TOL on the three gradients."""
    rows, labels, ref = p[0], p[4], p[7][form]
    dt, C = tag[0], rows.shape[1]
    for det in (False, True):
        loss, d_rows, d_table, d_bias = _run(p, form, det)
        assert loss.dtype == torch.float32 and d_rows.dtype == DT[dt] and d_table.dtype == torch.float32
        assert d_table.shape == (I_, C) and d_bias.shape == (I_ - 1,)
        err = abs(float(loss) - ref["loss"]) / abs(ref["loss"])
        print(tag, form, det, "loss", float(loss), ref["loss"], err)
        assert err <= LOSS_TOL[dt], (tag, form, det)
        for name, got in (("d_rows", d_rows), ("d_table", d_table), ("d_bias", d_bias)):
            assert torch.isfinite(got.float()).all(), (tag, form, det, name)
            ok, e = grad_ok(_f64(got), ref[name], dt)
            print(tag, form, det, name, e)
            assert ok, (tag, form, det, name, e)
        assert not d_table[0].any()                          # item 0's row is no parameter
        lab = labels.cpu().numpy()
        zero = (lab < 1) | (lab >= I_)
        assert not _f64(d_rows)[zero].any()                  # rows of weight 0: written as zeros


# ---- (1) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,N", [(1, 1), (3, 5), (130, 100), (7, 257)])
@pytest.mark.parametrize("C", [32, 128, 512])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("form", FORMS)
def test_per_row_lists_match_the_restatement(form, dt, C, R, N):
    _check_parity(_cand_problem(R, C, N, dt), form, (dt, C, R, N))


@pytest.mark.parametrize("R,S", [(1, 1), (5, 5), (130, 130), (7, 300)])
@pytest.mark.parametrize("C", [32, 128])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("form", FORMS)
def test_shared_list_matches_the_restatement(form, dt, C, R, S):
    _check_parity(_shared_problem(R, C, S, dt), form, (dt, C, R, S))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("form", FORMS)
def test_shared_list_with_a_row_whose_every_slot_is_dead(form, dt):
    """The list is one id and one empty slot: the row of that label has no live slot (bpr: loss and gradient 0, never NaN), the other
    row has one; and the pad columns 2 .. 7 of the dv image stay zero (sigma(0) = 0.5 there would reach d_rows through W_S = 0 only,
    but the bias sums would see it)."""
    _, rows, master, bias, lab, _ = _base(2, 32, dt, I_, 5)
    lab[:] = [17, 40]
    sh = np.array([17, -1])
    table_c = master.to(DT[dt])
    p = (rows, master, bias, table_c, torch.tensor(lab).cuda(), torch.tensor(sh, dtype=torch.int32).cuda(), None,
         _refs(rows, table_c, bias, lab, sh))
    assert len(p[7][form]["values"][0]) == 1 and len(p[7][form]["values"][1]) == 2
    _check_parity(p, form, (dt, 32, 2, 2))
    if form == "bpr":
        assert not _run(p, form, True)[1][0].any()           # d_rows of the all-dead row


# ---- (2) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("form", FORMS)
def test_log_q_on_both_list_families(form, dt):
    for p in (_cand_problem(7, 128, 257, dt, q=True), _shared_problem(7, 128, 300, dt, q=True)):
        ref, plain = p[7][form], (_cand_problem(7, 128, 257, dt) if p[5].dim() == 2 else _shared_problem(7, 128, 300, dt))[7][form]
        assert p[6] is not None and abs(ref["loss"] - plain["loss"]) > 0.05 * abs(plain["loss"])      # the term is felt
        assert bool(p[6][p[4][0]] != 0)                      # ... on a weighted row's label
        _check_parity(p, form, (dt, 128, 7, "q"))


# ---- (3) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_form_softmax_is_the_call_without_the_argument(dt, det):
    for p in (_cand_problem(130, 128, 100, dt, q=True), _shared_problem(130, 128, 130, dt, q=True)):
        rows, master, bias, table_c, labels, lists, logq = p[:7]
        fn = ops().SharedCEFn if lists.dim() == 1 else ops().SampledCEFn
        for q in (None, logq):
            out = []
            for tail in ((), ("softmax",)):
                r, m, b = (t.clone().requires_grad_(True) for t in (rows, master, bias))
                args = (r, m, b, table_c, labels, lists, det) + ((None, q) if (q is not None or tail) else ()) + tail
                loss = fn.apply(*args)
                loss.backward()
                out.append((loss.detach().reshape(1), r.grad.float(), m.grad, b.grad))
            names = ("loss", "d_rows", "d_table", "d_bias") if det else ("loss", "d_rows")      # (atomic sums: order not fixed)
            for name, x, y in zip(names, *out):
                assert torch.equal(_bits(x), _bits(y)), (dt, det, name)
            for x, y in zip(out[0][2:], out[1][2:]):
                assert grad_ok(_f64(x), _f64(y), "f32")[0]


# ---- (4) ---------------------------------------------------------------------------------------------------------------------------
def _row_losses(p, form):
    rows, _, bias, table_c, labels, lists, logq = p[:7]
    if lists.dim() == 2:
        vals, _, _ = ops().cand_ce_fwd(rows, table_c, bias, lists, labels, logq)
        return ops().sampled_row_loss(vals, None, labels, None, table_c.shape[0], form)
    vals, label_val, _ = ops().shared_ce_fwd(rows, table_c, bias, lists, labels, logq)
    return ops().sampled_row_loss(vals, label_val, labels, None, table_c.shape[0], form)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("form", FORMS)
def test_same_bits_twice(form, dt):
    for p in (_cand_problem(130, 128, 100, dt), _shared_problem(130, 128, 130, dt)):
        a, b = _run(p, form, True), _run(p, form, True)
        for x, y in zip(a, b):                               # deterministic: every output
            assert torch.equal(_bits(x.float()), _bits(y.float()))
        c, d = _run(p, form, False), _run(p, form, False)
        for x, y in zip(c[:2], d[:2]):                       # atomic: the loss and d_rows hold no atomics
            assert torch.equal(_bits(x.float()), _bits(y.float()))
        assert torch.equal(_bits(a[0]), _bits(c[0])) and torch.equal(_bits(a[1].float()), _bits(c[1].float()))
        for x, y in zip(_row_losses(p, form), _row_losses(p, form)):
            assert torch.equal(_bits(x), _bits(y))


# ---- (5) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("form", FORMS)
def test_a_row_does_not_depend_on_the_batch(form, dt):
    for p in (_cand_problem(130, 128, 100, dt), _shared_problem(130, 128, 130, dt)):
        rows, master, bias, table_c, labels, lists, logq = p[:7]
        assert 1 <= int(labels[0]) < I_
        one = (rows[:1].contiguous(), master, bias, table_c, labels[:1].contiguous(),
               lists[:1].contiguous() if lists.dim() == 2 else lists, logq)
        big, small = _row_losses(p, form), _row_losses(one, form)
        ref = p[7][form]["row_loss"][0]
        assert abs(float(big[3][0]) - ref) <= LOSS_TOL[dt] * abs(ref) and ref > 0
        assert torch.equal(_bits(big[3][:1]), _bits(small[3])) and torch.equal(_bits(big[2][:1]), _bits(small[2]))


# ---- (6) ---------------------------------------------------------------------------------------------------------------------------
def _easydgl(form, B=8, det=False, lazy=False, dt="f32", **neg):
    import easydgl_amd
    prob = make_problem(seed=3, batch=B, num_items=300, seqslen=20, num_units=32, num_heads=2, num_blocks=1, learning_rate=1e-2,
                        ct_reg=0.0, l2_reg=0.0)
    F = flags_from(prob["cfg"], prob["mark_table"], dt)
    F.sampled_loss, F.deterministic, F.lazy_adam, F.train_neg_seed = form, det, lazy, 5
    for k, v in neg.items():
        setattr(F, k, v)
    m = easydgl_amd.ranking(F).finalize("cuda")
    m.load_tf_variables(prob["params"])
    return m, to_dev(prob["feats"]), torch.as_tensor(prob["labels"]).cuda()


def _sasrec(form, B=8, det=False, **neg):
    from tests import test_gpu_seq_baselines as SB
    prob = SB._problem("SASREC", 31, B=B, I=300, T=10, C=32, h=2)
    m = SB._model(prob, "f32", l2_reg=0.0, lr=1e-2, sampled_loss=form, deterministic=det, train_neg_seed=5, **neg)
    return m, to_dev(prob["feats"]), torch.as_tensor(prob["tokens"][:, 1:].copy()).cuda()


MODELS = {"EasyDGL": _easydgl, "SASREC": _sasrec}


def _scored_rows(name, m, feats):
    out = m.encoder(feats, True, m._gather_pos(feats, True) if name == "EasyDGL" else None)
    rows = out[0] if isinstance(out, tuple) else out
    return rows.reshape(-1, m.num_units).contiguous()


@pytest.mark.parametrize("family", ["train_negatives", "shared_negatives"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_models_train_on_the_objective(name, form, family):
    n = 4 if family == "train_negatives" else 8
    m, feats, labels = MODELS[name](form, **{family: n})
    assert m.sampled_loss == form and getattr(m, family) == n
    lab = labels.reshape(-1).contiguous()
    with torch.no_grad():
        rows = _scored_rows(name, m, feats)
        tab = m.compute(m.item_embs.lookup_table)
        if family == "train_negatives":
            lists = m._sample(None, lab, n, m.train_neg_seed, m.neg_step, 0, None)
            fixed = dict(candidates=lists)
        else:
            lists = m.draw_shared_negatives(lab.device)
            fixed = dict(shared=lists)
        got = float(m.train_loss(feats, labels))
        want = SL.reference(_f64(rows), _f64(tab), _f64(m.output_bias), lab.cpu().numpy(), lists.cpu().numpy().astype(np.int64), None,
                            form)["loss"]
        print(name, form, family, got, want)
        assert abs(got - want) <= LOSS_TOL["f32"] * abs(want), (name, form, family, got, want)
        assert float(m.train_loss(feats, labels, **fixed)) == got and m.neg_step == 0
        before = got
    # bce and bpr are not invariant under a common shift of the logits, and a list is descended on only while it is trained on: the
    # lists are keyed by neg_step, so holding it at 0 makes the 30 steps descend on ONE objective, the loss measured before and after
    for _ in range(30):
        m.neg_step = 0
        assert math.isfinite(float(m.train_step(feats, labels))) and m.neg_step == 1
    with torch.no_grad():
        after = float(m.train_loss(feats, labels, **fixed))
    assert after < before, (name, form, family, before, after)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_models_deterministic_twice(name, form):
    for family, n in (("train_negatives", 4), ("shared_negatives", 8)):
        arenas = []
        for _ in range(2):
            m, feats, labels = MODELS[name](form, det=True, **{family: n})
            assert m.deterministic is True
            for _ in range(3):
                m.train_step(feats, labels)
            m.settle_state()
            arenas.append((m._arena.detach().clone(), m._adam_m.clone(), m._adam_v.clone()))
        for x, y in zip(*arenas):
            assert torch.equal(_bits(x), _bits(y)), (name, form, family)


# ---- (7) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,n", [("train_negatives", 4), ("shared_negatives", 8)])
def test_lazy_adam_takes_one_step_like_the_dense_model(family, n):
    lazy, feats, labels = _easydgl("bce", det=True, lazy=True, **{family: n})
    dense, _, _ = _easydgl("bce", det=True, lazy=False, **{family: n})
    assert lazy.lazy_adam and not dense.lazy_adam and torch.equal(_bits(lazy._arena), _bits(dense._arena))
    lab = labels.reshape(-1)
    lists = lazy._sample(None, lab, n, 5, 0, 0, None) if family == "train_negatives" else lazy.draw_shared_negatives(lab.device)
    before = lazy.item_embs.lookup_table.data.clone()
    la, da = lazy.train_step(feats, labels), dense.train_step(feats, labels)
    assert torch.equal(_bits(la.reshape(1)), _bits(da.reshape(1)))
    I = before.shape[0]
    touched = torch.zeros(I, dtype=torch.bool, device=before.device)
    for ids in (feats["seqs_i"].reshape(-1), lab, lists.reshape(-1).long()):
        ids = ids[(ids >= 0) & (ids < I)]
        touched[ids] = True
    assert bool(touched.any()) and bool((~touched[1:]).any())
    after_l, after_d = lazy.item_embs.lookup_table.data, dense.item_embs.lookup_table.data
    assert torch.equal(_bits(after_l[~touched]), _bits(before[~touched]))          # untouched rows: every bit kept
    ok, e = grad_ok(_f64(after_l[touched] - before[touched]), _f64(after_d[touched] - before[touched]), "f32")
    assert ok and bool((after_d[touched] != before[touched]).any()), e


# ---- (8) ---------------------------------------------------------------------------------------------------------------------------
def test_driver_trains_with_bce(tmp_path, monkeypatch):
    sp = pytest.importorskip("scipy.sparse")
    from easydgl_amd import data as D
    from easydgl_amd import formats as F
    from easydgl_amd import train as TR
    num_items, seqslen, E = 300, 20, 4
    ids, ts = D.synthetic_batch(num_items, seqslen, 200, seed=3)

    def dump(name, lo, hi):
        F.write_tfrecord(str(tmp_path / name), [F.encode_example({"seqs_i": ids[i], "seqs_t": ts[i]}) for i in range(lo, hi)])
    dump("train000.tfrec", 0, 140); dump("validation.tfrec", 140, 170); dump("test.tfrec", 170, 200)
    with open(tmp_path / "mark.pkl", "wb") as f:
        pickle.dump(sp.csr_matrix(D.synthetic_mark_table(num_items, E).astype(np.int64)), f)
    seen = []
    real = ops().sampled_row_loss

    def spy(vals, label_val, labels, nvalid, I, form):
        out = real(vals, label_val, labels, nvalid, I, form)
        seen.append((form, vals.shape[1], float(out[0])))
        return out
    monkeypatch.setattr(ops(), "sampled_row_loss", spy)
    res = TR.main(["--model", "TiSASREC", "--timelen", "32", "--train", str(tmp_path / "train*.tfrec"), "--valid",
                   str(tmp_path / "validation.tfrec"), "--test", str(tmp_path / "test.tfrec"), "--num_items", str(num_items),
                   "--num_units", "32", "--num_heads", "2", "--num_blocks", "1", "--seqslen", str(seqslen), "--masklen", "4",
                   "--time_scale", "86400", "--mark", str(tmp_path / "mark.pkl"), "--ct_reg", "1e-7", "--batch_size", "64",
                   "--num_epochs", "1", "--learning_rate", "1e-3", "--l2_reg", "1e-4", "--mask_seen", "--dtype", "f32",
                   "--ckpt_dir", str(tmp_path / "ckpt"), "--sampled_loss", "bce", "--train_negatives", "4", "--train_neg_seed", "2"])
    assert all(0.0 <= v <= 1.0 and math.isfinite(v) for v in res.values())
    # 140 sequences in batches of 64: three sampled steps, each with a finite bce loss over the label and four negatives
    assert len(seen) == 3 and all(f == "bce" and w == 5 and math.isfinite(x) and x > 0 for f, w, x in seen), seen
