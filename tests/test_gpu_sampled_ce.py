"""Sampled-softmax training (csrc/k_cand_ce.hip): the cross-entropy of every row over its label and its OWN list.

(1) parity of loss and the three gradients with the fp64 reference (tests/_cand_ce_ref.py), atomic and ordered table gradient;
(2) the forward's values are the bits of ops.score_candidates; (3) a list that holds the whole catalogue gives ScoreCEFn's loss and
gradients; (4) a row does not depend on the order of its list beyond f32 rounding, nor on the batch at all; (5) the deterministic
form gives the same bits twice; (6) the four models train on sampled lists; (7) the driver; (8) refusals."""
import functools
import math
import pickle

import numpy as np
import pytest
import torch

from tests import _cand_ce_ref as CE
from tests import _cand_ref as CR
from tests._util import LOSS_TOL, build_model, grad_ok, make_problem, to_dev

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f32": torch.float32}
I_ = 300


def ops():
    from easydgl_amd import ops as _ops
    return _ops


def _f64(t):
    return t.detach().double().cpu().numpy()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _problem(R, C, N, dt, I=I_, hot=False, seed=0):
    """rows / table with logits of O(1); about a quarter of the rows with label 0; lists drawn by the device sampler (no slot comes
    back empty at this range), then — N >= 5 — given empty slots, accidental hits, item 0 and a repeated id.  hot: the labels come
    from four ids, so some table rows collect many batch rows.  Returns device tensors and the fp64 reference (computed once)."""
    rng = np.random.default_rng(1000 * C + 10 * N + R + seed)
    s = C ** -0.25
    rows = torch.tensor(rng.standard_normal((R, C)) * s, dtype=DT[dt]).cuda()
    master = torch.tensor(rng.standard_normal((I, C)) * s, dtype=torch.float32).cuda()
    bias = torch.tensor(rng.standard_normal(I - 1) * 0.3, dtype=torch.float32).cuda()
    lab = rng.choice([7, 8, 150, I - 1], size=R) if hot else rng.integers(1, I, size=R)
    if R >= 3:
        lab[2::4] = 0
    labels = torch.tensor(lab, dtype=torch.int64).cuda()
    cand = ops().sample_negatives(None, labels, N, 1, I, seed=11, step=3)
    assert int((cand < 0).sum()) == 0                        # 32 attempts against one banned id of 299: no empty slot
    c = cand.cpu().numpy().astype(np.int64)
    if N >= 5:
        c[1::5, 0] = -1                                      # empty
        c[0::3, 1] = lab[0::3]                               # accidental hit
        c[0::2, 2] = 0                                       # item 0: the zero row with bias -1000
        c[:, 3] = c[:, 4]                                    # a repeated id
        c[0, N - 1] = I + 5                                  # at or past I
    cand = torch.tensor(c, dtype=torch.int32).cuda()
    table_c = master.to(DT[dt])
    ref = CE.reference(_f64(rows), _f64(table_c), _f64(bias), c, lab)
    return rows, master, bias, table_c, labels, cand, ref


def _run(rows, master, bias, table_c, labels, cand, det):
    r = rows.clone().requires_grad_(True)
    m = master.clone().requires_grad_(True)
    b = bias.clone().requires_grad_(True)
    loss = ops().SampledCEFn.apply(r, m, b, table_c, labels, cand, det)
    loss.backward()
    return loss.detach(), r.grad, m.grad, b.grad


# ---- (1) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,N", [(1, 1), (3, 5), (130, 100), (7, 257), (2, 1500)])
@pytest.mark.parametrize("C", [16, 64, 128, 256, 512])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_parity_with_the_fp64_reference(dt, C, R, N):
    _check_parity(dt, C, R, N)


@pytest.mark.parametrize("C", [48, 80, 496])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_parity_at_widths_that_are_no_power_of_two(dt, C):
    """Lane groups with idle lanes (3 / 5 / 31 pieces of bf16 rows in groups of 4 / 8 / 32), and atomic sweeps whose last
    instruction covers part of a row."""
    _check_parity(dt, C, 5, 37)


def _check_parity(dt, C, R, N):
    rows, master, bias, table_c, labels, cand, ref = _problem(R, C, N, dt)
    for det in (False, True):
        loss, d_rows, d_table, d_bias = _run(rows, master, bias, table_c, labels, cand, det)
        tag = (dt, C, R, N, det)
        assert loss.dtype == torch.float32 and d_rows.dtype == DT[dt] and d_table.dtype == torch.float32
        assert d_table.shape == (I_, C) and d_bias.shape == (I_ - 1,)
        err = abs(float(loss) - ref["loss"]) / abs(ref["loss"])
        print(tag, "loss", float(loss), ref["loss"], err)
        assert err <= LOSS_TOL[dt], tag
        for name, got in (("d_rows", d_rows), ("d_table", d_table), ("d_bias", d_bias)):
            ok, e = grad_ok(_f64(got), ref[name], dt)
            print(tag, name, e)
            assert ok, (tag, name, e)
        assert not d_table[0].any()                          # item 0's row is no parameter
        zero = (labels == 0).cpu().numpy()
        assert not _f64(d_rows)[zero].any()                  # rows of weight 0: written as zeros


# ---- (2) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 128, 512])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_values_are_the_bits_of_score_candidates(dt, C):
    rows, _, bias, table_c, labels, cand, _ = _problem(130, C, 100, dt)
    vals, label_val, lse = ops().cand_ce_fwd(rows, table_c, bias, cand, labels)
    sc, lv, _ = ops().score_candidates(rows, table_c, bias, cand, None, labels)
    w = labels != 0
    assert torch.equal(_bits(label_val)[w], _bits(lv)[w]) and torch.equal(_bits(vals[:, 0])[w], _bits(lv)[w])
    live = vals[:, 1:] > -math.inf
    assert torch.equal(_bits(vals[:, 1:])[live], _bits(sc)[live]) and int(live.sum()) > 0.6 * 130 * 100
    hit = cand.long() == labels[:, None]
    dead_here = ~live & w[:, None]
    assert torch.equal(dead_here, ((sc == -math.inf) | hit) & w[:, None])      # accidental hits read -inf here only
    assert int((hit & w[:, None] & (sc > -math.inf)).sum()) > 0
    assert not live[~w].any() and not lse[~w].any() and not label_val[~w].any()


# ---- (3) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I", [50, 300])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_full_list_equals_the_full_softmax(dt, I):
    R, C = 40, 128
    rng = np.random.default_rng(I)
    s = C ** -0.25
    rows = torch.tensor(rng.standard_normal((R, C)) * s, dtype=DT[dt]).cuda()
    master = torch.tensor(rng.standard_normal((I, C)) * s, dtype=torch.float32).cuda()
    bias = torch.tensor(rng.standard_normal(I - 1) * 0.3, dtype=torch.float32).cuda()
    lab = rng.integers(1, I, size=R)
    lab[3::4] = 0
    cand = np.stack([rng.permutation(np.setdiff1d(np.arange(I), [y])) if y else np.arange(1, I) for y in lab])
    labels, cand = torch.tensor(lab, dtype=torch.int64).cuda(), torch.tensor(cand, dtype=torch.int32).cuda()
    table_c = master.to(DT[dt])
    a = _run(rows, master, bias, table_c, labels, cand, False)
    r, m, b = (t.clone().requires_grad_(True) for t in (rows, master, bias))
    full = ops().ScoreCEFn.apply(r, m, b, table_c, labels)
    full.backward()
    full = full.detach()
    assert abs(float(a[0]) - float(full)) <= LOSS_TOL[dt] * min(abs(float(a[0])), abs(float(full)))
    for name, got, want in (("d_rows", a[1], r.grad), ("d_table", a[2], m.grad), ("d_bias", a[3], b.grad)):
        for x, y in ((got, want), (want, got)):              # two-sided: either is the other's reference
            ok, e = grad_ok(_f64(x), _f64(y), dt)
            assert ok, (dt, I, name, e)


# ---- (4) ---------------------------------------------------------------------------------------------------------------------------
def _terms(label_val, lse):
    return -torch.log(torch.exp(label_val.double() - lse.double()) + 1e-5)


@pytest.mark.parametrize("R,N", [(3, 5), (7, 257)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_a_row_does_not_depend_on_the_order_of_its_list(dt, R, N):
    C = 128
    rows, master, bias, table_c, labels, cand, ref = _problem(R, C, N, dt)
    perm = torch.tensor(np.random.default_rng(4).permutation(N)).cuda()
    cand2 = cand[:, perm].contiguous()
    a = _run(rows, master, bias, table_c, labels, cand, False)
    b = _run(rows, master, bias, table_c, labels, cand2, False)
    fa, fb = ops().cand_ce_fwd(rows, table_c, bias, cand, labels), ops().cand_ce_fwd(rows, table_c, bias, cand2, labels)
    w = (labels != 0).cpu().numpy()
    ta, tb = _terms(fa[1], fa[2]).cpu().numpy()[w], _terms(fb[1], fb[2]).cpu().numpy()[w]
    assert np.all(np.abs(ta - tb) <= LOSS_TOL[dt] * np.abs(ta))
    # d_rows[r] = sum_s dv_s t_s in f32: N + 1 terms in another order differ by <= (N + 1) u sum |dv_s t_s|; dv_s itself moves with
    # the order of the log-sum-exp (<= (N + 1) u relative) and with the fast exponential at another running maximum (<= |v - m| u
    # relative, |v - m| < 30 here): (4 N + 64) u sum |dv_s t_s| covers both with u = 2^-24.  bf16 rows add one rounding of the output.
    tu, _ = CE.used(_f64(table_c), _f64(bias))
    c, lab = cand.cpu().numpy().astype(np.int64), labels.cpu().numpy()
    diff = np.abs(_f64(a[1]) - _f64(b[1]))
    for r in range(R):
        if lab[r] == 0:
            assert not diff[r].any()
            continue
        ids, _ = CE.slots(c[r], lab[r], I_)
        v = tu[ids] @ _f64(rows)[r] + CE.used(_f64(table_c), _f64(bias))[1][ids]
        p = np.exp(v - ref["lse"][r])
        p[0] = 1.0 - p[0]
        coef = 1.0 / (ref["weight"] + 1e-5)
        mag = coef * (p[:, None] * np.abs(tu[ids])).sum(axis=0)
        bound = (4 * N + 64) * 2.0 ** -24 * mag
        if dt == "bf16":
            bound = bound + 2.0 ** -8 * np.abs(ref["d_rows"][r])
        assert np.all(diff[r] <= bound), (dt, R, N, r, float((diff[r] / np.maximum(bound, 1e-300)).max()))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_a_row_does_not_depend_on_the_batch(dt):
    rows, _, bias, table_c, labels, cand, _ = _problem(130, 128, 100, dt)
    big = ops().cand_ce_fwd(rows, table_c, bias, cand, labels)
    small = ops().cand_ce_fwd(rows[:8].contiguous(), table_c, bias, cand[:8].contiguous(), labels[:8].contiguous())
    assert int((labels[:8] != 0).sum()) >= 4
    for x, y in zip(big, small):
        assert torch.equal(_bits(x[:8]), _bits(y))


# ---- (5) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,N,C", [(130, 100, 128), (7, 257, 256)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_deterministic_form_gives_the_same_bits_twice(dt, R, N, C):
    p = _problem(R, C, N, dt, hot=True)
    lab = p[4].cpu().numpy()
    assert max(np.bincount(lab[lab > 0])) >= R // 8           # segments that span many rows
    a, b = _run(*p[:6], True), _run(*p[:6], True)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x.float()), _bits(y.float()))
    c = _run(*p[:6], False)
    assert torch.equal(_bits(a[0]), _bits(c[0]))             # one forward for both modes
    assert torch.equal(_bits(a[1].float()), _bits(c[1].float()))      # ... and one d_rows: no atomics in it
    for k in (2, 3):
        ok, e = grad_ok(_f64(a[k]), p[6][("d_table", "d_bias")[k - 2]], dt)
        assert ok, e


# ---- (6) ---------------------------------------------------------------------------------------------------------------------------
def _easydgl(B, det=False, lr=1e-2):
    prob = make_problem(seed=3, batch=B, num_items=300, seqslen=20, num_units=32, num_heads=2, num_blocks=1, learning_rate=lr)
    m = build_model(prob, "f32")
    m.deterministic = det
    return m, to_dev(prob["feats"]), torch.as_tensor(prob["labels"]).cuda()


def _regressive(kind, seed, mode, B, det, **dims):
    from tests import test_gpu_det_models as DM
    mod = DM.KINDS[kind][0]
    prob = mod._problem(seed, B=B, **dims)
    m = DM._model(kind, prob, mode, deterministic=det)
    m.learning_rate = 1e-2
    return m, to_dev(prob["feats"]), torch.as_tensor(prob["tokens"][:, 1:].copy()).cuda()


MODELS = {
    "EasyDGL": lambda B, det=False: _easydgl(B, det),
    "CTSMA": lambda B, det=False: _regressive("ctsma", 7, "f32", B, det, T=20, C=32, h=2, E=4, I=300, nb=1),
    "TGAT": lambda B, det=False: _regressive("tgat", 11, "f32", B, det, T=12, C=32, h=2, I=300, nb=2),
    "TiSASRec": lambda B, det=False: _regressive("tisasrec", 80, "bf16", B, det, T=12, C=32, h=2, I=300, nb=1, timelen=32),
}


def _train_rows(name, m, feats):
    out = m.encoder(feats, True, m._gather_pos(feats, True) if name == "EasyDGL" else None)
    rows = out[0] if isinstance(out, tuple) else out
    return rows.reshape(-1, m.num_units).contiguous()


def _parent_train_loss(name, m, feats, labels):
    """train_loss as it stood before sampled training existed: ScoreCEFn, then the l2 and TPP terms in the models' order."""
    o = ops()
    out = m.encoder(feats, True, m._gather_pos(feats, True) if name == "EasyDGL" else None)
    rows, lams = out if isinstance(out, tuple) else (out, [])
    tab = m.item_embs.lookup_table
    loss = o.ScoreCEFn.apply(rows.reshape(-1, m.num_units), tab, m.output_bias, m.compute(tab), labels.reshape(-1).contiguous(),
                             m.deterministic)
    if m.l2_reg != 0.0:
        l2 = {"EasyDGL": lambda: (m.item_embs.lookup_table, m.mark_embs.lookup_table, m.pcoding.pembs.lookup_table),
              "CTSMA": lambda: (m.item_embs.lookup_table, m.pcoding.pembs.lookup_table)}.get(
                  name, lambda: tuple(m.get_parameter(n) for n in m.l2_param_names()))()
        for p in l2:
            loss = loss + o.L2Fn.apply(p, m.l2_reg)
    if name in ("EasyDGL", "CTSMA") and m.ct_reg != 0.0:
        for lam in lams:
            if name == "EasyDGL":
                loss = loss + o.TppFn.apply(lam, feats["masked_positions"].contiguous(), labels.contiguous(), feats["seqs_t"],
                                            m.mark_lookup_table, m.num_heads, m.ct_reg / m.num_heads)
            else:
                loss = loss + o.TppFn.apply(lam, None, labels.contiguous(), feats["seqs_t"].contiguous(), m.mark_lookup_table,
                                            m.num_heads, m.ct_reg)
    return loss


@pytest.mark.parametrize("name", sorted(MODELS))
def test_models_train_on_sampled_lists(name):
    N = 8
    m, feats, labels = MODELS[name](8)
    mode = "bf16" if m.act_dtype == torch.bfloat16 else "f32"
    lab = labels.reshape(-1).contiguous()
    # the default: the parent's loss, bit for bit
    assert m.train_negatives == 0 and m.neg_step == 0
    full = m.train_loss(feats, labels).detach()              # (with a tape: the flash forward a training step runs)
    parent = _parent_train_loss(name, m, feats, labels).detach()
    assert torch.equal(_bits(full.reshape(1)), _bits(parent.reshape(1)))
    with torch.no_grad():
        # what the l2 / TPP terms add: untouched by the sampled loss
        rows = _train_rows(name, m, feats)
        tab = m.compute(m.item_embs.lookup_table)
        reg = float(full) - float(ops().ScoreCEFn.apply(rows, m.item_embs.lookup_table, m.output_bias, tab, lab))
        # the sampled loss, rebuilt: the model's encoder rows, the numpy sampler's lists, the fp64 reference
        m.train_negatives, m.train_neg_seed, m.neg_step = N, 5, 2
        got = float(m.train_loss(feats, labels))
        hi = m.mask if name == "EasyDGL" else m.num_items
        cand, _ = CR.sample_negatives(None, lab.cpu().numpy(), N, 1, hi, 5, step=2, row0=0)
        assert (cand >= 1).all() and (cand < hi).all()
        ref = CE.reference(_f64(rows), _f64(tab), _f64(m.output_bias), cand, lab.cpu().numpy())
        want = ref["loss"] + reg
        assert abs(got - want) <= LOSS_TOL[mode] * abs(want), (name, got, want)
        assert m.neg_step == 2                               # train_loss does not advance the lists; train_step does
        assert float(m.train_loss(feats, labels)) == got
        fixed = torch.tensor(cand, dtype=torch.int32).cuda()
        assert float(m.train_loss(feats, labels, candidates=fixed)) == got
        m.train_negatives = 0                                # an explicit list needs no flag
        assert float(m.train_loss(feats, labels, candidates=fixed)) == got
        m.train_negatives = N
    # three steps change the weights and lower that loss on the fixed batch
    start = m._arena.detach().clone()
    with torch.no_grad():
        before = float(m.train_loss(feats, labels, candidates=fixed))
    for _ in range(3):
        step_loss = m.train_step(feats, labels)
        assert math.isfinite(float(step_loss))
    with torch.no_grad():
        after = float(m.train_loss(feats, labels, candidates=fixed))
    assert m.neg_step == 5 and not torch.equal(start, m._arena) and after < before, (name, before, after)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_models_deterministic_twice(name):
    arenas = []
    for _ in range(2):
        m, feats, labels = MODELS[name](8, True)
        assert m.deterministic is True
        m.train_negatives, m.train_neg_seed = 8, 1
        for _ in range(3):
            m.train_step(feats, labels)
        m.settle_state()
        arenas.append((m._arena.detach().clone(), m._adam_m.clone(), m._adam_v.clone()))
    for x, y in zip(*arenas):
        assert torch.equal(_bits(x), _bits(y))


# ---- (7) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_name,extra", [("TiSASREC", []), ("EasyDGL", ["--deterministic"])])
def test_driver_trains_on_sampled_negatives(tmp_path, monkeypatch, model_name, extra):
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
    drawn = []
    real = ops().sample_negatives

    def spy(seen, labels, n, lo, hi, seed, step=0, row0=0):
        drawn.append((seen is None, int(n), int(seed), int(step)))
        return real(seen, labels, n, lo, hi, seed, step, row0)
    monkeypatch.setattr(ops(), "sample_negatives", spy)
    res = TR.main(["--model", model_name, "--timelen", "32", "--train", str(tmp_path / "train*.tfrec"), "--valid",
                   str(tmp_path / "validation.tfrec"), "--test", str(tmp_path / "test.tfrec"), "--num_items", str(num_items),
                   "--num_units", "32", "--num_heads", "2", "--num_blocks", "1", "--seqslen", str(seqslen), "--masklen", "4",
                   "--time_scale", "86400", "--mark", str(tmp_path / "mark.pkl"), "--ct_reg", "1e-7", "--batch_size", "64",
                   "--num_epochs", "1", "--learning_rate", "1e-3", "--l2_reg", "1e-4", "--mask_seen", "--dtype", "f32",
                   "--ckpt_dir", str(tmp_path / "ckpt"), "--eval_negatives", "20", "--eval_neg_seed", "3",
                   "--train_negatives", "8", "--train_neg_seed", "2"] + extra)
    assert set(res) == {"H1", "H5", "H10", "N1", "N5", "N10", "MRR"}
    assert all(0.0 <= v <= 1.0 and math.isfinite(v) for v in res.values())
    # 140 sequences in batches of 64: three sampled steps (none on the static engine), lists keyed by the step count
    assert [d for d in drawn if d[0]] == [(True, 8, 2, 0), (True, 8, 2, 1), (True, 8, 2, 2)]
    assert any(d == (False, 20, 3, 0) for d in drawn)        # ... and the evaluation on its own lists


def test_checkpointed_and_resumed_run_ends_with_the_same_weights(tmp_path):
    from easydgl_amd import train as TR
    from tests import test_gpu_det_models as DM
    dims = dict(T=12, C=32, h=2, I=300, nb=1, timelen=32)
    probs = [DM.TT._problem(500 + i, B=8, **dims) for i in range(4)]
    batches = [(to_dev(p["feats"]), torch.as_tensor(p["tokens"][:, 1:].copy()).cuda()) for p in probs]

    def fresh():
        m = DM._model("tisasrec", probs[0], "bf16", hidden_drop=0.1, att_drop=0.1, deterministic=True)
        m.train_negatives, m.train_neg_seed = 8, 4
        return m
    whole = fresh()
    for f, l in batches:
        whole.train_step(f, l)
    first = fresh()
    for f, l in batches[:2]:
        first.train_step(f, l)
    TR.save_checkpoint(first, str(tmp_path / "m.pt"))
    second = fresh()
    TR.load_checkpoint(second, str(tmp_path / "m.pt"))
    assert second.neg_step == 2
    for f, l in batches[2:]:
        second.train_step(f, l)
    assert torch.equal(_bits(whole._arena), _bits(second._arena)) and whole.neg_step == second.neg_step == 4
    # a checkpoint from before the field existed still loads: the count starts at 0
    ck = torch.load(str(tmp_path / "m.pt"), map_location="cpu")
    del ck["neg_step"]
    torch.save(ck, str(tmp_path / "old.pt"))
    TR.load_checkpoint(second, str(tmp_path / "old.pt"))
    assert second.neg_step == 0


def test_engine_refuses_a_model_with_train_negatives():
    from easydgl_amd import _lib
    from easydgl_amd.engine import TrainEngine
    m, _, _ = _easydgl(4)
    m.train_negatives = 8
    with pytest.raises(_lib.EdglError, match="model.train_step"):
        TrainEngine(m, 4, use_graph=False)
    with pytest.raises(ValueError, match="train_step"):
        m.graphed_train_step({}, torch.zeros(1))


# ---- (8) ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from easydgl_amd import _lib
    o = ops()
    R, I = 4, 100

    def call(C=64, N=10, table=None):
        rows = torch.zeros((R, C), device="cuda")
        tab = torch.zeros((I, C), device="cuda") if table is None else table
        bias = torch.zeros(I - 1, device="cuda")
        cand = torch.ones((R, N), device="cuda", dtype=torch.int32)
        labels = torch.ones(R, device="cuda", dtype=torch.int64)
        return o.cand_ce_fwd(rows, tab, bias, cand, labels)
    assert call()[0].shape == (R, 11)
    for kw, text in ((dict(C=24), "multiple of 16"), (dict(N=0), "1 <= N <= 8192"), (dict(N=8193), "1 <= N <= 8192")):
        with pytest.raises(_lib.EdglError, match=text):
            call(**kw)
    off = torch.zeros(I * 64 + 1, device="cuda")[1:].view(I, 64)      # 4 bytes past a 16-byte boundary
    assert off.data_ptr() % 16 == 4
    with pytest.raises(_lib.EdglError, match="16-byte aligned"):
        call(table=off)
