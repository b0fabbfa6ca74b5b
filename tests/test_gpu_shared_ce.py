"""Sampled-softmax training on ONE negative list per step (csrc/k_shared_ce.hip): the per-row definition of DESIGN 4.13
with cand[r, :] = shared[:], so tests/_cand_ce_ref.reference on the broadcast list is the fp64 reference and ops.SampledCEFn on the
broadcast list a second, GPU-side one.

(1) parity of loss and the three gradients with the fp64 reference, atomic and deterministic; (2) against SampledCEFn / cand_ce_fwd
on the broadcast list; (3) the full list gives ScoreCEFn's loss and gradients; (4) edge lists; (5) reproducibility: the
deterministic form twice, one forward / d_rows for both modes, a row does not depend on the batch or on the compaction;
(6) d_table_out; (7) the four models; (8) lazy Adam; (9) the driver; (10) refusals."""
import functools
import math
import pickle

import numpy as np
import pytest
import torch

from tests import _cand_ce_ref as CE
from tests import _cand_ref as CR
from tests._util import LOSS_TOL, grad_ok, to_dev

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


def _bcast(shared, R):
    return np.broadcast_to(np.asarray(shared, dtype=np.int64), (R, len(shared)))


@functools.lru_cache(maxsize=None)
def _problem(R, C, S, dt, I=I_, hot=False, seed=0):
    """rows / table with logits of O(1); about a quarter of the rows with label 0; the list drawn by the device sampler (no slot
    comes back empty at this range), then — S >= 5 — given an empty slot, item 0, an id past I, a repeated id and the label of a
    weighted row.  hot: the labels come from four ids.  Returns device tensors and the fp64 reference (computed once)."""
    rng = np.random.default_rng(1000 * C + 10 * S + R + seed)
    s = C ** -0.25
    rows = torch.tensor(rng.standard_normal((R, C)) * s, dtype=DT[dt]).cuda()
    master = torch.tensor(rng.standard_normal((I, C)) * s, dtype=torch.float32).cuda()
    bias = torch.tensor(rng.standard_normal(I - 1) * 0.3, dtype=torch.float32).cuda()
    lab = rng.choice([7, 8, 150, I - 1], size=R) if hot else rng.integers(1, I, size=R)
    if R >= 3:
        lab[2::4] = 0
    labels = torch.tensor(lab, dtype=torch.int64).cuda()
    one = torch.zeros(1, dtype=torch.int64).cuda()
    sh = ops().sample_negatives(None, one, S, 1, I, seed=11, step=3).reshape(-1).cpu().numpy().astype(np.int64)
    assert (sh >= 1).all() and (sh < I).all()                # no empty slot
    if S >= 5:
        sh[0] = -1                                           # empty
        sh[1] = 0                                            # item 0: the zero row with bias -1000
        sh[2] = I + 5                                        # at or past I
        sh[3] = sh[4]                                        # a repeated id
        sh[S - 1] = lab[0]                                   # an accidental hit for row 0 (and every row of that label)
        assert lab[0] != 0 and (lab[:, None] == sh[None, :]).any()
    shared = torch.tensor(sh, dtype=torch.int32).cuda()
    table_c = master.to(DT[dt])
    ref = CE.reference(_f64(rows), _f64(table_c), _f64(bias), _bcast(sh, R), lab)
    return rows, master, bias, table_c, labels, shared, ref


def _run(rows, master, bias, table_c, labels, shared, det, fn=None):
    r = rows.clone().requires_grad_(True)
    m = master.clone().requires_grad_(True)
    b = bias.clone().requires_grad_(True)
    loss = (fn or ops().SharedCEFn).apply(r, m, b, table_c, labels, shared, det)
    loss.backward()
    return loss.detach(), r.grad, m.grad, b.grad


# ---- (1) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", [(1, 1), (3, 5), (130, 100), (7, 257), (2, 1500), (129, 129)])
@pytest.mark.parametrize("C", [16, 64, 128, 256, 512])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_parity_with_the_fp64_reference(dt, C, R, S):
    _check_parity(_problem(R, C, S, dt), (dt, C, R, S))


@pytest.mark.parametrize("C", [48, 80, 496])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_parity_at_widths_that_are_no_multiple_of_the_k_tile(dt, C):
    _check_parity(_problem(5, C, 37, dt), (dt, C, 5, 37))


@pytest.mark.parametrize("R,S,C", [(130, 128, 128), (1100, 1024, 128), (1100, 512, 256)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_parity_where_the_dense_products_take_their_other_kernels(dt, R, S, C):
    """The two backward products go through the library's dense GEMMs, which pick a kernel by shape: a list of 32 k (register strips),
    a list past 512 under >= 1024 rows (the tiled kernel), several row splits of the slab."""
    _check_parity(_problem(R, C, S, dt), (dt, C, R, S))


def _check_parity(p, tag):
    rows, master, bias, table_c, labels, shared, ref = p
    dt, C = tag[0], tag[1]
    for det in (False, True):
        loss, d_rows, d_table, d_bias = _run(rows, master, bias, table_c, labels, shared, det)
        assert loss.dtype == torch.float32 and d_rows.dtype == DT[dt] and d_table.dtype == torch.float32
        assert d_table.shape == (I_, C) and d_bias.shape == (I_ - 1,)
        err = abs(float(loss) - ref["loss"]) / abs(ref["loss"])
        print(tag, det, "loss", float(loss), ref["loss"], err)
        assert err <= LOSS_TOL[dt], (tag, det)
        for name, got in (("d_rows", d_rows), ("d_table", d_table), ("d_bias", d_bias)):
            ok, e = grad_ok(_f64(got), ref[name], dt)
            print(tag, det, name, e)
            assert ok, (tag, det, name, e)
        assert not d_table[0].any()                          # item 0's row is no parameter
        zero = (labels == 0).cpu().numpy()
        assert not _f64(d_rows)[zero].any()                  # rows of weight 0: written as zeros


# ---- (2) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S,C", [(130, 100, 128), (7, 257, 256), (129, 129, 16)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_against_the_per_row_op_on_the_broadcast_list(dt, R, S, C):
    rows, master, bias, table_c, labels, shared, _ = _problem(R, C, S, dt)
    cand = shared[None, :].expand(R, S).contiguous()
    a = _run(rows, master, bias, table_c, labels, shared, False)
    b = _run(rows, master, bias, table_c, labels, cand, False, ops().SampledCEFn)
    assert abs(float(a[0]) - float(b[0])) <= LOSS_TOL[dt] * min(abs(float(a[0])), abs(float(b[0])))
    for name, got, want in zip(("d_rows", "d_table", "d_bias"), a[1:], b[1:]):
        for x, y in ((got, want), (want, got)):              # two-sided: either is the other's reference
            ok, e = grad_ok(_f64(x), _f64(y), dt)
            assert ok, (dt, R, S, C, name, e)
    vals, label_val, lse = ops().shared_ce_fwd(rows, table_c, bias, shared, labels)
    pv, pl, plse = ops().cand_ce_fwd(rows, table_c, bias, cand, labels)
    assert vals.shape == (R, S)
    live = vals > -math.inf
    assert torch.equal(live, pv[:, 1:] > -math.inf) and int(live.sum()) > 0.6 * R * S       # the same dead-slot pattern
    w = labels != 0
    assert not live[~w].any() and not lse[~w].any() and not label_val[~w].any()
    # logits of O(1): LOSS_TOL as an absolute bound, scaled by 1 + |value|.  Both ops add the same exact products in f32; the
    # matrix pipe adds them in another order than the gather, so there is no bit equality
    def near(x, y):
        return bool(((x - y).abs() <= LOSS_TOL[dt] * (1.0 + y.abs())).all())
    assert near(vals[live], pv[:, 1:][live]) and near(label_val, pl) and near(lse, plse)


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
    labels = torch.tensor(lab, dtype=torch.int64).cuda()
    shared = torch.arange(1, I, dtype=torch.int32).cuda()    # every item; a row's label is removed as a hit and scored as the label
    table_c = master.to(DT[dt])
    a = _run(rows, master, bias, table_c, labels, shared, False)
    r, m, b = (t.clone().requires_grad_(True) for t in (rows, master, bias))
    full = ops().ScoreCEFn.apply(r, m, b, table_c, labels)
    full.backward()
    full = full.detach()
    # (the full softmax also holds item 0 at bias -1000: exp(-1000) is 0 in f32)
    assert abs(float(a[0]) - float(full)) <= LOSS_TOL[dt] * min(abs(float(a[0])), abs(float(full)))
    for name, got, want in (("d_rows", a[1], r.grad), ("d_table", a[2], m.grad), ("d_bias", a[3], b.grad)):
        for x, y in ((got, want), (want, got)):
            ok, e = grad_ok(_f64(x), _f64(y), dt)
            assert ok, (dt, I, name, e)


# ---- (4) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_every_slot_dead(dt):
    rows, master, bias, table_c, labels, _, _ = _problem(7, 64, 5, dt)
    shared = torch.tensor([-1, I_, I_ + 7, -5, 2 ** 31 - 1], dtype=torch.int32).cuda()
    for det in (False, True):
        loss, d_rows, d_table, d_bias = _run(rows, master, bias, table_c, labels, shared, det)
        n = float((labels != 0).sum())
        want = -math.log(1.0 + 1e-5) * n / (n + 1e-5)        # p_label = 1 in every weighted row
        assert abs(float(loss) - want) <= 1e-6
        for g in (d_rows, d_table, d_bias):
            assert float(g.float().abs().max()) <= 1e-6
    vals, _, _ = ops().shared_ce_fwd(rows, table_c, bias, shared, labels)
    assert bool((vals == -math.inf).all())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_every_row_of_weight_zero(dt):
    rows, master, bias, table_c, labels, shared, _ = _problem(7, 64, 37, dt)
    for det in (False, True):
        loss, d_rows, d_table, d_bias = _run(rows, master, bias, table_c, torch.zeros_like(labels), shared, det)
        assert float(loss) == 0.0
        for g in (d_rows, d_table, d_bias):
            assert not g.any()


@pytest.mark.parametrize("R,S,C", [(130, 100, 128), (7, 257, 256)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_hot_labels(dt, R, S, C):
    p = _problem(R, C, S, dt, hot=True)
    lab = p[4].cpu().numpy()
    assert max(np.bincount(lab[lab > 0])) >= R // 8           # segments that span many rows
    _check_parity(p, (dt, C, R, S))


# ---- (5) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S,C", [(130, 100, 128), (7, 257, 256)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_deterministic_form_gives_the_same_bits_twice(dt, R, S, C):
    p = _problem(R, C, S, dt, hot=True)
    a, b = _run(*p[:6], True), _run(*p[:6], True)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x.float()), _bits(y.float()))
    c = _run(*p[:6], False)
    assert torch.equal(_bits(a[0]), _bits(c[0]))             # one forward for both modes
    assert torch.equal(_bits(a[1].float()), _bits(c[1].float()))      # ... and one d_rows: no atomics in it


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_a_row_does_not_depend_on_the_batch(dt):
    rows, _, bias, table_c, labels, shared, _ = _problem(130, 128, 100, dt)
    big = ops().shared_ce_fwd(rows, table_c, bias, shared, labels)
    small = ops().shared_ce_fwd(rows[:8].contiguous(), table_c, bias, shared, labels[:8].contiguous())
    assert int((labels[:8] != 0).sum()) >= 4
    for x, y in zip(big, small):
        assert torch.equal(_bits(x[:8]), _bits(y))
    perm = torch.tensor(np.random.default_rng(5).permutation(130)).cuda()
    moved = ops().shared_ce_fwd(rows[perm].contiguous(), table_c, bias, shared, labels[perm].contiguous())
    for x, y in zip(big, moved):
        assert torch.equal(_bits(x[perm]), _bits(y))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_compaction_leaks_nothing(dt):
    """SharedCEFn scores the compacted batch: permuting the rows permutes d_rows bit for bit and leaves the loss's row terms alone."""
    p = _problem(130, 128, 100, dt)
    rows, master, bias, table_c, labels, shared, _ = p
    perm = torch.tensor(np.random.default_rng(6).permutation(130)).cuda()
    a = _run(rows, master, bias, table_c, labels, shared, True)
    b = _run(rows[perm].contiguous(), master, bias, table_c, labels[perm].contiguous(), shared, True)
    assert torch.equal(_bits(a[1].float())[perm], _bits(b[1].float()))
    assert abs(float(a[0]) - float(b[0])) <= 1e-6 * abs(float(a[0]))       # (the sum over rows runs in another order)


# ---- (6) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [False, True])
def test_d_table_out_is_added_into(det):
    rows, master, bias, table_c, labels, shared, ref = _problem(130, 128, 100, "f32")
    pre = torch.full_like(master, 0.25)
    out = pre.clone()
    r, m, b = (t.clone().requires_grad_(True) for t in (rows, master, bias))
    loss = ops().SharedCEFn.apply(r, m, b, table_c, labels, shared, det, out)
    loss.backward()
    assert m.grad is None
    ok, e = grad_ok(_f64(out - pre), ref["d_table"], "f32")
    assert ok, e
    ok, e = grad_ok(_f64(b.grad), ref["d_bias"], "f32")
    assert ok, e
    from easydgl_amd import _lib
    with pytest.raises(_lib.EdglError, match="d_table_out"):
        ops().SharedCEFn.apply(r, m, b, table_c, labels, shared, det, out[:, :64].contiguous())


# ---- (7) ---------------------------------------------------------------------------------------------------------------------------
def _models():
    from tests import test_gpu_sampled_ce as SC
    return SC


@pytest.mark.parametrize("name", ["CTSMA", "EasyDGL", "TGAT", "TiSASRec"])
def test_models_train_on_a_shared_list(name):
    SC = _models()
    S = 16
    m, feats, labels = SC.MODELS[name](8)
    mode = "bf16" if m.act_dtype == torch.bfloat16 else "f32"
    lab = labels.reshape(-1).contiguous()
    assert m.shared_negatives == 0 and m.train_negatives == 0 and m.neg_step == 0
    full = m.train_loss(feats, labels).detach()              # the flag unset: the parent's loss, bit for bit
    parent = SC._parent_train_loss(name, m, feats, labels).detach()
    assert torch.equal(_bits(full.reshape(1)), _bits(parent.reshape(1)))
    with torch.no_grad():
        rows = SC._train_rows(name, m, feats)
        tab = m.compute(m.item_embs.lookup_table)
        reg = float(full) - float(ops().ScoreCEFn.apply(rows, m.item_embs.lookup_table, m.output_bias, tab, lab))
        m.shared_negatives, m.train_neg_seed, m.neg_step = S, 5, 2
        got = float(m.train_loss(feats, labels))
        hi = m.mask if name == "EasyDGL" else m.num_items
        sh, _ = CR.sample_negatives(None, np.zeros(1, dtype=np.int64), S, 1, hi, 5, step=2, row0=0)
        sh = sh.reshape(-1)
        assert sh.shape == (S,) and (sh >= 1).all() and (sh < hi).all()
        ref = CE.reference(_f64(rows), _f64(tab), _f64(m.output_bias), _bcast(sh, rows.shape[0]), lab.cpu().numpy())
        want = ref["loss"] + reg
        assert abs(got - want) <= LOSS_TOL[mode] * abs(want), (name, got, want)
        assert m.neg_step == 2                               # train_loss does not advance the list; train_step does
        assert float(m.train_loss(feats, labels)) == got
        fixed = torch.tensor(sh, dtype=torch.int32).cuda()
        assert float(m.train_loss(feats, labels, shared=fixed)) == got
        m.shared_negatives = 0                               # an explicit list needs no flag
        assert float(m.train_loss(feats, labels, shared=fixed)) == got
        with pytest.raises(ValueError, match="both"):
            m.train_loss(feats, labels, shared=fixed, candidates=fixed[None, :].expand(rows.shape[0], S).contiguous())
        m.shared_negatives = S
    start = m._arena.detach().clone()
    with torch.no_grad():
        before = float(m.train_loss(feats, labels, shared=fixed))
    for _ in range(3):
        assert math.isfinite(float(m.train_step(feats, labels)))
    with torch.no_grad():
        after = float(m.train_loss(feats, labels, shared=fixed))
    assert m.neg_step == 5 and not torch.equal(start, m._arena) and after < before, (name, before, after)


@pytest.mark.parametrize("name", ["CTSMA", "EasyDGL", "TGAT", "TiSASRec"])
def test_models_deterministic_twice(name):
    SC = _models()
    arenas = []
    for _ in range(2):
        m, feats, labels = SC.MODELS[name](8, True)
        assert m.deterministic is True
        m.shared_negatives, m.train_neg_seed = 16, 1
        for _ in range(3):
            m.train_step(feats, labels)
        m.settle_state()
        arenas.append((m._arena.detach().clone(), m._adam_m.clone(), m._adam_v.clone()))
    for x, y in zip(*arenas):
        assert torch.equal(_bits(x), _bits(y))


# ---- (8) ---------------------------------------------------------------------------------------------------------------------------
def _lazy_pair(mode):
    """The same EasyDGL twice — dense Adam and lazy_adam — with shared_negatives = 16, l2_reg = 0 (the dense mode decays every row)."""
    import easydgl_amd
    from tests._util import flags_from, make_problem
    prob = make_problem(seed=3, batch=8, num_items=300, seqslen=20, num_units=32, num_heads=2, num_blocks=1, learning_rate=1e-2,
                        l2_reg=0.0)
    out = []
    for lazy in (False, True):
        F = flags_from(prob["cfg"], prob["mark_table"], mode)
        F.shared_negatives, F.train_neg_seed, F.lazy_adam, F.deterministic = 16, 4, lazy, True
        m = easydgl_amd.ranking(F).finalize("cuda")
        m.load_tf_variables(prob["params"])
        out.append(m)
    return out[0], out[1], to_dev(prob["feats"]), torch.as_tensor(prob["labels"]).cuda()


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_lazy_adam_touches_ids_labels_and_the_shared_list(mode):
    dense, lazy, feats, labels = _lazy_pair(mode)
    assert lazy.lazy_adam and lazy.shared_negatives == 16
    tab = lazy.item_embs.lookup_table
    lo = (tab.data_ptr() - lazy._arena.data_ptr()) // 4
    n = tab.numel()

    def table_state(m):
        sl = slice(lo, lo + n)
        st = [m._arena[sl].clone(), m._adam_m[sl].clone(), m._adam_v[sl].clone()]
        if m._shadow is not None:
            st.append(m._shadow[sl].float().clone())
        return [t.view(tab.shape) for t in st]
    before = table_state(lazy)
    sh = lazy.draw_shared_negatives(labels.device).long()
    dense.train_step(feats, labels)
    lazy.train_step(feats, labels)
    dense.settle_state(); lazy.settle_state()
    touched = torch.zeros(tab.shape[0], dtype=torch.bool, device="cuda")
    for ids in (feats["seqs_i"].reshape(-1), labels.reshape(-1), sh):
        ids = ids[(ids > 0) & (ids < tab.shape[0])]
        touched[ids] = True
    assert 0 < int(touched.sum()) < tab.shape[0] - 1
    after = table_state(lazy)
    for b, a in zip(before, after):                          # untouched rows keep every bit of w / m / v / shadow
        assert torch.equal(_bits(b[~touched]), _bits(a[~touched]))
    assert not torch.equal(before[0][touched], after[0][touched])
    # every other parameter: the dense step, bit for bit; the touched rows: the dense step
    mask = torch.ones(lazy._arena.numel(), dtype=torch.bool, device="cuda")
    mask[lo:lo + n] = False
    for x, y in ((dense._arena, lazy._arena), (dense._adam_m, lazy._adam_m), (dense._adam_v, lazy._adam_v)):
        assert torch.equal(_bits(x[mask]), _bits(y[mask]))
    # the table: at m = v = 0 the dense update of a zero-gradient row is zero, so the whole table is comparable; the bound of
    # tests/test_gpu_lazy_adam.py (2e-6 of the largest reference value for w, m, v)
    for k, (d, l) in enumerate(zip(table_state(dense)[:3], after[:3])):
        e = float((d.double() - l.double()).abs().max() / (d.double().abs().max() + 1e-30))
        print(mode, "table array", k, e)
        assert e <= 2e-6, (mode, k, e)
    if lazy._shadow is not None:
        assert torch.equal(lazy._shadow.view(torch.int16), lazy._arena.to(torch.bfloat16).view(torch.int16))
    assert not lazy.item_embs.lookup_table.grad.any() and lazy._lazy_pending == []


# ---- (9) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_name,extra", [("TiSASREC", []), ("EasyDGL", ["--deterministic"])])
def test_driver_trains_on_shared_negatives(tmp_path, monkeypatch, model_name, extra):
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
        drawn.append((seen is None, int(n), int(seed), int(step), int(labels.numel())))
        return real(seen, labels, n, lo, hi, seed, step, row0)
    monkeypatch.setattr(ops(), "sample_negatives", spy)
    res = TR.main(["--model", model_name, "--timelen", "32", "--train", str(tmp_path / "train*.tfrec"), "--valid",
                   str(tmp_path / "validation.tfrec"), "--test", str(tmp_path / "test.tfrec"), "--num_items", str(num_items),
                   "--num_units", "32", "--num_heads", "2", "--num_blocks", "1", "--seqslen", str(seqslen), "--masklen", "4",
                   "--time_scale", "86400", "--mark", str(tmp_path / "mark.pkl"), "--ct_reg", "1e-7", "--batch_size", "64",
                   "--num_epochs", "1", "--learning_rate", "1e-3", "--l2_reg", "1e-4", "--mask_seen", "--dtype", "f32",
                   "--ckpt_dir", str(tmp_path / "ckpt"), "--eval_negatives", "20", "--eval_neg_seed", "3",
                   "--shared_negatives", "16", "--train_neg_seed", "2"] + extra)
    assert set(res) == {"H1", "H5", "H10", "N1", "N5", "N10", "MRR"}
    assert all(0.0 <= v <= 1.0 and math.isfinite(v) for v in res.values())
    # 140 sequences in batches of 64: three steps (none on the static engine), ONE draw of 16 per step, keyed by the step count
    assert [d for d in drawn if d[0]] == [(True, 16, 2, 0, 1), (True, 16, 2, 1, 1), (True, 16, 2, 2, 1)]


# ---- (10) --------------------------------------------------------------------------------------------------------------------------
def test_engine_and_graph_refuse_a_model_with_shared_negatives():
    from easydgl_amd import _lib
    from easydgl_amd.engine import TrainEngine
    m, _, _ = _models()._easydgl(4)
    m.shared_negatives = 8
    with pytest.raises(_lib.EdglError, match="model.train_step"):
        TrainEngine(m, 4, use_graph=False)
    with pytest.raises(ValueError, match="train_step"):
        m.graphed_train_step({}, torch.zeros(1))
    from easydgl_amd import train as TR
    base = ["--train", "a", "--valid", "b", "--test", "c", "--model", "EasyDGL", "--num_items", "100"]
    assert TR.args(base + ["--shared_negatives", "8"]).shared_negatives == 8
    with pytest.raises(SystemExit):
        TR.args(base + ["--shared_negatives", "8", "--graph"])


def test_refusals():
    from easydgl_amd import _lib
    o = ops()
    R, I = 4, 100

    def call(C=64, S=10, dt=torch.float32, shared=None, fn=False, dev="cuda"):
        rows = torch.zeros((R, C), device=dev, dtype=dt)
        tab = torch.zeros((I, C), device=dev, dtype=dt)
        bias = torch.zeros(I - 1, device=dev)
        sh = torch.ones(S, device=dev, dtype=torch.int32) if shared is None else shared
        labels = torch.ones(R, device=dev, dtype=torch.int64)
        if fn:
            return o.SharedCEFn.apply(rows, tab.float(), bias, tab, labels, sh)
        return o.shared_ce_fwd(rows, tab, bias, sh, labels)
    assert call()[0].shape == (R, 10)
    assert call(C=24, dt=torch.bfloat16)[0].shape == (R, 10) and call(C=20)[0].shape == (R, 10)
    for fn in (False, True):
        for kw, text in ((dict(S=0), "1 <= S <= 8192"), (dict(S=8193), "1 <= S <= 8192"),
                         (dict(shared=torch.ones(10, device="cuda", dtype=torch.int64)), "int32"),
                         (dict(shared=torch.ones((R, 10), device="cuda", dtype=torch.int32)), r"int32 \[S\]"),
                         (dict(C=20, dt=torch.bfloat16), "multiple of 8"), (dict(C=528), "16 <= C <= 512"),
                         (dict(dev="cpu"), "GPU only")):
            with pytest.raises(_lib.EdglError, match=text):
                call(fn=fn, **kw)
