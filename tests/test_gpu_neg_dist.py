"""Popularity-weighted negatives with the log-Q correction on the device.

(1) edgl_sample_negatives_alias equals the numpy replica (tests/_neg_dist_ref.py) id for id, -1 slots included, and the uniform
sampler is untouched; (2) the two corrected forwards against the fp64 reference, against themselves with logq = 0 (bit equality
with the old entry points) and against the old entry points fed a shifted bias; (3) the backwards — unchanged code — against the
reference's gradients, both table-gradient modes; lazy Adam's touched set; (4) the four models, checkpoints and the driver.

The bound on a value.  v' = fl(v - q) with v the value of score_candidates.  tests/_cand_ref.py bounds v by (C + 2) u m with
u = 2^-24 and m = |b| + sum_k |x_k w_k|, for any order of the sum; the subtraction rounds once more (u |v'|) — the issue allows
2 u |v'|.  Two computed values that share the dot product d (the new op, and the old op fed b' = fl(b - q)) differ by the roundings
of fl(d + b), fl(b - q) and twice fl(. ) of the result: u (|d + b| + |b - q| + 2 |v'|), which the same bound covers when m also
counts |q|: bound = (C + 2) u (m + |q|) + 2 u |v'|."""
import math
import pickle

import numpy as np
import pytest
import torch

from tests import _cand_ce_ref as CE
from tests import _cand_ref as CR
from tests import _neg_dist_ref as ND
from tests._util import LOSS_TOL, grad_ok, to_dev

pytestmark = pytest.mark.gpu

I_ = 300
U = 2.0 ** -24


def ops():
    from easydgl_amd import ops as _ops
    return _ops


def _f64(t):
    return t.detach().double().cpu().numpy()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _zipf(I=I_):
    w = np.zeros(I)
    w[1:] = 1.0 / np.arange(1, I)
    return w


def _dist(T_reject=0, I=I_):
    return ops().build_neg_dist(_zipf(I), 1, I, T_reject)


def _dev(a, dt):
    return torch.tensor(np.asarray(a), dtype=dt).cuda()


# ---- (1) the sampler ---------------------------------------------------------------------------------------------------------------
def _seen_labels(R, T, rng):
    """Row 0 rejects the heaviest ids (1 .. T) and the next one as its label; the other rows random ids."""
    labels = rng.integers(1, I_, size=R)
    seen = None
    if T:
        seen = rng.integers(1, I_, size=(R, T))
        seen[0] = np.arange(1, T + 1)
        labels[0] = T + 1
    return seen, labels


@pytest.mark.parametrize("R,n,T", [(3, 5, 0), (3, 5, 8), (2, 257, 8)])
def test_sampler_equals_the_replica(R, n, T):
    d = _dist(T)
    seen, labels = _seen_labels(R, T, np.random.default_rng(R + n + T))
    want, _ = ND.sample_negatives(seen, labels, n, 1, I_, 11, d.thr, d.alias, step=3)
    got = ops().sample_negatives(None if seen is None else _dev(seen, torch.int64), _dev(labels, torch.int64), n, 1, I_, 11, 3, 0,
                                 dist=d)
    assert got.dtype == torch.int32 and got.shape == (R, n)
    assert np.array_equal(got.cpu().numpy(), want) and (want >= 1).all()
    for r in range(R):
        assert labels[r] not in want[r] and (seen is None or not np.isin(want[r], seen[r]).any())
    # the uniform sampler: untouched
    uni, _ = CR.sample_negatives(seen, labels, n, 1, I_, 11, step=3)
    got_u = ops().sample_negatives(None if seen is None else _dev(seen, torch.int64), _dev(labels, torch.int64), n, 1, I_, 11, 3, 0)
    assert np.array_equal(got_u.cpu().numpy(), uni) and not np.array_equal(uni, want)


def test_sampler_leaves_minus_one_where_the_replica_does():
    """A row that rejects far more than the table was checked for (the heaviest 120 ids of Zipf(1): 0.85 of the weight) runs out of
    attempts in some slots: the same slots, and the same ids elsewhere."""
    d = _dist(0)
    d.T_reject = 120                                         # (a table checked for fewer ids: the draw itself does not depend on it)
    seen = np.tile(np.arange(1, 121), (2, 1))
    labels = np.array([121, 0])
    want, worst = ND.sample_negatives(seen, labels, 257, 1, I_, 5, d.thr, d.alias)
    assert worst == 32 and int((want < 0).sum()) == 5
    got = ops().sample_negatives(_dev(seen, torch.int64), _dev(labels, torch.int64), 257, 1, I_, 5, dist=d)
    assert np.array_equal(got.cpu().numpy(), want)


def test_sampler_at_the_tightest_legal_range():
    T = 8
    hi = 1 + 2 * (T + 1)
    d = ops().build_neg_dist(np.ones(hi), 1, hi, T)          # uniform weights, hi - lo = 2 (T + 1)
    rng = np.random.default_rng(2)
    seen = np.stack([rng.permutation(np.arange(1, hi))[:T + 1] for _ in range(3)])
    labels, seen = seen[:, 0].copy(), seen[:, 1:]
    want, _ = ND.sample_negatives(seen, labels, 64, 1, hi, 9, d.thr, d.alias)
    got = ops().sample_negatives(_dev(seen, torch.int64), _dev(labels, torch.int64), 64, 1, hi, 9, dist=d)
    assert np.array_equal(got.cpu().numpy(), want)
    # every bucket is full: the weighted draw IS the uniform draw
    assert np.array_equal(want, CR.sample_negatives(seen, labels, 64, 1, hi, 9)[0])


def test_sampler_shared_draw_and_row0():
    d = _dist(0)
    one = np.zeros(1, dtype=np.int64)
    want, _ = ND.sample_negatives(None, one, 1500, 1, I_, 4, d.thr, d.alias, step=6)
    got = ops().sample_negatives(None, _dev(one, torch.int64), 1500, 1, I_, 4, 6, 0, dist=d)
    assert np.array_equal(got.cpu().numpy(), want) and (want >= 1).all()
    cnt = np.bincount(want.reshape(-1), minlength=I_)
    assert cnt[1] > 5 * max(cnt[150:].max(), 1)              # the head of Zipf(1) is drawn far more often than the tail
    labels = np.array([3, 4, 5, 6])
    full = ops().sample_negatives(None, _dev(labels, torch.int64), 16, 1, I_, 4, 6, 0, dist=d).cpu().numpy()
    part = ops().sample_negatives(None, _dev(labels[2:], torch.int64), 16, 1, I_, 4, 6, 2, dist=d).cpu().numpy()
    assert np.array_equal(full[2:], part)
    assert np.array_equal(full, ND.sample_negatives(None, labels, 16, 1, I_, 4, d.thr, d.alias, step=6)[0])


def test_sampler_refusals():
    from easydgl_amd import _lib
    d = _dist(0)
    lab = torch.ones(2, dtype=torch.int64).cuda()
    with pytest.raises(_lib.EdglError, match=r"NegDist over \[1, 200\)"):
        ops().sample_negatives(None, lab, 4, 1, 200, 0, dist=d)
    with pytest.raises(_lib.EdglError, match="T_reject = 0"):
        ops().sample_negatives(torch.ones((2, 3), dtype=torch.int64).cuda(), lab, 4, 1, I_, 0, dist=d)
    logq = d.logq_on("cuda")
    rows = torch.zeros((2, 64)).cuda()
    tab, bias = torch.zeros((I_, 64)).cuda(), torch.zeros(I_ - 1).cuda()
    for bad in (logq[:-1].contiguous(), logq.double(), logq.cpu()):
        with pytest.raises(_lib.EdglError, match="logq must be a contiguous f32"):
            ops().cand_ce_fwd(rows, tab, bias, torch.ones((2, 4), dtype=torch.int32).cuda(), lab, bad)
        with pytest.raises(_lib.EdglError, match="logq must be a contiguous f32"):
            ops().shared_ce_fwd(rows, tab, bias, torch.ones(4, dtype=torch.int32).cuda(), lab, bad)


# ---- (2) the forwards ----------------------------------------------------------------------------------------------------------------
def _logq(seed=0):
    """logq of a popularity table over [1, I): counts from a Zipf draw, alpha 0.75 — terms between about -7.5 and -2.5."""
    rng = np.random.default_rng(seed)
    cnt = np.bincount(rng.zipf(1.3, size=20000) % I_, minlength=I_)
    d = ops().build_neg_dist(ops().neg_weights("popularity", I_, 1, I_, cnt, 0.75), 1, I_, 0)
    return d.logq, d.logq_on("cuda")


def _value_bounds(rows, table_c, bias, logq, ids_of_row, C):
    """fp64 v', and the bound of the module docstring, for the ids of every row (ids_of_row[r]: int array; dead ids give -inf)."""
    rows, tab, b = _f64(rows), _f64(table_c), _f64(bias)
    out_v, out_b = [], []
    for r, ids in enumerate(ids_of_row):
        v, mag = CR.values(rows, tab, b, ids, None, r)
        ok = (np.asarray(ids) >= 0) & (np.asarray(ids) < tab.shape[0])
        q = np.where(ok, logq.astype(np.float64)[np.where(ok, ids, 0)], 0.0)
        vq = v - q
        out_v.append(vq)
        out_b.append((C + 2) * U * (mag + np.abs(q)) + 2 * U * np.abs(np.where(np.isfinite(vq), vq, 0.0)))
    return out_v, out_b


def _lse_bound(value_bounds, N, lse):
    """lse moves by at most the largest error of a value; the f32 sum of N + 1 exponentials adds (N + 1) u relative to the sum, the
    fast exponential |v - m| u with |v - m| < 30 here (the reasoning of tests/test_gpu_sampled_ce.py), both absolute on the
    logarithm; M + log S rounds twice."""
    return float(value_bounds.max()) + (N + 32) * U + 2 * U * abs(lse)


PER_ROW = [(3, 5, 16), (7, 257, 256), (130, 100, 128)]
SHARED = [(129, 129, 16), (7, 257, 256), (130, 100, 128)]


@pytest.mark.parametrize("R,N,C", PER_ROW)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_per_row_forward(dt, R, N, C):
    from tests import test_gpu_sampled_ce as SC
    rows, _, bias, table_c, labels, cand, _ = SC._problem(R, C, N, dt)
    c, lab = cand.cpu().numpy().astype(np.int64), labels.cpu().numpy()
    assert (c == -1).any() and (c == lab[:, None]).any() and (c == 0).any() and (c[:, 3] == c[:, 4]).any()
    logq_h, logq = _logq()
    vals, label_val, lse = ops().cand_ce_fwd(rows, table_c, bias, cand, labels, logq)
    # logq = 0: the old entry point, bit for bit
    old = ops().cand_ce_fwd(rows, table_c, bias, cand, labels)
    zero = ops().cand_ce_fwd(rows, table_c, bias, cand, labels, torch.zeros_like(logq))
    for x, y in zip(old, zero):
        assert torch.equal(_bits(x), _bits(y))
    # the fp64 reference, value by value
    ids = [np.concatenate([[lab[r]], c[r]]) for r in range(R)]
    want, bound = _value_bounds(rows, table_c, bias, logq_h, ids, C)
    shifted = ops().cand_ce_fwd(rows, table_c, (bias - logq[1:]).contiguous(), cand, labels)
    ref = ND.reference(_f64(rows), _f64(table_c), _f64(bias), logq_h, c, lab)
    g, s = _f64(vals), _f64(shifted[0])
    worst = 0.0
    for r in range(R):
        if lab[r] == 0:
            assert (g[r] == -math.inf).all() and float(lse[r]) == 0.0 and float(label_val[r]) == 0.0
            continue
        dead = np.concatenate([[False], (c[r] < 0) | (c[r] >= I_) | (c[r] == lab[r])])
        assert (g[r][dead] == -math.inf).all() and np.isfinite(g[r][~dead]).all()
        for other in (want[r], s[r]):                        # the reference, and the old op fed out_bias - logq[1:]
            e = np.abs(g[r][~dead] - other[~dead]) / bound[r][~dead]
            worst = max(worst, float(e.max()))
            assert (e <= 1.0).all(), (dt, R, N, C, r, float(e.max()))
        assert float(label_val[r]) == g[r][0]
        assert abs(float(lse[r]) - ref["lse"][r]) <= _lse_bound(bound[r][~dead], N, ref["lse"][r])
    print((dt, R, N, C), "worst error / bound", worst)
    assert not torch.equal(vals, old[0])


@pytest.mark.parametrize("R,S,C", SHARED)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_shared_forward(dt, R, S, C):
    from tests import test_gpu_shared_ce as SH
    rows, _, bias, table_c, labels, shared, _ = SH._problem(R, C, S, dt)
    sh, lab = shared.cpu().numpy().astype(np.int64), labels.cpu().numpy()
    assert sh[0] == -1 and sh[1] == 0 and sh[3] == sh[4] and (sh[None, :] == lab[:, None]).any()
    logq_h, logq = _logq()
    vals, label_val, lse = ops().shared_ce_fwd(rows, table_c, bias, shared, labels, logq)
    old = ops().shared_ce_fwd(rows, table_c, bias, shared, labels)
    zero = ops().shared_ce_fwd(rows, table_c, bias, shared, labels, torch.zeros_like(logq))
    for x, y in zip(old, zero):
        assert torch.equal(_bits(x), _bits(y))
    ids = [np.concatenate([[lab[r]], sh]) for r in range(R)]
    want, bound = _value_bounds(rows, table_c, bias, logq_h, ids, C)
    shifted = ops().shared_ce_fwd(rows, table_c, (bias - logq[1:]).contiguous(), shared, labels)
    ref = ND.reference(_f64(rows), _f64(table_c), _f64(bias), logq_h, SH._bcast(sh, R), lab)
    g = np.concatenate([_f64(label_val)[:, None], _f64(vals)], axis=1)
    s = np.concatenate([_f64(shifted[1])[:, None], _f64(shifted[0])], axis=1)
    worst = 0.0
    for r in range(R):
        if lab[r] == 0:
            assert (g[r][1:] == -math.inf).all() and float(lse[r]) == 0.0 and float(label_val[r]) == 0.0
            continue
        dead = np.concatenate([[False], (sh < 0) | (sh >= I_) | (sh == lab[r])])
        assert (g[r][dead] == -math.inf).all() and np.isfinite(g[r][~dead]).all()
        for other in (want[r], s[r]):
            e = np.abs(g[r][~dead] - other[~dead]) / bound[r][~dead]
            worst = max(worst, float(e.max()))
            assert (e <= 1.0).all(), (dt, R, S, C, r, float(e.max()))
        assert abs(float(lse[r]) - ref["lse"][r]) <= _lse_bound(bound[r][~dead], S, ref["lse"][r])
    print((dt, R, S, C), "worst error / bound", worst)


# ---- (3) the backwards -----------------------------------------------------------------------------------------------------------------
def _run(fn, rows, master, bias, table_c, labels, lists, det, logq):
    r, m, b = (t.clone().requires_grad_(True) for t in (rows, master, bias))
    loss = fn.apply(r, m, b, table_c, labels, lists, det, None, logq)
    loss.backward()
    return loss.detach(), r.grad, m.grad, b.grad


@pytest.mark.parametrize("kind,R,N,C", [("rows",) + s for s in PER_ROW] + [("shared",) + s for s in SHARED])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_loss_and_gradients(dt, kind, R, N, C):
    """The backward kernels are the parent's: dv comes from the saved (corrected) vals and lse, and the correction is a constant."""
    if kind == "rows":
        from tests import test_gpu_sampled_ce as M
        fn = ops().SampledCEFn
    else:
        from tests import test_gpu_shared_ce as M
        fn = ops().SharedCEFn
    rows, master, bias, table_c, labels, lists, plain = M._problem(R, C, N, dt)
    logq_h, logq = _logq()
    li = lists.cpu().numpy().astype(np.int64)
    ref = ND.reference(_f64(rows), _f64(table_c), _f64(bias), logq_h, li if kind == "rows" else M._bcast(li, R), labels.cpu().numpy())
    assert abs(ref["loss"] - plain["loss"]) > LOSS_TOL[dt] * abs(plain["loss"])            # the correction moves the loss
    outs = {}
    for det in (False, True):
        loss, d_rows, d_table, d_bias = outs[det] = _run(fn, rows, master, bias, table_c, labels, lists, det, logq)
        err = abs(float(loss) - ref["loss"]) / abs(ref["loss"])
        print((dt, kind, R, N, C, det), "loss", float(loss), ref["loss"], err)
        assert err <= LOSS_TOL[dt]
        for name, got in (("d_rows", d_rows), ("d_table", d_table), ("d_bias", d_bias)):
            ok, e = grad_ok(_f64(got), ref[name], dt)
            print((dt, kind, R, N, C, det), name, e)
            assert ok, (name, e)
        assert not d_table[0].any()
    again = _run(fn, rows, master, bias, table_c, labels, lists, True, logq)
    for x, y in zip(outs[True], again):                      # the deterministic form: the same bits twice
        assert torch.equal(_bits(x.float()), _bits(y.float()))
    assert torch.equal(_bits(outs[True][0]), _bits(outs[False][0]))
    # logq = 0 through the autograd functions: the parent's loss and d_rows, bit for bit
    z = _run(fn, rows, master, bias, table_c, labels, lists, True, torch.zeros_like(logq))
    r, m, b = (t.clone().requires_grad_(True) for t in (rows, master, bias))
    p = fn.apply(r, m, b, table_c, labels, lists, True)
    p.backward()
    assert torch.equal(_bits(z[0]), _bits(p.detach())) and torch.equal(_bits(z[1].float()), _bits(r.grad.float()))
    assert torch.equal(_bits(z[2]), _bits(m.grad)) and torch.equal(_bits(z[3]), _bits(b.grad))


def _lazy_model(mode, **kw):
    import easydgl_amd
    from tests._util import flags_from, make_problem
    prob = make_problem(seed=3, batch=8, num_items=300, seqslen=20, num_units=32, num_heads=2, num_blocks=1, learning_rate=1e-2,
                        l2_reg=0.0)
    F = flags_from(prob["cfg"], prob["mark_table"], mode)
    F.train_neg_seed, F.deterministic = 4, True
    for k, v in kw.items():
        setattr(F, k, v)
    m = easydgl_amd.ranking(F).finalize("cuda")
    m.load_tf_variables(prob["params"])
    return m, to_dev(prob["feats"]), torch.as_tensor(prob["labels"]).cuda()


@pytest.mark.parametrize("est", ["train_negatives", "shared_negatives"])
def test_lazy_adam_touches_what_the_weighted_step_used(est):
    """lazy_adam with a weighted sampler: the rows outside (input ids, labels, the step's weighted lists) keep every bit, and every
    other parameter takes the dense model's step bit for bit (deterministic mode on both)."""
    dense, feats, labels = _lazy_model("f32", neg_sampler="log_uniform", **{est: 16})
    lazy, _, _ = _lazy_model("f32", neg_sampler="log_uniform", lazy_adam=True, **{est: 16})
    tab = lazy.item_embs.lookup_table
    lo = (tab.data_ptr() - lazy._arena.data_ptr()) // 4
    n = tab.numel()
    sl = slice(lo, lo + n)
    before = [t[sl].clone().view(tab.shape) for t in (lazy._arena, lazy._adam_m, lazy._adam_v)]
    lab = labels.reshape(-1).contiguous()
    d = lazy._negative_dist()
    if est == "shared_negatives":
        lists = lazy.draw_shared_negatives(labels.device).long()
        want, _ = ND.sample_negatives(None, np.zeros(1, dtype=np.int64), 16, 1, lazy.mask, 4, d.thr, d.alias)
    else:
        lists = ops().sample_negatives(None, lab, 16, 1, lazy.mask, 4, 0, 0, dist=d).long().reshape(-1)
        want, _ = ND.sample_negatives(None, lab.cpu().numpy(), 16, 1, lazy.mask, 4, d.thr, d.alias)
    assert np.array_equal(lists.cpu().numpy().reshape(-1), want.reshape(-1))
    dense.train_step(feats, labels)
    lazy.train_step(feats, labels)
    dense.settle_state(); lazy.settle_state()
    touched = torch.zeros(tab.shape[0], dtype=torch.bool, device="cuda")
    for ids in (feats["seqs_i"].reshape(-1), lab, lists):
        ids = ids[(ids > 0) & (ids < tab.shape[0])]
        touched[ids] = True
    assert 0 < int(touched.sum()) < tab.shape[0] - 1
    after = [t[sl].clone().view(tab.shape) for t in (lazy._arena, lazy._adam_m, lazy._adam_v)]
    for b, a in zip(before, after):
        assert torch.equal(_bits(b[~touched]), _bits(a[~touched]))
    assert not torch.equal(before[0][touched], after[0][touched])
    mask = torch.ones(lazy._arena.numel(), dtype=torch.bool, device="cuda")
    mask[sl] = False
    for x, y in ((dense._arena, lazy._arena), (dense._adam_m, lazy._adam_m), (dense._adam_v, lazy._adam_v)):
        assert torch.equal(_bits(x[mask]), _bits(y[mask]))
    for k, (x, y) in enumerate(zip((dense._arena, dense._adam_m, dense._adam_v), after)):
        x = x[sl].view(tab.shape)
        e = float((x.double() - y.double()).abs().max() / (x.double().abs().max() + 1e-30))
        assert e <= 2e-6, (est, k, e)                        # (the bound of tests/test_gpu_lazy_adam.py)


# ---- (4) the models --------------------------------------------------------------------------------------------------------------------
def _counts(hi, seed=0):
    rng = np.random.default_rng(seed)
    return np.bincount(rng.zipf(1.3, size=5000) % hi, minlength=hi)


@pytest.mark.parametrize("est", ["train_negatives", "shared_negatives"])
@pytest.mark.parametrize("name", ["CTSMA", "EasyDGL", "TGAT", "TiSASRec"])
def test_models_train_on_weighted_negatives(name, est, tmp_path):
    from easydgl_amd import train as TR
    from tests import test_gpu_sampled_ce as SC
    N = 8
    m, feats, labels = SC.MODELS[name](8)
    mode = "bf16" if m.act_dtype == torch.bfloat16 else "f32"
    lab = labels.reshape(-1).contiguous()
    assert m.neg_sampler == "uniform" and m.neg_alpha == 0.75
    full = m.train_loss(feats, labels).detach()              # the flags unset: the parent's loss, bit for bit
    parent = SC._parent_train_loss(name, m, feats, labels).detach()
    assert torch.equal(_bits(full.reshape(1)), _bits(parent.reshape(1)))
    hi = m.mask if name == "EasyDGL" else m.num_items
    w = ops().neg_weights("popularity", hi, 1, hi, _counts(hi), 0.75)
    with torch.no_grad():
        rows = SC._train_rows(name, m, feats)
        tab = m.compute(m.item_embs.lookup_table)
        reg = float(full) - float(ops().ScoreCEFn.apply(rows, m.item_embs.lookup_table, m.output_bias, tab, lab))
        setattr(m, est, N)
        m.train_neg_seed, m.neg_step = 5, 2
        uniform = float(m.train_loss(feats, labels))
        m.neg_sampler = "popularity"
        with pytest.raises(ValueError, match="set_negative_weights"):
            m.train_loss(feats, labels)
        m.set_negative_weights(w)
        d = m._negative_dist()
        got = float(m.train_loss(feats, labels))
        if est == "train_negatives":
            cand, _ = ND.sample_negatives(None, lab.cpu().numpy(), N, 1, hi, 5, d.thr, d.alias, step=2)
            kw = dict(candidates=torch.tensor(cand, dtype=torch.int32).cuda())
        else:
            sh, _ = ND.sample_negatives(None, np.zeros(1, dtype=np.int64), N, 1, hi, 5, d.thr, d.alias, step=2)
            cand = np.broadcast_to(sh.reshape(-1), (rows.shape[0], N))
            kw = dict(shared=torch.tensor(sh.reshape(-1), dtype=torch.int32).cuda())
        assert (cand >= 1).all() and (cand < hi).all()
        ref = ND.reference(_f64(rows), _f64(tab), _f64(m.output_bias), d.logq, cand, lab.cpu().numpy())
        want = ref["loss"] + reg
        assert abs(got - want) <= LOSS_TOL[mode] * abs(want), (name, est, got, want)
        assert abs(got - uniform) > LOSS_TOL[mode] * abs(want)
        assert float(m.train_loss(feats, labels, **kw)) == got          # an explicit list gets the correction too
        assert m.neg_step == 2
    start = m._arena.detach().clone()
    with torch.no_grad():
        before = float(m.train_loss(feats, labels, **kw))
    for _ in range(3):
        assert math.isfinite(float(m.train_step(feats, labels)))
    with torch.no_grad():
        after = float(m.train_loss(feats, labels, **kw))
    assert m.neg_step == 5 and not torch.equal(start, m._arena) and after < before, (name, est, before, after)
    # save and restore: the next step's lists are the ones the uninterrupted run draws
    TR.save_checkpoint(m, str(tmp_path / "m.pt"))
    m2, _, _ = SC.MODELS[name](8)
    setattr(m2, est, N)
    m2.train_neg_seed = 5
    with pytest.raises(ValueError, match="a resumed run keeps its negative sampler"):
        TR.load_checkpoint(m2, str(tmp_path / "m.pt"))
    m2.neg_sampler = "popularity"
    m2.set_negative_weights(w)                               # rebuilt from the same counts: the same table
    TR.load_checkpoint(m2, str(tmp_path / "m.pt"))
    assert m2.neg_step == 5
    d2 = m2._negative_dist()
    assert np.array_equal(d2.thr, d.thr) and np.array_equal(d2.alias, d.alias)
    if est == "shared_negatives":
        a, b = m.draw_shared_negatives("cuda"), m2.draw_shared_negatives("cuda")
        assert torch.equal(a, b) and not torch.equal(a, m.draw_shared_negatives("cuda", step=4))
    with torch.no_grad():
        assert float(m.train_loss(feats, labels)) == float(m2.train_loss(feats, labels))


def test_eval_candidates_draws_by_the_weights():
    from tests import test_gpu_sampled_ce as SC
    m, feats, labels = SC.MODELS["TiSASRec"](8)
    hi = m.num_items
    T = feats["seqs_i"].shape[1]
    d = m.negative_dist(ops().neg_weights("popularity", hi, 1, hi, _counts(hi), 0.75), T_reject=T)
    lab = m._last_labels(labels)
    want, _ = ND.sample_negatives(feats["seqs_i"].cpu().numpy(), lab.cpu().numpy(), 20, 1, hi, 3, d.thr, d.alias, row0=5)
    rank = m.eval_candidates(feats, labels, None, 20, True, 3, 0, 5, dist=d)
    # raw logits, no correction: the rank of the label inside the replica's lists
    again = m.eval_candidates(feats, labels, torch.tensor(want, dtype=torch.int32).cuda(), mask_seen=True)
    assert torch.equal(rank, again) and rank.dtype == torch.int32
    uni = m.eval_candidates(feats, labels, None, 20, True, 3, 0, 5)
    m.reset_metrics((1, 5, 10))
    m.eval_step(feats, labels, negatives=20, neg_seed=3, row0=5, neg_dist=d)
    got = m.metrics()
    m.reset_metrics((1, 5, 10))
    m.eval_step(feats, labels, candidates=torch.tensor(want, dtype=torch.int32).cuda())
    assert got == m.metrics() and uni.shape == rank.shape


@pytest.mark.parametrize("model_name,extra", [("TiSASREC", ["--train_negatives", "8"]),
                                              ("EasyDGL", ["--shared_negatives", "16", "--deterministic", "--device_data"])])
def test_driver_trains_on_popularity_negatives(tmp_path, monkeypatch, model_name, extra):
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

    def spy(seen, labels, n, lo, hi, seed, step=0, row0=0, dist=None):
        drawn.append((seen is None, int(n), int(seed), int(step), None if dist is None else dist.T_reject))
        return real(seen, labels, n, lo, hi, seed, step, row0, dist=dist)
    monkeypatch.setattr(ops(), "sample_negatives", spy)
    res = TR.main(["--model", model_name, "--timelen", "32", "--train", str(tmp_path / "train*.tfrec"), "--valid",
                   str(tmp_path / "validation.tfrec"), "--test", str(tmp_path / "test.tfrec"), "--num_items", str(num_items),
                   "--num_units", "32", "--num_heads", "2", "--num_blocks", "1", "--seqslen", str(seqslen), "--masklen", "4",
                   "--time_scale", "86400", "--mark", str(tmp_path / "mark.pkl"), "--ct_reg", "1e-7", "--batch_size", "64",
                   "--num_epochs", "1", "--learning_rate", "1e-3", "--l2_reg", "1e-4", "--mask_seen", "--dtype", "f32",
                   "--ckpt_dir", str(tmp_path / "ckpt"), "--eval_negatives", "20", "--eval_neg_seed", "3", "--train_neg_seed", "2",
                   "--neg_sampler", "popularity", "--eval_neg_sampler", "popularity"] + extra)
    assert set(res) == {"H1", "H5", "H10", "N1", "N5", "N10", "MRR"}
    assert all(0.0 <= v <= 1.0 and math.isfinite(v) for v in res.values())
    n = int(extra[1])
    # three training steps on weighted lists (T_reject 0), the evaluation on its own weighted lists (the history is rejected)
    assert [d for d in drawn if d[0]] == [(True, n, 2, 0, 0), (True, n, 2, 1, 0), (True, n, 2, 2, 0)]
    ev = [d for d in drawn if not d[0]]
    assert ev and all(d[:4] == (False, 20, 3, 0) and d[4] is not None and d[4] >= seqslen - 1 for d in ev)
