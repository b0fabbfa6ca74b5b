"""Lazy row-wise Adam for the item table of sampled-softmax training on the GPU: edgl_adam_rows against the fp64
reference of tests/_lazy_adam_ref.py (touched rows updated once, every other bit kept), against the dense edgl_adam_step, and
the model mode FLAGS.lazy_adam against a dense twin — first step, later steps, l2, no dense temporaries, reproducibility.
Tolerances: those of test_gpu_ops.py::test_adam_matches_tf_form (2e-6 of the largest reference value for w, m, v; 5e-3 for
a bf16 shadow held to fp64 weights)."""
import numpy as np
import pytest
import torch

from tests import _cand_ref as CR
from tests import _lazy_adam_ref as LA
from tests._util import flags_from, make_problem, to_dev

pytestmark = pytest.mark.gpu

TOL = 2e-6
# The C ABI takes lr, beta1, beta2 and eps as f32: the reference is given the values the kernel receives (0.999f is
# 0.99900001287..., which moves 1 - beta2 by 1.3e-5 of itself), so that the bound holds the arithmetic, not the rounding of an input.
LR = float(np.float32(1e-2))
HP = dict(b1=float(np.float32(0.9)), b2=float(np.float32(0.999)), eps=float(np.float32(1e-8)))


def ops():
    from easydgl_amd import ops as o
    return o


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _close(got, want, what, tol=TOL):
    e = float(np.abs(got - want).max() / (np.abs(want).max() + 1e-30))
    print(f"{what}: max-abs-err / max-abs-ref = {e:.3e}")
    assert e <= tol, f"{what}: {e:.3e} > {tol:.1e}"


def _advance(state, steps=1):
    """The step count and learning rate of `steps` more Adam steps in `state`, as the model leaves them: edgl_adam_step on a
    range of its own."""
    d = torch.zeros(8, device="cuda")
    for _ in range(steps):
        ops().adam_step(d, torch.zeros_like(d), torch.zeros_like(d), torch.zeros_like(d), LR, state, 0.0, None, None)


def _arrays(I, C, seed, shadow):
    rng = np.random.default_rng(seed)
    w = torch.tensor(rng.standard_normal((I, C)), dtype=torch.float32).cuda()
    g = torch.tensor(rng.standard_normal((I, C)) * 0.1, dtype=torch.float32).cuda()
    m = torch.tensor(rng.standard_normal((I, C)) * 0.05, dtype=torch.float32).cuda()
    v = torch.tensor(rng.random((I, C)) * 0.01, dtype=torch.float32).cuda()
    sh = torch.tensor(rng.standard_normal((I, C)), dtype=torch.float32).cuda().to(torch.bfloat16) if shadow else None
    return w, g, m, v, sh


def _check_rows(after, before, ref, what):
    """after / before: (w, g, m, v, shadow | None) on the device; ref: LA.adam_rows of `before`."""
    rw, rm, rv, _, t = ref
    tt = torch.tensor(t).cuda()
    w, g, m, v, sh = after
    assert t.any() and (~t).any()
    _close(_f64(w)[t], rw[t], what + " w")
    _close(_f64(m)[t], rm[t], what + " m")
    _close(_f64(v)[t], rv[t], what + " v")
    assert not g[tt].any(), what + ": the gradient rows of touched rows read zero"
    if sh is not None:
        assert torch.equal(_bits(sh[tt]), _bits(w[tt].to(torch.bfloat16))), what + ": shadow = bf16(w) bit for bit"
    for k, (a, b) in enumerate(zip(after, before)):
        if a is not None:
            assert torch.equal(_bits(a[~tt]), _bits(b[~tt])), f"{what}: untouched rows of array {k} keep every bit"


# ---- (1) the kernel against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("C", [4, 16, 48, 64, 256, 512])
def test_kernel_matches_the_reference(C, shadow):
    I = 37
    before = _arrays(I, C, C, shadow)
    ids = np.array([0, I, I + 3, 5, 5, 9, 12, 36], dtype=np.int64)
    labels = np.array([9, 0, 14, 5], dtype=np.int64)
    cand = np.array([[-1, 9, 12, 20],            # an empty slot, a slot equal to the row's label, an id also in `ids`
                     [30, 31, 32, 33],           # the row of label 0: rows listed nowhere else
                     [5, 20, 20, 21],            # repeats within the list and across the sources
                     [14, I + 2, 0, 22]], dtype=np.int32)
    after = tuple(None if a is None else a.clone() for a in before)
    state = torch.zeros(2, dtype=torch.int64).cuda()
    stamp = torch.zeros(I, dtype=torch.int32).cuda()
    _advance(state, 3)
    w, g, m, v, sh = after
    ops().adam_rows(w, g, m, v, sh, torch.tensor(ids).cuda(), torch.tensor(labels).cuda(), torch.tensor(cand).cuda(), stamp, state,
                    l2=1e-2)
    ref = LA.adam_rows(_f64(before[0]), _f64(before[1]), _f64(before[2]), _f64(before[3]), 3, LR, ids, labels, cand, l2=1e-2, **HP)
    assert sorted(np.nonzero(ref[4])[0].tolist()) == [5, 9, 12, 14, 20, 21, 22, 36]
    _check_rows(after, before, ref, f"C={C}")
    assert sorted(torch.nonzero(stamp).reshape(-1).tolist()) == [5, 9, 12, 14, 20, 21, 22, 36] and int(stamp.max()) == 3


# ---- (2) one update per row under contention ------------------------------------------------------------------------------------
def test_one_update_per_row_under_contention():
    I, C, n = 37, 64, 4096
    before = _arrays(I, C, 2, True)
    w, g, m, v, sh = tuple(a.clone() for a in before)
    labels = torch.full((n,), 7, dtype=torch.int64).cuda()
    ids = torch.full((n,), 11, dtype=torch.int64).cuda()
    state = torch.zeros(2, dtype=torch.int64).cuda()
    stamp = torch.zeros(I, dtype=torch.int32).cuda()
    _advance(state)
    ops().adam_rows(w, g, m, v, sh, ids, labels, None, stamp, state)
    r1 = LA.adam_rows(_f64(before[0]), _f64(before[1]), _f64(before[2]), _f64(before[3]), 1, LR, ids.cpu().numpy(), labels.cpu().numpy(), **HP)
    assert np.nonzero(r1[4])[0].tolist() == [7, 11]
    _check_rows((w, g, m, v, sh), before, r1, "first call")
    # the same step again: the rows are claimed, nothing moves (the gradient, filled again, stays)
    g2 = before[1].clone()
    mid = tuple(a.clone() for a in (w, g2, m, v, sh))
    ops().adam_rows(w, g2, m, v, sh, ids, labels, None, stamp, state)
    for a, b in zip((w, g2, m, v, sh), mid):
        assert torch.equal(_bits(a), _bits(b))
    # the step advanced: a second update
    _advance(state)
    ops().adam_rows(w, g2, m, v, sh, ids, labels, None, stamp, state)
    r2 = LA.adam_rows(r1[0], _f64(before[1]), r1[1], r1[2], 2, LR, ids.cpu().numpy(), labels.cpu().numpy(), **HP)
    _check_rows((w, g2, m, v, sh), mid, r2, "second step")
    assert int(stamp[7]) == 2 and int(stamp[11]) == 2


@pytest.mark.parametrize("n", [100, 1200000])
def test_partial_wave_and_more_than_one_pass_of_the_grid(n):
    """The grid is capped at 4096 workgroups of 256 entries per pass: 100 entries are less than two waves, 1.2 M need a second
    pass; ids drawn from a third of the table, so most are repeats."""
    I, C = 1000, 64
    before = _arrays(I, C, n, True)
    w, g, m, v, sh = tuple(a.clone() for a in before)
    ids = np.random.default_rng(n).integers(-3, I // 3, size=n)
    labels = np.array([I - 1, 0, I], dtype=np.int64)
    cand = np.array([[I - 2, I - 2], [I - 3, I - 4], [I - 5, I - 6]], dtype=np.int32)
    state = torch.zeros(2, dtype=torch.int64).cuda()
    stamp = torch.zeros(I, dtype=torch.int32).cuda()
    _advance(state, 2)
    ops().adam_rows(w, g, m, v, sh, torch.tensor(ids).cuda(), torch.tensor(labels).cuda(), torch.tensor(cand).cuda(), stamp, state)
    ref = LA.adam_rows(_f64(before[0]), _f64(before[1]), _f64(before[2]), _f64(before[3]), 2, LR, ids, labels, cand, **HP)
    assert ref[4][I - 1] and ref[4][I - 2] and not ref[4][I - 6:I - 2].any()
    _check_rows((w, g, m, v, sh), before, ref, f"n={n}")


# ---- (3) every row listed equals the dense kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [48, 256])
def test_every_row_listed_equals_the_dense_adam_step(C):
    I = 37
    before = _arrays(I, C, 100 + C, True)
    w, g, m, v, sh = tuple(a.clone() for a in before)
    dw, dg, dm, dv, dsh = tuple(a.clone() for a in before)
    st_a, st_b = torch.zeros(2, dtype=torch.int64).cuda(), torch.zeros(2, dtype=torch.int64).cuda()
    stamp = torch.zeros(I, dtype=torch.int32).cuda()
    ids = torch.arange(I, dtype=torch.int64).cuda()
    for t in (1, 2):
        _advance(st_a)
        w_pre = w.clone()
        ops().adam_rows(w, g, m, v, sh, ids, None, None, stamp, st_a)
        ops().adam_step(dw.view(-1), dg.view(-1), dm.view(-1), dv.view(-1), LR, st_b, 0.0, None, dsh.view(-1))
        _close(_f64(w)[1:], _f64(dw)[1:], f"t={t} w vs dense")
        _close(_f64(m)[1:], _f64(dm)[1:], f"t={t} m vs dense")
        _close(_f64(v)[1:], _f64(dv)[1:], f"t={t} v vs dense")
        _close(_f64(sh)[1:], _f64(dw)[1:], f"t={t} shadow vs dense w", 5e-3)
        assert torch.equal(_bits(w[0]), _bits(w_pre[0])) and not g[1:].any()      # row 0 is never touched; the gradient is consumed
        g.copy_(dg)                                                                # the same gradient again for the next step
        dw[0], dm[0], dv[0] = before[0][0], before[2][0], before[3][0]             # (the dense kernel updates row 0 too)


# ---- the model mode ------------------------------------------------------------------------------------------------------------
def _model(prob, dt, lazy, l2=0.0, N=5, seed=0, det=True, drop=0.0):
    import easydgl_amd
    F = flags_from(prob["cfg"], prob["mark_table"], dt, drop, drop)
    F.l2_reg, F.learning_rate = l2, LR
    F.train_negatives, F.train_neg_seed, F.deterministic, F.lazy_adam = N, seed, det, lazy
    m = easydgl_amd.ranking(F).finalize("cuda")
    m.load_tf_variables(prob["params"])
    return m


def _small(seed=5, **kw):
    return make_problem(seed=seed, batch=4, num_items=50, seqslen=8, num_units=32, num_heads=2, num_blocks=1, ct_reg=0.0, **kw)


def _batch(prob):
    return to_dev(prob["feats"]), torch.as_tensor(prob["labels"]).cuda()


def _table_state(m):
    lo = m._lazy_range[0] if m.lazy_adam else m._offsets["item_embs.lookup_table"]
    tab = m.item_embs.lookup_table
    n = tab.numel()
    return tab.data, m._adam_m[lo:lo + n].view(tab.shape), m._adam_v[lo:lo + n].view(tab.shape)


def _sync(dst, src):
    """dst becomes src's twin: weights, moments, counters."""
    with torch.no_grad():
        dst._arena.copy_(src._arena)
        dst._adam_m.copy_(src._adam_m)
        dst._adam_v.copy_(src._adam_v)
        dst._adam_state.copy_(src._adam_state)
        dst._rng_state.copy_(src._rng_state)
    dst.neg_step = src.neg_step
    dst.sync_shadow()


def _collected_table_grad(m, feats, labels):
    m.detach_grads()
    loss = m.train_loss(feats, labels)
    loss.backward()
    m.collect_grads()
    return loss.detach(), m.item_embs.lookup_table.grad.clone()


# ---- (4) first-step equivalence and invariants ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_first_step_equals_the_dense_model(dt):
    prob = _small()
    feats, labels = _batch(prob)
    lazy, dense = _model(prob, dt, True), _model(prob, dt, False)
    assert torch.equal(_bits(lazy._arena), _bits(dense._arena)) and lazy._offsets == dense._offsets
    assert not lazy._lazy_grad.any() and lazy._stamp.shape == (lazy.num_items,) and not hasattr(dense, "_stamp")
    table0 = lazy.item_embs.lookup_table.data.clone()
    la, da = lazy.train_step(feats, labels), dense.train_step(feats, labels)
    assert torch.equal(_bits(la.reshape(1)), _bits(da.reshape(1)))
    lo, hi = lazy._lazy_range
    assert hi - lo >= lazy.item_embs.lookup_table.numel() and hi < lazy._arena.numel()
    for name, a, b in (("arena", lazy._arena, dense._arena), ("m", lazy._adam_m, dense._adam_m), ("v", lazy._adam_v, dense._adam_v)):
        assert torch.equal(_bits(a[:lo]), _bits(b[:lo])) and torch.equal(_bits(a[hi:]), _bits(b[hi:])), name
    assert torch.equal(_bits(lazy.output_bias.data), _bits(dense.output_bias.data)) and bool(lazy.output_bias.data.any())
    assert torch.equal(lazy._adam_state, dense._adam_state) and int(lazy._adam_state[0]) == 1
    # the table: at m = v = 0 the dense update of a zero-gradient row is zero, so the whole table is comparable
    for k, (a, b) in enumerate(zip(_table_state(lazy), _table_state(dense))):
        _close(_f64(a), _f64(b), f"{dt} table array {k}")
    assert not torch.equal(_bits(lazy.item_embs.lookup_table.data), _bits(table0))      # (the step moved the table)
    if lazy._shadow is not None:
        assert torch.equal(_bits(lazy._shadow), _bits(lazy._arena.to(torch.bfloat16)))
    # the invariant: the table's view of the gradient arena is all zeros between steps, and .grad is that view
    assert lazy.item_embs.lookup_table.grad is lazy._lazy_grad and not lazy._lazy_grad.any()
    assert bool(dense.item_embs.lookup_table.grad.any()) and lazy._lazy_pending == []


# ---- (5) later steps against the reference -----------------------------------------------------------------------------------------
def _step_lists(prob, feats, labels, seed, step, hi):
    """(seqs_i, labels, candidates) of sampled step `step`, by the CPU reference of the sampler."""
    lab = np.asarray(prob["labels"]).reshape(-1)
    cand, _ = CR.sample_negatives(None, lab, 5, 1, hi, seed, step, 0)
    return np.asarray(prob["feats"]["seqs_i"]), lab, cand


def _pick_seed(prob, hi, I):
    """On the CPU: the first sampler seed whose lists touch some row in step 1 that step 2 leaves alone."""
    for seed in range(64):
        t1 = LA.touched_rows(I, *_step_lists(prob, None, None, seed, 0, hi))
        t2 = LA.touched_rows(I, *_step_lists(prob, None, None, seed, 1, hi))
        if (t1 & ~t2).any():
            return seed
    raise AssertionError("no seed leaves a row of step 1 untouched in step 2")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_later_steps_match_the_reference(dt):
    prob = _small()
    feats, labels = _batch(prob)
    I, hi = prob["cfg"].num_items + 1, prob["cfg"].num_items
    seed = _pick_seed(prob, hi, I)
    lazy, dense = _model(prob, dt, True, seed=seed), _model(prob, dt, False, seed=seed)
    assert lazy._negatives_hi() == hi and lazy.num_items == I
    seen_stale = False
    for step in (1, 2, 3):
        _sync(dense, lazy)
        pre = tuple(a.clone() for a in _table_state(lazy))
        _, g = _collected_table_grad(dense, feats, labels)
        dense.optimizer_step()
        ids, lab, cand = _step_lists(prob, feats, labels, seed, step - 1, hi)
        gpu_cand = ops().sample_negatives(None, labels.reshape(-1).contiguous(), 5, 1, hi, seed, step - 1, 0)
        assert np.array_equal(gpu_cand.cpu().numpy(), cand)
        lazy.train_step(feats, labels)
        assert lazy.neg_step == step and int(lazy._adam_state[0]) == step
        rw, rm, rv, _, t = LA.adam_rows(_f64(pre[0]), _f64(g), _f64(pre[1]), _f64(pre[2]), step, LR, ids, lab, cand, **HP)
        assert not _f64(g)[~t].any(), "the dense gradient is zero outside the touched set"
        post = _table_state(lazy)
        tt = torch.tensor(t).cuda()
        for k, (a, r) in enumerate(zip(post, (rw, rm, rv))):
            _close(_f64(a)[t], r[t], f"{dt} step {step} array {k}")
            assert torch.equal(_bits(a[~tt]), _bits(pre[k][~tt])), (step, k)
        assert not lazy._lazy_grad.any()
        if step == 2:      # a row with history that this step does not name: it moves under the dense Adam and keeps its bits here
            stale = torch.nonzero(~tt & pre[1].ne(0).any(1)).reshape(-1)
            assert stale.numel() >= 1
            r = int(stale[0])
            assert not torch.equal(_bits(_table_state(dense)[0][r]), _bits(pre[0][r])), "the dense twin moved it"
            assert torch.equal(_bits(post[0][r]), _bits(pre[0][r])) and torch.equal(_bits(post[1][r]), _bits(pre[1][r]))
            seen_stale = True
    assert seen_stale


# ---- (6) l2 --------------------------------------------------------------------------------------------------------------------
def test_l2_reaches_touched_rows_only():
    prob = _small()
    feats, labels = _batch(prob)
    I, hi, l2 = prob["cfg"].num_items + 1, prob["cfg"].num_items, 1e-2
    lazy, dense0, dense = _model(prob, "f32", True, l2=l2), _model(prob, "f32", False, l2=0.0), _model(prob, "f32", False, l2=l2)
    pre = tuple(a.clone() for a in _table_state(lazy))
    _, g = _collected_table_grad(dense0, feats, labels)           # the table gradient without its l2 term
    loss_dense, g_l2 = _collected_table_grad(dense, feats, labels)
    assert bool(g_l2[0].any()) and not g[0].any()                 # (the dense l2 gradient reaches every row, row 0 included)
    loss = lazy.train_step(feats, labels)
    assert torch.equal(_bits(loss.reshape(1)), _bits(loss_dense.reshape(1))), "the reported loss carries the item table's l2 term"
    ids, lab, cand = _step_lists(prob, feats, labels, 0, 0, hi)
    rw, rm, rv, _, t = LA.adam_rows(_f64(pre[0]), _f64(g), _f64(pre[1]), _f64(pre[2]), 1, LR, ids, lab, cand, l2=l2, **HP)
    no_l2 = LA.adam_rows(_f64(pre[0]), _f64(g), _f64(pre[1]), _f64(pre[2]), 1, LR, ids, lab, cand, l2=0.0, **HP)
    post = _table_state(lazy)
    tt = torch.tensor(t).cuda()
    for k, (a, r) in enumerate(zip(post, (rw, rm, rv))):
        _close(_f64(a)[t], r[t], f"l2 array {k}")
        assert torch.equal(_bits(a[~tt]), _bits(pre[k][~tt])), k
    # ... and the l2 term is what the tolerance sees: the same state without it is out of bounds in m
    assert np.abs(no_l2[1][t] - rm[t]).max() > 100 * TOL * np.abs(rm[t]).max()
    # the mark and position tables keep the dense l2 gradient
    for name in ("mark_embs.lookup_table", "pcoding.pembs.lookup_table"):
        a, b = dict(lazy.named_parameters())[name].grad, dict(dense.named_parameters())[name].grad
        assert bool(a.any()) and torch.equal(_bits(a), _bits(b)), name


# ---- (7) no dense temporaries ------------------------------------------------------------------------------------------------------
def test_no_dense_temporaries():
    I, C = 200000, 64
    prob = make_problem(seed=9, batch=4, perturb=False, num_items=I, seqslen=8, num_units=C, num_heads=2, num_blocks=1, ct_reg=0.0)
    feats, labels = _batch(prob)
    lazy = _model(prob, "bf16", True, l2=1e-3, det=False)
    lazy.train_step(feats, labels)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    lazy.train_step(feats, labels)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"peak rise over one lazy step: {rise} bytes; one [I, C] f32 tensor: {(I + 1) * C * 4}")
    assert rise < I * C * 4
    assert not lazy._lazy_grad.any()


# ---- (8) reproducibility -------------------------------------------------------------------------------------------------------
def test_reproducible_and_resumable(tmp_path):
    from easydgl_amd import train as TR
    probs = [_small(seed=20 + i) for i in range(4)]
    batches = [_batch(p) for p in probs]

    def run(m, bs):
        for f, l in bs:
            m.train_step(f, l)
        return m
    fresh = lambda: _model(probs[0], "bf16", True, l2=1e-3, seed=3, drop=0.1)  # noqa: E731
    whole, again = run(fresh(), batches), run(fresh(), batches)
    for a, b in ((whole._arena, again._arena), (whole._adam_m, again._adam_m), (whole._adam_v, again._adam_v), (whole._shadow, again._shadow)):
        assert torch.equal(_bits(a), _bits(b))
    first = run(fresh(), batches[:2])
    TR.save_checkpoint(first, str(tmp_path / "m.pt"))
    ck = torch.load(str(tmp_path / "m.pt"), map_location="cpu")
    assert not any("stamp" in k for k in ck)                      # the claim words are not saved
    # resumed in a model that has been four steps further: its claim words start over with the restored step count
    assert int(again._stamp.max()) == 4
    TR.load_checkpoint(again, str(tmp_path / "m.pt"))
    assert again.neg_step == 2 and int(again._adam_state[0]) == 2 and not again._stamp.any()
    run(again, batches[2:])
    assert torch.equal(_bits(whole._arena), _bits(again._arena)) and torch.equal(_bits(whole._adam_m), _bits(again._adam_m))
    assert whole.neg_step == again.neg_step == 4
