"""The grouped weight-gradient tiles as workgroups of the QKVT dX GEMM's launch (edgl_gemm_dw_ride, DESIGN rule 79) against the
sequence they replace: edgl_gemm_dw_defer(0) — the grouped launch — and then edgl_dx_encode_bwd_label.

Op level.  Five queued edgl_gemm_dw products of the engine's shapes, outputs pre-filled with NaN.  Riding changes WHERE the tiles run,
not what a tile computes nor how the slabs are laid out and summed (same split count, same kernel bodies): every dW / db, d_pos /
d_mark and dx0_out must be bit-identical to the unridden sequence.  d_item / d_bias are sums of f32 atomics whose order varies from run
to run in both forms; they keep the bound of tests/test_gpu_dx_encode.py, whose inputs, fp64 reference and unfused errors are shared:
at most 2x the unfused pair's largest error of three runs (relative L2 and max).  Every figure is printed in front of its assertion.
Outputs are read once BEFORE the grouped mode is left: what rode is final there, and leaving the mode adds nothing.

Fall-backs (switch off, empty queue, an accumulating product, a full queue plus one, a reduction list longer than one batch, an
aborted group) must leave the bits of the unridden sequence.

Engine level.  B = 128, T = 17, M = 3, bf16, dropout 0.1 with EDGL_DW_RIDE 0 / 1: same printed losses, the weight gradients of the five
dense layers bit-identical, everything else within the bf16 bounds of tests/_util.py; the same under a captured graph; nothing changes
in deterministic mode."""
import functools

import numpy as np
import pytest
import torch

from tests._util import GRAD_TOL, grad_errors, grad_ok
from tests.test_gpu_dx_encode import JOBS, C, E, I, R, _baseline

pytestmark = pytest.mark.gpu

DW = [(3 * C, 4 * C), (C, C), (2 * C, C), (C, 2 * C), (C, C)]      # (Kf, N) of the block's five weight gradients


@functools.lru_cache(maxsize=None)
def _operands(rows, shapes=tuple(DW)):
    g = torch.Generator(device="cuda").manual_seed(77 + rows)
    n = lambda *s: torch.randn(*s, device="cuda", generator=g).to(torch.bfloat16)      # noqa: E731
    return [(n(rows, kf), n(rows, nn)) for kf, nn in shapes]


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b, keys, what):
    for k in keys:
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k, float((a[k].float() - b[k].float()).abs().nan_to_num(nan=1e30).max()))


def _run(inp, mode, rate=0.0, riders=0, want_dx0=False, shapes=tuple(DW), accumulate=(), split_db=(4,), abort=False):
    """One sequence from fresh outputs.  mode "seq": queue, edgl_gemm_dw_defer(0), fused call; "ride": queue, edgl_gemm_dw_ride(1), fused
    call, edgl_gemm_dw_defer(0); "off": as "ride" without the request.  riders: that many further reductions queued in deferred mode
    (0: the reductions are not deferred at all).  abort: edgl_gemm_dw_defer(-1) between queueing and the call.
    Returns (final, after_call, before_call): dicts of tensors, the last two read in front of edgl_gemm_dw_defer(0) / the call."""
    from easydgl_amd import _lib, ops
    lib, P_ = _lib.lib, ops._ptr
    B, T = inp["B"], inp["T"]
    rows = B * T
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")   # noqa: E731
    d_item, d_bias = torch.zeros((I, C), device="cuda"), torch.zeros(I - 1, device="cuda")
    d_pos, d_mark = nan(T, C), nan(E, C)
    dx0 = torch.full((rows, 3 * C), float("nan"), device="cuda", dtype=torch.bfloat16) if want_dx0 else None
    ws = torch.empty(lib.edgl_encode_bwd_workspace(B, T, C), device="cuda")
    ops_ = _operands(rows, tuple(shapes))
    dws, dbs, wss = [], [], []
    for i, (kf, nn) in enumerate(shapes):      # (dW, db) contiguous as in the gradient arena; split_db: a bias gradient of its own
        both = torch.ones((kf + 1) * nn, device="cuda") if i in accumulate else nan((kf + 1) * nn)
        dws.append(both[:kf * nn])
        dbs.append((torch.ones(nn, device="cuda") if i in accumulate else nan(nn)) if i in split_db else both[kf * nn:])
        wss.append(torch.empty(lib.edgl_gemm_dw_workspace(rows, kf, nn, _lib.BF16), device="cuda"))
    jobs = [JOBS[i % len(JOBS)] for i in range(riders)]
    g = torch.Generator(device="cuda").manual_seed(5)
    parts = [torch.randn(P, ld, device="cuda", generator=g) for P, _, ld in jobs]
    outs = [nan(N) for _, N, _ in jobs]
    st = ops._stream()
    rng = P_(inp["rng"]) if rate > 0 else None
    named = lambda: dict(d_item=d_item.clone(), d_bias=d_bias.clone(), d_pos=d_pos.clone(), d_mark=d_mark.clone(),      # noqa: E731
                         **({"dx0": dx0.clone()} if want_dx0 else {}), **{f"dw{i}": t.clone() for i, t in enumerate(dws)},
                         **{f"db{i}": t.clone() for i, t in enumerate(dbs)}, **{f"job{i}": o.clone() for i, o in enumerate(outs)})

    def fused():
        _lib.check(lib.edgl_dx_encode_bwd_label(P_(inp["dqkvt"]), P_(inp["W"]), 4 * C, 4 * C, P_(dx0), P_(inp["ids"]), P_(inp["marks"]),
                                                P_(inp["add1"]), P_(inp["add2"]), B, T, C, E, I, float(rate), rng, 1, P_(d_item), P_(d_pos),
                                                P_(d_mark), P_(ws), 0, P_(inp["lab_rows"]), P_(inp["labels"]), P_(inp["coef"]),
                                                P_(inp["nvalid"]), R, P_(d_bias), _lib.BF16, st), "edgl_dx_encode_bwd_label")

    try:
        if riders:
            _lib.check(lib.edgl_reduce_defer(1, st), "edgl_reduce_defer")
            for p, (P, N, ld), o in zip(parts, jobs, outs):
                _lib.check(lib.edgl_reduce_partials(P_(p), P, N, ld, P_(o), 0, st), "edgl_reduce_partials")
            _lib.check(lib.edgl_reduce_ride(1), "edgl_reduce_ride")
        _lib.check(lib.edgl_gemm_dw_defer(1, st), "edgl_gemm_dw_defer")
        for i, ((kf, nn), (X, Y)) in enumerate(zip(shapes, ops_)):
            _lib.check(lib.edgl_gemm_dw(P_(X), P_(Y), P_(dws[i]), P_(dbs[i]), rows, kf, nn, kf, nn, int(i in accumulate), P_(wss[i]),
                                        _lib.BF16, st), "edgl_gemm_dw")
        if mode == "ride":
            _lib.check(lib.edgl_gemm_dw_ride(1), "edgl_gemm_dw_ride")
        if abort:
            _lib.check(lib.edgl_gemm_dw_defer(-1, st), "edgl_gemm_dw_defer")
        if mode == "seq":
            _lib.check(lib.edgl_gemm_dw_defer(0, st), "edgl_gemm_dw_defer")
        torch.cuda.synchronize()
        before = named()
        fused()
        torch.cuda.synchronize()
        after = named()
        _lib.check(lib.edgl_gemm_dw_defer(0, st), "edgl_gemm_dw_defer")
        if riders:
            _lib.check(lib.edgl_reduce_flush(st), "edgl_reduce_flush")
            _lib.check(lib.edgl_reduce_defer(0, st), "edgl_reduce_defer")
    except BaseException:
        lib.edgl_gemm_dw_defer(-1, st)
        lib.edgl_reduce_defer(-1, st)
        raise
    torch.cuda.synchronize()
    return named(), after, before


def _dw_keys(n=len(DW)):
    return [f"dw{i}" for i in range(n)] + [f"db{i}" for i in range(n)]


@pytest.mark.parametrize("riders", [0, 3])
@pytest.mark.parametrize("rate", [0.0, 0.1])
@pytest.mark.parametrize("T", [1, 17, 101])      # T = 1: R = 120 ... 250 rows, one split with a partial 64-row step; 17 / 101: ragged last splits
@pytest.mark.parametrize("B", [120, 128, 250])
def test_riding_group_matches_the_grouped_launch(B, T, rate, riders):
    inp, _, ref, worst = _baseline(B, T, rate)
    seq, _, _ = _run(inp, "seq", rate, riders, want_dx0=True)
    ride, after, before = _run(inp, "ride", rate, riders, want_dx0=True)
    # nothing of the queue has run before the call; behind it everything is final, and leaving the two deferred modes changes no bit
    assert all(bool(torch.isnan(before[k]).all()) for k in _dw_keys())
    _same(after, ride, ride.keys(), "ride: behind the call / behind edgl_gemm_dw_defer(0) + edgl_reduce_flush")
    _same(seq, ride, _dw_keys() + ["d_pos", "d_mark", "dx0"] + [f"job{i}" for i in range(riders)], "seq / ride")
    assert all(bool(torch.isfinite(v.float()).all()) for v in ride.values())
    X, Y = _operands(B * T)[0]
    assert torch.allclose(ride["dw0"].reshape(3 * C, 4 * C).double(), X.double().t() @ Y.double(), rtol=1e-4, atol=1e-2 * np.sqrt(B * T))
    assert torch.allclose(ride["db0"].double(), Y.double().sum(0), rtol=1e-4, atol=1e-3 * np.sqrt(B * T))
    errs = {k: grad_errors(ride[k].cpu().numpy(), ref[k].cpu().numpy()) for k in ("d_item", "d_bias")}
    for k, e in errs.items():
        print(f"{k} B={B} T={T} rate={rate} riders={riders}: riding rel-L2 {e[0]:.3e} rel-max {e[1]:.3e} | unridden, unfused (max of 3) "
              f"rel-L2 {worst[k][0]:.3e} rel-max {worst[k][1]:.3e}")
    for k, e in errs.items():
        assert e[0] <= 2.0 * worst[k][0] and e[1] <= 2.0 * worst[k][1], (k, e, worst[k])


# ---- fall-backs: the unridden sequence's bits ------------------------------------------------------------------------------------------
def _small():
    return _baseline(128, 17, 0.0)[0]


EXACT = ["d_pos", "d_mark"]


def test_switch_off_keeps_the_queue_for_the_flush():
    inp = _small()
    seq, _, _ = _run(inp, "seq", riders=3)
    off, after, _ = _run(inp, "off", riders=3)
    assert all(bool(torch.isnan(after[k]).all()) for k in _dw_keys())      # the call launched nothing of the queue
    _same(seq, off, _dw_keys() + EXACT, "seq / switch off")


def test_empty_queue_rides_nothing():
    inp = _small()
    seq, _, _ = _run(inp, "seq", riders=3, shapes=())
    ride, after, _ = _run(inp, "ride", riders=3, shapes=())
    _same(seq, ride, EXACT + ["job0", "job1", "job2"], "seq / ride, empty queue")
    _same(after, ride, ride.keys(), "empty queue: behind the call / at the end")


def test_accumulating_product_is_flushed_in_front_of_the_call():
    inp = _small()
    seq, _, _ = _run(inp, "seq", riders=3, accumulate=(1,))
    ride, _, _ = _run(inp, "ride", riders=3, accumulate=(1,))
    _same(seq, ride, _dw_keys() + EXACT, "seq / ride, accumulating product")
    X, Y = _operands(128 * 17)[1]
    assert torch.allclose(ride["dw1"].reshape(C, C).double(), 1.0 + X.double().t() @ Y.double(), rtol=1e-4, atol=0.5)


def test_full_queue_plus_one():
    inp = _small()
    shapes = tuple([(C, C)] * 8 + [(2 * C, C)])      # the ninth call flushes the eight, then rides alone
    seq, _, _ = _run(inp, "seq", riders=3, shapes=shapes, split_db=())
    ride, after, before = _run(inp, "ride", riders=3, shapes=shapes, split_db=())
    assert bool(torch.isnan(before["dw8"]).all())
    _same(seq, ride, _dw_keys(9) + EXACT, "seq / ride, nine products")
    _same(after, ride, ride.keys(), "nine products: behind the call / at the end")
    assert all(bool(torch.isfinite(ride[k]).all()) for k in _dw_keys(9))


def test_reduction_list_longer_than_one_batch():
    inp = _small()
    seq, _, _ = _run(inp, "seq", riders=24)      # a full list in front of the products' own reductions
    ride, _, _ = _run(inp, "ride", riders=24)
    _same(seq, ride, _dw_keys() + EXACT + [f"job{i}" for i in range(24)], "seq / ride, 24 queued reductions")
    assert all(bool(torch.isfinite(v).all()) for v in ride.values())


def test_aborted_group_launches_nothing_and_clears_the_switch():
    inp = _small()
    final, after, _ = _run(inp, "ride", riders=3, abort=True)
    assert all(bool(torch.isnan(after[k]).all()) and bool(torch.isnan(final[k]).all()) for k in _dw_keys())
    assert bool(torch.isfinite(final["d_pos"]).all())
    # the request went with the group: the next group (no request of its own) waits for its flush
    off, after, _ = _run(inp, "off", riders=3)
    assert all(bool(torch.isnan(after[k]).all()) for k in _dw_keys())
    seq, _, _ = _run(inp, "seq", riders=3)
    _same(seq, off, _dw_keys() + EXACT, "seq / after an abort")


# ---- engine level ----------------------------------------------------------------------------------------------------------------------
class _Count:      # engine.lib with a count of the riding requests
    def __init__(self, inner):
        self.inner, self.n = inner, 0

    def __getattr__(self, name):
        fn = getattr(self.inner, name)
        if name != "edgl_gemm_dw_ride":
            return fn

        def call(*a):
            self.n += 1
            return fn(*a)
        return call


def _dense_grads(m):
    blk = m.layers[0]
    ps = [blk.attention.dense_kernel, blk.attention.dense_bias, blk.att_out.kernel, blk.att_out.bias, blk.inter.kernel, blk.inter.bias,
          blk.out.kernel, blk.out.bias, m.transform.kernel, m.transform.bias]
    return [p.grad.clone() for p in ps]


def _engine_run(prob, flag, bare, monkeypatch, use_graph=False, deterministic=None):
    import easydgl_amd.engine as engine_mod
    from easydgl_amd.engine import TrainEngine
    from tests._util import build_model, to_dev
    monkeypatch.setenv("EDGL_DW_RIDE", flag)
    m = build_model(prob, "bf16", hidden_drop=0.1, att_drop=0.1)
    e = TrainEngine(m, 128, use_graph=use_graph, deterministic=deterministic)
    e.load_batch(to_dev(prob["feats"]), torch.as_tensor(prob["labels"]).cuda())
    spy = _Count(engine_mod.lib)
    monkeypatch.setattr(engine_mod, "lib", spy)
    try:
        if bare:
            e._issue()
            torch.cuda.synchronize()
            out = [float(e.loss)], {"arena": m._grad_arena.clone()}, _dense_grads(m)
        else:
            losses = [float(e.step()) for _ in range(3)]
            torch.cuda.synchronize()
            out = losses, {"params": m._arena.clone()}, []
    finally:
        monkeypatch.setattr(engine_mod, "lib", spy.inner)
    return out, spy.n


@functools.lru_cache(maxsize=None)
def _prob():
    from tests._util import make_problem
    return make_problem(seed=95, batch=128, num_units=128, num_heads=8, num_blocks=1, seqslen=16, masklen=3, num_events=16, num_items=399)


def _compare(r0, r1, what):
    (l0, t0, w0), (l1, t1, w1) = r0, r1
    for a, b in zip(l0, l1):
        print(f"{what}: loss {a:.6f} (EDGL_DW_RIDE=0) {b:.6f} (1)")
        assert np.isfinite(a) and f"{a:.6f}" == f"{b:.6f}", (l0, l1)
    for i, (a, b) in enumerate(zip(w0, w1)):
        assert torch.equal(a, b) and float(a.abs().max()) > 0.0, (what, "dense layer gradient", i)
    for k in t0:
        ok, e = grad_ok(t1[k].float().cpu().numpy(), t0[k].float().cpu().numpy(), "bf16")
        print(f"{what} {k}: rel-L2 {e[0]:.3e} rel-max {e[1]:.3e} (bounds {GRAD_TOL['bf16']})")
        assert ok and bool(torch.isfinite(t1[k]).all()), (k, e)


@pytest.mark.parametrize("bare", [False, True])
def test_engine_agrees_with_the_grouped_launch(bare, monkeypatch):
    r0, n0 = _engine_run(_prob(), "0", bare, monkeypatch)
    r1, n1 = _engine_run(_prob(), "1", bare, monkeypatch)
    assert n0 == 0 and n1 == (1 if bare else 3), (n0, n1)
    _compare(r0, r1, f"bare={bare}")


def test_engine_agrees_under_a_captured_graph(monkeypatch):
    r0, _ = _engine_run(_prob(), "0", False, monkeypatch, use_graph=True)
    r1, _ = _engine_run(_prob(), "1", False, monkeypatch, use_graph=True)
    _compare(r0, r1, "graph")


def test_switch_changes_nothing_in_deterministic_mode(monkeypatch):
    (l0, t0, _), n0 = _engine_run(_prob(), "0", False, monkeypatch, deterministic=True)
    (l1, t1, _), n1 = _engine_run(_prob(), "1", False, monkeypatch, deterministic=True)
    assert n0 == 0 and n1 == 0
    assert l0 == l1 and torch.equal(t0["params"], t1["params"])
