"""The QKVT dX GEMM of the first block with the embedding backward in its epilogue (edgl_dx_encode_bwd_label) against the unfused
pair it replaces (edgl_gemm's dX call, then edgl_encode_bwd_add_label).

Op level.  dX0 written on request must be the unfused GEMM's, bit for bit.  d_item, d_bias, d_pos, d_mark are compared with an
fp64 sum formed in torch from that dX0 (same bf16 operands of the segmented sum, same dropout decisions); only the grouping of the
f32 additions differs between the two forms, so the fused error (relative L2 and max) may be at most 2x the largest error the unfused
pair shows against the same reference over three runs.  Every figure is printed in front of its assertion.
Measured (profiles/dx_encode.txt, section 5): largest fused / unfused ratio over the 36 cases 1.10 (rel-L2) and 1.54 (rel-max), both
d_item; d_pos and d_mark are summed in f64 inside the tile and in the call's two reductions and stay below the unfused errors.
d_item's f32 atomics land in another order from run to run in BOTH forms (rel-max 0.3 ... 0.9e-6): in one earlier run one case of the
36 (B = 250, T = 101, no dropout) showed 8.8e-7 against an unfused maximum of 3.2e-7.

Engine level.  B = 128, T = 17, M = 3, bf16, dropout 0.1: three step()s and a bare _issue() with EDGL_DX_ENCODE 0 and 1 agree within
the bf16 bounds of tests/_util.py; at B = 4 the query says 0 and the old entry points are called."""
import functools

import numpy as np
import pytest
import torch

from tests._util import GRAD_TOL, LOSS_TOL, grad_errors, grad_ok

pytestmark = pytest.mark.gpu

C, E, I, R, NVALID = 128, 16, 300, 15, 9
HOT, HOT_N = 7, 45
JOBS = [(1, 4, 4), (28, 3 * 128, 3 * 128), (70, 128, 128)]      # (P, N, ld) of the riding reductions: column form, row-lane form


def _inputs(B, T, seed):
    g = np.random.default_rng(seed)
    rows = B * T
    ids = np.minimum(g.zipf(1.3, (B, T)), I - 1).astype(np.int64)
    ids[g.random((B, T)) < 0.05] = 0
    ids[:HOT_N, 0] = HOT                    # one id >= 40 times inside one 128-sample tile (chunk 0, position 0)
    ids[B - 1, :] = 0                       # one sample that is all padding
    if T > 1:
        ids[:, T - 1] = 0                   # one position where every sample is padding
    # (checked on the CPU: the cases the kernel's leader scan, row map and masks have to get right are really in the data)
    assert int((ids[:128, 0] == HOT).sum()) >= 40 and not ids[B - 1].any() and (T == 1 or not ids[:, T - 1].any())
    assert ids.any() and ids.max() < I
    n = lambda shape, s=1.0: torch.from_numpy((s * g.standard_normal(shape)).astype(np.float32))      # noqa: E731
    labels = g.integers(0, 12, R).astype(np.int64)
    coef = g.random(R).astype(np.float32)
    coef[3] = 0.0
    marks = (g.random((rows, E)) < 0.3).astype(np.uint8)
    dev = lambda t: t.cuda().contiguous()                  # noqa: E731
    bf = lambda t: dev(t.to(torch.bfloat16))               # noqa: E731
    return dict(B=B, T=T, ids=dev(torch.from_numpy(ids.reshape(rows))), dqkvt=bf(n((rows, 4 * C))), W=bf(n((3 * C, 4 * C), 1.0 / np.sqrt(4 * C))),
                add1=bf(n((rows, C))), add2=bf(n((rows, C))), marks=dev(torch.from_numpy(marks)), lab_rows=bf(n((R, C))),
                labels=dev(torch.from_numpy(labels)), coef=dev(torch.from_numpy(coef)),
                nvalid=torch.tensor([NVALID], dtype=torch.int32, device="cuda"),
                rng=torch.tensor([1234567, 3], dtype=torch.int64, device="cuda"),
                parts=[dev(n((P, ld))) for P, _, ld in JOBS])


def _run(inp, fused, rate, riders):
    """One call sequence from zeroed gradients; returns dict(dx0, d_item, d_bias, d_pos, d_mark, job*)."""
    from easydgl_amd import _lib, ops
    lib, P_ = _lib.lib, ops._ptr
    B, T = inp["B"], inp["T"]
    rows = B * T
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")   # noqa: E731
    d_item, d_bias = torch.zeros((I, C), device="cuda"), torch.zeros(I - 1, device="cuda")
    d_pos, d_mark = nan(T, C), nan(E, C)
    dx0 = torch.full((rows, 3 * C), float("nan"), device="cuda", dtype=torch.bfloat16)
    ws = torch.empty(lib.edgl_encode_bwd_workspace(B, T, C), device="cuda")
    outs = [nan(N) for _, N, _ in JOBS] if riders else []
    st = ops._stream()
    rng = P_(inp["rng"]) if rate > 0 else None
    enc = (P_(inp["ids"]), P_(inp["marks"]))
    tail = (P_(inp["add1"]), P_(inp["add2"]), B, T, C, E, I, float(rate), rng, 1, P_(d_item), P_(d_pos), P_(d_mark), P_(ws), 0,
            P_(inp["lab_rows"]), P_(inp["labels"]), P_(inp["coef"]), P_(inp["nvalid"]), R, P_(d_bias), _lib.BF16, st)
    try:
        if riders:
            _lib.check(lib.edgl_reduce_defer(1, st), "edgl_reduce_defer")
            for p, (P, N, ld), o in zip(inp["parts"], JOBS, outs):
                _lib.check(lib.edgl_reduce_partials(P_(p), P, N, ld, P_(o), 0, st), "edgl_reduce_partials")
            _lib.check(lib.edgl_reduce_ride(1), "edgl_reduce_ride")
        if fused:
            _lib.check(lib.edgl_dx_encode_bwd_label(P_(inp["dqkvt"]), P_(inp["W"]), 4 * C, 4 * C, P_(dx0), *enc, *tail), "edgl_dx_encode_bwd_label")
        else:
            _lib.check(lib.edgl_gemm(P_(inp["dqkvt"]), P_(inp["W"]), P_(dx0), rows, 3 * C, 4 * C, 4 * C, 4 * C, 3 * C, 1, 1, None, None, 0, 1,
                                     None, _lib.BF16, st), "edgl_gemm")
            _lib.check(lib.edgl_encode_bwd_add_label(*enc, P_(dx0), *tail), "edgl_encode_bwd_add_label")
        if riders:
            _lib.check(lib.edgl_reduce_defer(0, st), "edgl_reduce_defer")
    except BaseException:
        lib.edgl_reduce_defer(-1, st)
        raise
    torch.cuda.synchronize()
    return dict(dx0=dx0, d_item=d_item, d_bias=d_bias, d_pos=d_pos, d_mark=d_mark, **{f"job{i}": o for i, o in enumerate(outs)})


def _reference(inp, dx0, rate):
    """fp64 sums from the unfused GEMM's bf16 dX0: the operands of the segmented sum rounded to bf16 as both forms round them."""
    from easydgl_amd import _lib, ops
    B, T = inp["B"], inp["T"]
    rows = B * T
    keep = torch.ones((rows, 3 * C), device="cuda")
    if rate > 0:      # the kernels' own dropout decisions (element index row * 3C + channel), scale included
        _lib.check(_lib.lib.edgl_dropout(ops._ptr(keep.clone()), ops._ptr(keep), keep.numel(), float(rate), ops._ptr(inp["rng"]), 1,
                                         _lib.F32, ops._stream()), "edgl_dropout")
    keep = keep.double()
    x = (dx0[:, :C].float() + inp["add1"].float() + inp["add2"].float()).to(torch.bfloat16).double() * keep[:, :C]
    x = x * float(np.sqrt(np.float32(C)))
    ids = inp["ids"]
    d_item = torch.zeros((I, C), device="cuda", dtype=torch.float64).index_add_(0, ids[ids != 0], x[ids != 0])
    live = (torch.arange(R, device="cuda") < NVALID) & (inp["labels"] != 0) & (inp["coef"] != 0)
    lr = (inp["coef"][:, None] * inp["lab_rows"].float()).to(torch.bfloat16).double()
    lab = inp["labels"][live]
    d_item.index_add_(0, lab, -lr[live])
    d_bias = torch.zeros(I - 1, device="cuda", dtype=torch.float64).index_add_(0, lab - 1, -inp["coef"][live].double())
    d_pos = (dx0[:, C:2 * C].double() * keep[:, C:2 * C]).reshape(B, T, C).sum(0)
    nm = inp["marks"].double().sum(1, keepdim=True)
    d_mark = torch.zeros((E, C), device="cuda", dtype=torch.float64)
    d_mark[1] = (nm * dx0[:, 2 * C:].double() * keep[:, 2 * C:]).sum(0)
    return dict(d_item=d_item, d_bias=d_bias, d_pos=d_pos, d_mark=d_mark)


@functools.lru_cache(maxsize=None)
def _baseline(B, T, rate):
    """Inputs, the unfused dX0, the fp64 reference and the largest (rel-L2, rel-max) error of the unfused pair over three runs."""
    inp = _inputs(B, T, seed=1000 * B + T)
    runs = [_run(inp, False, rate, False) for _ in range(3)]
    ref = _reference(inp, runs[0]["dx0"], rate)
    worst = {}
    for k in ref:
        errs = [grad_errors(r[k].cpu().numpy(), ref[k].cpu().numpy()) for r in runs]
        worst[k] = (max(e[0] for e in errs), max(e[1] for e in errs))
    return inp, runs[0], ref, worst


@pytest.mark.parametrize("riders", [False, True])
@pytest.mark.parametrize("rate", [0.0, 0.1])
@pytest.mark.parametrize("T", [1, 17, 101])
@pytest.mark.parametrize("B", [120, 128, 250])
def test_fused_entry_matches_the_unfused_pair(B, T, rate, riders):
    from easydgl_amd import _lib
    assert _lib.lib.edgl_dx_encode_supported(B, T, C, _lib.BF16) == 1
    inp, unfused, ref, worst = _baseline(B, T, rate)
    got = _run(inp, True, rate, riders)
    assert torch.equal(got["dx0"].view(torch.int16), unfused["dx0"].view(torch.int16)), "dx0_out differs from edgl_gemm's dX0"
    for k in ref:
        e = grad_errors(got[k].cpu().numpy(), ref[k].cpu().numpy())
        print(f"{k} B={B} T={T} rate={rate} riders={riders}: fused rel-L2 {e[0]:.3e} rel-max {e[1]:.3e} | unfused (max of 3) "
              f"rel-L2 {worst[k][0]:.3e} rel-max {worst[k][1]:.3e}")
    for k in ref:
        e = grad_errors(got[k].cpu().numpy(), ref[k].cpu().numpy())
        assert bool(torch.isfinite(got[k]).all()), k
        assert e[0] <= 2.0 * worst[k][0] and e[1] <= 2.0 * worst[k][1], (k, e, worst[k])
    if riders:      # the riding list: the same kernel body in the same order as the stand-alone reduction launch
        want = _run(inp, False, rate, True)
        for i, (p, (P, N, ld)) in enumerate(zip(inp["parts"], JOBS)):
            assert torch.equal(got[f"job{i}"], want[f"job{i}"]), i
            assert torch.allclose(got[f"job{i}"].double(), p[:, :N].double().sum(0), rtol=1e-5, atol=1e-5), i


def test_query_names_the_shapes_the_fused_form_takes():
    from easydgl_amd import _lib
    q = _lib.lib.edgl_dx_encode_supported
    assert [q(B, 101, 128, _lib.BF16) for B in (120, 128, 250, 512, 4, 129)] == [1, 1, 1, 1, 0, 0]
    assert q(128, 101, 128, _lib.F32) == 0 and q(128, 101, 256, _lib.BF16) == 0 and q(128, 101, 64, _lib.BF16) == 0


# ---- engine level -------------------------------------------------------------------------------------------------------------------
class _Count:      # engine.lib with a count of the calls of the two forms
    def __init__(self, inner):
        self.inner, self.n = inner, {"edgl_dx_encode_bwd_label": 0, "edgl_encode_bwd_add_label": 0}

    def __getattr__(self, name):
        fn = getattr(self.inner, name)
        if name not in self.n:
            return fn

        def call(*a):
            self.n[name] += 1
            return fn(*a)
        return call


def _engine_run(prob, batch, flag, bare, monkeypatch):
    import easydgl_amd.engine as engine_mod
    from easydgl_amd.engine import TrainEngine
    from tests._util import build_model, to_dev
    monkeypatch.setenv("EDGL_DX_ENCODE", flag)
    m = build_model(prob, "bf16", hidden_drop=0.1, att_drop=0.1)
    e = TrainEngine(m, batch, use_graph=False)
    e.load_batch(to_dev(prob["feats"]), torch.as_tensor(prob["labels"]).cuda())
    spy = _Count(engine_mod.lib)
    monkeypatch.setattr(engine_mod, "lib", spy)
    try:
        if bare:
            e._issue()
            torch.cuda.synchronize()
            grads = {"arena": m._grad_arena.clone(), "item": m.item_embs.lookup_table.grad.clone(),
                     "pos": m.pcoding.pembs.lookup_table.grad.clone(), "mark": m.mark_embs.lookup_table.grad.clone(),
                     "bias": m.output_bias.grad.clone()}
            out = [float(e.loss)], grads
        else:
            losses = [float(e.step()) for _ in range(3)]
            torch.cuda.synchronize()
            out = losses, {"params": m._arena.clone()}
    finally:
        monkeypatch.setattr(engine_mod, "lib", spy.inner)
    return out, spy.n


def test_engine_agrees_with_the_unfused_backward_end(monkeypatch):
    from tests._util import make_problem
    prob = make_problem(seed=93, batch=128, num_units=128, num_heads=8, num_blocks=1, seqslen=16, masklen=3, num_events=16, num_items=399)
    for bare in (False, True):
        (l0, t0), n0 = _engine_run(prob, 128, "0", bare, monkeypatch)
        (l1, t1), n1 = _engine_run(prob, 128, "1", bare, monkeypatch)
        calls = 1 if bare else 3
        assert n0 == {"edgl_dx_encode_bwd_label": 0, "edgl_encode_bwd_add_label": calls}, n0
        assert n1 == {"edgl_dx_encode_bwd_label": calls, "edgl_encode_bwd_add_label": 0}, n1
        for a, b in zip(l0, l1):
            print(f"bare={bare}: loss {a:.6f} (unfused) {b:.6f} (fused)")
            assert np.isfinite(a) and abs(a - b) <= LOSS_TOL["bf16"] * abs(a), (l0, l1)
        for k in t0:
            ok, e = grad_ok(t1[k].float().cpu().numpy(), t0[k].float().cpu().numpy(), "bf16")
            print(f"bare={bare} {k}: rel-L2 {e[0]:.3e} rel-max {e[1]:.3e} (bounds {GRAD_TOL['bf16']})")
            assert ok and bool(torch.isfinite(t1[k]).all()) and float(t1[k].abs().max()) > 0.0, (k, e)


def test_engine_keeps_the_old_entry_points_at_a_small_batch(monkeypatch):
    from easydgl_amd import _lib
    from tests._util import make_problem
    assert _lib.lib.edgl_dx_encode_supported(4, 17, 128, _lib.BF16) == 0
    prob = make_problem(seed=94, batch=4, num_units=128, num_heads=8, num_blocks=1, seqslen=16, masklen=3, num_events=16, num_items=399)
    (_, _), n = _engine_run(prob, 4, "1", True, monkeypatch)
    assert n == {"edgl_dx_encode_bwd_label": 0, "edgl_encode_bwd_add_label": 1}, n
