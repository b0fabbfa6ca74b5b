"""The key-streamed BiMAU kernels (csrc/k_bimau_stream.hip): parity with the fp64 restatement beyond the bounds of the in-register
kernels, agreement of the two kernel families where both run (EDGL_MAU_STREAM), identical dropout masks, flags, mark groups and edge
cases.  Procedure and case generator of tests/test_gpu_ops.py::test_bimau_fwd_bwd.

bf16 bounds beyond T = 208: the project's bounds at its longest in-register T (201) times sqrt(T / 201) — the growth of independently
rounded terms in a T-term sum — while the f32 twin of the case passes the unscaled f32 bounds."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import easydgl_oracle as O
from oracle import torch_ref as R
from tests._util import assert_close, dump_errors, grad_errors, rel_err

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
GRADS = ("dx", "dWqkvt", "dbqkvt", "dW1", "db1", "dw", "dscaling")
ST = "sequential_temporal_combined/"


def ops():
    from easydgl_amd import ops as _ops
    return _ops


def _rand(shape, rng, scale=1.0):
    return rng.standard_normal(shape) * scale


@functools.lru_cache(maxsize=None)
def _bimau_case(B, T, C, H, E, seed, cin_mult=3):
    """tests/test_gpu_ops.py::_bimau_case: every sample left-padded, sample 2 fully padded when B > 2"""
    cfg = O.Config(num_items=30, seqslen=T - 1, num_units=C, num_heads=H, num_events=E, time_scale=1.0)
    rng = np.random.default_rng(seed)
    dh = C // H
    cin = cin_mult * C
    x = _rand((B, T, cin), rng)
    ids = rng.integers(1, cfg.num_items, size=(B, T))
    for b in range(B):
        ids[b, :rng.integers(0, T // 2 + 1)] = 0
    if B > 2:
        ids[2, :] = 0
    mt = O.synthetic_mark_table(cfg.num_items, E, multi_hot=True)
    marks = mt[ids]
    spans = rng.uniform(0, 5, size=(B, T))
    W = dict(Wq=_rand((cin, 4 * C), rng, 0.15 * min(1.0, math.sqrt(768.0 / cin))), bq=_rand((4 * C,), rng, 0.1), W1=O.glorot_uniform(rng, (dh + 1, dh * E)),
             b1=_rand((dh * E,), rng, 0.1), w=O.glorot_uniform(rng, (E, dh)), sc=_rand((E,), rng, 0.2))
    return cfg, x, ids, marks, spans, W


def _cotangents(B, T, C, H, E):
    rng = np.random.default_rng(9)
    return _rand((B, T, C), rng), _rand((H * B, T, E), rng, 0.3)


def _run_unit(shape, name, flags=0, drop=None, backward=True):
    """projection + attention unit + backward on the GPU; returns the outputs and the seven gradients as float64 numpy arrays"""
    o = ops()
    B, T, C, H, E = shape
    dt = DT[name]
    cfg, x, ids, marks, spans, W = _bimau_case(B, T, C, H, E, T + C)
    xt = torch.tensor(x, dtype=dt).cuda().requires_grad_(backward)
    Wq = torch.tensor(W["Wq"], dtype=torch.float32).cuda().requires_grad_(backward)
    Wq_c = Wq.detach().to(dt)
    bq = torch.tensor(W["bq"], dtype=torch.float32).cuda().requires_grad_(backward)
    W1, b1, w, sc = (torch.tensor(W[k], dtype=torch.float32).cuda().requires_grad_(backward) for k in ("W1", "b1", "w", "sc"))
    args = (torch.tensor(ids).cuda(), torch.tensor(spans, dtype=torch.float32).cuda(), torch.tensor(marks.astype(np.uint8)).cuda(), H,
            drop if drop is not None else o.NO_DROP, flags)
    if not backward:
        with torch.no_grad():
            qkvt = o.LinearFn.apply(xt, Wq, bq, Wq_c, False)
            out, lam = o.BiMAUFn.apply(qkvt, xt[:, :, :C], W1, b1, w, sc, *args)
        return dict(out=out.float().cpu().numpy().astype(np.float64), lam=lam.cpu().numpy().astype(np.float64))
    qkvt = o.LinearFn.apply(xt, Wq, bq, Wq_c, False)
    out, lam = o.BiMAUFn.apply(qkvt, xt[:, :, :C], W1, b1, w, sc, *args)
    g1, g2 = _cotangents(B, T, C, H, E)
    G1 = torch.tensor(g1, dtype=dt).cuda()
    G2 = torch.tensor(g2, dtype=torch.float32).cuda()
    ((out.float() * G1.float()).sum() + (lam * G2).sum()).backward()
    res = dict(out=out.float().detach(), lam=lam.detach(), dx=xt.grad.float(), dWqkvt=Wq.grad, dbqkvt=bq.grad, dW1=W1.grad, db1=b1.grad,
               dw=w.grad, dscaling=sc.grad)
    return {k: v.cpu().numpy().astype(np.float64) for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def _reference(shape, name, causal=False, set_diag=True):
    """oracle/torch_ref.py::bimau in fp64 on the CPU, fed the rounded inputs the kernel saw (x, the projection kernel and the
    cotangent of `out` in the activation dtype)"""
    B, T, C, H, E = shape
    dt = DT[name]
    cfg, x, ids, marks, spans, W = _bimau_case(B, T, C, H, E, T + C)
    xr = torch.tensor(x, dtype=dt).double().requires_grad_()
    t64 = lambda a: torch.tensor(a, dtype=torch.float32).double().requires_grad_()   # noqa: E731
    pr = {"dense/kernel": torch.tensor(W["Wq"], dtype=torch.float32).to(dt).double().requires_grad_(), "dense/bias": t64(W["bq"]),
          ST + "dense/kernel": t64(W["W1"]), ST + "dense/bias": t64(W["b1"]), ST + "weight": t64(W["w"]), ST + "scaling": t64(W["sc"])}
    km3 = torch.tensor((ids != 0).astype(np.float64)).unsqueeze(1).repeat(H, T, 1)
    out_r, lam_r = R.bimau(C, H, xr, km3, torch.tensor(spans), torch.tensor(marks, dtype=torch.float64), pr, "", 0.0, False,
                           causal=causal, set_diag=set_diag)
    g1, g2 = _cotangents(B, T, C, H, E)
    ((out_r * torch.tensor(g1, dtype=dt).double()).sum() + (lam_r * torch.tensor(g2, dtype=torch.float32).double()).sum()).backward()
    res = dict(out=out_r.detach(), lam=lam_r.detach(), dx=xr.grad, dWqkvt=pr["dense/kernel"].grad, dbqkvt=pr["dense/bias"].grad,
               dW1=pr[ST + "dense/kernel"].grad, db1=pr[ST + "dense/bias"].grad, dw=pr[ST + "weight"].grad, dscaling=pr[ST + "scaling"].grad)
    return {k: v.numpy() for k, v in res.items()}


def _bounds(name, T, dh):
    """(forward, gradient) bounds of tests/test_gpu_ops.py::test_bimau_fwd_bwd at its longest T"""
    if name == "f32":
        return (6e-5 if dh >= 64 else 3e-5), 2e-4
    grow = math.sqrt(T / 201.0) if T > 208 else 1.0
    return 5e-2 * grow, 6e-2 * grow


# ---- 1. parity beyond the old bounds -----------------------------------------------------------------------------------------
LONG_CASES = [(2, 209, 32, 2, 4),     # one key in the last tile
              (3, 257, 32, 2, 16),    # includes the all-padded sample
              (1, 256, 32, 2, 2), (1, 513, 16, 1, 3), (2, 224, 64, 2, 7),
              (1, 150, 64, 2, 3),     # f32 at head dim 32 past T = 128
              (2, 129, 128, 2, 5), (1, 113, 64, 1, 16),
              (2, 201, 512, 8, 16),   # the published recipe's width at seqslen 200
              (1, 129, 128, 1, 5),
              (2, 65, 256, 2, 3)]     # f32 at head dim 128 past T = 64


@pytest.mark.parametrize("name", ["f32", "bf16"])
@pytest.mark.parametrize("shape", LONG_CASES)
def test_parity_beyond_the_in_register_bounds(name, shape):
    B, T, C, H, E = shape
    o = ops()
    if o.lib.edgl_bimau_form(T, C, H, o._lib.F32 if name == "f32" else o._lib.BF16, 0) != 1:
        flags = o.MAU_STREAM    # a shape only one of the dtypes has outgrown: the other is forced onto the same kernels
    else:
        flags = 0
    got, ref = _run_unit(shape, name, flags), _reference(shape, name)
    ftol, gtol = _bounds(name, T, C // H)
    errs = {f"{name} {shape} {k}": grad_errors(got[k], ref[k]) for k in ("out", "lam") + GRADS}
    for k, v in errs.items():
        print(f"{k}: rel-l2 {v[0]:.3e} rel-max {v[1]:.3e}")
    dump_errors("bimau_stream", errs)
    for k in ("lam", "out"):
        assert_close(got[k], ref[k], ftol, k)
    for k in GRADS:
        assert_close(got[k], ref[k], gtol, k)


# ---- 2. the two forms agree where both run -----------------------------------------------------------------------------------
BOTH_CASES = [(2, 101, 128, 8, 16), (2, 31, 64, 2, 7), (2, 201, 256, 8, 16), (1, 128, 128, 1, 5), (2, 31, 512, 8, 16)]


def _both_run(shape, name):
    B, T, C, H, E = shape
    if name == "f32" and ((C // H == 32 and T > 128) or (C // H == 64 and T > 112) or (C // H == 128 and T > 64)):
        return False
    return True


@pytest.mark.parametrize("name", ["f32", "bf16"])
@pytest.mark.parametrize("shape", BOTH_CASES)
def test_streamed_and_in_register_forms_agree(name, shape):
    o = ops()
    B, T, C, H, E = shape
    code = o._lib.F32 if name == "f32" else o._lib.BF16
    if not _both_run(shape, name):
        assert o.lib.edgl_bimau_form(T, C, H, code, 0) == 1     # f32 has one form here: nothing to compare (the bf16 twin compares)
        return
    assert o.lib.edgl_bimau_form(T, C, H, code, 0) == 0 and o.lib.edgl_bimau_form(T, C, H, code, o.MAU_STREAM) == 1
    reg, stm = _run_unit(shape, name, 0), _run_unit(shape, name, o.MAU_STREAM)
    if name == "f32":   # each form is within the project's bound of fp64: twice one bound
        for k in ("lam", "out"):
            assert_close(stm[k], reg[k], 6e-5, k)
        for k in GRADS:
            assert_close(stm[k], reg[k], 4e-4, k)
    else:               # two independent roundings of equal size against fp64
        ref = _reference(shape, name)
        for k in ("lam", "out") + GRADS:
            e_reg, e_stm = rel_err(reg[k], ref[k]), rel_err(stm[k], ref[k])
            print(f"{shape} {k}: in-register {e_reg:.3e} streamed {e_stm:.3e}")
            assert e_stm <= 1.5 * e_reg + 1e-3, f"{k}: streamed {e_stm:.3e} vs in-register {e_reg:.3e}"


# ---- 3. same dropout masks in both forms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 101, 128, 8, 16), (2, 64, 128, 2, 5)])
def test_dropout_masks_are_the_same_in_both_forms(shape):
    o = ops()
    st = torch.tensor([1234, 7], dtype=torch.int64).cuda()
    drop = o.Drop(0.25, st, 3)
    reg, stm = _run_unit(shape, "f32", 0, drop), _run_unit(shape, "f32", o.MAU_STREAM, drop)
    plain = _run_unit(shape, "f32", o.MAU_STREAM, None, backward=False)
    assert rel_err(stm["out"], plain["out"]) > 1e-2          # the dropout is on
    for k in ("lam", "out"):
        assert_close(stm[k], reg[k], 6e-5, k)
    for k in GRADS:
        assert_close(stm[k], reg[k], 4e-4, k)


def test_dropout_beyond_the_in_register_bounds():
    """(rng state, stream) decides the mask; forward and backward take the same decisions.  The output is linear in V under a fixed
    mask, out - resid = A.V, so <out - resid, G> = <V, dV> holds iff the backward used the forward's mask; with the cotangent on a
    single query row q0, dV[k] = A[q0, k] G[q0] is exactly zero where (q0, k) was dropped."""
    o = ops()
    B, T, C, H, E = 2, 209, 32, 2, 4
    dh = C // H
    cfg, x, ids, marks, spans, W = _bimau_case(B, T, C, H, E, T + C)
    ids = np.maximum(ids, 1)                                  # no padding: every probability is positive
    rng = np.random.default_rng(5)
    qkvt0 = _rand((B, T, 4 * C), rng, 0.3)
    qkvt0[:, :, 2 * C:3 * C] = 1.0 + 0.1 * qkvt0[:, :, 2 * C:3 * C]     # V close to 1
    mk = np.ones((B, T, E), dtype=np.uint8)                   # G > 0 everywhere (lambda > 0)
    W1, b1, w, sc = (torch.tensor(W[k], dtype=torch.float32).cuda() for k in ("W1", "b1", "w", "sc"))
    ids_t, sp_t, mk_t = torch.tensor(ids).cuda(), torch.tensor(spans, dtype=torch.float32).cuda(), torch.tensor(mk).cuda()
    resid = torch.zeros((B, T, C)).cuda()
    st = torch.tensor([99, 3], dtype=torch.int64).cuda()
    drop = o.Drop(0.25, st, 5)

    def fwd(q):
        return o.BiMAUFn.apply(q, resid, W1, b1, w, sc, ids_t, sp_t, mk_t, H, drop, 0)
    q = torch.tensor(qkvt0, dtype=torch.float32).cuda().requires_grad_()
    out1, lam1 = fwd(q)
    out2, _ = fwd(q)
    assert torch.equal(out1, out2)                            # same (seed, step, stream) -> same mask
    G = torch.randn_like(out1)
    (dq,) = torch.autograd.grad((out1 * G).sum(), q, retain_graph=True)
    V, dV = q.detach()[:, :, 2 * C:3 * C].double(), dq[:, :, 2 * C:3 * C].double()
    lhs, rhs = float((out1.detach().double() * G.double()).sum()), float((V * dV).sum())
    assert abs(lhs - rhs) <= 1e-4 * max(abs(lhs), 1.0), (lhs, rhs)
    zeros = total = 0
    for q0 in (0, 15, 16, 100, 111, 192, 207, 208):           # first / last rows of tiles, the one-row last tile
        G0 = torch.zeros_like(out1)
        G0[:, q0, :] = 1.0
        (d0,) = torch.autograd.grad((out1 * G0).sum(), q, retain_graph=True)
        dv = d0[:, :, 2 * C:3 * C].reshape(B, T, H, dh)
        dropped = (dv == 0).all(dim=-1)                       # [B, T(k), H]
        kept = (dv != 0).all(dim=-1)
        assert bool((dropped | kept).all())                   # a key row of a head is dropped or kept as a whole
        zeros += int(dropped.sum()); total += dropped.numel()
    assert abs(zeros / total - 0.25) < 0.02, zeros / total
    o.rng_advance(st)
    out3, _ = fwd(q)
    assert not torch.equal(out1, out3)                        # next step -> new mask


# ---- 4. flags and mark groups -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32", "bf16"])
@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("shape", [(2, 230, 32, 2, 5), (2, 140, 128, 2, 6)])
def test_causal_and_diag_flags_streamed(name, flags, shape):
    """EDGL_MAU_CAUSAL / EDGL_MAU_NO_DIAG as tests/test_gpu_ops.py::test_mau_causal_and_diag_flags: separately given qkvt and residual"""
    o = ops()
    B, T, C, H, E = shape
    dt = DT[name]
    assert o.lib.edgl_bimau_form(T, C, H, o._lib.F32 if name == "f32" else o._lib.BF16, flags) == 1
    cfg, x, ids, marks, spans, W = _bimau_case(B, T, C, H, E, 17, 1)
    rng = np.random.default_rng(4)
    qkvt = torch.tensor(_rand((B, T, 4 * C), rng, 0.7), dtype=dt).cuda().requires_grad_()
    resid = torch.tensor(_rand((B, T, C), rng), dtype=dt).cuda().requires_grad_()
    W1, b1, w, sc = (torch.tensor(W[k], dtype=torch.float32).cuda().requires_grad_() for k in ("W1", "b1", "w", "sc"))
    out, lam = o.BiMAUFn.apply(qkvt, resid, W1, b1, w, sc, torch.tensor(ids).cuda(), torch.tensor(spans, dtype=torch.float32).cuda(),
                               torch.tensor(marks.astype(np.uint8)).cuda(), H, o.NO_DROP, flags)
    G1 = torch.tensor(_rand((B, T, C), rng), dtype=dt).cuda()
    G2 = torch.tensor(_rand((H * B, T, E), rng, 0.3), dtype=torch.float32).cuda()
    ((out.float() * G1.float()).sum() + (lam * G2).sum()).backward()
    qr = qkvt.detach().double().cpu().requires_grad_()
    rr = resid.detach().double().cpu().requires_grad_()
    pr = {ST + "dense/kernel": W1.detach().double().cpu().requires_grad_(), ST + "dense/bias": b1.detach().double().cpu().requires_grad_(),
          ST + "weight": w.detach().double().cpu().requires_grad_(), ST + "scaling": sc.detach().double().cpu().requires_grad_()}
    km3 = torch.tensor((ids != 0).astype(np.float64)).unsqueeze(1).repeat(H, T, 1)
    out_r, lam_r = R.bimau(C, H, None, km3, torch.tensor(spans), torch.tensor(marks, dtype=torch.float64), pr, "", 0.0, False,
                           causal=bool(flags & 1), set_diag=not (flags & 2), qkvt=qr, resid=rr)
    ((out_r * G1.double().cpu()).sum() + (lam_r * G2.double().cpu()).sum()).backward()
    ftol, gtol = _bounds(name, T, C // H)
    if name == "f32":
        ftol = 3e-5      # test_mau_causal_and_diag_flags holds every head dim to 3e-5
    assert_close(lam.detach().cpu().numpy(), lam_r.detach().numpy(), ftol, "lambda")
    assert_close(out.float().detach().cpu().numpy(), out_r.detach().numpy(), ftol, "out")
    assert_close(qkvt.grad.float().cpu().numpy(), qr.grad.numpy(), gtol, "dqkvt")
    assert_close(resid.grad.float().cpu().numpy(), rr.grad.numpy(), gtol, "dresid")
    assert_close(W1.grad.cpu().numpy(), pr[ST + "dense/kernel"].grad.numpy(), gtol, "dW1")
    assert_close(b1.grad.cpu().numpy(), pr[ST + "dense/bias"].grad.numpy(), gtol, "db1")
    assert_close(w.grad.cpu().numpy(), pr[ST + "weight"].grad.numpy(), gtol, "dw")
    assert_close(sc.grad.cpu().numpy(), pr[ST + "scaling"].grad.numpy(), gtol, "dscaling")
    if flags & 1:   # a causal row never looks ahead
        q2 = qkvt.detach().clone()
        q2[:, T - 1, C:] += 1.0
        out2, _ = o.BiMAUFn.apply(q2, resid.detach(), W1.detach(), b1.detach(), w.detach(), sc.detach(), torch.tensor(ids).cuda(),
                                  torch.tensor(spans, dtype=torch.float32).cuda(), torch.tensor(marks.astype(np.uint8)).cuda(), H,
                                  o.NO_DROP, flags)
        live = torch.tensor(np.cumsum(ids != 0, axis=1) > 0).cuda()
        live[:, T - 1] = False
        assert torch.equal(out2[live], out.detach()[live])


@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_mark_groups_streamed(name):
    """24 mark types at T = 209, head dim 16, through module.temporal.modulated_attention: two launches (16 + 8 marks), the second
    with EDGL_MAU_DIAG_ZERO and a zero residual, on the shared key mask"""
    from easydgl_amd.module import temporal as Tm
    o = ops()
    shape = (2, 209, 32, 2, 24)
    B, T, C, H, E = shape
    dt = DT[name]
    cfg, x, ids, marks, spans, W = _bimau_case(B, T, C, H, E, T + C)
    xt = torch.tensor(x, dtype=dt).cuda().requires_grad_()
    Wq = torch.tensor(W["Wq"], dtype=torch.float32).cuda().requires_grad_()
    Wq_c = Wq.detach().to(dt)
    bq = torch.tensor(W["bq"], dtype=torch.float32).cuda().requires_grad_()
    W1, b1, w, sc = (torch.tensor(W[k], dtype=torch.float32).cuda().requires_grad_() for k in ("W1", "b1", "w", "sc"))
    qkvt = o.LinearFn.apply(xt, Wq, bq, Wq_c, False)
    out, lam = Tm.modulated_attention(qkvt, xt[:, :, :C], W1, b1, w, sc, torch.tensor(ids).cuda(), torch.tensor(spans, dtype=torch.float32).cuda(),
                                      torch.tensor(marks.astype(np.uint8)).cuda(), H, o.NO_DROP)
    g1, g2 = _cotangents(B, T, C, H, E)
    ((out.float() * torch.tensor(g1, dtype=dt).cuda().float()).sum() + (lam * torch.tensor(g2, dtype=torch.float32).cuda()).sum()).backward()
    got = dict(out=out.float().detach(), lam=lam.detach(), dx=xt.grad.float(), dWqkvt=Wq.grad, dbqkvt=bq.grad, dW1=W1.grad, db1=b1.grad,
               dw=w.grad, dscaling=sc.grad)
    ref = _reference(shape, name)
    ftol, gtol = _bounds(name, T, C // H)
    for k in ("lam", "out"):
        assert_close(got[k].cpu().numpy(), ref[k], ftol, k)
    for k in GRADS:
        assert_close(got[k].cpu().numpy(), ref[k], gtol, k)


# ---- 5. edge cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [209, 257])
def test_fully_masked_row_is_uniform_streamed(T):
    """KAT temporal.py:425-429 (tests/test_gpu_ops.py::test_bimau_fully_masked_row_is_uniform) through the key-streamed kernels"""
    o = ops()
    B, C, H, E = 1, 32, 2, 2
    rng = np.random.default_rng(0)
    qkvt = torch.tensor(_rand((B, T, 4 * C), rng), dtype=torch.float32).cuda()
    resid = torch.zeros((B, T, C)).cuda()
    dh = C // H
    W1 = torch.zeros((dh + 1, dh * E)).cuda(); b1 = torch.zeros(dh * E).cuda()
    w = torch.zeros((E, dh)).cuda(); sc = torch.zeros(E).cuda()
    ids = torch.zeros((B, T), dtype=torch.int64).cuda()
    marks = torch.ones((B, T, E), dtype=torch.uint8).cuda()
    out, lam = o.BiMAUFn.apply(qkvt, resid, W1, b1, w, sc, ids, torch.ones((B, T)).cuda(), marks, H, o.NO_DROP)
    np.testing.assert_allclose(lam.cpu().numpy(), math.log(2.0), rtol=1e-6)
    V = qkvt[0, :, 2 * C:3 * C].double().cpu().numpy()
    G = np.full((T, T), E * math.log(2.0)); G[np.arange(T), np.arange(T)] = 1.0
    want = (G / T) @ V
    np.testing.assert_allclose(out[0].cpu().numpy(), want, rtol=2e-5, atol=1e-6)


@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_streamed_backward_is_deterministic_and_inference_equals_training(name):
    shape = (3, 257, 32, 2, 16)
    a, b = _run_unit(shape, name), _run_unit(shape, name)
    for k in ("out", "lam") + GRADS:
        assert np.array_equal(a[k], b[k]), k            # no atomics: bit-identical
    inf = _run_unit(shape, name, backward=False)
    assert np.array_equal(inf["out"], a["out"]) and np.array_equal(inf["lam"], a["lam"])


def test_streamed_forward_fills_zero_rows_and_backward_repeats_bitwise():
    """edgl_bimau_fwd_zr on the key-streamed path fills the [H*B, T, E] array with zeros; two edgl_bimau_bwd calls on the same
    inputs give bit-identical d_qkvt and parameter gradients"""
    o = ops()
    lib, _ptr, _stream = o.lib, o._ptr, o._stream
    B, T, C, H, E = 2, 209, 32, 2, 4
    dh, code = C // H, o._lib.F32
    cfg, x, ids, marks, spans, W = _bimau_case(B, T, C, H, E, T + C)
    rng = np.random.default_rng(2)
    dev = "cuda"
    qkvt = torch.tensor(_rand((B, T, 4 * C), rng, 0.5), dtype=torch.float32, device=dev)
    resid = torch.tensor(_rand((B, T, C), rng), dtype=torch.float32, device=dev)
    W1, b1, w, sc = (torch.tensor(W[k], dtype=torch.float32, device=dev) for k in ("W1", "b1", "w", "sc"))
    ids_t, sp_t = torch.tensor(ids, device=dev), torch.tensor(spans, dtype=torch.float32, device=dev)
    mk_t = torch.tensor(marks.astype(np.uint8), device=dev)
    pack = torch.empty(lib.edgl_bimau_pack_bytes(C, H, E, code), device=dev, dtype=torch.uint8)
    o.check(lib.edgl_bimau_pack(_ptr(W1), _ptr(b1), _ptr(w), _ptr(sc), C, H, E, _ptr(pack), code, _stream()), "pack")
    out = torch.empty((B, T, C), device=dev)
    lam = torch.empty((H * B, T, E), device=dev)
    zr = torch.full((H * B, T, E), 7.0, device=dev)
    saved = torch.empty(lib.edgl_bimau_saved_bytes(B, T, C, H, code), device=dev, dtype=torch.uint8)
    o.check(lib.edgl_bimau_fwd_zr(_ptr(qkvt), _ptr(resid), C, _ptr(ids_t), _ptr(sp_t), _ptr(mk_t), _ptr(pack), B, T, C, H, E, 0.0, None, 0,
                                  _ptr(out), _ptr(lam), _ptr(saved), _ptr(zr), 0, code, _stream()), "fwd_zr")
    assert float(zr.abs().max()) == 0.0
    # inference without `saved` is refused (three launches hand H rows, z and the statistics through it)
    rc = lib.edgl_bimau_fwd(_ptr(qkvt), _ptr(resid), C, _ptr(ids_t), _ptr(sp_t), _ptr(mk_t), _ptr(pack), B, T, C, H, E, 0.0, None, 0,
                            _ptr(out.clone()), _ptr(lam.clone()), None, 0, code, _stream())
    assert rc == -5 and b"saved" in lib.edgl_last_error()
    d_out = torch.tensor(_rand((B, T, C), rng), dtype=torch.float32, device=dev)
    ws = torch.empty(lib.edgl_bimau_bwd_workspace(B, T, C, H, E, code), device=dev, dtype=torch.uint8)
    res = []
    for _ in range(2):
        dq = torch.full_like(qkvt, float("nan"))
        g = [torch.empty_like(t) for t in (W1, b1, w, sc)]
        ws.fill_(255)
        o.check(lib.edgl_bimau_bwd(_ptr(qkvt), _ptr(ids_t), _ptr(sp_t), _ptr(mk_t), _ptr(pack), _ptr(d_out), None, _ptr(lam), _ptr(saved),
                                   B, T, C, H, E, 0.0, None, 0, _ptr(dq), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]), _ptr(g[3]), _ptr(ws), 0, code,
                                   _stream()), "bwd")
        res.append([dq] + g)
    assert bool(torch.isfinite(res[0][0]).all())          # every element of d_qkvt has a writer
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # the fused TPP form does not exist on this path
    rc = lib.edgl_bimau_bwd_tpp(_ptr(qkvt), _ptr(ids_t), _ptr(sp_t), _ptr(mk_t), _ptr(pack), _ptr(d_out), _ptr(ws), 4, None, 0.1, _ptr(lam),
                                _ptr(lam), _ptr(saved), B, T, C, H, E, 0.0, None, 0, None, 0.0, _ptr(dq), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]),
                                _ptr(g[3]), _ptr(ws), 0, code, _stream())
    assert rc == -1
