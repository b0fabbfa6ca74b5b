"""Per-op parity of the HIP kernels (through the C ABI) against the fp64 oracle.
Tolerances: f32 path (exact-f32 MFMA) 2e-5 relative to the tensor's max magnitude unless stated; bf16 path 2e-2."""
import math

import numpy as np
import pytest
import torch

from oracle import easydgl_oracle as O
from oracle import torch_ref as R
from tests._util import assert_close, rel_err

pytestmark = pytest.mark.gpu

DTYPES = [("f32", torch.float32, 3e-5), ("bf16", torch.bfloat16, 2.5e-2)]


def ops():
    from easydgl_amd import ops as _ops
    return _ops


def _rand(shape, rng, scale=1.0):
    return rng.standard_normal(shape) * scale


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dt,tol", DTYPES)
@pytest.mark.parametrize("a_kc,b_kc", [(1, 1), (1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (200, 72, 104), (1000, 384, 40), (64, 256, 1024)])
def test_gemm_layouts(name, dt, tol, a_kc, b_kc, M, N, K):
    o = ops()
    rng = np.random.default_rng(M + N + K)
    A, Bm = _rand((M, K), rng), _rand((K, N), rng)
    At = torch.tensor(A if a_kc else A.T.copy(), dtype=dt).cuda().contiguous()
    Bt = torch.tensor(Bm.T.copy() if b_kc else Bm, dtype=dt).cuda().contiguous()
    ref = At.double().cpu().numpy() if a_kc else At.double().cpu().numpy().T
    refB = Bt.double().cpu().numpy().T if b_kc else Bt.double().cpu().numpy()
    want = ref @ refB
    got = o.gemm(At, Bt, M, N, K, At.stride(0), Bt.stride(0), a_kc, b_kc, torch.float32)
    assert_close(got.cpu().numpy(), want, 2e-6 if name == "f32" else 1e-5, f"gemm {name} {a_kc}{b_kc}")


@pytest.mark.parametrize("b_kc", [0, 1])
@pytest.mark.parametrize("M,N,K,flags", [(4100, 512, 384, "bias"), (4352, 384, 512, "plain"), (4100, 384, 384, "gelu"),
                                         (4100, 512, 512, "accum"), (300, 128, 128, "dgelu"), (5000, 256, 128, "accum"),
                                         # the wide layers of the 512-unit recipes (K > 512: tiled kernel, general epilogue)
                                         (2100, 2048, 1536, "bias"), (1500, 512, 1024, "plain"), (1100, 1024, 1024, "gelu"),
                                         (1300, 512, 1024, "accum"), (1030, 1536, 2048, "dgelu")])
def test_gemm_bf16_activation_kernels(b_kc, M, N, K, flags):
    """bf16 dense fast paths at sizes that reach them: weights-resident strips, the weights-streamed kernel for wide
    outputs (M >= 4096, K in {384, 512}, N >= 384), and the fused epilogues (bias, GELU + saved pre-activation,
    x GELU'(aux), += C)."""
    o = ops()
    rng = np.random.default_rng(M + N + K + b_kc)
    dt = torch.bfloat16
    A = torch.tensor(_rand((M, K), rng), dtype=dt).cuda()
    W = torch.tensor(_rand((K, N), rng, 0.05), dtype=dt).cuda()
    Wt = W.t().contiguous() if b_kc else W
    bias = torch.tensor(_rand((N,), rng), dtype=torch.float32).cuda()
    ref = A.double().cpu() @ W.double().cpu()
    from easydgl_amd import _lib as L
    if flags == "bias":
        got = o.gemm(A, Wt, M, N, K, K, Wt.stride(0), True, bool(b_kc), dt, bias=bias, flags=L.EPI_BIAS)
        want = ref + bias.double().cpu()
    elif flags == "plain":
        got = o.gemm(A, Wt, M, N, K, K, Wt.stride(0), True, bool(b_kc), dt)
        want = ref
    elif flags == "gelu":
        pre = torch.empty((M, N), dtype=dt, device="cuda")
        got = o.gemm(A, Wt, M, N, K, K, Wt.stride(0), True, bool(b_kc), dt, bias=bias, aux=pre, flags=L.EPI_BIAS | L.EPI_GELU | L.EPI_SAVE_PRE)
        z = ref + bias.double().cpu()
        want = R.gelu(z)
        assert_close(pre.float().cpu().numpy(), z.numpy(), 1e-2, "saved pre-activation")
    elif flags == "dgelu":
        aux = torch.tensor(_rand((M, N), rng), dtype=dt).cuda()
        got = o.gemm(A, Wt, M, N, K, K, Wt.stride(0), True, bool(b_kc), dt, aux=aux, flags=L.EPI_MUL_DGELU)
        a64 = aux.double().cpu().requires_grad_()
        R.gelu(a64).sum().backward()
        want = ref * a64.grad
    else:
        c0 = torch.tensor(_rand((M, N), rng), dtype=dt).cuda()
        got = o.gemm(A, Wt, M, N, K, K, Wt.stride(0), True, bool(b_kc), dt, flags=L.EPI_ACCUM, out=c0.clone())
        want = ref + c0.double().cpu()
    assert_close(got.float().cpu().numpy(), want.detach().numpy(), 1.2e-2, f"bf16 gemm {flags} b_kc={b_kc}")


@pytest.mark.parametrize("name,dt,tol", DTYPES)
def test_gemm_epilogues_and_splitk(name, dt, tol):
    o = ops()
    from easydgl_amd import _lib
    rng = np.random.default_rng(5)
    M, N, K = 300, 96, 2000
    A = torch.tensor(_rand((M, K), rng, 0.1), dtype=dt).cuda()
    W = torch.tensor(_rand((K, N), rng, 0.1), dtype=dt).cuda()
    b = torch.tensor(_rand((N,), rng), dtype=torch.float32).cuda()
    z = A.double().cpu().numpy() @ W.double().cpu().numpy() + b.double().cpu().numpy()
    pre = torch.empty((M, N), dtype=dt, device="cuda")
    y = o.gemm(A, W, M, N, K, K, N, True, False, dt, bias=b, aux=pre,
               flags=_lib.EPI_BIAS | _lib.EPI_GELU | _lib.EPI_SAVE_PRE)
    assert_close(pre.float().cpu().numpy(), z, tol, "pre-activation")
    assert_close(y.float().cpu().numpy(), O.gelu(z), tol, "gelu")
    ys = o.gemm(A, W, M, N, K, K, N, True, False, torch.float32, bias=b, flags=_lib.EPI_BIAS, splitk=7)
    assert_close(ys.cpu().numpy(), z, 1e-5, "split-K")
    acc = torch.ones((M, N), dtype=torch.float32, device="cuda")
    o.gemm(A, W, M, N, K, K, N, True, False, torch.float32, flags=_lib.EPI_ACCUM, out=acc)
    assert_close(acc.cpu().numpy(), z - b.double().cpu().numpy() + 1.0, 1e-5, "accumulate")
    cs = o.colsum(pre, M, N)
    assert_close(cs.cpu().numpy(), pre.double().cpu().numpy().sum(0), 1e-5, "colsum")


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dt,tol", DTYPES)
@pytest.mark.parametrize("B,T,C,gather,resid", [(3, 11, 32, False, True), (5, 101, 128, True, True), (2, 7, 64, False, False)])
def test_layernorm_fwd_bwd(name, dt, tol, B, T, C, gather, resid):
    o = ops()
    rng = np.random.default_rng(B * T)
    x = torch.tensor(_rand((B, T, C), rng), dtype=dt).cuda().requires_grad_()
    big = torch.tensor(_rand((B, T, 3 * C), rng), dtype=dt).cuda().requires_grad_() if resid else None
    g = torch.tensor(1 + 0.1 * _rand((C,), rng), dtype=torch.float32).cuda().requires_grad_()
    be = torch.tensor(0.1 * _rand((C,), rng), dtype=torch.float32).cuda().requires_grad_()
    gp = None
    if gather:
        gp = torch.tensor(np.stack([rng.choice(T - 1, 4, replace=False) + 1 for _ in range(B)]), dtype=torch.int64).cuda()
    y = o.AddLayerNormFn.apply(x, big[:, :, :C] if resid else None, g, be, o.NO_DROP, gp)
    dy = torch.tensor(_rand(tuple(y.shape), rng), dtype=dt).cuda()
    y.backward(dy)
    # fp64 reference on the same (possibly bf16-rounded) inputs
    xr = x.detach().double().cpu().requires_grad_()
    br = big.detach().double().cpu().requires_grad_() if resid else None
    gr, ber = g.detach().double().cpu().requires_grad_(), be.detach().double().cpu().requires_grad_()
    s = xr + (br[:, :, :C] if resid else 0)
    yr = R.layernorm(s, gr, ber)
    if gather:
        yr = yr[torch.arange(B)[:, None], gp.cpu()].reshape(-1, C)
    yr.backward(dy.double().cpu())
    assert_close(y.detach().float().cpu().numpy(), yr.detach().numpy(), tol, "ln y")
    assert_close(x.grad.float().cpu().numpy(), xr.grad.numpy(), tol * 3, "ln dx")
    if resid:
        assert_close(big.grad.float().cpu().numpy(), br.grad.numpy(), tol * 3, "ln dresid")
    assert_close(g.grad.cpu().numpy(), gr.grad.numpy(), tol * 3, "ln dgamma")
    assert_close(be.grad.cpu().numpy(), ber.grad.numpy(), tol * 3, "ln dbeta")


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [32, 128, 512])     # 128 / 512: the one-hot MFMA scatter (bf16), one / four channel slices
@pytest.mark.parametrize("name,dt,tol", DTYPES)
def test_encode_fwd_bwd(name, dt, tol, width):
    o = ops()
    cfg = O.Config(num_items=40, seqslen=12 if width == 32 else 37, num_units=width, num_heads=2, time_scale=86400.0, num_events=5)
    rng = np.random.default_rng(3)
    p = O.init_params(cfg, rng)
    mt = O.synthetic_mark_table(cfg.num_items, cfg.num_events, multi_hot=True)
    ids, ts = O.synthetic_sequences(cfg, 6 if width == 32 else 9, rng, min_len=2)
    ids[0, -1] = cfg.mask_id
    item = torch.tensor(p["CSTMA/item_embs/lookup_table"], dtype=torch.float32).cuda().requires_grad_()
    pos = torch.tensor(p["CSTMA/spatial_embs/embedding/lookup_table"], dtype=torch.float32).cuda().requires_grad_()
    mk = torch.tensor(p["CSTMA/mark_embs/lookup_table"], dtype=torch.float32).cuda().requires_grad_()
    item_c = item.detach().to(dt)
    tscale = torch.tensor(O.time_sinusoid_scale(cfg.num_units)).cuda()
    x0, spans, marks = o.EncodeFn.apply(item, pos, mk, item_c, torch.tensor(ids).cuda(), torch.tensor(ts).cuda(),
                                        torch.tensor(mt.astype(np.uint8)).cuda(), tscale, cfg.mask_id, cfg.time_scale,
                                        o.NO_DROP, dt)
    pp = dict(p)
    pp["CSTMA/item_embs/lookup_table"] = item_c.double().cpu().numpy()
    want_x0, want_sp, want_mk, _ = O.input_encode(cfg, pp, mt, ids, ts)
    np.testing.assert_array_equal(marks.cpu().numpy(), want_mk)
    np.testing.assert_array_equal(spans.cpu().numpy(), want_sp.astype(np.float32))
    assert_close(x0.detach().float().cpu().numpy(), want_x0, 2e-6 if name == "f32" else 8e-3, "x0")
    G = torch.tensor(_rand(tuple(x0.shape), rng), dtype=dt).cuda()
    x0.backward(G)
    # reference gradients
    Gd = G.double().cpu().numpy()
    C = cfg.num_units
    d_item = np.zeros_like(p["CSTMA/item_embs/lookup_table"])
    np.add.at(d_item, ids.reshape(-1), math.sqrt(C) * Gd[..., :C].reshape(-1, C))
    d_item[0] = 0
    d_pos = Gd[..., C:2 * C].sum(0)
    d_mk = np.zeros_like(p["CSTMA/mark_embs/lookup_table"])
    d_mk[1] = (want_mk.sum(-1)[..., None] * Gd[..., 2 * C:]).sum((0, 1))
    assert_close(item.grad.cpu().numpy(), d_item, 1e-5, "d_item")
    assert_close(pos.grad.cpu().numpy(), d_pos, 1e-5, "d_pos")
    assert_close(mk.grad.cpu().numpy(), d_mk, 1e-5, "d_mark")


def test_time_code_matches_oracle_at_large_arguments():
    """coding.py:141-145 with Netflix-scale timestamps (float32 seconds ~1e9 / 86400)."""
    o = ops()
    cfg = O.Config(num_items=10, seqslen=63, num_units=128, num_heads=8, time_scale=86400.0, num_events=2)
    rng = np.random.default_rng(1)
    p = O.init_params(cfg, rng)
    mt = O.synthetic_mark_table(cfg.num_items, 2)
    ids, ts = O.synthetic_sequences(cfg, 4, rng, min_len=60)
    item = torch.zeros((cfg.I, 128), dtype=torch.float32).cuda()
    x0, _, _ = o.EncodeFn.apply(item, torch.zeros((cfg.T, 128)).cuda(), torch.zeros((2, 128)).cuda(), item,
                                torch.tensor(ids).cuda(), torch.tensor(ts).cuda(), torch.tensor(mt.astype(np.uint8)).cuda(),
                                torch.tensor(O.time_sinusoid_scale(128)).cuda(), cfg.mask_id, cfg.time_scale, o.NO_DROP,
                                torch.float32)
    want = O.time_sinusoid_code(O.scaled_times(ts, cfg.time_scale), 128)
    assert np.abs(x0[..., :128].cpu().numpy() - want).max() < 5e-7


# ---------------------------------------------------------------------------------------------------
def _bimau_case(B, T, C, H, E, seed, cin_mult=3):
    cfg = O.Config(num_items=30, seqslen=T - 1, num_units=C, num_heads=H, num_events=E, time_scale=1.0)
    rng = np.random.default_rng(seed)
    dh = C // H
    cin = cin_mult * C
    x = _rand((B, T, cin), rng)
    ids = rng.integers(1, cfg.num_items, size=(B, T))
    for b in range(B):
        ids[b, :rng.integers(0, T // 2 + 1)] = 0
    if B > 2:
        ids[2, :] = 0  # a fully padded sample: uniform attention (temporal.py:425-429)
    mt = O.synthetic_mark_table(cfg.num_items, E, multi_hot=True)
    marks = mt[ids]
    spans = rng.uniform(0, 5, size=(B, T))
    # projection scale: 0.15 up to 768 inputs, shrunk beyond so that the Q.K scores of the num_units = 512 cases stay in the
    # same range as the others (a 1536-long contraction at 0.15 saturates the softmax and measures bf16 rounding of Q, K only)
    W = dict(Wq=_rand((cin, 4 * C), rng, 0.15 * min(1.0, math.sqrt(768.0 / cin))), bq=_rand((4 * C,), rng, 0.1), W1=O.glorot_uniform(rng, (dh + 1, dh * E)),
             b1=_rand((dh * E,), rng, 0.1), w=O.glorot_uniform(rng, (E, dh)), sc=_rand((E,), rng, 0.2))
    return cfg, x, ids, marks, spans, W


@pytest.mark.parametrize("name,dt,tol", DTYPES)
@pytest.mark.parametrize("B,T,C,H,E", [(3, 11, 32, 2, 4), (2, 31, 64, 2, 7), (2, 101, 128, 8, 16), (1, 128, 32, 2, 2),
                                       (2, 201, 256, 8, 16), (1, 150, 32, 2, 3),
                                       # head dims 64 / 128 (k_bimau_big.hip): the published recipes' shapes — EasyDGL
                                       # runme.sh:15-23 (C=512, h=8, T=31) and CTSMA's head dim (runme.sh:107-115: h=4) —
                                       # plus the longest sequences each head dim takes and odd mark counts
                                       (3, 31, 512, 8, 16), (2, 31, 512, 4, 16), (2, 101, 128, 2, 5), (1, 112, 64, 1, 16),
                                       (2, 64, 128, 1, 3), (3, 17, 256, 2, 7),
                                       # bf16 only: T up to 128 at head dims 64 and 128 (CTSMA's head dim at L = 100: sweep 2 runs
                                       # as two channel slices beyond 4 key tiles)
                                       (2, 128, 128, 2, 6), (2, 101, 256, 2, 16), (1, 128, 128, 1, 5)])
def test_bimau_fwd_bwd(name, dt, tol, B, T, C, H, E):
    o = ops()
    if name == "f32" and T > 128 and C // H == 32:
        pytest.skip("f32 staging of 13 key tiles at head dim 32 needs 241 KB of LDS: T > 128 at dh = 32 is a bf16-only shape")
    if name == "f32" and ((C // H == 64 and T > 112) or (C // H == 128 and T > 64)):
        pytest.skip("f32 staging (four-byte elements + transposed images) bounds head dim 64 at T = 112 and head dim 128 at T = 64")
    cfg, x, ids, marks, spans, W = _bimau_case(B, T, C, H, E, seed=T + C)
    xt = torch.tensor(x, dtype=dt).cuda().requires_grad_()
    Wq = torch.tensor(W["Wq"], dtype=torch.float32).cuda().requires_grad_()
    Wq_c = Wq.detach().to(dt)
    bq = torch.tensor(W["bq"], dtype=torch.float32).cuda().requires_grad_()
    W1, b1, w, sc = (torch.tensor(W[k], dtype=torch.float32).cuda().requires_grad_() for k in ("W1", "b1", "w", "sc"))
    qkvt = o.LinearFn.apply(xt, Wq, bq, Wq_c, False)
    out, lam = o.BiMAUFn.apply(qkvt, xt[:, :, :C], W1, b1, w, sc, torch.tensor(ids).cuda(),
                               torch.tensor(spans, dtype=torch.float32).cuda(), torch.tensor(marks.astype(np.uint8)).cuda(),
                               H, o.NO_DROP)
    rng = np.random.default_rng(9)
    G1 = torch.tensor(_rand((B, T, C), rng), dtype=dt).cuda()
    G2 = torch.tensor(_rand((H * B, T, E), rng, 0.3), dtype=torch.float32).cuda()
    ((out.float() * G1.float()).sum() + (lam * G2).sum()).backward()
    # fp64 reference evaluated on the rounded inputs the kernel saw
    xr = xt.detach().double().cpu().requires_grad_()
    pr = {"dense/kernel": Wq_c.double().cpu().requires_grad_(), "dense/bias": bq.detach().double().cpu().requires_grad_(),
          "sequential_temporal_combined/dense/kernel": W1.detach().double().cpu().requires_grad_(),
          "sequential_temporal_combined/dense/bias": b1.detach().double().cpu().requires_grad_(),
          "sequential_temporal_combined/weight": w.detach().double().cpu().requires_grad_(),
          "sequential_temporal_combined/scaling": sc.detach().double().cpu().requires_grad_()}
    km3 = torch.tensor((ids != 0).astype(np.float64)).unsqueeze(1).repeat(H, T, 1)
    out_r, lam_r = R.bimau(C, H, xr, km3, torch.tensor(spans), torch.tensor(marks, dtype=torch.float64), pr, "", 0.0, False)
    ((out_r * G1.double().cpu()).sum() + (lam_r * G2.double().cpu()).sum()).backward()
    ftol = 3e-5 if name == "f32" else (3e-2 if T <= 128 else 5e-2)   # 201 bf16 probabilities per row at the config-3 shape
    if C // H >= 64 and name == "f32":
        ftol = 6e-5    # 64-/128-long f32 contractions in the intensity MLP (dh*E sigmoids per row feed one z)
    assert_close(lam.detach().cpu().numpy(), lam_r.detach().numpy(), ftol, "lambda")
    assert_close(out.float().detach().cpu().numpy(), out_r.detach().numpy(), ftol, "out")
    gtol = 2e-4 if name == "f32" else 6e-2
    assert_close(xt.grad.float().cpu().numpy(), xr.grad.numpy(), gtol, "dx")
    assert_close(Wq.grad.cpu().numpy(), pr["dense/kernel"].grad.numpy(), gtol, "dWqkvt")
    assert_close(bq.grad.cpu().numpy(), pr["dense/bias"].grad.numpy(), gtol, "dbqkvt")
    assert_close(W1.grad.cpu().numpy(), pr["sequential_temporal_combined/dense/kernel"].grad.numpy(), gtol, "dW1")
    assert_close(b1.grad.cpu().numpy(), pr["sequential_temporal_combined/dense/bias"].grad.numpy(), gtol, "db1")
    assert_close(w.grad.cpu().numpy(), pr["sequential_temporal_combined/weight"].grad.numpy(), gtol, "dw")
    assert_close(sc.grad.cpu().numpy(), pr["sequential_temporal_combined/scaling"].grad.numpy(), gtol, "dscaling")


@pytest.mark.parametrize("B,T,C,H,E", [(512, 101, 128, 8, 16), (512, 201, 256, 8, 16)])
def test_bimau_at_the_full_batch_against_fp64_on_the_gpu(B, T, C, H, E):
    """K3 at the benchmarked shape (BASELINE.json configs[1]: 4096 (sample, head) jobs of 101 positions) and at config 3's (201 positions,
    head dim 32), bf16, the whole batch of 512: outputs, lambda and every gradient against the fp64 restatement (oracle/torch_ref.py,
    evaluated on the GPU in float64 on the rounded inputs the kernels saw: ~ 50 GB of [h B, T, T] / [h B, T, dh E] tensors at config 3)."""
    o = ops()
    dt = torch.bfloat16
    cfg, x, ids, marks, spans, W = _bimau_case(B, T, C, H, E, seed=T + C)
    xt = torch.tensor(x, dtype=dt).cuda().requires_grad_()
    Wq = torch.tensor(W["Wq"], dtype=torch.float32).cuda().requires_grad_()
    Wq_c = Wq.detach().to(dt)
    bq = torch.tensor(W["bq"], dtype=torch.float32).cuda().requires_grad_()
    W1, b1, w, sc = (torch.tensor(W[k], dtype=torch.float32).cuda().requires_grad_() for k in ("W1", "b1", "w", "sc"))
    ids_d = torch.tensor(ids).cuda()
    qkvt = o.LinearFn.apply(xt, Wq, bq, Wq_c, False)
    out, lam = o.BiMAUFn.apply(qkvt, xt[:, :, :C], W1, b1, w, sc, ids_d, torch.tensor(spans, dtype=torch.float32).cuda(),
                               torch.tensor(marks.astype(np.uint8)).cuda(), H, o.NO_DROP)
    g = torch.Generator(device="cuda").manual_seed(9)
    G1 = torch.randn((B, T, C), device="cuda", generator=g).to(dt)
    G2 = torch.randn((H * B, T, E), device="cuda", generator=g) * 0.3
    ((out.float() * G1.float()).sum() + (lam * G2).sum()).backward()
    xr = xt.detach().double().requires_grad_()
    pr = {"dense/kernel": Wq_c.double().requires_grad_(), "dense/bias": bq.detach().double().requires_grad_(),
          "sequential_temporal_combined/dense/kernel": W1.detach().double().requires_grad_(),
          "sequential_temporal_combined/dense/bias": b1.detach().double().requires_grad_(),
          "sequential_temporal_combined/weight": w.detach().double().requires_grad_(),
          "sequential_temporal_combined/scaling": sc.detach().double().requires_grad_()}
    # the samples are independent: the reference runs over chunks of 64 (its [h B, T, T, E] broadcast of lambda is 21 GB at config 3's
    # full batch); parameter gradients accumulate over the chunks, lambda's head-major rows b' = head * B + b are re-stacked
    sp_d, mk_d = torch.tensor(spans).cuda(), torch.tensor(marks, dtype=torch.float64).cuda()
    outs, lams = [], []
    for b0 in range(0, B, 64):
        b1_ = min(B, b0 + 64)
        km3 = (ids_d[b0:b1_] != 0).double().unsqueeze(1).repeat(H, T, 1)
        o_c, l_c = R.bimau(C, H, xr[b0:b1_], km3, sp_d[b0:b1_], mk_d[b0:b1_], pr, "", 0.0, False)
        g2 = G2.view(H, B, T, E)[:, b0:b1_].reshape(H * (b1_ - b0), T, E)
        ((o_c * G1[b0:b1_].double()).sum() + (l_c * g2.double()).sum()).backward()
        outs.append(o_c.detach()); lams.append(l_c.detach().view(H, b1_ - b0, T, E))
    out_r, lam_r = torch.cat(outs, dim=0), torch.cat(lams, dim=1).reshape(H * B, T, E)
    # Max-norm over 6.6 M / 26 M outputs: the tail of what the bf16 rounding of Q and K does to a sharp softmax reaches 4e-2 of the largest
    # output on a handful of elements (measured: 1e-6 of them above 2e-2; against the restatement fed with the kernel's own bf16 QKVT the
    # kernel itself is within 6e-3) — so the max-norm bound is 6e-2 here and the relative L2 norm carries the claim
    ftol, gtol = 6e-2, 6e-2
    n = lambda t: t.detach().double().cpu().numpy()
    rel2 = lambda a, b: float((a.double() - b).norm() / b.norm())
    assert rel2(out.detach(), out_r) < 1.5e-2, rel2(out.detach(), out_r)
    assert rel2(lam.detach(), lam_r) < 1.5e-2, rel2(lam.detach(), lam_r)
    assert rel2(xt.grad, xr.grad) < 3e-2, rel2(xt.grad, xr.grad)
    assert_close(n(lam), n(lam_r), ftol, "lambda")
    assert_close(n(out), n(out_r), ftol, "out")
    assert_close(n(xt.grad), n(xr.grad), gtol, "dx")
    assert_close(n(Wq.grad), n(pr["dense/kernel"].grad), gtol, "dWqkvt")
    assert_close(n(bq.grad), n(pr["dense/bias"].grad), gtol, "dbqkvt")
    assert_close(n(W1.grad), n(pr["sequential_temporal_combined/dense/kernel"].grad), gtol, "dW1")
    assert_close(n(b1.grad), n(pr["sequential_temporal_combined/dense/bias"].grad), gtol, "db1")
    assert_close(n(w.grad), n(pr["sequential_temporal_combined/weight"].grad), gtol, "dw")
    assert_close(n(sc.grad), n(pr["sequential_temporal_combined/scaling"].grad), gtol, "dscaling")


@pytest.mark.parametrize("name,dt,tol", DTYPES)
@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("B,T,C,H,E", [(3, 21, 32, 2, 5), (2, 30, 512, 4, 16), (2, 40, 128, 2, 6)])
def test_mau_causal_and_diag_flags(name, dt, tol, flags, B, T, C, H, E):
    """EDGL_MAU_CAUSAL / EDGL_MAU_NO_DIAG (MAU.__call__, temporal.py:335-390) with separately projected Q and K|V|T_
    and the queries as residual, forward and every gradient against the fp64 restatement; the second shape is CTSMA's
    published recipe (runme.sh:107-115: num_units 512, 4 heads -> head dim 128, 30 positions)."""
    o = ops()
    cfg, x, ids, marks, spans, W = _bimau_case(B, T, C, H, E, seed=17, cin_mult=1)
    rng = np.random.default_rng(4)
    qkvt = torch.tensor(_rand((B, T, 4 * C), rng, 0.7), dtype=dt).cuda().requires_grad_()
    resid = torch.tensor(_rand((B, T, C), rng), dtype=dt).cuda().requires_grad_()
    W1 = torch.tensor(W["W1"], dtype=torch.float32).cuda().requires_grad_()
    b1 = torch.tensor(W["b1"], dtype=torch.float32).cuda().requires_grad_()
    w = torch.tensor(W["w"], dtype=torch.float32).cuda().requires_grad_()
    sc = torch.tensor(W["sc"], dtype=torch.float32).cuda().requires_grad_()
    out, lam = o.BiMAUFn.apply(qkvt, resid, W1, b1, w, sc, torch.tensor(ids).cuda(), torch.tensor(spans, dtype=torch.float32).cuda(),
                               torch.tensor(marks.astype(np.uint8)).cuda(), H, o.NO_DROP, flags)
    G1 = torch.tensor(_rand((B, T, C), rng), dtype=dt).cuda()
    G2 = torch.tensor(_rand((H * B, T, E), rng, 0.3), dtype=torch.float32).cuda()
    ((out.float() * G1.float()).sum() + (lam * G2).sum()).backward()
    qr = qkvt.detach().double().cpu().requires_grad_()
    rr = resid.detach().double().cpu().requires_grad_()
    pr = {"sequential_temporal_combined/dense/kernel": W1.detach().double().cpu().requires_grad_(),
          "sequential_temporal_combined/dense/bias": b1.detach().double().cpu().requires_grad_(),
          "sequential_temporal_combined/weight": w.detach().double().cpu().requires_grad_(),
          "sequential_temporal_combined/scaling": sc.detach().double().cpu().requires_grad_()}
    km3 = torch.tensor((ids != 0).astype(np.float64)).unsqueeze(1).repeat(H, T, 1)
    out_r, lam_r = R.bimau(C, H, None, km3, torch.tensor(spans), torch.tensor(marks, dtype=torch.float64), pr, "", 0.0, False,
                           causal=bool(flags & 1), set_diag=not (flags & 2), qkvt=qr, resid=rr)
    ((out_r * G1.double().cpu()).sum() + (lam_r * G2.double().cpu()).sum()).backward()
    ftol = 3e-5 if name == "f32" else (3e-2 if T <= 128 else 5e-2)   # 201 bf16 probabilities per row at the config-3 shape
    assert_close(lam.detach().cpu().numpy(), lam_r.detach().numpy(), ftol, "lambda")
    assert_close(out.float().detach().cpu().numpy(), out_r.detach().numpy(), ftol, "out")
    gtol = 2e-4 if name == "f32" else 6e-2
    assert_close(qkvt.grad.float().cpu().numpy(), qr.grad.numpy(), gtol, "dqkvt")
    assert_close(resid.grad.float().cpu().numpy(), rr.grad.numpy(), gtol, "dresid")
    assert_close(W1.grad.cpu().numpy(), pr["sequential_temporal_combined/dense/kernel"].grad.numpy(), gtol, "dW1")
    assert_close(w.grad.cpu().numpy(), pr["sequential_temporal_combined/weight"].grad.numpy(), gtol, "dw")
    assert_close(sc.grad.cpu().numpy(), pr["sequential_temporal_combined/scaling"].grad.numpy(), gtol, "dscaling")
    if flags & 1:   # a causal row never looks ahead: perturbing a future key leaves earlier outputs unchanged
        q2 = qkvt.detach().clone()
        q2[:, T - 1, C:] += 1.0
        out2, _ = o.BiMAUFn.apply(q2, resid.detach(), W1.detach(), b1.detach(), w.detach(), sc.detach(), torch.tensor(ids).cuda(),
                                  torch.tensor(spans, dtype=torch.float32).cuda(), torch.tensor(marks.astype(np.uint8)).cuda(), H,
                                  o.NO_DROP, flags)
        rows = [(b, t) for b in range(B) for t in range(T - 1) if ids[b, :t + 1].any()]
        for b, t in rows:
            assert torch.equal(out2[b, t], out.detach()[b, t])


def test_bimau_fully_masked_row_is_uniform():
    """KAT temporal.py:425-429 through the kernel: all keys padded -> P = 1/T -> out = mean_k(G*V) + resid."""
    o = ops()
    B, T, C, H, E = 1, 9, 32, 2, 2
    rng = np.random.default_rng(0)
    qkvt = torch.tensor(_rand((B, T, 4 * C), rng), dtype=torch.float32).cuda()
    resid = torch.zeros((B, T, C)).cuda()
    dh = C // H
    W1 = torch.zeros((dh + 1, dh * E)).cuda(); b1 = torch.zeros(dh * E).cuda()
    w = torch.zeros((E, dh)).cuda(); sc = torch.zeros(E).cuda()
    ids = torch.zeros((B, T), dtype=torch.int64).cuda()
    marks = torch.ones((B, T, E), dtype=torch.uint8).cuda()
    out, lam = o.BiMAUFn.apply(qkvt, resid, W1, b1, w, sc, ids, torch.ones((B, T)).cuda(), marks, H, o.NO_DROP)
    np.testing.assert_allclose(lam.cpu().numpy(), math.log(2.0), rtol=1e-6)   # temporal.py:299-306
    V = qkvt[0, :, 2 * C:3 * C].double().cpu().numpy()
    G = np.full((T, T), E * math.log(2.0)); G[np.arange(T), np.arange(T)] = 1.0   # temporal.py:438-439
    want = (G / T) @ V
    np.testing.assert_allclose(out[0].cpu().numpy(), want, rtol=2e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dt,tol", DTYPES)
@pytest.mark.parametrize("R_,C,I", [(37, 32, 300), (260, 128, 2701), (130, 64, 5200), (300, 256, 1500),
                                    # num_units = 512: every published recipe (runme.sh:15-115); 17772 = Netflix's table rows
                                    (300, 512, 1500), (3072, 512, 17772), (70, 256, 700)])
def test_score_ce_fwd_bwd(name, dt, tol, R_, C, I):
    o = ops()
    rng = np.random.default_rng(R_)
    rows = torch.tensor(_rand((R_, C), rng, 0.5), dtype=dt).cuda().requires_grad_()
    tab = torch.tensor(_rand((I, C), rng, 0.3), dtype=torch.float32).cuda().requires_grad_()
    tab_c = tab.detach().to(dt)
    bias = torch.tensor(_rand((I - 1,), rng, 0.2), dtype=torch.float32).cuda().requires_grad_()
    labels = rng.integers(0, I, size=R_)
    labels[:3] = 0
    labels[rng.random(R_) < 0.4] = 0          # weight-0 rows (masked positions on padding) are compacted away
    lab = torch.tensor(labels, dtype=torch.int64).cuda()
    loss = o.ScoreCEFn.apply(rows, tab, bias, tab_c, lab)
    (loss * 1.7).backward()
    rr = rows.detach().double().cpu().requires_grad_()
    tr = tab_c.double().cpu().requires_grad_()
    br = bias.detach().double().cpu().requires_grad_()
    logits = rr @ R.zero_padded(tr).t() + torch.cat([torch.full((1,), -1000.0, dtype=torch.float64), br])
    lp = torch.log(torch.softmax(logits, -1) + 1e-5)
    wgt = (torch.tensor(labels) != 0).double()
    ref = (wgt * -lp[torch.arange(R_), torch.tensor(labels)]).sum() / (wgt.sum() + 1e-5)
    (ref * 1.7).backward()
    assert_close(loss.item(), ref.item(), 2e-5 if name == "f32" else 5e-3, "ce loss")
    gt = 1e-4 if name == "f32" else 3e-2
    assert_close(rows.grad.float().cpu().numpy(), rr.grad.numpy(), gt, "d_rows")
    assert_close(tab.grad.cpu().numpy(), tr.grad.numpy(), gt, "d_table")
    assert_close(bias.grad.cpu().numpy(), br.grad.numpy(), gt, "d_bias")
    assert float(tab.grad[0].abs().max()) == 0.0
    # materialised logits path (EasyDGL.py:149-151)
    lg = o.ScoreLogitsFn.apply(rows.detach(), tab.detach(), bias.detach(), tab_c)
    assert_close(lg.cpu().numpy(), logits.detach().numpy(), 1e-5 if name == "f32" else 1e-5, "logits")
    assert float((lg[:, 0] + 1000.0).abs().max()) == 0.0


@pytest.mark.parametrize("R_,frac", [(1, 0.0), (7, 1.0), (1000, 0.5), (5000, 0.0), (10240, 0.47)])
def test_compact_rows_is_a_stable_partition(R_, frac):
    o = ops()
    rng = np.random.default_rng(R_)
    C = 32
    rows = torch.tensor(_rand((R_, C), rng), dtype=torch.bfloat16).cuda()
    labels = rng.integers(1, 900, size=R_)
    labels[rng.random(R_) < frac] = 0
    lab = torch.tensor(labels, dtype=torch.int64).cuda()
    rows_c, lab_c, perm, inv, nvalid = o.compact_rows(rows, lab)
    keep = np.nonzero(labels)[0]
    n = len(keep)
    assert int(nvalid.item()) == n
    np.testing.assert_array_equal(perm.cpu().numpy()[:n], keep)
    assert (perm.cpu().numpy()[n:] == -1).all()
    want_inv = np.full(R_, -1)
    want_inv[keep] = np.arange(n)
    np.testing.assert_array_equal(inv.cpu().numpy(), want_inv)
    np.testing.assert_array_equal(lab_c.cpu().numpy()[:n], labels[keep])
    assert (lab_c.cpu().numpy()[n:] == 0).all()
    assert torch.equal(rows_c[:n], rows[torch.tensor(keep, dtype=torch.int64).cuda()])
    assert float(rows_c[n:].float().abs().sum()) == 0.0


def test_score_ce_all_rows_unweighted_gives_zero_loss_and_grads():
    o = ops()
    rng = np.random.default_rng(3)
    rows = torch.tensor(_rand((40, 32), rng), dtype=torch.float32).cuda().requires_grad_()
    tab = torch.tensor(_rand((200, 32), rng), dtype=torch.float32).cuda().requires_grad_()
    bias = torch.zeros(199).cuda().requires_grad_()
    lab = torch.zeros(40, dtype=torch.int64).cuda()
    loss = o.ScoreCEFn.apply(rows, tab, bias, tab.detach(), lab)
    loss.backward()
    assert loss.item() == 0.0
    assert float(rows.grad.abs().max()) == 0.0 and float(tab.grad.abs().max()) == 0.0 and float(bias.grad.abs().max()) == 0.0


@pytest.mark.parametrize("name,dt,tol", DTYPES)
def test_layernorm_gather_with_repeated_positions(name, dt, tol):
    """Base.py mask_random pads masked_positions with 0: several gathered rows may name one position; grads add."""
    o = ops()
    rng = np.random.default_rng(11)
    B, T, C, M = 4, 13, 32, 6
    x = torch.tensor(_rand((B, T, C), rng), dtype=dt).cuda().requires_grad_()
    g = torch.tensor(1 + 0.1 * _rand((C,), rng), dtype=torch.float32).cuda().requires_grad_()
    be = torch.tensor(0.1 * _rand((C,), rng), dtype=torch.float32).cuda().requires_grad_()
    gp_np = rng.integers(0, T, size=(B, M))
    gp_np[:, 3:] = 0
    gp_np[1, 0] = 0
    gp = torch.tensor(gp_np, dtype=torch.int64).cuda()
    y = o.AddLayerNormFn.apply(x, None, g, be, o.NO_DROP, gp)
    dy = torch.tensor(_rand(tuple(y.shape), rng), dtype=dt).cuda()
    y.backward(dy)
    xr = x.detach().double().cpu().requires_grad_()
    gr, ber = g.detach().double().cpu().requires_grad_(), be.detach().double().cpu().requires_grad_()
    yr = R.layernorm(xr, gr, ber)[torch.arange(B)[:, None], gp.cpu()].reshape(-1, C)
    yr.backward(dy.double().cpu())
    assert_close(y.detach().float().cpu().numpy(), yr.detach().numpy(), tol, "ln y")
    assert_close(x.grad.float().cpu().numpy(), xr.grad.numpy(), tol * 3, "ln dx")
    assert_close(g.grad.cpu().numpy(), gr.grad.numpy(), tol * 3, "ln dgamma")
    assert_close(be.grad.cpu().numpy(), ber.grad.numpy(), tol * 3, "ln dbeta")


def test_topk_ties_masking_merge_and_metrics():
    o = ops()
    rng = np.random.default_rng(4)
    R_, n, K, T = 9, 3000, 100, 12
    x = rng.standard_normal((R_, n)).astype(np.float32)
    x[0, :] = 0.5                      # all ties -> lowest indices
    x[1, 100:400] = 7.0                # 300-way tie at the top
    x[2, 5] = np.inf
    seen = rng.integers(0, n, size=(R_, T))
    seen[3, :] = np.argsort(-x[3])[:T]  # mask exactly the current top-T of row 3
    want_x = x.copy()
    want_x[np.arange(R_)[:, None], seen] = -np.inf
    want = O.top_k(want_x, K)
    val, idx = o.mask_topk(torch.tensor(x).cuda(), 0, torch.tensor(seen).cuda(), K)
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    np.testing.assert_array_equal(val.cpu().numpy(), np.take_along_axis(want_x, want, 1))
    # sharded: 4 contiguous shards, local top-K with global ids, merged (K7)
    S = 4
    bounds = np.linspace(0, n, S + 1).astype(int)
    cv, ci = [], []
    for s in range(S):
        lo, hi = bounds[s], bounds[s + 1]
        v, i = o.mask_topk(torch.tensor(x[:, lo:hi].copy()).cuda(), int(lo), torch.tensor(seen).cuda(), K)
        cv.append(v); ci.append(i)
    mv, mi = o.topk_merge(torch.stack(cv), torch.stack(ci))
    np.testing.assert_array_equal(mi.cpu().numpy(), want)
    # metrics (Base.py:181-201)
    labels = np.array([want[r, r * 11 % K] for r in range(R_)])
    labels[4] = n - 1 if (n - 1) not in want[4] else n - 2
    met = torch.zeros(6).cuda()
    o.rank_metrics(idx, torch.tensor(labels).cuda(), met)
    per = O.ranking_metrics(want, labels)
    np.testing.assert_allclose(met.cpu().numpy(), [per[k].sum() for k in ("H10", "H50", "H100", "N10", "N50", "N100")], rtol=1e-5)


def test_tpp_regulariser_fwd_bwd():
    o = ops()
    rng = np.random.default_rng(2)
    B, T, H, E, M, NI = 5, 14, 2, 4, 3, 30
    lam = torch.tensor(rng.uniform(0.2, 2.0, size=(H * B, T, E)), dtype=torch.float32).cuda().requires_grad_()
    mp = torch.tensor(np.stack([rng.choice(T - 1, M, replace=False) + 1 for _ in range(B)])).cuda()
    labels = rng.integers(1, NI, size=(B, M)); labels[0, 0] = 0
    ts = np.cumsum(rng.exponential(40.0, size=(B, T)), axis=1).astype(np.float32) + 9.5e8
    mt = O.synthetic_mark_table(NI, E, multi_hot=True)
    coef = 0.37
    reg = o.TppFn.apply(lam, mp, torch.tensor(labels).cuda(), torch.tensor(ts).cuda(),
                        torch.tensor(mt.astype(np.uint8)).cuda(), H, coef)
    (reg * 2.0).backward()
    lr = lam.detach().double().cpu().requires_grad_()
    sp = torch.tensor(O.spans_from_times(ts))[torch.arange(B)[:, None], mp.cpu()].repeat(H, 1)
    nm = torch.tensor(mt[labels], dtype=torch.float64).repeat(H, 1, 1)
    lg = lr[torch.arange(H * B)[:, None], mp.cpu().repeat(H, 1)]
    ref = coef * R.biased_likelihood(lg, nm, sp)
    (ref * 2.0).backward()
    assert_close(reg.item(), ref.item(), 1e-5, "tpp reg")
    assert_close(lam.grad.cpu().numpy(), lr.grad.numpy(), 1e-5, "tpp dlam")


@pytest.mark.parametrize("repeat", [False, True])
def test_tpp_fused_launch_matches_the_reference(repeat):
    """edgl_tpp_fwd_bwd (regulariser, its sums and the FULL d lambda in one launch, the engine's form) against the fp64 oracle:
    rows of unmasked positions are zero without a memset, and a masked position that occurs twice in a sample (padding
    slots repeat position 0) receives the SUM of its slots' gradients — the gradient of tf.gather (EasyDGL.py:157-175)."""
    from easydgl_amd import _lib
    lib = _lib.lib
    rng = np.random.default_rng(12)
    B, T, H, E, M, NI = 6, 21, 3, 5, 4, 40
    lam = torch.tensor(rng.uniform(0.2, 2.0, size=(H * B, T, E)), dtype=torch.float32).cuda()
    mpn = np.stack([rng.choice(T - 1, M, replace=False) + 1 for _ in range(B)])
    labels = rng.integers(1, NI, size=(B, M)); labels[0, 0] = 0
    if repeat:
        mpn[1, 2] = mpn[1, 0]          # the same position twice, two different labels
        mpn[2, 3] = mpn[2, 1]; labels[2, 3] = 0   # ... and once as a zero-weight padding slot
    mp = torch.tensor(mpn).cuda()
    ts = np.cumsum(rng.exponential(40.0, size=(B, T)), axis=1).astype(np.float32) + 9.5e8
    mt = O.synthetic_mark_table(NI, E, multi_hot=True)
    coef = 0.41
    sums = torch.zeros(int(lib.edgl_tpp_workspace()), device="cuda")
    reg = torch.full((1,), 3.0, device="cuda")
    dlam = torch.full((H * B, T, E), float("nan"), device="cuda")
    lab_t, ts_t, mt_t = torch.tensor(labels).cuda(), torch.tensor(ts).cuda(), torch.tensor(mt.astype(np.uint8)).cuda()
    for _ in range(2):   # twice: the ticket of the last-workgroup reduction must come back to zero
        reg.fill_(3.0)
        _lib.check(lib.edgl_tpp_fwd_bwd(lam.data_ptr(), mp.data_ptr(), lab_t.data_ptr(), ts_t.data_ptr(), mt_t.data_ptr(), B, T, H, E,
                                        M, coef, sums.data_ptr(), reg.data_ptr(), 1, dlam.data_ptr(), None), "edgl_tpp_fwd_bwd")
    torch.cuda.synchronize()
    lr = lam.double().cpu().requires_grad_()
    sp = torch.tensor(O.spans_from_times(ts))[torch.arange(B)[:, None], mp.cpu()].repeat(H, 1)
    nm = torch.tensor(mt[labels], dtype=torch.float64).repeat(H, 1, 1)
    lg = lr[torch.arange(H * B)[:, None], mp.cpu().repeat(H, 1)]
    ref = coef * R.biased_likelihood(lg, nm, sp)
    ref.backward()
    assert_close(reg.item() - 3.0, ref.item(), 1e-5, "tpp reg (accumulated)")
    assert_close(dlam.cpu().numpy(), lr.grad.numpy(), 1e-5, "tpp dlam (dense)")


@pytest.mark.parametrize("E,M,repeat", [(5, 4, False), (5, 4, True), (16, 20, True), (16, 300, False), (20, 4, False), (20, 4, True)])
def test_tpp_rows_launch_matches_the_reference(E, M, repeat):
    """edgl_tpp_norm + edgl_tpp_fwd_bwd_rows (the engine's form: one thread per masked slot, d lambda pre-zeroed by
    edgl_bimau_fwd_zr — here by the test) against the fp64 oracle: rows of unmasked positions stay zero, a position drawn into two
    slots gets the sum of its slots' gradients exactly once (EasyDGL.py:157-175), M = 300 slots per sample crosses workgroups,
    E = 20 marks takes the plain-loop kernel for more than 16 marks."""
    from easydgl_amd import _lib
    lib = _lib.lib
    rng = np.random.default_rng(12 + E + M)
    B, T, H, NI = 6, max(21, M + 5), 3, 40
    lam = torch.tensor(rng.uniform(0.2, 2.0, size=(H * B, T, E)), dtype=torch.float32).cuda()
    mpn = np.stack([rng.choice(T - 1, M, replace=False) + 1 for _ in range(B)])
    labels = rng.integers(1, NI, size=(B, M)); labels[0, 0] = 0
    if repeat:
        mpn[1, 2] = mpn[1, 0]          # the same position twice, two different labels
        mpn[2, 3] = mpn[2, 1]; labels[2, 3] = 0   # ... and once as a zero-weight padding slot
        mpn[3, :3] = 0; labels[3, :3] = 0          # padding slots all on position 0
    mp = torch.tensor(mpn).cuda()
    ts = np.cumsum(rng.exponential(40.0, size=(B, T)), axis=1).astype(np.float32) + 9.5e8
    mt = O.synthetic_mark_table(NI, E, multi_hot=True)
    coef = 0.41
    sums = torch.zeros(int(max(lib.edgl_tpp_workspace(), lib.edgl_tpp_rows_workspace(B, H, M))), device="cuda")
    reg = torch.full((1,), 3.0, device="cuda")
    dlam = torch.zeros((H * B, T, E), device="cuda")
    lab_t, ts_t, mt_t = torch.tensor(labels).cuda(), torch.tensor(ts).cuda(), torch.tensor(mt.astype(np.uint8)).cuda()
    for _ in range(2):   # twice: the normaliser accumulator must come back to zero
        reg.fill_(3.0); dlam.zero_()
        _lib.check(lib.edgl_tpp_norm(lab_t.data_ptr(), mt_t.data_ptr(), B, M, E, sums.data_ptr(), None), "edgl_tpp_norm")
        _lib.check(lib.edgl_tpp_fwd_bwd_rows(lam.data_ptr(), mp.data_ptr(), lab_t.data_ptr(), ts_t.data_ptr(), mt_t.data_ptr(), B, T, H,
                                             E, M, coef, sums.data_ptr(), reg.data_ptr(), 1, dlam.data_ptr(), None), "edgl_tpp_fwd_bwd_rows")
    torch.cuda.synchronize()
    lr = lam.double().cpu().requires_grad_()
    sp = torch.tensor(O.spans_from_times(ts))[torch.arange(B)[:, None], mp.cpu()].repeat(H, 1)
    nm = torch.tensor(mt[labels], dtype=torch.float64).repeat(H, 1, 1)
    lg = lr[torch.arange(H * B)[:, None], mp.cpu().repeat(H, 1)]
    ref = coef * R.biased_likelihood(lg, nm, sp)
    ref.backward()
    assert_close(reg.item() - 3.0, ref.item(), 1e-5, "tpp reg (accumulated)")
    assert_close(dlam.cpu().numpy(), lr.grad.numpy(), 1e-5, "tpp dlam (rows form)")


def test_tpp_rows_launch_skips_masked_positions_outside_the_sequence():
    """A masked position outside [0, T) (malformed input) is a skipped slot, not an out-of-bounds row of lambda / d lambda: guard
    bands around d lambda stay untouched and the in-range slots of the other samples get the gradient of the clean problem."""
    from easydgl_amd import _lib
    lib = _lib.lib
    rng = np.random.default_rng(77)
    B, T, H, NI, E, M = 4, 23, 2, 40, 16, 5
    lam = torch.tensor(rng.uniform(0.2, 2.0, size=(H * B, T, E)), dtype=torch.float32).cuda()
    mpn = np.stack([rng.choice(T - 1, M, replace=False) + 1 for _ in range(B)])
    labels = rng.integers(1, NI, size=(B, M))
    bad = mpn.copy()
    bad[B - 1, 0] = T + 1000          # the last sample: a row far behind the arrays
    bad[0, 1] = -7                    # the first sample: a row in front of them
    ts = np.cumsum(rng.exponential(40.0, size=(B, T)), axis=1).astype(np.float32) + 9.5e8
    mt = O.synthetic_mark_table(NI, E, multi_hot=True)
    lab_t, ts_t, mt_t = torch.tensor(labels).cuda(), torch.tensor(ts).cuda(), torch.tensor(mt.astype(np.uint8)).cuda()
    n = H * B * T * E
    outs = []
    for pos in (mpn, bad):
        buf = torch.full((n + 2 * 4096,), 123.0, device="cuda")
        dlam = buf[4096:4096 + n].view(H * B, T, E)
        dlam.zero_()
        sums = torch.zeros(int(max(lib.edgl_tpp_workspace(), lib.edgl_tpp_rows_workspace(B, H, M))), device="cuda")
        reg = torch.zeros(1, device="cuda")
        _lib.check(lib.edgl_tpp_norm(lab_t.data_ptr(), mt_t.data_ptr(), B, M, E, sums.data_ptr(), None), "edgl_tpp_norm")
        _lib.check(lib.edgl_tpp_fwd_bwd_rows(lam.data_ptr(), torch.tensor(pos).cuda().data_ptr(), lab_t.data_ptr(), ts_t.data_ptr(),
                                             mt_t.data_ptr(), B, T, H, E, M, 0.3, sums.data_ptr(), reg.data_ptr(), 0, dlam.data_ptr(), None),
                   "edgl_tpp_fwd_bwd_rows")
        torch.cuda.synchronize()
        assert torch.all(buf[:4096] == 123.0) and torch.all(buf[4096 + n:] == 123.0)
        assert torch.isfinite(reg).all()
        outs.append(dlam.clone())
    clean, dirty = outs
    keep = torch.ones_like(clean, dtype=torch.bool)
    for h in range(H):                # rows the two skipped slots would have written
        keep[h * B + B - 1, mpn[B - 1, 0]] = False
        keep[h * B + 0, mpn[0, 1]] = False
    assert torch.equal(clean[keep], dirty[keep])
    assert torch.all(dirty[~keep] == 0)


def test_bimau_forward_zero_fills_the_d_lambda_buffer():
    """edgl_bimau_fwd_zr: same outputs as edgl_bimau_fwd, and the extra [H*B, T, E] array comes back all zero (head dims 16 and 64:
    fused kernel / memset in front of the three-launch form)."""
    from easydgl_amd import _lib
    lib = _lib.lib
    o = ops()
    rng = np.random.default_rng(3)
    for C, H, E, T in ((32, 2, 16, 19), (32, 2, 5, 19), (128, 2, 16, 23)):
        B = 3
        qkvt = torch.tensor(rng.standard_normal((B, T, 4 * C)) * 0.3, dtype=torch.bfloat16).cuda()
        resid = torch.tensor(rng.standard_normal((B, T, C)), dtype=torch.bfloat16).cuda()
        ids = torch.tensor(rng.integers(1, 30, size=(B, T))).cuda()
        spans = torch.tensor(rng.uniform(0, 5, size=(B, T)), dtype=torch.float32).cuda()
        marks = torch.tensor(O.synthetic_mark_table(30, E, multi_hot=True)[ids.cpu().numpy()].astype(np.uint8)).cuda()
        dh = C // H
        W1 = torch.tensor(rng.standard_normal((dh + 1, dh * E)) * 0.2, dtype=torch.float32).cuda()
        b1 = torch.zeros(dh * E, device="cuda"); w = torch.tensor(rng.standard_normal((E, dh)) * 0.3, dtype=torch.float32).cuda()
        sc = torch.zeros(E, device="cuda")
        code = o._code(qkvt)
        pack = torch.empty(lib.edgl_bimau_pack_bytes(C, H, E, code), device="cuda", dtype=torch.uint8)
        _lib.check(lib.edgl_bimau_pack(W1.data_ptr(), b1.data_ptr(), w.data_ptr(), sc.data_ptr(), C, H, E, pack.data_ptr(), code, None), "pack")
        saved = torch.empty(lib.edgl_bimau_saved_bytes(B, T, C, H, code), device="cuda", dtype=torch.uint8)
        outs = []
        for zr in (False, True):
            out = torch.empty((B, T, C), device="cuda", dtype=torch.bfloat16)
            lam = torch.empty((H * B, T, E), device="cuda")
            z = torch.full((H * B, T, E), float("nan"), device="cuda")
            if zr:
                _lib.check(lib.edgl_bimau_fwd_zr(qkvt.data_ptr(), resid.data_ptr(), C, ids.data_ptr(), spans.data_ptr(), marks.data_ptr(),
                                                 pack.data_ptr(), B, T, C, H, E, 0.0, None, 0, out.data_ptr(), lam.data_ptr(),
                                                 saved.data_ptr(), z.data_ptr(), 0, code, None), "edgl_bimau_fwd_zr")
            else:
                _lib.check(lib.edgl_bimau_fwd(qkvt.data_ptr(), resid.data_ptr(), C, ids.data_ptr(), spans.data_ptr(), marks.data_ptr(),
                                              pack.data_ptr(), B, T, C, H, E, 0.0, None, 0, out.data_ptr(), lam.data_ptr(),
                                              saved.data_ptr(), 0, code, None), "edgl_bimau_fwd")
            torch.cuda.synchronize()
            outs.append((out, lam, z))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        assert float(outs[1][2].abs().max()) == 0.0, (C, H, E)


@pytest.mark.parametrize("T", [19, 101, 128])
def test_stored_dropout_keep_bits_equal_the_hashed_masks(T):
    """edgl_bimau_dropbits + edgl_bimau_fwd_db / _bwd_db against the hashing kernels on the same (rng state, stream id): the stored
    bits ARE the hash decisions, so outputs, lambda, d_qkvt and the weight gradients are identical bit for bit (bf16, head dim 16,
    16 marks: the family with a stored-bits form; T = 101 is the benchmarked length, 128 the last supported one)."""
    from easydgl_amd import _lib
    lib = _lib.lib
    o = ops()
    rng = np.random.default_rng(5 + T)
    B, C, H, E, rate, sid = 3, 64, 4, 16, 0.3, 14
    dh = C // H
    qkvt = torch.tensor(rng.standard_normal((B, T, 4 * C)) * 0.4, dtype=torch.bfloat16).cuda()
    resid = torch.tensor(rng.standard_normal((B, T, C)), dtype=torch.bfloat16).cuda()
    ids = rng.integers(1, 30, size=(B, T)); ids[1, :5] = 0
    ids = torch.tensor(ids).cuda()
    spans = torch.tensor(rng.uniform(0, 5, size=(B, T)), dtype=torch.float32).cuda()
    marks = torch.tensor(O.synthetic_mark_table(30, E, multi_hot=True)[ids.cpu().numpy()].astype(np.uint8)).cuda()
    W1 = torch.tensor(rng.standard_normal((dh + 1, dh * E)) * 0.2, dtype=torch.float32).cuda()
    b1 = torch.tensor(rng.standard_normal(dh * E) * 0.1, dtype=torch.float32).cuda()
    w = torch.tensor(rng.standard_normal((E, dh)) * 0.3, dtype=torch.float32).cuda()
    sc = torch.zeros(E, device="cuda")
    d_out = torch.tensor(rng.standard_normal((B, T, C)), dtype=torch.bfloat16).cuda()
    d_lam = torch.tensor(rng.standard_normal((H * B, T, E)) * 0.01, dtype=torch.float32).cuda()
    code = o._code(qkvt)
    state = o.make_rng_state("cuda", seed=77)
    o.rng_advance(state)
    pack = torch.empty(lib.edgl_bimau_pack_bytes(C, H, E, code), device="cuda", dtype=torch.uint8)
    _lib.check(lib.edgl_bimau_pack(W1.data_ptr(), b1.data_ptr(), w.data_ptr(), sc.data_ptr(), C, H, E, pack.data_ptr(), code, None), "pack")
    nbits = int(lib.edgl_bimau_dropbits_bytes(B, T, H))
    assert nbits == B * H * ((T + 15) // 16) * 64 * 4
    bits = torch.zeros(nbits // 4, device="cuda", dtype=torch.int32)
    _lib.check(lib.edgl_bimau_dropbits(B, T, H, rate, state.data_ptr(), sid, bits.data_ptr(), None), "edgl_bimau_dropbits")
    # the keep rate of the stored bits (rows / keys inside the sequence)
    nt = (T + 15) // 16
    wds = bits.view(H * B, nt, 64).cpu().numpy().astype(np.uint32)
    keep = np.zeros((H * B, nt * 16, nt * 16), bool)
    for lane in range(64):
        for kt in range(nt):
            for r in range(4):
                keep[:, np.arange(nt) * 16 + (lane & 15), kt * 16 + (lane >> 4) * 4 + r] = (wds[:, :, lane] >> (kt * 4 + r)) & 1
    frac = keep[:, :T, :T].mean()
    assert abs(frac - (1 - rate)) < 0.01, frac
    res = []
    for db in (None, bits):
        out = torch.empty((B, T, C), device="cuda", dtype=torch.bfloat16)
        lam = torch.empty((H * B, T, E), device="cuda")
        saved = torch.empty(lib.edgl_bimau_saved_bytes(B, T, C, H, code), device="cuda", dtype=torch.uint8)
        _lib.check(lib.edgl_bimau_fwd_db(qkvt.data_ptr(), resid.data_ptr(), C, ids.data_ptr(), spans.data_ptr(), marks.data_ptr(),
                                         pack.data_ptr(), B, T, C, H, E, rate, state.data_ptr(), sid, None if db is None else db.data_ptr(),
                                         0.0, out.data_ptr(), lam.data_ptr(), saved.data_ptr(), None, 0, code, None), "edgl_bimau_fwd_db")
        dq = torch.empty_like(qkvt)
        n1, n2, n3 = (dh + 1) * dh * E, dh * E, E * dh
        g = torch.empty(n1 + n2 + n3 + E, device="cuda")
        ws = torch.empty(lib.edgl_bimau_bwd_workspace(B, T, C, H, E, code), device="cuda", dtype=torch.uint8)
        _lib.check(lib.edgl_bimau_bwd_db(qkvt.data_ptr(), ids.data_ptr(), spans.data_ptr(), marks.data_ptr(), pack.data_ptr(),
                                         d_out.data_ptr(), d_lam.data_ptr(), lam.data_ptr(), saved.data_ptr(), B, T, C, H, E, rate,
                                         state.data_ptr(), sid, None if db is None else db.data_ptr(), 0.0, dq.data_ptr(), g.data_ptr(),
                                         g[n1:].data_ptr(), g[n1 + n2:].data_ptr(), g[n1 + n2 + n3:].data_ptr(), ws.data_ptr(), 0, code, None),
                   "edgl_bimau_bwd_db")
        torch.cuda.synchronize()
        res.append((out, lam, dq, g))
    undropped = torch.empty((B, T, C), device="cuda", dtype=torch.bfloat16)
    lam0 = torch.empty((H * B, T, E), device="cuda")
    _lib.check(lib.edgl_bimau_fwd(qkvt.data_ptr(), resid.data_ptr(), C, ids.data_ptr(), spans.data_ptr(), marks.data_ptr(),
                                  pack.data_ptr(), B, T, C, H, E, 0.0, None, 0, undropped.data_ptr(), lam0.data_ptr(), None, 0, code, None), "fwd")
    assert not torch.equal(res[0][0], undropped)              # dropout is on
    for a, b_, what in zip(res[0], res[1], ("out", "lambda", "d_qkvt", "weight gradients")):
        assert torch.equal(a, b_), what


def test_tpp_fused_launch_all_position_mode():
    """edgl_tpp_fwd_bwd without masked positions (CTSMA's form: every position scored, T + 1 raw timestamps per row) against
    the separate forward / backward kernels behind TppFn."""
    from easydgl_amd import _lib
    lib = _lib.lib
    o = ops()
    rng = np.random.default_rng(21)
    B, T, H, E, NI = 5, 37, 2, 16, 50
    lam = torch.tensor(rng.uniform(0.2, 2.0, size=(H * B, T, E)), dtype=torch.float32).cuda()
    labels = torch.tensor(rng.integers(0, NI, size=(B, T))).cuda()
    ts = torch.tensor(np.cumsum(rng.exponential(40.0, size=(B, T + 1)), axis=1).astype(np.float32) + 9.5e8).cuda()
    mt = torch.tensor(O.synthetic_mark_table(NI, E, multi_hot=True).astype(np.uint8)).cuda()
    coef = 0.23
    lam_a = lam.clone().requires_grad_()
    reg_ref = o.TppFn.apply(lam_a, None, labels, ts, mt, H, coef)
    reg_ref.backward()
    sums = torch.zeros(int(lib.edgl_tpp_workspace()), device="cuda")
    reg = torch.zeros(1, device="cuda")
    dlam = torch.full((H * B, T, E), float("nan"), device="cuda")
    _lib.check(lib.edgl_tpp_fwd_bwd(lam.data_ptr(), None, labels.data_ptr(), ts.data_ptr(), mt.data_ptr(), B, T, H, E, T, coef,
                                    sums.data_ptr(), reg.data_ptr(), 0, dlam.data_ptr(), None), "edgl_tpp_fwd_bwd")
    torch.cuda.synchronize()
    assert_close(reg.item(), reg_ref.item(), 1e-5, "tpp reg, all positions")
    assert_close(dlam.cpu().numpy(), lam_a.grad.cpu().numpy(), 1e-5, "tpp dlam, all positions")


def test_adam_matches_tf_form():
    o = ops()
    rng = np.random.default_rng(6)
    n = 1000
    w0, g = rng.standard_normal(n), rng.standard_normal(n) * 0.1
    w = torch.tensor(w0, dtype=torch.float32).cuda()
    m = torch.zeros(n).cuda(); v = torch.zeros(n).cuda()
    st = torch.zeros(2, dtype=torch.int64).cuda()
    shadow = torch.empty(n, dtype=torch.bfloat16).cuda()
    wn, mn, vn = w0.copy(), np.zeros(n), np.zeros(n)
    for t in range(1, 5):
        gt = torch.tensor(g * t, dtype=torch.float32).cuda()
        o.adam_step(w, gt, m, v, 1e-2, st, 0.0, None, shadow)
        wn, mn, vn = O.adam_tf(wn, np.float32(g * t).astype(np.float64), mn, vn, t, 1e-2)
    assert int(st[0]) == 4
    assert_close(w.cpu().numpy(), wn, 2e-6, "adam w")
    assert_close(shadow.float().cpu().numpy(), wn, 5e-3, "adam shadow")


@pytest.mark.parametrize("E", [16, 5])
def test_tpp_norm_counts_the_marks_of_a_large_batch_exactly(E):
    """edgl_tpp_norm at B * M = 258 * 255 = 65 790 labels (more than one workgroup's 65 536: memset + integer atomics): sums[4], read
    as an int, is the numpy sum of the labels' mark bytes — exactly, and again on a second call (the count is formed from zero)."""
    from easydgl_amd import _lib
    lib = _lib.lib
    rng = np.random.default_rng(40 + E)
    B, M, NI = 258, 255, 40
    mt = O.synthetic_mark_table(NI, E, multi_hot=True).astype(np.uint8)
    labels = rng.integers(0, NI, size=(B, M))
    want = int(mt[labels].astype(np.int64).sum())
    assert want > 0
    lab_t, mt_t = torch.tensor(labels).cuda(), torch.tensor(mt).cuda()
    sums = torch.zeros(8, device="cuda")
    for _ in range(2):
        _lib.check(lib.edgl_tpp_norm(lab_t.data_ptr(), mt_t.data_ptr(), B, M, E, sums.data_ptr(), None), "edgl_tpp_norm")
        torch.cuda.synchronize()
        assert int(sums.view(torch.int32)[4]) == want


@pytest.mark.parametrize("entry", ["apply", "apply_l2p", "apply_ex"])
def test_adam_apply_forms_match_tf_form_with_l2_segments(entry):
    """edgl_adam_apply / _l2p / _ex against O.adam_tf with the l2 term on five segments (more than the four the vector path of
    edgl_adam_apply_ex keeps in registers), n = 4099 (not a multiple of 4), three steps, the bounds of test_adam_matches_tf_form.
    _l2p / _ex: l2_part sums to the sum of squares of the updated weights over the segments.  _ex also: the gradient is
    grad + the slabs of two ranges (one 4-aligned with zero_first, one of odd stride), the ranges are zero afterwards, and the next
    step's counters land in the second pair of buffers."""
    from easydgl_amd import _lib
    lib = _lib.lib
    rng = np.random.default_rng(16)
    n, lr, l2, b1, b2, eps = 4099, 1e-2, 0.01, 0.9, 0.999, 1e-8
    segs = np.array([[0, 500], [600, 601], [1000, 2047], [2050, 3000], [4000, 4099]])
    in_seg = np.zeros(n, dtype=bool)
    for lo, hi in segs:
        in_seg[lo:hi] = True
    w0, g0 = rng.standard_normal(n), rng.standard_normal(n) * 0.1
    w = torch.tensor(w0, dtype=torch.float32).cuda()
    m, v = torch.zeros(n).cuda(), torch.zeros(n).cuda()
    shadow = torch.empty(n, dtype=torch.bfloat16).cuda()
    seg = torch.tensor(segs).cuda()
    l2p = torch.full((int(lib.edgl_adam_l2_parts(n)),), float("nan"), device="cuda")
    state = [torch.zeros(2, dtype=torch.int64).cuda(), torch.zeros(2, dtype=torch.int64).cuda()]
    rngs = [torch.tensor([1234, 7]).cuda(), torch.zeros(2, dtype=torch.int64).cuda()]
    (lo_a, hi_a, zf), (lo_b, hi_b), ns = (1024, 1536, 4), (3001, 3078), 3
    slab_a, slab_b = rng.standard_normal((ns, hi_a - lo_a)) * 0.1, rng.standard_normal((ns, hi_b - lo_b)) * 0.1
    sa_t, sb_t = torch.tensor(slab_a, dtype=torch.float32).cuda(), torch.tensor(slab_b, dtype=torch.float32).cuda()
    wn, mn, vn = np.float32(w0).astype(np.float64), np.zeros(n), np.zeros(n)
    if entry == "apply_ex":
        _lib.check(lib.edgl_step_begin(rngs[0].data_ptr(), state[0].data_ptr(), lr, b1, b2, None), "edgl_step_begin")
    for t in range(1, 4):
        gt = torch.tensor(g0 * t, dtype=torch.float32).cuda()
        gr = np.float32(g0 * t).astype(np.float64)
        if entry == "apply_ex":
            gr[lo_a + zf:hi_a] += np.float32(slab_a).astype(np.float64).sum(0)[zf:]
            gr[lo_b:hi_b] += np.float32(slab_b).astype(np.float64).sum(0)
            _lib.check(lib.edgl_adam_apply_ex(w.data_ptr(), gt.data_ptr(), m.data_ptr(), v.data_ptr(), n, b1, b2, eps, state[0].data_ptr(), l2,
                                              seg.data_ptr(), len(segs), shadow.data_ptr(), l2p.data_ptr(),
                                              sa_t.data_ptr(), hi_a - lo_a, lo_a, hi_a, zf, sb_t.data_ptr(), hi_b - lo_b, lo_b, hi_b, ns,
                                              rngs[0].data_ptr(), state[1].data_ptr(), rngs[1].data_ptr(), lr, None), "edgl_adam_apply_ex")
            torch.cuda.synchronize()
            gz = gt.cpu().numpy()
            assert not gz[lo_a:hi_a].any() and not gz[lo_b:hi_b].any()          # the consumed ranges start the next step at zero
            keep = np.ones(n, dtype=bool); keep[lo_a:hi_a] = False; keep[lo_b:hi_b] = False
            np.testing.assert_array_equal(gz[keep], np.float32(g0 * t)[keep])
            # the next step's counters are in the second buffers; the pair this launch read is unchanged
            assert rngs[1].tolist() == [1234, 7 + t + 1] and rngs[0].tolist() == [1234, 7 + t]
            assert int(state[1][0]) == t + 1 and int(state[0][0]) == t
            # (in double on the betas as the C ABI passes them, floats: 1 - b2^t magnifies the rounding of 0.999 to 7e-6)
            fb1, fb2, flr = float(np.float32(b1)), float(np.float32(b2)), float(np.float32(lr))
            lr_next = flr * math.sqrt(1 - fb2 ** (t + 1)) / (1 - fb1 ** (t + 1))
            assert_close(float(state[1][1:].view(torch.float32)[0]), lr_next, 2e-6, "next step's learning rate")
            state.reverse(); rngs.reverse()
        else:
            _lib.check(lib.edgl_step_begin(rngs[0].data_ptr(), state[0].data_ptr(), lr, b1, b2, None), "edgl_step_begin")
            if entry == "apply":
                _lib.check(lib.edgl_adam_apply(w.data_ptr(), gt.data_ptr(), m.data_ptr(), v.data_ptr(), n, b1, b2, eps, state[0].data_ptr(), l2,
                                               seg.data_ptr(), len(segs), shadow.data_ptr(), None), "edgl_adam_apply")
            else:
                _lib.check(lib.edgl_adam_apply_l2p(w.data_ptr(), gt.data_ptr(), m.data_ptr(), v.data_ptr(), n, b1, b2, eps,
                                                   state[0].data_ptr(), l2, seg.data_ptr(), len(segs), shadow.data_ptr(), l2p.data_ptr(), None),
                           "edgl_adam_apply_l2p")
        gr[in_seg] += l2 * wn[in_seg]
        wn, mn, vn = O.adam_tf(wn, gr, mn, vn, t, lr)
    torch.cuda.synchronize()
    assert_close(w.cpu().numpy(), wn, 2e-6, "adam w")
    assert_close(shadow.float().cpu().numpy(), wn, 5e-3, "adam shadow")
    if entry != "apply":
        assert_close(float(l2p.double().sum()), float((wn[in_seg] ** 2).sum()), 2e-6, "sum of squares over the l2 segments")


def test_dropout_is_consistent_between_forward_and_backward():
    o = ops()
    B, T, C = 6, 50, 64
    x = torch.randn((B, T, C), device="cuda").requires_grad_()
    g = torch.ones(C, device="cuda"); b = torch.zeros(C, device="cuda")
    st = torch.tensor([1234, 7], dtype=torch.int64).cuda()
    drop = o.Drop(0.25, st, 3)
    y1 = o.AddLayerNormFn.apply(x, None, g, b, drop, None)
    y2 = o.AddLayerNormFn.apply(x, None, g, b, drop, None)
    assert torch.equal(y1, y2)                       # same (seed, step, stream) -> same mask
    o.rng_advance(st)
    y3 = o.AddLayerNormFn.apply(x, None, g, b, drop, None)
    assert not torch.equal(y1, y3)                   # next step -> new mask
    (y3 * torch.randn_like(y3)).sum().backward()
    # gradient w.r.t. x is exactly zero where the element was dropped; keep-rate ~ 0.75
    zero_frac = float((x.grad == 0).float().mean())
    assert abs(zero_frac - 0.25) < 0.02


@pytest.mark.parametrize("name,dt,tol", DTYPES)
@pytest.mark.parametrize("masked", [False, True])
def test_ff_tail_equals_dropout_add_mask(name, dt, tol, masked):
    """edgl_ff_tail == edgl_dropout -> edgl_add -> edgl_mask_rows with the same counter-based mask, forward and backward."""
    o = ops()
    rng = np.random.default_rng(3)
    B, T, C = 5, 13, 32
    a0, b0 = torch.tensor(_rand((B, T, C), rng), dtype=dt).cuda(), torch.tensor(_rand((B, T, C), rng), dtype=dt).cuda()
    ids = torch.tensor(rng.integers(0, 3, size=(B, T))).cuda() if masked else None
    state = torch.tensor([11, 4], dtype=torch.int64, device="cuda")
    drop = o.Drop(0.3, state, 9)
    g = torch.tensor(_rand((B, T, C), rng), dtype=dt).cuda()
    outs = []
    for fused in (True, False):
        a, b = a0.clone().requires_grad_(), b0.clone().requires_grad_()
        if fused:
            y = o.ff_tail(a, b, ids, drop)
        else:
            y = o.add(o.dropout(a, drop), b)
            if masked:
                y = o.mask_rows(y, ids)
        y.backward(g)
        outs.append((y.detach(), a.grad, b.grad))
    for u, v in zip(*outs):
        # same mask (zero pattern); values agree to one rounding: the fused kernel contracts x*scale + b into one fma and, in
        # bf16, rounds once where the unfused chain rounds after the dropout and again after the add
        assert torch.equal(u == 0, v == 0)
        assert_close(u.float().cpu().numpy(), v.float().cpu().numpy(), 1e-6 if name == "f32" else 1e-2, "fused vs unfused")
    if masked:
        assert float((outs[0][0] == 0).float().mean()) > 0.3      # a third of the rows carries id 0
    assert float((outs[0][1] == 0).float().mean()) > 0.2          # the dropout zeroes ~30 % of d_a


@pytest.mark.parametrize("name,dt,tol", DTYPES)
@pytest.mark.parametrize("R_,C,I", [(300, 128, 2701), (700, 64, 20001), (130, 256, 1500), (260, 512, 3000)])
def test_score_flash_matches_the_two_pass_kernels(name, dt, tol, R_, C, I):
    """edgl_score_flash_fwd / _bwd (one pass gives the row log-sum-exp AND the unnormalised row gradients, flash-style running
    maxima) against edgl_score_lse_fwd + edgl_score_ce_bwd on the same operands: lse, label logits, d_rows, d_table, d_bias."""
    from easydgl_amd._lib import check, lib
    o = ops()
    rng = np.random.default_rng(R_ + C)
    rows = torch.tensor(_rand((R_, C), rng, 0.6), dtype=dt).cuda()
    tab_c = torch.tensor(_rand((I, C), rng, 0.4), dtype=dt).cuda()
    bias = torch.tensor(_rand((I - 1,), rng, 0.3), dtype=torch.float32).cuda()
    labels = rng.integers(0, I, size=R_)
    labels[rng.random(R_) < 0.3] = 0
    rows_c, lab_c, _perm, _inv, nvalid = o.compact_rows(rows, torch.tensor(labels, dtype=torch.int64).cuda())
    code = o._code(rows)
    p, st = o._ptr, o._stream()
    # two-pass path
    lse0, ll0, _ = o.score_lse(rows_c, tab_c, bias, lab_c, 0, I, nvalid=nvalid)
    loss = torch.empty(1, device="cuda"); coef = torch.empty(R_, device="cuda")
    check(lib.edgl_ce_loss_fwd(p(lse0), p(ll0), p(lab_c), R_, p(loss), p(coef), st))
    d_rows0 = torch.empty_like(rows_c); d_tab0 = torch.empty((I, C), device="cuda"); d_b0 = torch.empty(I - 1, device="cuda")
    ws = torch.empty(lib.edgl_score_bwd_workspace(R_, C, I, I, code), device="cuda")
    check(lib.edgl_score_ce_bwd(p(rows_c), p(tab_c), p(bias), p(lab_c), p(lse0), p(coef), None, R_, C, I, 0, I, p(nvalid), p(d_rows0),
                                p(d_tab0), p(d_b0), p(ws), code, st), "edgl_score_ce_bwd")
    # flash path
    wsf = torch.empty(lib.edgl_score_flash_workspace(R_, C, I, I, code), device="cuda")
    lse1 = torch.empty(R_, device="cuda"); ll1 = torch.zeros(R_, device="cuda")
    check(lib.edgl_score_flash_fwd(p(rows_c), p(tab_c), p(bias), p(lab_c), R_, C, I, 0, I, p(nvalid), p(lse1), p(ll1), p(wsf), code, st),
          "edgl_score_flash_fwd")
    d_rows1 = torch.empty_like(rows_c); d_tab1 = torch.empty((I, C), device="cuda"); d_b1 = torch.empty(I - 1, device="cuda")
    check(lib.edgl_score_flash_bwd(p(rows_c), p(tab_c), p(bias), p(lab_c), p(lse1), p(coef), None, R_, C, I, 0, I, p(nvalid), p(d_rows1),
                                   p(d_tab1), p(d_b1), p(wsf), code, st), "edgl_score_flash_bwd")
    n = int(nvalid.item())
    assert_close(lse1[:n].cpu().numpy(), lse0[:n].cpu().numpy(), 1e-6 if name == "f32" else 1e-5, "lse")
    assert torch.equal(ll0, ll1)
    # the flash form rounds exp(l - max) to the activation dtype and scales in f32 afterwards; the two-pass form rounds coef * p
    gt = 2e-5 if name == "f32" else 2e-2
    assert_close(d_rows1.float().cpu().numpy(), d_rows0.float().cpu().numpy(), gt, "d_rows")
    assert_close(d_tab1.cpu().numpy(), d_tab0.cpu().numpy(), 1e-6, "d_table (same kernel, same lse up to rounding)") if name == "f32" else None
    assert_close(d_b1.cpu().numpy(), d_b0.cpu().numpy(), 1e-5 if name == "f32" else 1e-3, "d_bias")
    # the forward that also writes the loss coefficients (row count = the compaction's): same lse / label logits, and the
    # coefficients of edgl_ce_loss_fwd computed from them; the loss kernel then runs with coef = NULL
    lse2 = torch.empty(R_, device="cuda"); ll2 = torch.zeros(R_, device="cuda"); coef2 = torch.full((R_,), 7.0, device="cuda")
    check(lib.edgl_score_flash_fwd_coef(p(rows_c), p(tab_c), p(bias), p(lab_c), R_, C, I, p(nvalid), p(lse2), p(ll2), p(coef2), p(wsf),
                                        code, st), "edgl_score_flash_fwd_coef")
    assert torch.equal(lse2, lse1) and torch.equal(ll2, ll1)
    coef1 = torch.empty(R_, device="cuda"); loss1 = torch.empty(1, device="cuda"); loss2 = torch.empty(1, device="cuda")
    check(lib.edgl_ce_loss_fwd(p(lse1), p(ll1), p(lab_c), R_, p(loss1), p(coef1), st))
    assert_close(coef2.cpu().numpy(), coef1.cpu().numpy(), 1e-6, "coef")
    assert float(coef2[n:].abs().max()) == 0.0 if n < R_ else True
    check(lib.edgl_ce_loss_fwd_add(p(lse1), p(ll1), p(lab_c), R_, p(loss2), None, None, None, st))
    assert float(loss1) == float(loss2)


def test_score_flash_fwd_pre_with_a_prepared_table_matches_flash_fwd():
    """edgl_score_prepare_table + edgl_score_flash_fwd_pre(table_ready = 1) against edgl_score_flash_fwd: the transposed table
    image written ahead of time is the one the forward writes itself (f32 — the dtype that reads it), so lse, label logits and
    the three gradients of the edgl_score_flash_bwd that follows are the same bits."""
    from easydgl_amd._lib import F32, check, lib
    o = ops()
    R_, C, I = 24, 32, 41
    rng = np.random.default_rng(5)
    rows = torch.tensor(_rand((R_, C), rng, 0.6), dtype=torch.float32).cuda()
    tab = torch.tensor(_rand((I, C), rng, 0.4), dtype=torch.float32).cuda()
    bias = torch.tensor(_rand((I - 1,), rng, 0.3), dtype=torch.float32).cuda()
    labels = rng.integers(1, I, size=R_)
    labels[[2, 3, 11, 23]] = 0
    rows_c, lab_c, _perm, _inv, nvalid = o.compact_rows(rows, torch.tensor(labels, dtype=torch.int64).cuda())
    assert int(nvalid.item()) == R_ - 4
    p, st = o._ptr, o._stream()
    outs = []
    for prepared in (False, True):
        ws = torch.zeros(lib.edgl_score_flash_workspace(R_, C, I, I, F32), device="cuda")
        lse = torch.zeros(R_, device="cuda"); ll = torch.zeros(R_, device="cuda")
        if prepared:
            check(lib.edgl_score_prepare_table(p(tab), R_, C, I, 0, I, p(ws), F32, st), "edgl_score_prepare_table")
            check(lib.edgl_score_flash_fwd_pre(p(rows_c), p(tab), p(bias), p(lab_c), R_, C, I, 0, I, p(nvalid), p(lse), p(ll), p(ws), 1, F32,
                                               st), "edgl_score_flash_fwd_pre")
        else:
            check(lib.edgl_score_flash_fwd(p(rows_c), p(tab), p(bias), p(lab_c), R_, C, I, 0, I, p(nvalid), p(lse), p(ll), p(ws), F32, st),
                  "edgl_score_flash_fwd")
        loss = torch.zeros(1, device="cuda"); coef = torch.zeros(R_, device="cuda")
        check(lib.edgl_ce_loss_fwd(p(lse), p(ll), p(lab_c), R_, p(loss), p(coef), st), "edgl_ce_loss_fwd")
        d_rows = torch.zeros_like(rows_c); d_tab = torch.zeros((I, C), device="cuda"); d_b = torch.zeros(I - 1, device="cuda")
        check(lib.edgl_score_flash_bwd(p(rows_c), p(tab), p(bias), p(lab_c), p(lse), p(coef), None, R_, C, I, 0, I, p(nvalid), p(d_rows),
                                       p(d_tab), p(d_b), p(ws), F32, st), "edgl_score_flash_bwd")
        outs.append((lse[:R_ - 4], ll, d_rows, d_tab, d_b))
    for what, a, b in zip(("lse", "label logits", "d_rows", "d_table", "d_bias"), *outs):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, what
        assert torch.equal(a, b), what


def test_deferred_reductions_match_the_immediate_ones():
    """edgl_reduce_defer(1) ... edgl_reduce_flush: one launch for every queued slab reduction — the column form for the few row
    splits of a weight-gradient GEMM (2-24 slabs), the row-lane form for deep lists (one partial row per sample of a LayerNorm
    backward) — against the same calls reduced immediately."""
    from easydgl_amd import _lib as L
    lib = L.lib
    o = ops()
    shapes = [(4096, 512, 512), (2048, 1536, 2048), (640, 128, 256), (16384, 128, 128)]
    res = {}
    for mode in ("now", "deferred"):
        outs = []
        if mode == "deferred":
            L.check(lib.edgl_reduce_defer(1, None), "defer")
        keep = []
        for R_, Kf, N in shapes:
            g = np.random.default_rng(R_ + Kf + N)
            X = torch.tensor(_rand((R_, Kf), g), dtype=torch.bfloat16).cuda()
            dY = torch.tensor(_rand((R_, N), g, 0.1), dtype=torch.bfloat16).cuda()
            both = torch.full((Kf * N + N,), float("nan"), device="cuda")
            ws = torch.empty(lib.edgl_gemm_dw_workspace(R_, Kf, N, L.BF16), device="cuda")
            L.check(lib.edgl_gemm_dw(X.data_ptr(), dY.data_ptr(), both.data_ptr(), both.data_ptr() + 4 * Kf * N, R_, Kf, N, Kf, N, 0,
                                     ws.data_ptr(), L.BF16, None), "edgl_gemm_dw")
            keep.append((X, dY, ws))
            outs.append(both)
        # a deep job next to them: LayerNorm backward partials, one row per sample
        B, T, C = 300, 9, 64
        x = torch.tensor(_rand((B, T, C), np.random.default_rng(5)), dtype=torch.float32).cuda().requires_grad_()
        gam = torch.ones(C, device="cuda", requires_grad=True); bet = torch.zeros(C, device="cuda", requires_grad=True)
        y = o.AddLayerNormFn.apply(x, None, gam, bet, o.NO_DROP, None)
        (y * y).sum().backward()
        if mode == "deferred":
            L.check(lib.edgl_reduce_defer(0, None), "flush")
        torch.cuda.synchronize()
        res[mode] = [t.clone() for t in outs] + [gam.grad.clone(), bet.grad.clone()]
    for a, b in zip(res["now"], res["deferred"]):
        assert torch.isfinite(b).all()
        assert float((a - b).abs().max()) <= 1e-5 * (1.0 + float(a.abs().max()))


@pytest.mark.parametrize("n", [700, 4088, 4089, 9000, 10232, 20001, 20472, 20473])
def test_topk_register_form_matches_the_oracle_at_every_row_length(n):
    """mask_topk_reg_kernel (the row in registers, bitwise search of the K-th largest key) for every register count it is compiled
    at (n <= 4088 / 10232 / 20472: aligned 16-byte pieces may start three elements in front of a row) and the four-pass kernel behind it: exact indices and values against the oracle's top_k
    (value descending, index ascending; Base.py:156-163) — ties that exceed the places left, a tie block at the top, both zeros,
    infinities, masked items among the leaders."""
    o = ops()
    rng = np.random.default_rng(n)
    R_, K, T = 7, 100, 30
    x = (rng.standard_normal((R_, n)) * 3.0).astype(np.float32)
    x[0, :] = -1.25                                  # all ties -> lowest indices
    x[1, n // 3:n // 3 + 150] = 9.0                  # more ties at the top than places
    x[2, 7] = np.inf; x[2, 9] = -np.inf
    x[3, ::2] = 0.0; x[3, 1::2] = -0.0               # the two zeros compare equal: index order
    x[4] = np.round(x[4])                            # few distinct values: a tie block at the K-th place
    seen = rng.integers(0, n, size=(R_, T))
    seen[5, :] = np.argsort(-x[5], kind="stable")[:T]
    want_x = x.copy()
    want_x[np.arange(R_)[:, None], seen] = -np.inf
    want = O.top_k(want_x, K)
    val, idx = o.mask_topk(torch.tensor(x).cuda(), 0, torch.tensor(seen).cuda(), K)
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    np.testing.assert_array_equal(val.cpu().numpy(), np.take_along_axis(want_x, want, 1))


def test_topk_merge_by_rank_and_by_sort_agree():
    """edgl_topk_merge: candidates above the K-th largest thread maximum ranked by counting (the usual case) against inputs that end
    in the bitonic sort (a permutation changes nothing; more than 256 candidates above the bound: a tie block) — the same result,
    also with invalid entries, fewer valid candidates than K, ties across the lists and a repeated (value, id) pair."""
    o = ops()
    rng = np.random.default_rng(8)
    S, R_, K = 8, 37, 100
    val = np.sort(rng.standard_normal((S, R_, K)).astype(np.float32), axis=2)[:, :, ::-1].copy()
    val[:, 3] = np.round(val[:, 3])                                        # ties across and inside the lists
    idx = np.empty((S, R_, K), np.int32)
    for s in range(S):
        for r in range(R_):
            ids = np.sort(rng.choice(5000, K, replace=False)) + 5000 * s      # shard-disjoint global ids
            order = np.lexsort((ids, -val[s, r]))                               # (value desc, id asc) inside the list
            val[s, r] = val[s, r][order]; idx[s, r] = ids[order]
    idx[:, 5, 40:] = -1; val[:, 5, 40:] = -np.inf                           # invalid tails
    idx[1:, 6, :] = -1; val[1:, 6, :] = -np.inf; idx[0, 6, 30:] = -1; val[0, 6, 30:] = -np.inf   # fewer than K valid candidates
    val[1, 7, 0] = val[0, 7, 0]; idx[1, 7, 0] = idx[0, 7, 0]                # the same (value, id) in two lists
    def run(v, i):
        mv, mi = o.topk_merge(torch.tensor(v).cuda(), torch.tensor(i).cuda())
        return mv.cpu().numpy(), mi.cpu().numpy()
    mv, mi = run(val, idx)
    perm = rng.permutation(K)
    sv, si = run(val[:, :, perm].copy(), idx[:, :, perm].copy())             # unordered lists: the sorting path
    np.testing.assert_array_equal(mi, si)
    np.testing.assert_array_equal(mv, sv)
    tv, ti = val.copy(), idx.copy()
    tv[:, 9, :60] = 2.5                                                     # 480 candidates tie at the top: the sorting path
    for s in range(S):
        ti[s, 9] = np.sort(ti[s, 9])
    bv, bi = run(tv, ti)
    flat_v, flat_i = tv[:, 9].reshape(-1), ti[:, 9].reshape(-1).astype(np.int64)
    np.testing.assert_array_equal(bi[9], flat_i[np.lexsort((flat_i, -flat_v))[:K]])
    for r in (0, 3, 5, 6):
        flat_v, flat_i = val[:, r].reshape(-1), idx[:, r].reshape(-1).astype(np.int64)
        ok = flat_i >= 0
        order = np.lexsort((flat_i[ok], -flat_v[ok]))[:K]
        want = np.full(K, -1, np.int64); want[:len(order)] = flat_i[ok][order]
        np.testing.assert_array_equal(mi[r], want)
