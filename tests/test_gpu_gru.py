"""The GRU sequence recurrence (csrc/k_gru.hip) through ops.GruSeqFn and ops.LinearFn against the float64 restatement
tests/_seq_baselines_ref.py: forward and every gradient, on both sides of the LDS-resident / L2-streamed boundary, with partial
sample tiles and more than one tile; causality of the recurrence; bit-reproducibility.

Tolerances: f32 path 1e-4 on the output and tests/_util.py's GRAD_TOL["f32"] (1e-3 relative-L2 and max-norm) on every gradient;
bf16 path 3e-2 on the output (the bound of every bf16 forward check of this suite) and GRAD_TOL["bf16"]."""
import numpy as np
import pytest
import torch

from tests import _seq_baselines_ref as SR
from tests._util import GRAD_TOL, assert_close, dump_errors, grad_errors

pytestmark = pytest.mark.gpu


def _case(B, T, C, seed):
    """Inputs as the model feeds them: item rows that are zero on left padding of a different length per sample."""
    from easydgl_amd.module.sequential import GRU
    rng = np.random.default_rng(seed)
    gru = GRU(C, C, gen=torch.Generator().manual_seed(seed))
    with torch.no_grad():
        gru.w_bias.copy_(torch.tensor(0.1 * rng.standard_normal(3 * C), dtype=torch.float32))
        gru.r_bias.copy_(torch.tensor(0.1 * rng.standard_normal(3 * C), dtype=torch.float32))
    ids = rng.integers(1, 50, size=(B, T))
    for b in range(B):
        ids[b, :(b * 3) % T] = 0
    x = 0.7 * rng.standard_normal((B, T, C)) * (ids != 0)[..., None]
    d_out = rng.standard_normal((B, T, C))
    return gru, torch.tensor(x, dtype=torch.float32), torch.tensor(d_out, dtype=torch.float32)


def _run(gru, x, d_out, dt):
    from easydgl_amd import ops
    W, bW, R, bR = (p.detach().cuda().requires_grad_(True) for p in (gru.w_kernel, gru.w_bias, gru.r_kernel, gru.r_bias))
    xd = x.cuda().to(dt).requires_grad_(True)
    xp = ops.LinearFn.apply(xd, W, bW, W.detach().to(dt), False)
    xp.retain_grad()
    h = ops.GruSeqFn.apply(xp, R, bR, R.detach().to(dt))
    h.backward(d_out.cuda().to(dt))
    return h.detach(), dict(xp=xp.grad, R=R.grad, b_R=bR.grad, W=W.grad, b_W=bW.grad, X=xd.grad)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [32, 128, 256, 512])
@pytest.mark.parametrize("T", [1, 7])
@pytest.mark.parametrize("B", [1, 5, 33])
def test_gru_forward_and_every_gradient_match_float64(B, T, C, dt):
    mode = "f32" if dt == torch.float32 else "bf16"
    gru, x, d_out = _case(B, T, C, 100 * B + 10 * T + C)
    x, d_out = x.to(dt).float(), d_out.to(dt).float()          # (the values the op is handed)
    p64 = {n: p.detach().double().requires_grad_(True) for n, p in gru.named_parameters()}
    x64 = x.double().requires_grad_(True)
    xp64 = x64 @ p64["w_kernel"] + p64["w_bias"]
    xp64.retain_grad()
    want = SR.gru_seq(xp64, p64["r_kernel"], p64["r_bias"])
    want.backward(d_out.double())
    ref = dict(xp=xp64.grad, R=p64["r_kernel"].grad, b_R=p64["r_bias"].grad, W=p64["w_kernel"].grad, b_W=p64["w_bias"].grad,
               X=x64.grad)
    h, got = _run(gru, x, d_out, dt)
    assert_close(h.float().cpu().numpy(), want.detach().numpy(), 1e-4 if mode == "f32" else 3e-2, "h")
    t2, tm = GRAD_TOL[mode]
    bad, errs = {}, {}
    for name, g in got.items():
        l2, mx = grad_errors(g.float().cpu().numpy(), ref[name].numpy())
        errs[f"gru:{mode}:{name}"] = (l2, mx)
        print(f"gru B={B} T={T} C={C} {mode}: d{name} rel-L2 {l2:.3e} max {mx:.3e}")
        if l2 > t2 or mx > tm:
            bad[name] = (l2, mx)
    dump_errors("gru", errs)
    assert not bad, bad


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [32, 256])
def test_gru_is_causal(C, dt):
    """Changing xp at steps > t leaves h[:, :t + 1] bit-identical."""
    from easydgl_amd import ops
    B, T, t = 5, 7, 3
    gru, x, _ = _case(B, T, C, 7)
    R, bR = gru.r_kernel.detach().cuda(), gru.r_bias.detach().cuda()
    g = torch.Generator(device="cuda").manual_seed(1)
    xp = torch.randn((B, T, 3 * C), device="cuda", generator=g).to(dt)
    h1 = ops.GruSeqFn.apply(xp, R, bR, R.to(dt))
    xp2 = xp.clone()
    xp2[:, t + 1:] = torch.randn((B, T - t - 1, 3 * C), device="cuda", generator=g).to(dt)
    h2 = ops.GruSeqFn.apply(xp2, R, bR, R.to(dt))
    assert torch.equal(h1[:, :t + 1], h2[:, :t + 1]) and not torch.equal(h1[:, t + 1:], h2[:, t + 1:])


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [128, 512])
def test_gru_twice_gives_the_same_bits(C, dt):
    gru, x, d_out = _case(33, 7, C, 3)
    h1, g1 = _run(gru, x, d_out, dt)
    h2, g2 = _run(gru, x, d_out, dt)
    assert torch.equal(h1, h2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_gru_inference_call_saves_nothing_and_matches():
    from easydgl_amd import ops
    gru, x, d_out = _case(5, 7, 32, 9)
    R, bR = gru.r_kernel.detach().cuda(), gru.r_bias.detach().cuda()
    xp = torch.randn((5, 7, 96), device="cuda")
    with torch.no_grad():
        h0 = ops.GruSeqFn.apply(xp, R, bR, R)
    h1 = ops.GruSeqFn.apply(xp.clone().requires_grad_(True), R, bR, R)
    assert torch.equal(h0, h1.detach())
