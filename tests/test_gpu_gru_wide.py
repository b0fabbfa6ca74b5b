"""ops.GruSeqFn(..., wide=True) (csrc/k_gru_wide.hip) against the float64 SR.gru_seq: inputs and tolerances of tests/test_gpu_gru.py.
C = 96: two waves own no tile; 144: uneven tiles per wave, K zero-padded, idle ring entries; 512: published.  T = 1: the ring never wraps into
a next step.  B = 5: a partial sample tile; 33: two full tiles plus one sample."""
import pytest
import torch

from tests import _seq_baselines_ref as SR
from tests._util import GRAD_TOL, assert_close, grad_errors
from tests.test_gpu_gru import _case

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])


def _run(gru, x, d_out, dt):
    from easydgl_amd import ops
    W, bW, R, bR = (p.detach().cuda().requires_grad_(True) for p in (gru.w_kernel, gru.w_bias, gru.r_kernel, gru.r_bias))
    xd = x.cuda().to(dt).requires_grad_(True)
    xp = ops.LinearFn.apply(xd, W, bW, W.detach().to(dt), False)
    xp.retain_grad()
    h = ops.GruSeqFn.apply(xp, R, bR, R.detach().to(dt), True)
    h.backward(d_out.cuda().to(dt))
    return h.detach(), dict(xp=xp.grad, R=R.grad, b_R=bR.grad, W=W.grad, b_W=bW.grad, X=xd.grad)


@DTYPES
@pytest.mark.parametrize("C", [96, 144, 512])
@pytest.mark.parametrize("T", [1, 7])
@pytest.mark.parametrize("B", [5, 33])
def test_wide_gru_forward_and_every_gradient_match_float64(B, T, C, dt):
    mode = "f32" if dt == torch.float32 else "bf16"
    gru, x, d_out = _case(B, T, C, 100 * B + 10 * T + C)
    x, d_out = x.to(dt).float(), d_out.to(dt).float()          # (the values the op is handed)
    W, bW, R, bR, x64 = (p.detach().double().requires_grad_(True) for p in (gru.w_kernel, gru.w_bias, gru.r_kernel, gru.r_bias, x))
    xp64 = x64 @ W + bW
    xp64.retain_grad()
    want = SR.gru_seq(xp64, R, bR)
    want.backward(d_out.double())
    ref = dict(xp=xp64.grad, R=R.grad, b_R=bR.grad, W=W.grad, b_W=bW.grad, X=x64.grad)
    h, got = _run(gru, x, d_out, dt)
    assert_close(h.float().cpu().numpy(), want.detach().numpy(), 1e-4 if mode == "f32" else 3e-2, "h")
    errs = {k: grad_errors(g.float().cpu().numpy(), ref[k].numpy()) for k, g in got.items()}
    assert all(l2 <= GRAD_TOL[mode][0] and mx <= GRAD_TOL[mode][1] for l2, mx in errs.values()), errs


@DTYPES
def test_wide_gru_twice_gives_the_same_bits(dt):
    gru, x, d_out = _case(33, 7, 512, 3)
    (h1, g1), (h2, g2) = _run(gru, x, d_out, dt), _run(gru, x, d_out, dt)
    assert torch.equal(h1, h2) and all(torch.equal(g1[k], g2[k]) for k in g1)
