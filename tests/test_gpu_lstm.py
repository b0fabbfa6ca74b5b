"""ops.LinearFn + ops.LstmSeqFn (csrc/k_lstm.hip) against torch.nn.LSTM in float64 on the CPU (the weights copied in
transposed; inputs and d_out rounded to the op's dtype first).  C = 16: one tile, seven waves idle; 144: uneven tiles per wave, K
zero-padded, idle ring entries; 512: the published width and the f32 LDS tile.  T = 1: the ring never wraps into a next step and
c_{t-1} is the zero state only.  B = 5: a partial sample tile; 33: two full tiles plus one sample.  Bounds: h 1e-4 (f32) / 3e-2
(bf16), gradients GRAD_TOL."""
import pytest
import torch

from tests._util import GRAD_TOL, assert_close, grad_errors

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])


def _case(B, T, C, seed):
    from easydgl_amd.module import sequential as S
    gen = torch.Generator().manual_seed(seed)
    lstm = S.LSTM(C, gen=gen)
    with torch.no_grad():
        lstm.w_bias.copy_(torch.randn(4 * C, generator=gen) * 0.1)
        lstm.r_bias.copy_(torch.randn(4 * C, generator=gen) * 0.1)
    return lstm, torch.randn(B, T, C, generator=gen), torch.randn(B, T, C, generator=gen)


def _run(lstm, x, d_out, dt):
    from easydgl_amd import ops
    W, bW, R, bR = (p.detach().cuda().requires_grad_(True) for p in (lstm.w_kernel, lstm.w_bias, lstm.r_kernel, lstm.r_bias))
    xd = x.cuda().to(dt).requires_grad_(True)
    xp = ops.LinearFn.apply(xd, W, bW, W.detach().to(dt), False)
    xp.retain_grad()
    h = ops.LstmSeqFn.apply(xp, R, bR, R.detach().to(dt))
    h.backward(d_out.cuda().to(dt))
    return h.detach(), dict(xp=xp.grad, R=R.grad, b_R=bR.grad, W=W.grad, b_W=bW.grad, X=xd.grad)


@DTYPES
@pytest.mark.parametrize("C", [16, 144, 512])
@pytest.mark.parametrize("T", [1, 7])
@pytest.mark.parametrize("B", [5, 33])
def test_lstm_forward_and_every_gradient_match_float64(B, T, C, dt):
    mode = "f32" if dt == torch.float32 else "bf16"
    lstm, x, d_out = _case(B, T, C, 100 * B + 10 * T + C)
    x, d_out = x.to(dt).float(), d_out.to(dt).float()          # (the values the op is handed)
    ref = torch.nn.LSTM(C, C, batch_first=True).double()
    with torch.no_grad():
        for name, p in (("weight_ih_l0", lstm.w_kernel.t()), ("bias_ih_l0", lstm.w_bias), ("weight_hh_l0", lstm.r_kernel.t()),
                        ("bias_hh_l0", lstm.r_bias)):
            getattr(ref, name).copy_(p)
    x64 = x.double().requires_grad_(True)
    want = ref(x64)[0]
    want.backward(d_out.double())
    # torch.nn.LSTM does not expose the gradient of xp = x W + b_W: a second pass takes xp as its input through an identity W
    xp64 = (x.double() @ lstm.w_kernel.detach().double() + lstm.w_bias.detach().double()).requires_grad_(True)
    ref2 = torch.nn.LSTM(4 * C, C, batch_first=True).double()
    with torch.no_grad():
        for name, p in (("weight_ih_l0", torch.eye(4 * C)), ("bias_ih_l0", torch.zeros(4 * C)), ("weight_hh_l0", lstm.r_kernel.t()),
                        ("bias_hh_l0", lstm.r_bias)):
            getattr(ref2, name).copy_(p)
    ref2(xp64)[0].backward(d_out.double())
    g64 = dict(xp=xp64.grad, R=ref.weight_hh_l0.grad.t(), b_R=ref.bias_hh_l0.grad, W=ref.weight_ih_l0.grad.t(), b_W=ref.bias_ih_l0.grad,
               X=x64.grad)
    h, got = _run(lstm, x, d_out, dt)
    assert_close(h.float().cpu().numpy(), want.detach().numpy(), 1e-4 if mode == "f32" else 3e-2, "h")
    errs = {k: grad_errors(g.float().cpu().numpy(), g64[k].numpy()) for k, g in got.items()}
    print(f"lstm {mode} B={B} T={T} C={C}: (rel-L2, max) {errs}")
    assert all(l2 <= GRAD_TOL[mode][0] and mx <= GRAD_TOL[mode][1] for l2, mx in errs.values()), errs


@DTYPES
def test_lstm_twice_gives_the_same_bits(dt):
    lstm, x, d_out = _case(33, 7, 512, 3)
    (h1, g1), (h2, g2) = _run(lstm, x, d_out, dt), _run(lstm, x, d_out, dt)
    assert torch.equal(h1, h2) and all(torch.equal(g1[k], g2[k]) for k in g1)
