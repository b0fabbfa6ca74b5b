"""The dynamic-LDS limit of a kernel is raised by edgl_lds_limit (csrc/k_misc.hip) and remembered per (kernel, device): a launch
at or below 48 KB asks for nothing.  The one way this can go wrong on the GPU is a kernel that is first launched small and then
large — the large launch must still get its limit.  Each test below walks one kernel family across the 48 KB line and back, in
one process, and checks results on both sides.

  TAHE  B = 2, C = 32, T = 16 / 128 / 16 / 128: 1.3 KB forward and 2.4 KB backward at T = 16, 67.6 KB and 133.6 KB at T = 128
        (TAHE_MAXT).  f32 at T = 128 also against tests/_timelyrec_ref.tahe under the bounds of test_tahe_matches_float64.
  GRU   B = 5, T = 3, bf16, C = 32 / 128 / 32 on the LDS-resident kernel: the weight image is 7.7 KB at C = 32, about 104 KB at
        C = 128.  Each against float64 under the bounds of tests/test_gpu_gru.py.
  tail  C = 128, T = 17, B = 2 with the two-per-CU kernel, the one-per-CU kernel and the two-per-CU kernel again: each launch asks
        for the limit of the kernel it launches."""
import pytest
import torch

from tests import _seq_baselines_ref as SR
from tests import _timelyrec_ref as TR
from tests._util import GRAD_TOL, assert_close, grad_errors
from tests.test_gpu_gru import _case as gru_case, _run as gru_run
from tests.test_gpu_tail2_fwd import _forward as tail_forward, _problem as tail_problem
from tests.test_gpu_timelyrec_ops import _bits, _tahe_problem, _tahe_run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_tahe_small_then_large_then_small_then_large(mode):
    B, C = 2, 32
    prob = {T: _tahe_problem(B, T, C, mode, seed=T) for T in (16, 128)}
    runs = [(T, _tahe_run(*prob[T], mode)) for T in (16, 128, 16, 128)]
    for T, res in runs:
        for x in res:
            assert bool(torch.isfinite(x.float()).all()), T
    for first, again in ((0, 2), (1, 3)):
        for x, y in zip(runs[first][1], runs[again][1]):
            assert torch.equal(_bits(x.detach()), _bits(y.detach())), runs[first][0]
    if mode == "f32":
        R, Hs, d_out = prob[128]
        R64, H64 = R.clone().requires_grad_(True), Hs.clone().requires_grad_(True)
        want = TR.tahe(R64, R64, H64)
        want.backward(d_out)
        out, dR, dH = runs[1][1]
        e_out = float((out.detach().double().cpu() - want.detach()).abs().max() / want.detach().abs().max())
        errs = {"d_R": grad_errors(dR.float().cpu().numpy(), R64.grad.numpy()), "d_Hs": grad_errors(dH.float().cpu().numpy(), H64.grad.numpy())}
        print(f"tahe B={B} T=128 C={C} f32: output err {e_out:.3e} {errs}")
        t2, tm = GRAD_TOL["f32"]
        assert e_out <= 1e-4, e_out
        assert errs["d_R"][0] <= t2 and errs["d_R"][1] <= tm, errs
        assert errs["d_Hs"][0] <= t2 and errs["d_Hs"][1] <= tm, errs


def test_gru_resident_small_then_large_then_small():
    from easydgl_amd import _lib
    B, T, dt = 5, 3, torch.bfloat16
    assert _lib.lib.edgl_gru_seq_resident(32, _lib.BF16) == 1 and _lib.lib.edgl_gru_seq_resident(128, _lib.BF16) == 1
    cases, results = {}, []
    for C in (32, 128, 32):
        if C not in cases:
            gru, x, d_out = gru_case(B, T, C, 100 * B + 10 * T + C)
            cases[C] = (gru, x.to(dt).float(), d_out.to(dt).float())          # (the values the op is handed)
        gru, x, d_out = cases[C]
        results.append(gru_run(gru, x, d_out, dt))
    t2, tm = GRAD_TOL["bf16"]
    for C, (h, got) in zip((32, 128, 32), results):
        gru, x, d_out = cases[C]
        p64 = {n: p.detach().double().requires_grad_(True) for n, p in gru.named_parameters()}
        x64 = x.double().requires_grad_(True)
        xp64 = x64 @ p64["w_kernel"] + p64["w_bias"]
        xp64.retain_grad()
        want = SR.gru_seq(xp64, p64["r_kernel"], p64["r_bias"])
        want.backward(d_out.double())
        ref = dict(xp=xp64.grad, R=p64["r_kernel"].grad, b_R=p64["r_bias"].grad, W=p64["w_kernel"].grad, b_W=p64["w_bias"].grad, X=x64.grad)
        assert_close(h.float().cpu().numpy(), want.detach().numpy(), 3e-2, f"h at C={C}")
        for name, g in got.items():
            l2, mx = grad_errors(g.float().cpu().numpy(), ref[name].numpy())
            print(f"gru B={B} T={T} C={C} bf16: d{name} rel-L2 {l2:.3e} max {mx:.3e}")
            assert l2 <= t2 and mx <= tm, (C, name, l2, mx)
    (h0, g0), (h2, g2) = results[0], results[2]
    assert torch.equal(h0, h2)
    for k in g0:
        assert torch.equal(g0[k], g2[k]), k


def test_tail_two_per_cu_then_one_per_cu_then_two_per_cu():
    prob = tail_problem(2, 16, 1)
    outs = [tail_forward(prob, 2, variant) for variant in (1, 0, 1)]
    for out in outs[1:]:
        assert set(out) == set(outs[0])
        for k in out:
            assert not bool(torch.isnan(out[k].float()).any()), ("NaN left in", k)
            if k == "loss":
                assert abs(float(out[k]) - float(outs[0][k])) <= 1e-6 * abs(float(outs[0][k]))
            else:
                assert torch.equal(out[k], outs[0][k]), k
    assert torch.equal(outs[0]["loss"], outs[2]["loss"])
