"""The two new ops of TimelyREC against autograd through the literal float64 form (tests/_timelyrec_ref.py):
ops.MateFn (calendar slots + slot attention + gated combination, csrc/k_mate.hip), ops.TaheFn (time-aware history encoder,
csrc/k_tahe.hip) and ops.TaheMixFn (the histories).

Tolerances: tests/_util.py's — f32: output 1e-4 (assert_close), every gradient 1e-3 relative-L2 and max-norm; bf16: LOSS_TOL["bf16"]
on the output, GRAD_TOL["bf16"] on the gradients.  On the bf16 path the operands are rounded to bf16 first and the float64 form is
taken of the rounded values: what is measured is the kernel's arithmetic, not the rounding of its inputs."""
import numpy as np
import pytest
import torch

from tests import _timelyrec_ref as TR
from tests._util import GRAD_TOL, LOSS_TOL, assert_close, grad_errors

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
NAMES = ("month", "day", "weekday", "hour")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _rounded(a, mode):
    """float64 array of values the dtype holds exactly."""
    return torch.tensor(a, dtype=torch.float32).to(DT[mode]).double()


def _calendar_idx(B, T, rng):
    """[4,B,T] shifted indices: sample 0 left-padded (fields 0: month and day index -1, weekday and hour 0), sample 1 on one calendar
    value throughout, sample 2 visiting every value in turn; further samples random."""
    idx = np.zeros((4, B, T), dtype=np.int64)
    pad = T // 3
    for g, (name, M) in enumerate(TR.RANGES.items()):
        off = TR.OFFSET[name]
        for b in range(B):
            if b == 1:
                f = np.full(T, M - 1)
            elif b == 2:
                f = np.arange(T) % M
            else:
                f = rng.integers(0, M, size=T)
            if b == 0:
                f[:pad] = -off          # the files hold 0 at padding
            idx[g, b] = f
    return idx


def _mate_problem(T, C, ratio, mode, seed=0, B=3):
    rng = np.random.default_rng(seed)
    idx = _calendar_idx(B, T, rng)
    tabs = [_rounded(rng.uniform(-0.4, 0.4, size=(M, C)), mode) for M in TR.RANGES.values()]
    u = _rounded(rng.standard_normal((B, T, 4 * C)) * 0.7, mode)
    pq = _rounded(rng.standard_normal((B, T, C)) * 0.5, mode)
    d_out = _rounded(rng.standard_normal((B, T, C)), mode)
    return idx, tabs, u, pq, d_out


def _mate_run(idx, tabs, u, pq, d_out, ratio, mode):
    from easydgl_amd import ops
    dev = lambda x: x.to(DT[mode]).cuda()
    masters = [t.float().cuda().requires_grad_(True) for t in tabs]
    ud, pd = dev(u).requires_grad_(True), dev(pq).requires_grad_(True)
    out = ops.MateFn.apply(torch.tensor(idx).cuda(), *masters, *[dev(t) for t in tabs], ud, pd, ops.mate_windows(ratio))
    out.backward(dev(d_out))
    return out, [ud.grad, pd.grad] + [m.grad for m in masters]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("ratio", [0.05, 0.2, 0.5])
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("T", [1, 10, 17])
def test_mate_matches_float64(T, C, ratio, mode):
    idx, tabs, u, pq, d_out = _mate_problem(T, C, ratio, mode, seed=T + C)
    t64 = [t.clone().requires_grad_(True) for t in tabs]
    u64, pq64 = u.clone().requires_grad_(True), pq.clone().requires_grad_(True)
    want = TR.mate({n: torch.tensor(idx[g]) for g, n in enumerate(NAMES)}, dict(zip(NAMES, t64)), u64, pq64, ratio)
    want.backward(d_out)
    out, grads = _mate_run(idx, tabs, u, pq, d_out, ratio, mode)
    otol = 1e-4 if mode == "f32" else LOSS_TOL["bf16"]
    e_out = float((out.detach().double().cpu() - want.detach()).abs().max() / want.detach().abs().max())
    print(f"mate T={T} C={C} ratio={ratio} {mode}: output err {e_out:.3e}")
    t2, tm = GRAD_TOL[mode]
    bad = {}
    for name, g, ref in zip(("d_u", "d_pq") + tuple("d_" + n for n in NAMES), grads, [u64.grad, pq64.grad] + [t.grad for t in t64]):
        l2, mx = grad_errors(g.float().cpu().numpy(), ref.numpy())
        print(f"mate T={T} C={C} ratio={ratio} {mode}: {name} rel-L2 {l2:.3e} max {mx:.3e}")
        if l2 > t2 or mx > tm:
            bad[name] = (l2, mx)
    assert torch.isfinite(out.float()).all()
    assert e_out <= otol, e_out
    assert not bad, bad


def test_mate_aliased_window_offsets_sum_the_row_twice():
    """Month at ratio 0.5: W = 7 and w = 6 reads (f + 6) mod 12 == (f - 6) mod 12 — one row, twice.  With every other table at zero
    and constant projections the month slot w = 6 after one position is (e + 2 E[(f + 6) mod 12]) / 13; the float64 form agrees."""
    T, C, ratio = 4, 32, 0.5
    idx, tabs, u, pq, d_out = _mate_problem(T, C, ratio, "f32", seed=5)
    for k in (1, 2, 3):
        tabs[k] = torch.zeros_like(tabs[k])
    want = TR.mate({n: torch.tensor(idx[g]) for g, n in enumerate(NAMES)}, dict(zip(NAMES, tabs)), u, pq, ratio)
    out, grads = _mate_run(idx, tabs, u, pq, d_out, ratio, "f32")
    assert_close(out.detach().cpu().numpy(), want.numpy(), 1e-4, "aliased window")
    assert float(grads[2].abs().max()) > 0.0


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_mate_backward_twice_gives_the_same_bits(mode):
    idx, tabs, u, pq, d_out = _mate_problem(17, 64, 0.2, mode, seed=9, B=70)      # (more samples than slabs: two per workgroup)
    a = _mate_run(idx, tabs, u, pq, d_out, 0.2, mode)
    b = _mate_run(idx, tabs, u, pq, d_out, 0.2, mode)
    assert torch.equal(_bits(a[0]), _bits(b[0]))
    for x, y in zip(a[1], b[1]):
        assert torch.equal(_bits(x), _bits(y))


# ---- TAHE -----------------------------------------------------------------------------------------------------------------
def _tahe_problem(B, T, C, mode, seed=0):
    rng = np.random.default_rng(seed)
    R = rng.standard_normal((B, T, C))
    if B > 1:
        R[1] = 0.0                      # a sample whose R is all zero: both branches of max(sum x^2, 1e-12) are taken in one launch
    Hs = rng.standard_normal((B, T, C)) * 0.3
    Hs[0, :T // 3] = 0.0                # masked histories at the padded positions
    return _rounded(R, mode), _rounded(Hs, mode), _rounded(rng.standard_normal((B, T, C)), mode)


def _tahe_run(R, Hs, d_out, mode):
    from easydgl_amd.module.sequential import TAHEncoder
    dev = lambda x: x.to(DT[mode]).cuda()
    Rd, Hd = dev(R).requires_grad_(True), dev(Hs).requires_grad_(True)
    out = TAHEncoder()(Rd, Rd, Hd)
    out.backward(dev(d_out))
    return out, Rd.grad, Hd.grad


TAHE_SHAPES = [(3, T, C) for T in (1, 10, 17) for C in (32, 64)] + [(2, 30, 512)]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("B,T,C", TAHE_SHAPES)
def test_tahe_matches_float64(B, T, C, mode):
    """The all-zero sample sits on the clamped branch of the normalisation: its n is zero, every weight is 1/2, and its gradient with
    respect to R is exactly zero (dn = M n = 0) — finite, not NaN.  (A single zero row beside non-zero ones is NOT a zero gradient in
    the literal form: n = 1e6 x is linear there and the row receives 1e6 dn.)"""
    R, Hs, d_out = _tahe_problem(B, T, C, mode, seed=B + T + C)
    R64, H64 = R.clone().requires_grad_(True), Hs.clone().requires_grad_(True)
    want = TR.tahe(R64, R64, H64)
    want.backward(d_out)
    out, dR, dH = _tahe_run(R, Hs, d_out, mode)
    otol = 1e-4 if mode == "f32" else LOSS_TOL["bf16"]
    e_out = float((out.detach().double().cpu() - want.detach()).abs().max() / want.detach().abs().max())
    print(f"tahe B={B} T={T} C={C} {mode}: output err {e_out:.3e}")
    errs = {"d_R": grad_errors(dR.float().cpu().numpy(), R64.grad.numpy()), "d_Hs": grad_errors(dH.float().cpu().numpy(), H64.grad.numpy())}
    print(f"tahe B={B} T={T} C={C} {mode}: {errs}")
    assert torch.isfinite(dR.float()).all() and torch.isfinite(dH.float()).all()
    assert float(dR[1].float().abs().max()) == 0.0 and float(R64.grad[1].abs().max()) == 0.0
    assert e_out <= otol, e_out
    t2, tm = GRAD_TOL[mode]
    if T > 1:       # (T = 1: the only weight is the constant diagonal, the true d_R is zero — no relative error to take)
        assert errs["d_R"][0] <= t2 and errs["d_R"][1] <= tm, errs
    else:
        assert float(dR.float().abs().max()) <= 1e-5 * float(d_out.abs().max())
    assert errs["d_Hs"][0] <= t2 and errs["d_Hs"][1] <= tm, errs


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_tahe_diagonal_weight_is_one_and_the_future_is_masked(mode):
    """Hs one-hot in position: hist[q][k] is the weight itself — exactly 1 on k = q ((1 + n_q . n_q) / 2), exactly 0 on k > q."""
    B, T, C = 2, 17, 32
    rng = np.random.default_rng(4)
    R = _rounded(rng.standard_normal((B, T, C)), mode)
    Hs = torch.zeros(B, T, C, dtype=torch.float64)
    Hs[:, torch.arange(T), torch.arange(T)] = 1.0
    out, _, _ = _tahe_run(R, Hs, torch.zeros(B, T, C, dtype=torch.float64), mode)
    out = out.detach()
    w = out.float().cpu()[:, :, :T]
    assert torch.equal(torch.diagonal(w, dim1=1, dim2=2), torch.ones(B, T))
    assert float(torch.triu(w, diagonal=1).abs().max()) == 0.0
    assert float(out.float().cpu()[:, :, T:].abs().max()) == 0.0
    want = TR.tahe(R, R, Hs)
    assert_close(out.detach().float().cpu().numpy(), want.numpy(), 1e-4 if mode == "f32" else LOSS_TOL["bf16"], "weights")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_tahe_backward_twice_gives_the_same_bits(mode):
    R, Hs, d_out = _tahe_problem(3, 17, 64, mode, seed=8)
    a, b = _tahe_run(R, Hs, d_out, mode), _tahe_run(R, Hs, d_out, mode)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_tahe_mix_matches_float64_and_is_ordered(mode):
    from easydgl_amd import ops
    B, T, C = 5, 30, 32                 # 150 rows: three workgroups of partial sums for d_te
    rng = np.random.default_rng(2)
    ids = rng.integers(1, 40, size=(B, T))
    ids[0, :7] = 0
    emb, tc = _rounded(rng.standard_normal((B, T, C)) * 0.2, mode), _rounded(rng.uniform(-1, 1, size=(B, T, C)), mode)
    d_out = _rounded(rng.standard_normal((B, T, C)), mode)
    te = torch.tensor(0.83, dtype=torch.float64, requires_grad=True)
    e64 = emb.clone().requires_grad_(True)
    want = (e64 + te * tc) * torch.tensor(ids != 0).unsqueeze(-1)
    want.backward(d_out)
    runs = []
    for _ in range(2):
        ed, ted = emb.to(DT[mode]).cuda().requires_grad_(True), torch.tensor(0.83).cuda().requires_grad_(True)
        out = ops.TaheMixFn.apply(ed, tc.to(DT[mode]).cuda(), ted, torch.tensor(ids).cuda())
        out.backward(d_out.to(DT[mode]).cuda())
        runs.append((out, ed.grad, ted.grad))
    out, de, dte = runs[0]
    assert_close(out.detach().float().cpu().numpy(), want.detach().numpy(), 1e-4 if mode == "f32" else LOSS_TOL["bf16"], "Hs")
    assert torch.equal(de.float().cpu().double(), e64.grad) and dte.shape == ()
    assert abs(float(dte) - float(te.grad)) <= 1e-4 * abs(float(te.grad))
    for x, y in zip(*runs):
        assert torch.equal(_bits(x), _bits(y))
