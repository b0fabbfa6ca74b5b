"""The interval attention kernels (edgl_tiattn_fwd / _bwd / _bwd_det, edgl_add_pos2) through the C ABI against the float64
reference tests/_tiattn_ref.py on the kernels' own operands, at the edge shapes: every head width (DT = 1, 2, 4, 8), the narrow
bf16 path, NBp = 16 .. 272 (the launch above 64 KB of LDS), tab_rows below, at and above timelen, T = 1 / 16 / 17 / 241 / 256,
left / interior / all padding, decreasing and boundary timestamps, the non-causal form, the ordered forms, wide row strides.
tests/test_cpu_tiattn_ref.py checks the reference, the inputs, and that these bounds cannot hide a missing term.

Bounds, as (relative L2, max-abs-error / max-abs-reference) per tensor (tests/_tiattn_ref.py bounds):
  f32   1e-4 on the forward tensors (out, wbuf), 1e-3 on every gradient tensor — the project's kernel-level bounds.
  bf16  tests/golden/tiattn_bf16_bounds.json: 2 x the maximum measured on the GPU over all cases of this file, under the caps
        3e-2 (forward) and GRAD_TOL["bf16"] (gradients) — tests/golden/make_tiattn_bounds.py.
A tensor whose reference is exactly zero (T = 1: one key, P = 1, so dS = P (dP - D) = 0 and with it d_q, d_k and d_ktime) is held
to bound x the magnitude of the terms that cancel, dh max|dO| (max|V| + max|Vtime|) scale (max|K| + max|Ktime| + max|Q|).
Row sums of wbuf: f32 within the forward bound 1e-4; bf16 within 2^-8 (each bin is stored with a relative rounding of 2^-9)."""
import functools

import numpy as np
import pytest
import torch

from tests import _tiattn_ref as TR
from tests._util import dump_errors, grad_errors

pytestmark = pytest.mark.gpu

STREAM = 5
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
CASE_IDS = [TR.case_id(c) for c in TR.CASES]


@functools.lru_cache(maxsize=None)
def _problem(ci, mode):
    """(CPU operands, call constants, float64 reference) of case ci: computed once, shared by the tests, left unchanged"""
    o, kw = TR.make_inputs(**TR.CASES[ci], dtype=DTYPES[mode], seed=700 + ci)
    return o, kw, TR.reference(o, **kw)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class _Arena:
    """Outputs inside NaN-filled buffers: `guard` elements before and after, row stride `ld` >= the payload's width.  check():
    nothing but the payload changed (bit for bit) and every payload element was written with a finite value."""

    def __init__(self, guard):
        self.guard, self.items = guard, []

    @staticmethod
    def wide(t, ld):
        """input [.., C] as a view of a buffer with row stride ld, NaN in the gap"""
        C = t.shape[-1]
        if ld == C:
            return t
        w = torch.full(t.shape[:-1] + (ld,), float("nan"), device="cuda", dtype=t.dtype)
        w[..., :C] = t
        return w[..., :C]

    def out(self, name, shape, dtype, ld=None):
        cols = shape[-1]
        ld = ld or cols
        rows = int(np.prod(shape[:-1]))
        g, n = self.guard, rows * ld
        whole = torch.full((n + 2 * g,), float("nan"), device="cuda", dtype=dtype)
        pay = torch.zeros(n + 2 * g, dtype=torch.bool, device="cuda")
        pay[g:g + n].view(rows, ld)[:, :cols] = True
        self.items.append((name, whole, _bits(whole).clone(), pay))
        return whole[g:g + n].view(*shape[:-1], ld)[..., :cols]

    def check(self):
        for name, whole, before, pay in self.items:
            assert torch.equal(_bits(whole)[~pay], before[~pay]), f"{name}: a write outside the payload"
            assert torch.isfinite(whole[pay].float()).all(), f"{name}: payload not (finitely) written"


def _run(o, c, kw, *, ordered=False, det=False, rate=0.0, rng=None, pad=0, guard=0, backward=True):
    """forward (+ backward) through the C ABI on device operands `o`; every output by name, as contiguous copies"""
    from easydgl_amd import _lib, ops
    lib, P, V = _lib.lib, ops._ptr, ops._vptr
    B, T, H, dh, timelen, rows = (c[k] for k in ("B", "T", "H", "dh", "timelen", "tab_rows"))
    C, ld = H * dh, H * dh + pad
    dt, code = o["q"].dtype, ops._code(o["q"])
    flags = (_lib.TATTN_CAUSAL if kw["causal"] else 0) | (_lib.TATTN_ORDERED if ordered else 0)
    A = _Arena(guard)
    q, resid, d_out = (A.wide(o[k], ld) for k in ("q", "resid", "d_out"))
    kvp = o["kvp"]
    out = A.out("out", (B, T, C), dt, ld)
    nb = int(lib.edgl_tiattn_bucket_elems(B, T, H, timelen))
    NBp = nb // (B * T * H)
    assert NBp == (timelen + 1 + 15) // 16 * 16
    wbuf = A.out("wbuf", (H * B * T, NBp), dt)
    saved = torch.zeros(int(lib.edgl_tattn_saved_bytes(B, T, H, dh)), device="cuda", dtype=torch.uint8)
    fwd = lambda dst, sv, wb: _lib.check(lib.edgl_tiattn_fwd(
        V(q), ld, P(kvp), 2 * C, V(kvp[:, :, C:]), 2 * C, V(resid), ld, P(o["ids"]), P(o["ts"]), P(o["kt"]), P(o["vt"]), rows, B, T, H,
        dh, kw["scale"], kw["time_scale"], timelen, rate, P(rng), STREAM, V(dst), ld, P(sv), V(wb) if wb is not None else None, flags,
        code, ops._stream()), "edgl_tiattn_fwd")
    fwd(out, saved, wbuf)
    res = dict(out=out.contiguous(), wbuf=wbuf.clone().view(H * B, T, NBp))
    if rate == 0.0:                                     # the inference call: no saved buffer, no bins
        out2 = A.out("out (inference)", (B, T, C), dt, ld)
        fwd(out2, None, None)
        res["out_inference"] = out2.contiguous()
    if backward:
        d_q = A.out("d_q", (B, T, C), dt, ld)
        d_kv = A.out("d_kvp", (B, T, 2 * C), dt)
        dgbuf = A.out("dgbuf", (H * B * T, NBp), dt)
        d_kt, d_vt = A.out("d_ktime", (rows, C), torch.float32), A.out("d_vtime", (rows, C), torch.float32)
        head = (V(q), ld, P(kvp), 2 * C, V(kvp[:, :, C:]), 2 * C, P(o["ids"]), P(o["ts"]), P(o["kt"]), P(o["vt"]), rows, V(d_out), ld,
                P(saved), V(wbuf), B, T, H, dh, kw["scale"], kw["time_scale"], timelen, rate, P(rng), STREAM, V(d_q), ld, V(d_kv), 2 * C,
                V(d_kv[:, :, C:]), 2 * C, V(dgbuf), V(d_kt), V(d_vt))
        if det:
            ws = torch.full((int(lib.edgl_tiattn_det_workspace(H, dh, timelen)),), float("nan"), device="cuda")
            _lib.check(lib.edgl_tiattn_bwd_det(*head, P(ws), flags, code, ops._stream()), "edgl_tiattn_bwd_det")
        else:
            _lib.check(lib.edgl_tiattn_bwd(*head, flags, code, ops._stream()), "edgl_tiattn_bwd")
        res.update(d_q=d_q.contiguous(), d_k=d_kv[:, :, :C].contiguous(), d_v=d_kv[:, :, C:].contiguous(),
                   dgbuf=dgbuf.clone().view(H * B, T, NBp), d_ktime=d_kt.clone(), d_vtime=d_vt.clone())
    torch.cuda.synchronize()
    A.check()
    return res


def _dev(o):
    return {k: v.cuda() for k, v in o.items()}


def _compare(tag, mode, c, o, kw, ref, res):
    """every tensor against float64 under bounds(mode), in both norms; the dead columns and the row sums of the bins"""
    timelen, dh = c["timelen"], c["dh"]
    tol = TR.bounds(mode)
    amax = lambda t: float(t.double().abs().max())
    C = c["H"] * dh
    cancel = dh * amax(o["d_out"]) * (amax(o["kvp"][:, :, C:]) + amax(o["vt"])) * kw["scale"] * \
        (amax(o["kvp"][:, :, :C]) + amax(o["kt"]) + amax(o["q"]))
    got = dict(res, wbuf=res["wbuf"][:, :, :timelen + 1])
    errs, bad = {}, {}
    for k in TR.FORWARD + TR.GRADS:
        g, r = got[k].double().cpu().numpy(), ref["W" if k == "wbuf" else k].numpy()
        assert g.shape == r.shape, (k, g.shape, r.shape)
        if not np.any(r):
            e = float(np.abs(g).max()) / cancel
            print(f"{tag} {k}: reference exactly zero, max|got| / cancelling magnitude {e:.3e} (bound {tol[k][1]:.1e})")
            if e > tol[k][1]:
                bad[k] = (e, tol[k][1])
            continue
        errs[f"{mode}:{k}"] = e = grad_errors(g, r)
        print(f"{tag} {k}: rel-L2 {e[0]:.3e} (bound {tol[k][0]:.1e}), max-norm {e[1]:.3e} (bound {tol[k][1]:.1e})")
        if e[0] > tol[k][0] or e[1] > tol[k][1]:
            bad[k] = (e, tol[k])
    dump_errors("tiattn", errs)
    assert not bad, f"{tag}: against float64 (rel-L2, max-norm): {bad}"
    for k in ("wbuf", "dgbuf"):
        assert float(res[k][:, :, timelen + 1:].float().abs().sum()) == 0.0, f"{k}: columns [timelen + 1, NBp) not zero"
    sums = res["wbuf"].double().sum(-1)
    assert float((sums - 1).abs().max()) <= (1e-4 if mode == "f32" else 2.0 ** -8), float((sums - 1).abs().max())
    assert torch.equal(res["out"], res["out_inference"])


@pytest.mark.parametrize("mode", list(DTYPES))
@pytest.mark.parametrize("ci", range(len(TR.CASES)), ids=CASE_IDS)
def test_forward_and_backward_match_float64(ci, mode):
    c = TR.CASES[ci]
    o, kw, ref = _problem(ci, mode)
    _compare("default", mode, c, o, kw, ref, _run(_dev(o), c, kw))


@pytest.mark.parametrize("mode", list(DTYPES))
@pytest.mark.parametrize("ci", TR.ORDERED_CASES, ids=[CASE_IDS[i] for i in TR.ORDERED_CASES])
def test_ordered_bins_and_slab_backward_match_float64(ci, mode):
    """EDGL_TATTN_ORDERED and edgl_tiattn_bwd_det (NaN-filled workspace) against float64 — not against the default form — under
    the same bounds."""
    c = TR.CASES[ci]
    o, kw, ref = _problem(ci, mode)
    _compare("ordered", mode, c, o, kw, ref, _run(_dev(o), c, kw, ordered=True, det=True))


@pytest.mark.parametrize("mode", list(DTYPES))
@pytest.mark.parametrize("ordered", [False, True], ids=["default", "ordered"])
def test_no_write_outside_the_outputs(ordered, mode):
    """q, resid, out, d_out and d_q with row strides 8 columns wider than C (NaN in the gap), every output inside a NaN-filled
    buffer with a guard on both sides: gaps and guards keep their bits (_Arena.check), the results hold the float64 bounds and
    are those of the contiguous run bit for bit.  One exception: d_ktime / d_vtime of the default form are f32 atomics of the row
    splits' partial tiles from different workgroups, in whatever order they arrive — the slab form has one order and is compared
    bit for bit, the atomic form is held to the float64 bounds only.  (The LDS bins of the default form belong to one wave, whose
    atomics the LDS executes in program order: they are compared bit for bit.)"""
    ci = TR.STRIDED_CASE
    c = TR.CASES[ci]
    o, kw, ref = _problem(ci, mode)
    dev = _dev(o)
    plain = _run(dev, c, kw, ordered=ordered, det=ordered)
    wide = _run(dev, c, kw, ordered=ordered, det=ordered, pad=8, guard=64)
    _compare("strided", mode, c, o, kw, ref, wide)
    for k in [k for k in plain if ordered or k not in ("d_ktime", "d_vtime")]:
        assert torch.equal(plain[k], wide[k]), k


def test_dropout_at_odd_T_has_one_mask_in_all_three_sweeps():
    """f32, T = 37 (the row base of the mask counter is odd in every second row), rate 0.3.  For a fixed mask the output is linear
    in V and in vtime: <d_out, out(V + dV) - out(V)> = <d_v, dV> and the same for vtime, within 1e-3 max(1, |rhs|) (the bound of
    tests/test_gpu_tgat.py for this identity).  d_v comes from the key sweep, d_vtime from the bins of the forward: a mask that
    differs between the sweeps breaks one of them.  With V = 1, vtime = 0, resid = 0 the output is the kept mass."""
    c = dict(B=2, T=37, H=2, dh=16, timelen=16, tab_rows=16)
    o, kw = TR.make_inputs(**c, dtype=torch.float32, seed=41)
    o = _dev(o)
    C = c["H"] * c["dh"]
    rng = torch.tensor([1234, 5], dtype=torch.int64, device="cuda")
    base = _run(o, c, kw, rate=0.3, rng=rng)
    nodrop = _run(o, c, kw, backward=False)
    assert not torch.allclose(base["out"], nodrop["out"])
    g = torch.Generator(device="cuda").manual_seed(0)
    dV = torch.randn((c["B"], c["T"], C), device="cuda", generator=g)
    kvp2 = o["kvp"].clone()
    kvp2[:, :, C:] += dV
    out_v = _run(dict(o, kvp=kvp2), c, kw, rate=0.3, rng=rng, backward=False)["out"]
    lhs, rhs = float(((out_v - base["out"]) * o["d_out"]).sum()), float((base["d_v"] * dV).sum())
    print(f"V: lhs {lhs:.6f} rhs {rhs:.6f}")
    assert abs(lhs - rhs) <= 1e-3 * max(1.0, abs(rhs)), (lhs, rhs)
    dVt = 0.3 * torch.randn(o["vt"].shape, device="cuda", generator=g)
    out_t = _run(dict(o, vt=o["vt"] + dVt), c, kw, rate=0.3, rng=rng, backward=False)["out"]
    lhs, rhs = float(((out_t - base["out"]) * o["d_out"]).sum()), float((base["d_vtime"] * dVt).sum())
    print(f"vtime: lhs {lhs:.6f} rhs {rhs:.6f}")
    assert abs(lhs - rhs) <= 1e-3 * max(1.0, abs(rhs)), (lhs, rhs)
    ones = o["kvp"].clone()
    ones[:, :, C:] = 1.0
    unit = dict(o, kvp=ones, vt=torch.zeros_like(o["vt"]), resid=torch.zeros_like(o["resid"]))
    kept = _run(unit, c, kw, rate=0.3, rng=rng, backward=False)["out"]
    full = _run(unit, c, kw, backward=False)["out"]
    assert abs(float(kept.mean()) - 1.0) < 0.05 and not torch.allclose(kept, full)
    assert float((full - 1).abs().max()) < 1e-4


@pytest.mark.parametrize("mode", list(DTYPES))
@pytest.mark.parametrize("B,T,C", [(3, 17, 20), (2, 16, 128)])
def test_add_pos2(B, T, C, mode):
    from easydgl_amd import _lib, ops
    dt = DTYPES[mode]
    g = torch.Generator(device="cuda").manual_seed(B * T + C)
    kv = torch.randn((B, T, 2 * C), device="cuda", generator=g).to(dt)
    posK, posV = (torch.randn((T + 3, C), device="cuda", generator=g) for _ in range(2))
    A = _Arena(64)
    out = A.out("kvp", (B, T, 2 * C), dt)
    _lib.check(_lib.lib.edgl_add_pos2(ops._ptr(kv), ops._ptr(posK), ops._ptr(posV), B, T, C, ops._vptr(out), ops._code(kv),
                                      ops._stream()), "edgl_add_pos2")
    torch.cuda.synchronize()
    A.check()
    pos = torch.cat([posK[:T], posV[:T]], -1)
    want = kv + pos if mode == "f32" else (kv.float() + pos).to(torch.bfloat16)
    assert torch.equal(out, want)


def test_tiattn_function_adds_the_positions_and_returns_their_gradients():
    """ops.TiAttnFn at (3, 17, 2, 16, 15), f32, position tables of T + 3 rows: the output is the reference's on kv + positions;
    d_posK / d_posV are the batch sums of the reference's d_kvp halves in rows [0, T) and exactly 0 below."""
    from easydgl_amd import ops
    c = dict(B=3, T=17, H=2, dh=16, timelen=15, tab_rows=15)
    o, kw = TR.make_inputs(**c, dtype=torch.float32, seed=43)
    T, C = c["T"], c["H"] * c["dh"]
    g = np.random.default_rng(44)
    posK, posV = (torch.tensor(0.3 * g.standard_normal((T + 3, C)), dtype=torch.float32) for _ in range(2))
    ref = TR.reference(dict(o, kvp=o["kvp"] + torch.cat([posK[:T], posV[:T]], -1)), **kw)      # the f32 sum the kernel forms
    d = _dev(o)
    q, kv, pK, pV, kt, vt = (t.cuda().requires_grad_(True) for t in (o["q"], o["kvp"], posK, posV, o["kt"], o["vt"]))
    out = ops.TiAttnFn.apply(q, kv, d["resid"], pK, pV, kt, vt, kt.detach(), vt.detach(), d["ids"], d["ts"], c["H"], kw["time_scale"],
                             c["timelen"], ops.NO_DROP)
    out.backward(d["d_out"])
    tol = TR.bounds("f32")
    want = dict(out=ref["out"], d_q=ref["d_q"], d_kv=torch.cat([ref["d_k"], ref["d_v"]], -1), d_posK=ref["d_k"].sum(0),
                d_posV=ref["d_v"].sum(0), d_ktime=ref["d_ktime"], d_vtime=ref["d_vtime"])
    got = dict(out=out.detach(), d_q=q.grad, d_kv=kv.grad, d_posK=pK.grad[:T], d_posV=pV.grad[:T], d_ktime=kt.grad, d_vtime=vt.grad)
    for k, w in want.items():
        e = grad_errors(got[k].double().cpu().numpy(), w.numpy())
        b = tol["out"] if k == "out" else tol["d_k"]
        print(f"{k}: rel-L2 {e[0]:.3e}, max-norm {e[1]:.3e}")
        assert e[0] <= b[0] and e[1] <= b[1], (k, e, b)
    assert pK.grad.shape == (T + 3, C) and float(pK.grad[T:].abs().max()) == 0.0 and float(pV.grad[T:].abs().max()) == 0.0
