"""Deterministic item-table scatter (csrc/k_segsum.hip): the sorted plan is exact against numpy's stable sort, the ordered sums
stay within the rounding of an f32 sum of the segment against an fp64 index_add, and two calls give the same bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U23 = 2.0 ** -23


# ---- (a) the plan ---------------------------------------------------------------------------------------------------------------
def _patterns(n, I, rng):
    """name -> (keys, nvalid or None, (i0, i1))"""
    hi = I - 1
    uni = rng.integers(0, I, n)
    zipf = rng.integers(1, I, n)
    zipf[rng.random(n) < 1.0 / 3.0] = hi                      # a third of the rows on one id (the largest: every digit in use)
    zipf[rng.random(n) < 0.05] = 0
    return {
        "all_equal": (np.full(n, hi), None, (0, I)),
        "all_zero": (np.zeros(n, dtype=np.int64), None, (0, I)),
        "ascending": (np.sort(uni), None, (0, I)),
        "descending": (np.sort(uni)[::-1].copy(), None, (0, I)),
        "zipf": (zipf, None, (0, I)),
        "nvalid": (uni, max(n * 2 // 3, 0), (0, I)),
        "range": (uni, None, (I // 4, max(3 * I // 4, I // 4 + 1))),
    }


def _plan_ref(keys, nvalid, i0, i1):
    n = len(keys)
    live = np.arange(n) < (n if nvalid is None else min(n, nvalid))
    rows = np.nonzero(live & (keys != 0) & (keys >= i0) & (keys < i1))[0]
    perm = rows[np.argsort(keys[rows], kind="stable")]
    uk, start = np.unique(keys[perm], return_index=True)
    return perm, uk, np.append(start, len(perm))


@pytest.mark.parametrize("I", [2, 257, 65537, 1000001])
@pytest.mark.parametrize("n", [1, 63, 64, 255, 256, 257, 4097, 70001])
def test_plan_is_exact(n, I):
    from easydgl_amd import ops
    rng = np.random.default_rng(1000 * n + I)
    for name, (keys, nv, (i0, i1)) in _patterns(n, I, rng).items():
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        nvt = None if nv is None else torch.tensor([nv], dtype=torch.int32, device="cuda")
        perm, seg_key, seg_start, nseg, nkept = ops.segsum_plan(torch.from_numpy(keys).cuda(), I, nvt, i0, i1)
        wp, wk, ws = _plan_ref(keys, nv, i0, i1)
        ns, nk = int(nseg), int(nkept)
        assert (ns, nk) == (len(wk), len(wp)), (name, ns, nk, len(wk), len(wp))
        np.testing.assert_array_equal(perm[:nk].cpu().numpy(), wp, err_msg=name)
        np.testing.assert_array_equal(seg_key[:ns].cpu().numpy(), wk, err_msg=name)
        np.testing.assert_array_equal(seg_start[:ns + 1].cpu().numpy(), ws, err_msg=name)


# ---- (b) the ordered sums ---------------------------------------------------------------------------------------------------------
B_, T_, E_, I_ = 125, 96, 4, 500      # 12 000 rows: one id on 10 000 of them, the rest short segments and padding
HOT = 7


def _ids(seed, pattern="hot"):
    g = np.random.default_rng(seed)
    n = B_ * T_
    if pattern == "all_equal":
        ids = np.full(n, HOT, dtype=np.int64)
    elif pattern == "zipf":
        ids = g.integers(1, I_, n)
        ids[g.random(n) < 1.0 / 3.0] = HOT
        ids[g.random(n) < 0.05] = 0
    else:
        ids = g.integers(0, I_, n)
        ids[g.permutation(n)[:10000]] = HOT
    return torch.from_numpy(ids.reshape(B_, T_)).cuda()


def _rand(shape, dt, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, device="cuda", dtype=torch.float32, generator=g).to(dt)


def _encode_bwd(det, ids, dx0, add1, add2, C, c_true, rate=0.0, rng=None):
    from easydgl_amd import _lib, ops
    lib, P = _lib.lib, ops._ptr
    marks = (torch.arange(B_ * T_ * E_, device="cuda") % 3 == 0).to(torch.uint8).reshape(B_, T_, E_)
    d_item = torch.zeros((I_, C), device="cuda")
    d_pos = torch.zeros((T_, C), device="cuda")
    d_mark = torch.empty((E_, C), device="cuda")
    ws = torch.empty(lib.edgl_encode_bwd_workspace(B_, T_, C), device="cuda")
    code = ops._DT[dx0.dtype]
    head = (P(ids), P(marks), P(dx0), P(add1), P(add2), B_, T_, C, E_, I_, float(rate), P(rng), 1, P(d_item), P(d_pos), P(d_mark),
            P(ws), int(c_true))
    if det:
        plan = ops.segsum_plan_buffer(B_ * T_, I_, ids.device)
        _lib.check(lib.edgl_encode_bwd_add_det(*head, P(plan), code, ops._stream()), "edgl_encode_bwd_add_det")
    else:
        _lib.check(lib.edgl_encode_bwd_add_ct(*head, code, ops._stream()), "edgl_encode_bwd_add_ct")
    return d_item, d_pos, d_mark


def _embed_terms(dx0, add1, add2, C, c_true):
    """fp64 terms sqrt(C_true) * (dX0[:, :C] + add1 + add2) of the same f32 / bf16 inputs, [rows, C]"""
    t = dx0.reshape(-1, 3 * C)[:, :C].double()
    if add1 is not None:
        t = t + add1.reshape(-1, C).double() + add2.reshape(-1, C).double()
    return t * float(np.sqrt(np.float32(c_true if c_true else C)))


def _segment_sums(ids, terms, I):
    """(fp64 sum, sum of |term|, segment length) per id; id 0 dropped"""
    flat = ids.reshape(-1)
    keep = flat != 0
    ref = torch.zeros((I, terms.shape[1]), device="cuda", dtype=torch.float64).index_add_(0, flat[keep], terms[keep])
    S = torch.zeros_like(ref).index_add_(0, flat[keep], terms[keep].abs())
    cnt = torch.bincount(flat[keep], minlength=I).double()
    return ref, S, cnt


@pytest.mark.parametrize("adds", [False, True])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,c_true", [(32, 0), (128, 0), (512, 0), (64, 50)])
def test_embedding_rows_against_fp64_index_add(C, c_true, dt, adds):
    """Bound per element, n = segment length, S = sum |term|: (n + 2) 2^-23 S — a sum of n products has at most n + 1 f32 roundings,
    the factor 2 leaves room for chunked orders; + 2^-8 S in bf16 with add1 / add2 (the one permitted rounding of the three-way sum)."""
    ids = _ids(3)
    dx0 = _rand((B_, T_, 3 * C), dt, 11)
    add1, add2 = (_rand((B_, T_, C), dt, 12), _rand((B_, T_, C), dt, 13)) if adds else (None, None)
    d_item, _, _ = _encode_bwd(True, ids, dx0, add1, add2, C, c_true)
    ref, S, cnt = _segment_sums(ids, _embed_terms(dx0, add1, add2, C, c_true), I_)
    assert int(cnt[HOT]) >= 10000
    bound = (cnt[:, None] + 2) * U23 * S
    if adds and dt == torch.bfloat16:
        bound = bound + 2.0 ** -8 * S
    err = (d_item.double() - ref).abs()
    worst = float((err - bound).max())
    print(f"C={C} dt={dt} adds={adds}: max err {float(err.max()):.3e}, max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3e}")
    assert worst <= 0.0, worst
    assert float(d_item[0].abs().max()) == 0.0      # padding id: no row of its own


@pytest.mark.parametrize("C", [128, 512])
def test_label_rows_against_fp64_index_add(C):
    """d_table[label] -= gscale coef rows, d_bias[label - 1] -= gscale coef: same bound, d_bias included (C = 1 rows of |coef|).
    bf16 rows at the strip widths (elsewhere the product pass contains the term and the call is a no-op: checked in f32)."""
    from easydgl_amd import _lib, ops
    lib, P = _lib.lib, ops._ptr
    g = np.random.default_rng(5)
    R, I, nv = 12000, 400, 11500
    lab = g.integers(1, I, R)
    lab[g.permutation(R)[:10000]] = 9
    lab[nv:] = g.integers(0, I, R - nv)      # behind the row count: ignored whatever they hold
    labels = torch.from_numpy(lab).cuda()
    coef = torch.from_numpy(g.random(R).astype(np.float32)).cuda()
    coef[torch.from_numpy(g.random(R) < 0.1).cuda()] = 0.0
    gs = torch.tensor([0.37], device="cuda")
    nvalid = torch.tensor([nv], dtype=torch.int32, device="cuda")
    i0, i1 = 8, I - 40
    for dt in (torch.bfloat16, torch.float32):
        rows = _rand((R, C), dt, 21)
        d_table = torch.zeros((I, C), device="cuda")
        d_bias = torch.zeros(I - 1, device="cuda")
        plan = ops.segsum_plan_buffer(R, I, rows.device)
        _lib.check(lib.edgl_score_flash_label_term_det(P(rows), P(labels), P(coef), P(gs), R, C, I, i0, i1, P(nvalid), P(d_table),
                                                       P(d_bias), P(plan), ops._DT[dt], ops._stream()), "edgl_score_flash_label_term_det")
        if dt == torch.float32:
            assert not d_table.any() and not d_bias.any()      # the contract's no-op
            continue
        live = (torch.arange(R, device="cuda") < nv) & (labels >= i0) & (labels < i1) & (labels != 0)
        w = -(gs.double() * coef.double())
        ids = torch.where(live, labels, torch.zeros_like(labels))
        ref, S, cnt = _segment_sums(ids, w[:, None] * rows.double(), I)
        refb, Sb, _ = _segment_sums(ids, w[:, None], I)
        assert int(cnt[9]) > 9000
        err, bound = (d_table.double() - ref).abs(), (cnt[:, None] + 2) * U23 * S
        errb, boundb = (d_bias.double() - refb[1:, 0]).abs(), (cnt[1:] + 2) * U23 * Sb[1:, 0]
        print(f"label C={C}: table err / bound {float((err / bound.clamp_min(1e-300)).max()):.3e}, "
              f"bias err / bound {float((errb / boundb.clamp_min(1e-300)).max()):.3e}")
        assert float((err - bound).max()) <= 0.0 and float((errb - boundb).max()) <= 0.0
        assert float(d_table[:i0].abs().max()) == 0.0 and float(d_table[i1:].abs().max()) == 0.0


@pytest.mark.parametrize("dt,adds", [(torch.float32, False), (torch.bfloat16, False), (torch.bfloat16, True)])
def test_dropout_masks_match_the_atomic_path(dt, adds):
    """No oracle draws the masks: d_item of the deterministic call against edgl_encode_bwd_add_ct on the same inputs and generator
    state, within twice the bound with S over all rows times 1 / (1 - rate) (an upper bound under any mask); the position and
    mark gradients come from the same kernel and the same reduction: bit-identical.
    add1 / add2 in bf16 only: there the atomic path rounds the three-way sum once to bf16 (the 2^-8 S term).  In f32 it adds
    x + a + b as a plain chain, whose rounding is relative to |x + a| and not to the term — where the branches cancel, the
    REFERENCE's own error is outside any bound in S, so that case says nothing about the call under test (its sum is checked
    against fp64 in test_embedding_rows_against_fp64_index_add)."""
    from easydgl_amd import ops
    C, rate = 128, 0.1
    ids = _ids(4)
    dx0 = _rand((B_, T_, 3 * C), dt, 31)
    add1, add2 = (_rand((B_, T_, C), dt, 32), _rand((B_, T_, C), dt, 33)) if adds else (None, None)
    rng = ops.make_rng_state("cuda", 77)
    rng[1] = 5
    a_item, a_pos, a_mark = _encode_bwd(False, ids, dx0, add1, add2, C, 0, rate, rng)
    d_item, d_pos, d_mark = _encode_bwd(True, ids, dx0, add1, add2, C, 0, rate, rng)
    assert torch.equal(a_pos, d_pos) and torch.equal(a_mark, d_mark)
    _, S, cnt = _segment_sums(ids, _embed_terms(dx0, add1, add2, C, 0), I_)
    S = S / (1.0 - rate)
    bound = (cnt[:, None] + 2) * U23 * S + (2.0 ** -8 * S if adds else 0.0)
    err = (d_item.double() - a_item.double()).abs()
    print(f"dropout dt={dt} adds={adds}: max err {float(err.max()):.3e}, err / (2 bound) {float((err / (2 * bound).clamp_min(1e-300)).max()):.3e}")
    assert float((err - 2 * bound).max()) <= 0.0
    assert float(d_item.abs().max()) > 0.0
    # a mask was drawn: the sums differ from the rate-0 ones
    z_item, _, _ = _encode_bwd(True, ids, dx0, add1, add2, C, 0)
    assert not torch.equal(z_item, d_item)


@pytest.mark.parametrize("pattern", ["zipf", "all_equal"])
def test_two_calls_give_the_same_bits(pattern):
    from easydgl_amd import ops
    C = 128
    ids = _ids(6, pattern)
    dx0 = _rand((B_, T_, 3 * C), torch.bfloat16, 41)
    add1, add2 = _rand((B_, T_, C), torch.bfloat16, 42), _rand((B_, T_, C), torch.bfloat16, 43)
    rng = ops.make_rng_state("cuda", 3)
    a = _encode_bwd(True, ids, dx0, add1, add2, C, 0, 0.1, rng)
    b = _encode_bwd(True, ids, dx0, add1, add2, C, 0, 0.1, rng)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert float(a[0].abs().max()) > 0.0
