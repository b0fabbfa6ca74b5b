"""The block-tail backward on half a CU (csrc/k_tail_bwd.hip, t2::tail2_bwd_kernel: C = 128, T <= 101, three swizzled LDS images, <= 128
registers, LayerNorm inputs as quads straight from global memory) against tail_bwd_kernel, the one-workgroup-per-CU kernel it replaces
at that shape: the SAME arithmetic in the same order (rounding points, block-sum order, dropout element indices, chains summed in
ascending j), so the six gradient tensors, the three per-sample LayerNorm partials and the six LayerNorm parameter gradients must
agree BIT FOR BIT.  edgl_tail_bwd_ct is called directly under edgl_tail_variant(0) and (1) on random saved tensors (the backward is
arithmetic on its inputs: they need not come from a forward), at the smallest shapes where the kernels can go wrong: both sides of a
row-tile edge (T = 16 / 17), the four-tile form (T = 50), the one-row and the five-row last tile (T = 97 / 101), one to five workgroups, one and twenty gathered
rows.  The one-per-CU kernel itself is held to the unfused launches and the fp64 oracle by tests/test_gpu_engine.py."""
import itertools

import pytest
import torch

from tests._util import build_model, make_problem, to_dev

pytestmark = pytest.mark.gpu

# B, T, M (T = 50: the four-tile instantiation, beside the two- and seven-tile ones)
GRID = list(itertools.product((1, 3, 5), (1, 5, 16, 17, 50, 97, 101), (1, 20)))
OUT9 = ("d_pre_t", "d_o", "d_pre_f", "d_ao", "d_res1", "d_att", "part1", "part2", "part3")
LN6 = ("dg1", "db1", "dg2", "db2", "dg3", "db3")


def _inputs(B, T, M, C=128, head=1, inv_mode="some", mpos=None, seed=0, ld_x=None):
    g = torch.Generator(device="cpu").manual_seed(1000 * seed + 97 * B + 13 * T + M)
    dev = "cuda"
    ld_x = ld_x or 3 * C      # the first block reads the 3C-wide encoder output

    def act(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(dev)

    d = dict(B=B, T=T, M=M, C=C, head=head, ld_x=ld_x)
    d["xin"] = act(B * T, ld_x)
    for k in ("ao", "a1", "o", "so"):
        d[k] = act(B, T, C)
    d["pre_t"] = act(B, T, C, scale=0.5)      # (gelu' values)
    d["pre_f"] = act(B, T, 2 * C, scale=0.5)
    for k in ("st1", "st2", "st3"):
        st = torch.empty(B, 2)
        st[:, 0] = torch.randn(B, generator=g) * 0.1
        st[:, 1] = 0.5 + 1.5 * torch.rand(B, generator=g)
        d[k] = st.to(dev)
    d["Wo"], d["Wt"] = act(C, C, scale=C ** -0.5), act(C, C, scale=C ** -0.5)
    d["Wi"], d["Wout"] = act(C, 2 * C, scale=C ** -0.5), act(2 * C, C, scale=(2 * C) ** -0.5)
    for k in ("g1", "g2", "g3"):
        d[k] = (1.0 + 0.1 * torch.randn(C, generator=g)).to(dev)
    d["rng"] = torch.tensor([0x1234ABCD5678, 7], dtype=torch.int64, device=dev)
    if mpos is None:
        mpos = torch.randint(0, T, (B, M), generator=g)      # with replacement: repeated positions (chains) wherever M > 1
    d["mpos"] = mpos.to(torch.int64).to(dev)
    if inv_mode == "null":
        inv, R = None, B * M
    else:
        keep = torch.ones(B * M, dtype=torch.bool)
        if inv_mode in ("some", "all"):
            keep = torch.rand(B * M, generator=g) < 0.6
        if inv_mode == "all":
            keep[:M] = False      # every slot of sample 0 dropped
        inv = torch.where(keep, torch.cumsum(keep.to(torch.int32), 0) - 1, torch.full((B * M,), -1)).to(torch.int32).to(dev)
        R = int(keep.sum())
    d["inv"], d["kept"] = inv, R
    d["d_rows"] = act(max(R, 1), C)
    d["d_y_in"] = act(B, T, C)
    return d


def _bwd(d, variant, drop=0.0, pad=(0, 0)):
    from easydgl_amd import _lib
    from easydgl_amd.ops import _ptr, _stream
    lib = _lib.lib
    B, T, M, C, head = d["B"], d["T"], d["M"], d["C"], d["head"]
    dev = "cuda"
    out = {k: torch.zeros(B, T, 2 * C if k == "d_pre_f" else C, dtype=torch.bfloat16, device=dev) for k in OUT9[:6]}
    ws = torch.zeros(int(lib.edgl_tail_bwd_workspace(B, C)), dtype=torch.float32, device=dev)
    ln = {k: torch.zeros(C, dtype=torch.float32, device=dev) for k in LN6}
    prev = lib.edgl_tail_variant(variant)
    try:
        _lib.check(lib.edgl_tail_bwd_ct(
            _ptr(d["xin"]), d["ld_x"], _ptr(d["ao"]), _ptr(d["a1"]), _ptr(d["pre_f"]), _ptr(d["o"]), _ptr(d["pre_t"]), _ptr(d["so"]),
            _ptr(d["st1"]), _ptr(d["st2"]), _ptr(d["st3"]), _ptr(d["Wo"]), _ptr(d["Wi"]), _ptr(d["Wout"]), _ptr(d["Wt"]),
            _ptr(d["g1"]), _ptr(d["g2"]), _ptr(d["g3"]), B, T, C, float(drop), _ptr(d["rng"]), 11, 12, head,
            _ptr(d["d_rows"]), _ptr(d["mpos"]), M, _ptr(d["inv"]), None if head else _ptr(d["d_y_in"]),
            _ptr(out["d_pre_t"]), _ptr(out["d_o"]), _ptr(out["d_pre_f"]), _ptr(out["d_ao"]), _ptr(out["d_res1"]), _ptr(out["d_att"]),
            _ptr(ln["dg1"]), _ptr(ln["db1"]), _ptr(ln["dg2"]), _ptr(ln["db2"]), _ptr(ln["dg3"]), _ptr(ln["db3"]),
            _ptr(ws), pad[0], pad[1], _lib.BF16, _stream()), "edgl_tail_bwd_ct")
        torch.cuda.synchronize()
    finally:
        lib.edgl_tail_variant(prev)
    n = B * 2 * C
    out.update(part1=ws[:n], part2=ws[n:2 * n], part3=ws[2 * n:3 * n])
    out.update(ln)
    return out


def _same(a, b, what, nonzero=True):
    for k in OUT9 + LN6:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k].float() - b[k].float()).abs().max()))
    for k in ("d_o", "d_pre_f", "d_ao", "d_res1", "d_att", "part1", "part2", "dg1", "db2"):      # not vacuous: written, finite
        assert torch.isfinite(a[k].float()).all(), (what, k)
        assert not nonzero or float(a[k].float().abs().sum()) > 0, (what, k)      # (no kept slot at all: every gradient is zero)


@pytest.mark.parametrize("inv_mode", ["none", "some", "all", "null"])
@pytest.mark.parametrize("drop", [0.0, 0.1])
def test_head_block_is_bit_identical_on_the_shape_grid(inv_mode, drop):
    """head = 1: the compaction map drops no slot, some slots, every slot of sample 0, or is absent"""
    for B, T, M in GRID:
        d = _inputs(B, T, M, inv_mode=inv_mode, seed=1)
        a, b = _bwd(d, 0, drop), _bwd(d, 1, drop)
        _same(a, b, (inv_mode, drop, B, T, M), nonzero=d["kept"] > 0)
        if d["kept"] > 0:
            assert float(a["d_pre_t"].float().abs().sum()) > 0 and float(a["part3"].abs().sum()) > 0


@pytest.mark.parametrize("drop", [0.0, 0.1])
def test_block_without_the_head_is_bit_identical_on_the_shape_grid(drop):
    """head = 0 (a block that is not the last): d_y_in is the upstream gradient"""
    for B, T, M in GRID:
        if M != 1:
            continue
        d = _inputs(B, T, M, head=0, seed=2)
        _same(_bwd(d, 0, drop), _bwd(d, 1, drop), (drop, B, T))


@pytest.mark.parametrize("T", [5, 17, 101])
def test_repeated_masked_positions_are_summed_in_the_same_order(T):
    """positions named two and three times by one sample: the chains (ascending j), with some of their links dropped"""
    B, M = 3, 20
    g = torch.Generator().manual_seed(T)
    mpos = torch.stack([torch.randperm(max(T, M), generator=g)[:M] % T for _ in range(B)])
    mpos[0, 3] = mpos[0, 11] = mpos[0, 0]                       # three times
    mpos[0, 7] = mpos[0, 5]                                     # twice
    mpos[1, 19] = mpos[1, 18] = mpos[1, 17]                     # three times, adjacent slots, at the end
    mpos[2, 1] = mpos[2, 0]                                     # twice, at the start
    for inv_mode in ("none", "some", "null"):
        d = _inputs(B, T, M, inv_mode=inv_mode, mpos=mpos, seed=3)
        _same(_bwd(d, 0, 0.1), _bwd(d, 1, 0.1), (T, inv_mode))


def test_channel_padded_block_is_bit_identical():
    """head dim 50 stored as 64 (dh_pad / dh_true): the LayerNorm moments of the real channels, nothing into the padded ones"""
    for head in (1, 0):
        d = _inputs(3, 17, 20, head=head, seed=4)
        for k in ("g1", "g2", "g3"):      # (gamma is zero on a padded channel)
            d[k] = d[k] * ((torch.arange(128, device="cuda") % 64) < 50)
        a, b = _bwd(d, 0, 0.1, pad=(64, 50)), _bwd(d, 1, 0.1, pad=(64, 50))
        _same(a, b, ("padded", head))
        assert float(a["d_res1"].float().view(3, 17, 2, 64)[..., 50:].abs().max()) == 0.0


@pytest.mark.parametrize("T,C", [(102, 128), (101, 64)])
def test_shapes_outside_the_form_take_the_one_per_cu_kernel_under_either_variant(T, C):
    d = _inputs(3, T, 20, C=C, seed=5)
    _same(_bwd(d, 0, 0.1), _bwd(d, 1, 0.1), (T, C))


def test_more_than_112_gathered_rows_fall_back_to_the_one_per_cu_kernel():
    """M = 113, head = 1: the two-per-CU kernel stages at most 112 rows and has no unstaged path, so variant 1 must dispatch to
    tail_bwd_kernel.  Against M = 112 at the same shape, which does take the two-per-CU kernel under variant 1: the pair pins
    the `M <= 112` clause of the dispatch from both sides (run in the wrong kernel, 113 rows would be gathered wrongly, not refused)."""
    for M in (112, 113):
        for inv_mode in ("some", "null"):
            d = _inputs(3, 101, M, inv_mode=inv_mode, seed=7)
            _same(_bwd(d, 0, 0.1), _bwd(d, 1, 0.1), (M, inv_mode))


# ---- forward-only edge cases of t2::tail2_fwd_kernel: one row, a full row tile, one row into the second, the longest sequence ----------
FWD_OUT = ("ao", "a1", "st1", "pre_f", "f", "o", "y", "st2", "pre_t", "so", "st3", "hrows")


def _fwd(d, variant, drop):
    from easydgl_amd import _lib
    from easydgl_amd.ops import _ptr, _stream
    lib = _lib.lib
    B, T, M, C = d["B"], d["T"], d["M"], d["C"]
    dev = "cuda"
    pack = torch.empty(int(lib.edgl_tail_pack_elems(C)), dtype=torch.bfloat16, device=dev)
    _lib.check(lib.edgl_tail_pack(_ptr(d["Wo"]), _ptr(d["Wi"]), _ptr(d["Wout"]), _ptr(d["Wt"]), C, _ptr(pack), _stream()), "edgl_tail_pack")
    out = {k: torch.zeros(B, T, 2 * C if k in ("pre_f", "f") else C, dtype=torch.bfloat16, device=dev)
           for k in ("ao", "a1", "pre_f", "f", "o", "y", "pre_t", "so")}
    out.update({k: torch.zeros(B, 2, dtype=torch.float32, device=dev) for k in ("st1", "st2", "st3")})
    out["hrows"] = torch.zeros(B * M, C, dtype=torch.bfloat16, device=dev)
    bias = {k: d["g1"] * 0.1 + i for i, k in enumerate(("bo", "bout", "bt", "b1", "b2", "b3"))}
    bi = torch.cat([d["g2"], d["g3"]]) * 0.1
    prev = lib.edgl_tail_variant(variant)
    try:
        _lib.check(lib.edgl_tail_fwd_ct(
            _ptr(d["a1"]), _ptr(d["xin"]), d["ld_x"], _ptr(pack), _ptr(bias["bo"]), _ptr(bi), _ptr(bias["bout"]), _ptr(bias["bt"]),
            _ptr(d["g1"]), _ptr(bias["b1"]), _ptr(d["g2"]), _ptr(bias["b2"]), _ptr(d["g3"]), _ptr(bias["b3"]), B, T, C, float(drop),
            _ptr(d["rng"]), 11, 12, _ptr(d["mpos"]), M, 1, _ptr(out["ao"]), _ptr(out["a1"]), _ptr(out["st1"]), _ptr(out["pre_f"]),
            _ptr(out["f"]), _ptr(out["o"]), _ptr(out["y"]), _ptr(out["st2"]), _ptr(out["pre_t"]), _ptr(out["so"]), _ptr(out["st3"]),
            _ptr(out["hrows"]), _ptr(d["inv"]), 0, 0, _lib.BF16, _stream()), "edgl_tail_fwd_ct")
        torch.cuda.synchronize()
    finally:
        lib.edgl_tail_variant(prev)
    return out


@pytest.mark.parametrize("T", [1, 16, 17, 101])
def test_forward_row_tile_edges_are_bit_identical(T):
    for B, M in ((1, 1), (5, 20)):
        d = _inputs(B, T, M, inv_mode="some", seed=6)
        a, b = _fwd(d, 0, 0.1), _fwd(d, 1, 0.1)
        for k in FWD_OUT:
            assert torch.equal(a[k], b[k]), (T, B, M, k, float((a[k].float() - b[k].float()).abs().max()))
        assert torch.isfinite(a["y"].float()).all() and float(a["y"].float().abs().sum()) > 0


# ---- the engine, three steps, both forms -------------------------------------------------------------------------------------------------
def _engine_run(probs, variant, deterministic):
    from easydgl_amd import _lib
    from easydgl_amd.engine import TrainEngine
    prev = _lib.lib.edgl_tail_variant(variant)
    try:
        m = build_model(probs[0], "bf16", hidden_drop=0.1, att_drop=0.1)
        eng = TrainEngine(m, 4, use_graph=False, deterministic=deterministic)
        assert eng.fused_tail and eng.T == 31
        losses = []
        for p in probs:
            losses.append(eng.step(to_dev(p["feats"]), torch.as_tensor(p["labels"]).cuda()).clone())
            torch.cuda.synchronize()
        m.settle_state()
        return losses, m._arena.detach().clone()
    finally:
        _lib.lib.edgl_tail_variant(prev)


@pytest.mark.parametrize("deterministic", [True, False])
def test_engine_three_steps_under_both_forms(deterministic):
    """B = 4, T = 31.  Deterministic mode: losses and weights bit for bit.  Otherwise the f32 atomics of the embedding scatter land in
    another order from run to run: the trajectory bound of tests/test_gpu_engine.py (1e-5 relative on every loss) and, on the weights,
    the one-step bound of tests/test_gpu_loader_engine.py (1e-6 absolute) for each of the three steps."""
    kw = dict(num_units=128, num_heads=8, num_blocks=1, seqslen=30, masklen=6, num_events=16, num_items=700)
    probs = [make_problem(seed=640 + i, batch=4, **kw) for i in range(3)]
    (la, wa), (lb, wb) = _engine_run(probs, 0, deterministic), _engine_run(probs, 1, deterministic)
    print("losses", [float(x) for x in la], [float(x) for x in lb], "max |d w|", float((wa - wb).abs().max()))
    assert all(torch.isfinite(x) for x in la)
    if deterministic:
        assert all(torch.equal(x, y) for x, y in zip(la, lb)) and torch.equal(wa, wb)
    else:
        assert all(abs(float(x) - float(y)) <= 1e-5 * abs(float(x)) for x, y in zip(la, lb))
        assert float((wa - wb).abs().max()) <= 3e-6
