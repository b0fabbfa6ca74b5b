"""Evaluation by label rank (csrc/k_eval_rank.hip; Sequential.eval, Base.py:150-201): the place of the true next item in the
(logit desc, item id asc) order of the unseen catalogue as a COUNT, against an fp64 reference on the same operands, against the
lists of the top-K kernels, and through the models and the driver.

  (a) integer operands: every logit is exact in f32 whatever the accumulation order and ties are everywhere -> exact equality
  (b) duplicated items with real-valued operands: the label's value must be the bits the counting pass forms (the arithmetic rule)
  (c) real-valued operands: the rank lies in the bracket the reference leaves open at ORDER_GAP (test_gpu_eval_fused.py's figure:
      a reference gap above it cannot be reordered by f32 accumulation order)
  (d) the tile form (f32, C = 32, C = 512) against the same logits tiles in torch, and rank_from_logits against edgl_mask_topk
  (e) range additivity and table shards  (f) metric sums, models  (g) driver  (h) graph capture"""
import numpy as np
import pytest
import torch

from tests._util import build_model, make_problem, to_dev

pytestmark = pytest.mark.gpu

BF16 = 1
ORDER_GAP = 2e-4
FUSED_SHAPES = [(70, 64, 4099, 7), (70, 128, 4099, 1), (130, 256, 4500, 7)]


def ops():
    from easydgl_amd import ops as _ops
    return _ops


def lib():
    from easydgl_amd import _lib
    return _lib.lib


def _slice_items(R, C, I, T):
    """Items per slice of the fused plan (tiles of 128 items, 64 at C = 256)."""
    nz = 64 if C == 256 else 128
    ns = lib().edgl_score_rank_slices(R, C, min(I, 262144), T)
    ntile = (min(I, 262144) + nz - 1) // nz
    return (ntile + ns - 1) // ns * nz, ns


def _ref_logits(rows, table, bias):
    t = table.double().cpu().numpy().copy()
    t[0] = 0.0                                         # coding.py:56-57: the used table's row 0 is the zero constant
    return rows.double().cpu().numpy() @ t.T + np.concatenate([[-1000.0], bias.double().cpu().numpy()])


def _masked(lg, seen):
    lg = lg.copy()
    if seen is not None:
        s = seen.cpu().numpy()
        for r in range(lg.shape[0]):
            lg[r, s[r]] = -np.inf
    return lg


def _ref_rank(lg, seen, labels, i0=0, i1=None):
    """The lexsort((ids, -v)) position of the label among the items of [i0, i1) and itself."""
    v = _masked(lg, seen)
    i1 = v.shape[1] if i1 is None else i1
    y = labels.cpu().numpy()
    j = np.arange(i0, i1)
    out = np.empty(len(y), dtype=np.int64)
    for r in range(len(y)):
        vy = v[r, y[r]]
        out[r] = int((((v[r, j] > vy) | ((v[r, j] == vy) & (j < y[r]))) & (j != y[r])).sum())
        if (i0, i1) == (0, v.shape[1]):
            order = np.lexsort((np.arange(v.shape[1]), -v[r]))
            assert order[out[r]] == y[r]
    return out


def _int_problem(R, C, I, T, seed, dtype=torch.bfloat16):
    rng = np.random.default_rng(seed)
    rows = torch.tensor(rng.integers(-2, 3, size=(R, C)), dtype=dtype).cuda()
    table = torch.tensor(rng.integers(-2, 3, size=(I, C)), dtype=dtype).cuda()
    bias = torch.tensor(rng.integers(-32, 33, size=I - 1) * 0.25, dtype=torch.float32).cuda()
    seen = rng.integers(0, I, size=(R, T)) if T else None
    labels = rng.integers(0, I, size=R)
    sl, _ = _slice_items(R, C, I, T) if dtype == torch.bfloat16 and C in (64, 128, 256) else (I // 2 // 8 * 8, 0)
    labels[:4] = (0, I - 1, sl, sl - 1)                # item 0, the MASK column, the first and the last item of a slice
    if T:
        labels[4] = seen[4, 0]                             # labels that are themselves seen
        if R > 7:
            labels[5] = seen[5, T - 1]
            seen[6, 0], seen[6, T - 1] = 0, I - 1
        if T > 1:
            seen[:, T - 1] = np.where(np.arange(R) % 3 == 0, seen[:, 0], seen[:, T - 1])      # duplicated seen ids
            if R > 7:
                seen[7, 1] = labels[7]
    return rows, table, bias, (torch.tensor(seen).cuda() if T else None), torch.tensor(labels).cuda()


def _real_problem(R, C, I, T, seed, dtype=torch.bfloat16):
    """The distribution of test_gpu_eval_fused.py::_problem."""
    rng = np.random.default_rng(seed)
    rows = torch.tensor(rng.standard_normal((R, C)) * 0.5, dtype=dtype).cuda()
    table = torch.tensor(rng.standard_normal((I, C)) * 0.3, dtype=dtype).cuda()
    bias = torch.tensor(rng.standard_normal(I - 1) * 0.2, dtype=torch.float32).cuda()
    seen = rng.integers(0, I, size=(R, T))
    labels = rng.integers(1, I - 1, size=R)
    for r in range(R):
        while labels[r] in seen[r]:
            labels[r] = labels[r] % (I - 2) + 1
    return rows, table, bias, torch.tensor(seen).cuda(), torch.tensor(labels).cuda()


def _check_against_topk(o, rank, rows, table, bias, seen, labels, K=100):
    """For every row with rank < K the label sits at position `rank` of score_topk's list, fused and unfused."""
    I = table.shape[0]
    rk, y = rank.cpu().numpy(), labels.cpu().numpy()
    was = o.EVAL_FUSED
    try:
        for fused in (True, False):
            o.EVAL_FUSED = fused
            _, idx = o.score_topk(rows, table, bias, seen, K, 0, I)
            idx = idx.cpu().numpy()
            for r in np.where(rk < K)[0]:
                assert idx[r, rk[r]] == y[r], (fused, r, rk[r], y[r])
    finally:
        o.EVAL_FUSED = was
    assert (rk < K).sum() >= 1


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C,I,T", FUSED_SHAPES + [(33, 128, 4099, 0), (8, 64, 270001, 7)])
def test_integer_operands_give_the_reference_rank_exactly(R, C, I, T):
    o = ops()
    rows, table, bias, seen, labels = _int_problem(R, C, I, T, seed=R + I + T)
    assert lib().edgl_score_rank_supported(R, C, min(I, o.RANK_FUSED_ITEMS), T, BF16) == 1
    assert lib().edgl_score_rank_slices(R, C, min(I, o.RANK_FUSED_ITEMS), T) >= 2
    lg = _ref_logits(rows, table, bias)
    v = _masked(lg, seen)
    rng = np.random.default_rng(R)
    for r in [6] + list(range(8, R, 2)):                         # labels near the top too: the rows whose rank the lists can confirm
        labels[r] = int(np.lexsort((np.arange(I), -v[r]))[rng.integers(0, 100 if r == 6 else 150)])
    rank = o.score_label_rank(rows, table, bias, seen, labels)
    assert rank.dtype == torch.int32 and rank.shape == (R,)
    want = _ref_rank(lg, seen, labels)
    got = rank.cpu().numpy()
    assert np.array_equal(got, want), np.where(got != want)[0][:10]
    _check_against_topk(o, rank, rows, table, bias, seen, labels)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
DUP_CASES = [(70, 64, 4099, 7, torch.bfloat16, None), (70, 128, 4099, 7, torch.bfloat16, None), (130, 256, 4500, 7, torch.bfloat16, None),
             (6, 32, 4099, 5, torch.bfloat16, 1024), (6, 32, 4099, 5, torch.float32, 1024), (6, 512, 4099, 5, torch.bfloat16, 1024)]


@pytest.mark.parametrize("R,C,I,T,dtype,chunk", DUP_CASES)
def test_duplicated_items_tie_with_the_label_exactly(R, C, I, T, dtype, chunk, monkeypatch):
    """Five items share one table row and one bias: a0 < a1 < a2 < a3 unseen, each in another tile / slice (tile form: another
    chunk), and one in every row's seen set.  Rows come in identical pairs, the first with label a1, the second with label a2: the
    second label has exactly one more item in front of it (a1).  One bit of difference between the label's value and the value the
    counting pass forms for a copy moves a copy to the wrong side."""
    o = ops()
    if chunk:
        monkeypatch.setattr(o, "EVAL_TILE_BYTES", 4 * R * chunk)
    rows, table, bias, seen, labels = _real_problem(R, C, I, T, seed=C + I, dtype=dtype)
    a = np.array([37, 1203, 2311, 3467, 4097])                   # a0..a3, a_seen
    table[torch.tensor(a[1:]).cuda()] = table[a[0]].clone()
    bias[torch.tensor(a[1:] - 1).cuda()] = bias[a[0] - 1].clone()
    rows[1::2] = rows[0:R - 1:2][:rows[1::2].shape[0]].clone()
    s = seen.cpu().numpy()
    s[np.isin(s, a[:4])] = 5                                     # the unseen copies stay unseen
    s[:, 0] = a[4]
    s[1::2] = s[0:R - 1:2][:s[1::2].shape[0]].copy()
    seen = torch.tensor(s).cuda()
    npair = R // 2
    lab = np.empty(R, dtype=np.int64)
    lab[0::2], lab[1::2] = a[1], a[2]
    if R % 2:
        lab[R - 1] = a[3]
    labels = torch.tensor(lab).cuda()
    fused = dtype == torch.bfloat16 and C in (64, 128, 256)
    assert bool(lib().edgl_score_rank_supported(R, C, I, T, BF16 if dtype == torch.bfloat16 else 0)) == fused
    got = o.score_label_rank(rows, table, bias, seen, labels).cpu().numpy()
    low, high = got[0:2 * npair:2], got[1:2 * npair:2]
    print("rank(a2) - rank(a1):", (high - low).tolist()[:16])
    assert np.array_equal(high - low, np.ones(npair, dtype=got.dtype))
    # ... and the rank itself: the reference's count of the other unseen items (bracket of (c)) + the unseen copies below the label
    v = _masked(_ref_logits(rows, table, bias), seen)
    others = np.setdiff1d(np.arange(I), a)
    for r in range(R):
        vy = v[r, lab[r]]
        lo = int((v[r, others] > vy + ORDER_GAP).sum()) + int((a[:4] < lab[r]).sum())
        hi = int((v[r, others] >= vy - ORDER_GAP).sum()) + int((a[:4] < lab[r]).sum())
        assert lo <= got[r] <= hi, (r, lo, got[r], hi)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C,I,T", FUSED_SHAPES)
def test_real_operands_rank_within_the_reference_bracket(R, C, I, T):
    o = ops()
    rows, table, bias, seen, labels = _real_problem(R, C, I, T, seed=R + C)
    got = o.score_label_rank(rows, table, bias, seen, labels).cpu().numpy()
    v = _masked(_ref_logits(rows, table, bias), seen)
    y = labels.cpu().numpy()
    width = []
    for r in range(R):
        vy = v[r, y[r]]
        oth = np.delete(v[r], y[r])                              # (seen items are at -inf: in neither count)
        lo, hi = int((oth > vy + ORDER_GAP).sum()), int((oth >= vy - ORDER_GAP).sum())
        width.append(hi - lo)
        assert lo <= got[r] <= hi, (r, lo, got[r], hi)
    print("bracket widths: max", max(width), "share lo == hi", np.mean(np.array(width) == 0))


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
def _torch_rank(v, seen, labels, i0=0):
    """Rank on the GPU from f32 logits [R, n] of the items [i0, i0 + n): the same bits, the same rule."""
    R, n = v.shape
    v = v.clone()
    j = torch.arange(i0, i0 + n, device=v.device)[None]
    if seen is not None:
        for t in range(seen.shape[1]):
            v = torch.where(j == seen[:, t:t + 1], torch.full_like(v, float("-inf")), v)
    y = labels[:, None]
    vy = torch.gather(v, 1, y - i0)
    return (((v > vy) | ((v == vy) & (j < y))) & (j != y)).sum(1).to(torch.int32)


@pytest.mark.parametrize("R,C,I,T,dtype", [(5, 32, 300, 3, torch.float32), (5, 32, 300, 3, torch.bfloat16), (9, 512, 700, 4, torch.bfloat16)])
@pytest.mark.parametrize("integer", [True, False])
def test_tile_form_counts_on_the_bits_of_its_logits_tiles(R, C, I, T, dtype, integer, monkeypatch):
    o = ops()
    chunk = 104 if I == 300 else 240
    monkeypatch.setattr(o, "EVAL_TILE_BYTES", 4 * R * chunk)
    rows, table, bias, seen, labels = (_int_problem if integer else _real_problem)(R, C, I, T, seed=I + C, dtype=dtype)
    if not integer:
        labels[0], labels[1] = I - 2, chunk + 3
    assert lib().edgl_score_rank_supported(R, C, I, T, BF16 if dtype == torch.bfloat16 else 0) == 0
    bounds = [(lo, min(I, lo + chunk)) for lo in range(0, I, chunk)]
    assert len(bounds) >= 3 and int((labels >= chunk).sum()) >= 1
    tiles = [o.score_lse(rows, table, bias, None, lo, hi, want_logits=True, want_lse=False)[2] for lo, hi in bounds]
    want = _torch_rank(torch.cat(tiles, dim=1), seen, labels)
    got = o.score_label_rank(rows, table, bias, seen, labels)
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    if integer:
        assert np.array_equal(got.cpu().numpy(), _ref_rank(_ref_logits(rows, table, bias), seen, labels))
    # a range of the catalogue (a table shard): labels outside it still get their value
    part = o.score_label_rank(rows, table, bias, seen, labels, 104, 208) + o.score_label_rank(rows, table, bias, seen, labels, 0, 104) \
        + o.score_label_rank(rows, table, bias, seen, labels, 208, I)
    assert torch.equal(part, want)


@pytest.mark.parametrize("integer", [True, False])
def test_rank_from_logits_is_the_position_in_mask_topk(integer):
    o = ops()
    rng = np.random.default_rng(5)
    B, I, T = 9, 9001, 6
    lg = rng.integers(-6, 7, size=(B, I)).astype(np.float32) if integer else rng.standard_normal((B, I)).astype(np.float32)
    lg[0] = -np.abs(lg[0]) - 1.0
    lg[0, :10] = 0.0
    lg[0, 3] = -0.0                                            # -0.0 == +0.0
    logits = torch.tensor(lg).cuda()
    seen = torch.tensor(rng.integers(0, I, size=(B, T))).cuda()
    order = np.lexsort((np.broadcast_to(np.arange(I), (B, I)), -_masked(lg.astype(np.float64), seen)), axis=1)
    lab = order[np.arange(B), rng.integers(0, 128, size=B)]      # labels inside the top 128 ...
    lab[0], lab[1], lab[2] = 3, order[1, 500], int(seen[2, 0])   # ... a signed zero, one far outside, a seen one
    labels = torch.tensor(lab).cuda()
    keep = logits.clone()
    rank = o.rank_from_logits(logits, 0, seen, labels)
    assert torch.equal(logits, keep)                             # the logits are not modified
    assert np.array_equal(rank.cpu().numpy(), _ref_rank(lg.astype(np.float64), seen, labels))
    _, idx = o.mask_topk(logits.clone(), 0, seen, 128)
    rk, idx = rank.cpu().numpy(), idx.cpu().numpy()
    assert rk[0] <= 3 and (rk < 128).sum() >= B - 2
    for r in np.where(rk < 128)[0]:
        assert idx[r, rk[r]] == lab[r], (r, rk[r])


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------
def test_counts_add_over_item_ranges():
    o = ops()
    R, C, I, T = 70, 128, 4099, 7
    rows, table, bias, seen, labels = _int_problem(R, C, I, T, seed=1)
    full = o.score_label_rank(rows, table, bias, seen, labels)
    i1 = 2056                                                    # a multiple of 8 inside a slice
    assert i1 % _slice_items(R, C, I, T)[0] not in (0,) and i1 % 8 == 0
    a, b = o.score_label_rank(rows, table, bias, seen, labels, 0, i1), o.score_label_rank(rows, table, bias, seen, labels, i1, I)
    assert torch.equal(a + b, full)
    lg = _ref_logits(rows, table, bias)
    assert np.array_equal(a.cpu().numpy(), _ref_rank(lg, seen, labels, 0, i1))
    assert np.array_equal(b.cpu().numpy(), _ref_rank(lg, seen, labels, i1, I))


@pytest.fixture(scope="module")
def bf16_model():
    prob = make_problem(seed=4, batch=12, num_items=4200, seqslen=20, num_units=128, num_heads=2, num_blocks=1)
    return prob, build_model(prob, "bf16")


def test_sharded_rank_is_the_unsharded_rank_and_the_op_on_the_encoder_rows(bf16_model):
    prob, m = bf16_model
    o = ops()
    ef, el = to_dev(prob["efeats"]), torch.as_tensor(prob["elabels"]).cuda()
    rank = m.eval_rank(ef, el, mask_seen=True)
    for world in (3, 8):
        assert torch.equal(m.eval_rank_sharded(ef, el, mask_seen=True, world=world), rank)
    rows, _ = m.encoder(ef, False, m._gather_pos(ef, False))
    assert rows.dtype == torch.bfloat16
    want = o.score_label_rank(rows, m.compute(m.item_embs.lookup_table), m.output_bias, ef["seqs_i"], el[:, -1].contiguous())
    assert torch.equal(rank, want)


# ---- (f) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", [(10, 50, 100), (1, 5, 500)])
def test_metric_sums_from_ranks(ks):
    from tests.test_cpu_eval_rank import metrics_from_rank
    o = ops()
    I = 20001
    rng = np.random.default_rng(2)
    rk = np.concatenate([[0, 9, 10, 49, 50, 99, 100, I - 1], rng.integers(0, 700, size=700)]).astype(np.int32)
    sums = torch.zeros(2 * len(ks) + 1, device="cuda")
    kd = torch.tensor(ks, dtype=torch.int32).cuda()
    o.rank_metrics_from_rank(torch.tensor(rk).cuda(), kd, sums)
    want = metrics_from_rank(rk, ks)
    got = sums.cpu().numpy()
    nk = len(ks)
    assert got[:nk].tolist() == want[:nk]
    np.testing.assert_allclose(got[nk:], want[nk:], rtol=1e-6)
    o.rank_metrics_from_rank(torch.tensor(rk).cuda(), kd, sums)              # += : a second batch
    np.testing.assert_allclose(sums.cpu().numpy(), 2 * np.array(want), rtol=1e-6)


SIX = ("H10", "H50", "H100", "N10", "N50", "N100")


def _two_paths(m, batches):
    m.reset_metrics()
    for f, l in batches:
        m.eval_step(f, l)
    base = m.metrics()
    assert tuple(base) == SIX                                    # the default path: exactly today's six keys
    m.reset_metrics()
    for f, l in batches:
        m.eval_step(f, l, by_rank=True)
    by = m.metrics()
    assert tuple(by) == SIX + ("MRR",) and 0.0 < by["MRR"] <= 1.0
    for k in SIX:
        if k[0] == "H":
            assert by[k] == base[k], (k, by[k], base[k])
        else:
            assert abs(by[k] - base[k]) <= 1e-6 * max(base[k], 1e-30), (k, by[k], base[k])
    return by


def test_model_metrics_by_rank_equal_the_default_path_easydgl():
    prob = make_problem(seed=3, batch=12, num_items=300, seqslen=20, num_units=32, num_heads=2, num_blocks=1)
    m = build_model(prob, "f32")
    ef, el = to_dev(prob["efeats"]), torch.as_tensor(prob["elabels"]).cuda()
    halves = [({k: v[:6].contiguous() for k, v in ef.items()}, el[:6].contiguous()),
              ({k: v[6:].contiguous() for k, v in ef.items()}, el[6:].contiguous())]
    _two_paths(m, halves)
    m.reset_metrics(ks=(1, 500))
    m.eval_step(*halves[0], by_rank=True)
    got = m.metrics()
    assert tuple(got) == ("H1", "H500", "N1", "N500", "MRR") and got["H500"] == 1.0
    with pytest.raises(RuntimeError):
        m.eval_step(*halves[1])                                  # one accumulation holds one kind of step


def test_model_metrics_by_rank_equal_the_default_path_ctsma():
    from tests.test_gpu_ctsma import _model, _problem
    prob = _problem(7, B=12, T=20, C=32, h=2, E=4, I=300, nb=1)
    m = _model(prob, "f32")
    feats, tok = to_dev(prob["feats"]), torch.as_tensor(prob["tokens"]).cuda()
    halves = [({k: v[:6].contiguous() for k, v in feats.items()}, tok[:6].contiguous()),
              ({k: v[6:].contiguous() for k, v in feats.items()}, tok[6:].contiguous())]
    _two_paths(m, halves)


# ---- (g) ---------------------------------------------------------------------------------------------------------------------------
def test_driver_evaluate_by_rank_equals_the_default():
    from easydgl_amd import train
    prob = make_problem(seed=6, batch=20, num_items=300, seqslen=20, num_units=32, num_heads=2, num_blocks=1)
    m = build_model(prob, "f32")
    ids, ts = np.asarray(prob["ids"]), np.asarray(prob["ts"], dtype=np.float32)
    base = train.evaluate(m, ids, ts, 8, True)
    by = train.evaluate(m, ids, ts, 8, True, by_rank=True)
    assert tuple(base) == SIX and tuple(by) == SIX + ("MRR",)
    for k in SIX:
        if k[0] == "H":
            assert by[k] == base[k], (k, by[k], base[k])
        else:
            assert abs(by[k] - base[k]) <= 1e-6 * max(base[k], 1e-30), (k, by[k], base[k])


# ---- (h) ---------------------------------------------------------------------------------------------------------------------------
def test_score_label_rank_replays_in_a_graph():
    o = ops()
    R, C, I, T = 70, 64, 4099, 7
    rows, table, bias, seen, labels = _int_problem(R, C, I, T, seed=8)
    rows2, table2, bias2, seen2, labels2 = _int_problem(R, C, I, T, seed=9)
    eager = o.score_label_rank(rows2, table2, bias2, seen2, labels2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        o.score_label_rank(rows, table, bias, seen, labels)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = o.score_label_rank(rows, table, bias, seen, labels)
    for dst, src in ((rows, rows2), (table, table2), (bias, bias2), (seen, seen2), (labels, labels2)):
        dst.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
