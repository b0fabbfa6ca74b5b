"""Evaluation on candidate lists (csrc/k_eval_cand.hip): every row scores its OWN list of item ids.

  (a) integer operands: every value is exact in f32 in any order and ties are everywhere -> count, label_val and scores bit for bit
  (b) the order is the full sweep's: with cand = arange(I) the count equals score_label_rank / rank_from_logits
  (c) real-valued operands: |scores - s64| <= (C + 2) 2^-24 (|b| + sum |x w|) (an f32 FMA chain in any order; bf16 products are
      exact in f32), and the count equals the count recomputed from the returned values
  (d) slot independence  (e) the sampler against its numpy replica  (f) the four models  (g) the driver
The references are tests/_cand_ref.py, written from the definition."""
import math
import pickle

import numpy as np
import pytest
import torch

from tests import _cand_ref as CR
from tests._util import build_model, make_problem, to_dev

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f32": torch.float32}
DUPS = ((5, 60), (7, 90), (20, 21), (33, 80))        # (id, a second id with the same table row and bias)


def ops():
    from easydgl_amd import ops as _ops
    return _ops


def _f64(t):
    return t.detach().double().cpu().numpy()


def _int_problem(R, C, I, T, N, seed, dtype):
    """rows / table in {-2..2}, biases in multiples of 0.25, duplicated items, lists with -1 slots, id 0, seen ids, the label (once,
    twice), repeated ids and a seen label.  Rows 3 and 4 (R >= 5): one query, one list, the two copies of one item as labels."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(-2, 3, size=(R, C))
    table = rng.integers(-2, 3, size=(I, C))
    bias = rng.integers(-32, 33, size=I - 1) * 0.25
    for a, b in DUPS:
        table[b], bias[b - 1] = table[a], bias[a - 1]
    cand = rng.integers(0, I, size=(R, N))               # (N > I: repeated ids everywhere)
    cand[rng.random((R, N)) < 0.1] = -1
    seen = rng.integers(0, I, size=(R, T)) if T else None
    labels = rng.integers(1, I, size=R)
    cand[0, N // 2] = labels[0]                                                  # the label once
    if R > 1:
        cand[1, 0] = cand[1, N - 1] = labels[1]                                  # ... and twice (N = 1: once)
    if R > 2 and T:
        labels[2] = seen[2, 0]                                                   # a label that is seen
    if R >= 5:
        a, b = DUPS[2]                                                           # neighbouring ids: no third id can tie between them
        rows[4] = rows[3]
        cand[3][cand[3] == a] = a - 1
        cand[3, N // 3] = a                                                      # the lower copy exactly once
        cand[4] = cand[3]
        labels[3], labels[4] = a, b
        if T:
            seen[3][(seen[3] == a) | (seen[3] == b)] = 1
            seen[4] = seen[3]
        for r, y in zip(range(5, R), (b, a, DUPS[0][1], DUPS[0][0], DUPS[3][1], DUPS[1][0])):
            labels[r] = y
        for r in range(8, R):
            cand[r, N - 1] = 0                                                   # item 0: the zero row with bias -1000
            if T and N > 2:
                cand[r, 1] = seen[r, T - 1]                                      # a seen id in the list
    dev = lambda a, dt: torch.tensor(a, dtype=dt).cuda()
    return (dev(rows, dtype), dev(table, dtype), dev(bias, torch.float32), dev(cand, torch.int32),
            dev(seen, torch.int64) if T else None, dev(labels, torch.int64))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_exact(R, C, I, T, N, seed, dtype):
    o = ops()
    rows, table, bias, cand, seen, labels = _int_problem(R, C, I, T, N, seed, dtype)
    scores, label_val, count = o.score_candidates(rows, table, bias, cand, seen, labels)
    c_np, s_np, y_np = cand.cpu().numpy(), None if seen is None else seen.cpu().numpy(), labels.cpu().numpy()
    sc, lv, cnt, _, _ = CR.reference(_f64(rows), _f64(table), _f64(bias), c_np, s_np, y_np)
    tag = (R, C, T, N)
    assert np.array_equal(count.cpu().numpy(), cnt), tag
    assert np.array_equal(_bits(label_val.cpu().numpy()), _bits(lv)), tag
    assert np.array_equal(_bits(scores.cpu().numpy()), _bits(sc)), tag
    if R >= 5:
        assert int(count[4]) - int(count[3]) == 1, tag                           # the two copies of one item: by id alone
    assert scores.dtype == torch.float32 and count.dtype == torch.int32
    # outputs are optional: the count alone, the scores alone
    _, _, count2 = o.score_candidates(rows, table, bias, cand, seen, labels, want_scores=False)
    assert torch.equal(count2, count)
    s3, lv3, c3 = o.score_candidates(rows, table, bias, cand, seen)
    assert torch.equal(s3.view(torch.int32), scores.view(torch.int32)) and lv3 is None and c3 is None


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 32, 64, 128, 256, 512])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_exact_ranks_ties_included(dt, C):
    """N = 65 and 1030 cross the workgroup's chunk (64 slots at these R: edgl_score_candidates_chunk), 63 / 64 its edge."""
    seed = 0
    for R in (1, 3, 33):
        for N in (1, 63, 64, 65, 101, 1030):
            for T in (0, 1, 7, 100):
                seed += 1
                _check_exact(R, C, 97, T, N, seed, DT[dt])


@pytest.mark.parametrize("dt,C,R,N", [("bf16", 16, 33, 16500), ("f32", 48, 9, 700), ("bf16", 48, 9, 700), ("f32", 272, 9, 130),
                                      ("bf16", 496, 9, 130)])
def test_exact_ranks_at_the_other_paths(dt, C, R, N):
    """The largest chunk (1024 slots: many slots per row), widths that are no power of two (lanes past the row idle) and f32 rows
    longer than 1 KB that do not fill their second piece."""
    from easydgl_amd import _lib
    if N == 16500:
        assert _lib.lib.edgl_score_candidates_chunk(R, C, N, 1) == 1024
    _check_exact(R, C, 97, 7, N, 1000 + C, DT[dt])


def test_ids_past_the_table_read_minus_inf():
    o = ops()
    rows, table, bias, cand, seen, labels = _int_problem(9, 64, 97, 7, 40, 5, torch.bfloat16)
    cand[:, 3] = 97
    cand[:, 4] = 2 ** 31 - 1
    scores, _, count = o.score_candidates(rows, table, bias, cand, seen, labels)
    sc, _, cnt, _, _ = CR.reference(_f64(rows), _f64(table), _f64(bias), cand.cpu().numpy(), seen.cpu().numpy(), labels.cpu().numpy())
    assert np.array_equal(_bits(scores.cpu().numpy()), _bits(sc)) and np.isinf(sc[:, 3:5]).all()
    assert np.array_equal(count.cpu().numpy(), cnt)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,C", [("bf16", 64), ("bf16", 128), ("f32", 64)])
def test_same_order_as_the_full_sweep(dt, C):
    o = ops()
    R, I, T = 33, 300, 7
    rows, table, bias, _, seen, labels = _int_problem(R, C, I, T, 8, 11, DT[dt])
    labels[:3] = torch.tensor([0, I - 1, 5]).cuda()
    cand = torch.arange(I, dtype=torch.int32).cuda().repeat(R, 1).contiguous()
    _, _, count = o.score_candidates(rows, table, bias, cand, seen, labels, want_scores=False)
    if dt == "bf16":
        want = o.score_label_rank(rows, table, bias, seen, labels)
    else:
        want = o.rank_from_logits(o.ScoreLogitsFn.apply(rows, table, bias, table), 0, seen, labels)
    assert torch.equal(count, want)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
def _real_problem(R, C, I, T, N, seed, dtype):
    rng = np.random.default_rng(seed)
    rows = torch.tensor(rng.standard_normal((R, C)) * 0.5, dtype=dtype).cuda()
    table = torch.tensor(rng.standard_normal((I, C)) * 0.3, dtype=dtype).cuda()
    bias = torch.tensor(rng.standard_normal(I - 1) * 0.2, dtype=torch.float32).cuda()
    cand = rng.integers(0, I, size=(R, N))
    cand[rng.random((R, N)) < 0.05] = -1
    seen = rng.integers(0, I, size=(R, T))
    labels = rng.integers(1, I, size=R)
    cand[:, 0] = np.where(np.arange(R) % 2 == 0, labels, cand[:, 0])
    return rows, table, bias, torch.tensor(cand, dtype=torch.int32).cuda(), torch.tensor(seen).cuda(), torch.tensor(labels).cuda()


def _within_bound(got, ref, mag, C):
    got = np.asarray(got, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)) and np.isfinite(got[fin]).all()
    err = np.abs(got[fin] - ref[fin])
    bound = (C + 2) * 2.0 ** -24 * mag[fin]
    print("worst error / bound:", float((err / bound).max()) if err.size else 0.0)
    assert (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("C", [16, 64, 128, 272, 512])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_real_valued_scores_within_the_f32_bound(dt, C):
    o = ops()
    R, I, T, N = 33, 300, 7, 101
    rows, table, bias, cand, seen, labels = _real_problem(R, C, I, T, N, 40 + C, DT[dt])
    scores, label_val, count = o.score_candidates(rows, table, bias, cand, seen, labels)
    c_np, y_np = cand.cpu().numpy(), labels.cpu().numpy()
    sc, lv, _, mg, lm = CR.reference(_f64(rows), _f64(table), _f64(bias), c_np, seen.cpu().numpy(), y_np)
    _within_bound(scores.cpu().numpy(), sc, mg, C)
    _within_bound(label_val.cpu().numpy(), lv, lm, C)
    s_np, l_np = scores.cpu().numpy(), label_val.cpu().numpy()
    want = [CR.count_before(s_np[r], l_np[r], c_np[r], int(y_np[r])) for r in range(R)]
    assert count.cpu().numpy().tolist() == want
    # the label's value is the value of its slot: the same bits
    for r in range(0, R, 2):
        assert _bits(s_np[r, :1])[0] == _bits(l_np[r:r + 1])[0]


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,C,N", [("bf16", 128, 101), ("f32", 64, 331), ("bf16", 512, 70)])
def test_slot_independence(dt, C, N):
    o = ops()
    R, I, T = 9, 300, 7
    rows, table, bias, cand, seen, labels = _real_problem(R, C, I, T, N, 7, DT[dt])
    scores, label_val, count = o.score_candidates(rows, table, bias, cand, seen, labels)
    rng = np.random.default_rng(3)
    perm = torch.tensor(np.stack([rng.permutation(N) for _ in range(R)])).cuda()
    s2, lv2, c2 = o.score_candidates(rows, table, bias, torch.gather(cand, 1, perm).contiguous(), seen, labels)
    assert torch.equal(s2.view(torch.int32), torch.gather(scores, 1, perm).view(torch.int32))
    assert torch.equal(lv2.view(torch.int32), label_val.view(torch.int32)) and torch.equal(c2, count)
    # the list in two halves, the two counts added into one buffer; another R and N around the same pairs: the same bits
    h = N // 2
    sa, _, buf = o.score_candidates(rows, table, bias, cand[:, :h].contiguous(), seen, labels)
    sb, _, buf = o.score_candidates(rows, table, bias, cand[:, h:].contiguous(), seen, labels, count=buf)
    assert torch.equal(buf, count)
    assert torch.equal(torch.cat([sa, sb], 1).view(torch.int32), scores.view(torch.int32))
    s1, lv1, c1 = o.score_candidates(rows[4:5].contiguous(), table, bias, cand[4:5].contiguous(), seen[4:5].contiguous(),
                                     labels[4:5].contiguous())
    assert torch.equal(s1.view(torch.int32), scores[4:5].view(torch.int32)) and torch.equal(c1, count[4:5])


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------
def _sampler_inputs(R, T, hi, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, hi, size=(R, T)), rng.integers(1, hi, size=R)


@pytest.mark.parametrize("R,T,n,hi", [(5, 7, 100, 65), (33, 100, 100, 809)])
def test_sampler_equals_the_replica(R, T, n, hi):
    o = ops()
    seen, labels = _sampler_inputs(R, T, hi, R)
    got = o.sample_negatives(torch.tensor(seen).cuda(), torch.tensor(labels).cuda(), n, 1, hi, 9876, step=0, row0=0)
    want, worst = CR.sample_negatives(seen, labels, n, 1, hi, 9876, 0, 0)
    print("worst attempt count:", worst)
    g = got.cpu().numpy()
    assert got.dtype == torch.int32 and g.shape == (R, n)
    assert np.array_equal(g, want)
    assert (g >= 1).all() and (g < hi).all()
    for r in range(R):
        assert not np.isin(g[r], seen[r]).any() and labels[r] not in g[r]
    for kw in (dict(step=1), dict(seed=9877), dict(seed=9876 + (1 << 32))):
        a = dict(seed=9876, step=0)
        a.update(kw)
        other = o.sample_negatives(torch.tensor(seen).cuda(), torch.tensor(labels).cuda(), n, 1, hi, a["seed"], step=a["step"])
        assert not torch.equal(other, got), kw
        assert np.array_equal(other.cpu().numpy(), CR.sample_negatives(seen, labels, n, 1, hi, a["seed"], a["step"], 0)[0]), kw


def test_sampler_lists_do_not_depend_on_the_batch_size():
    o = ops()
    seen, labels = _sampler_inputs(64, 7, 65, 1)
    s, l = torch.tensor(seen).cuda(), torch.tensor(labels).cuda()
    whole = o.sample_negatives(s, l, 100, 1, 65, 9876)
    a = o.sample_negatives(s[:24].contiguous(), l[:24].contiguous(), 100, 1, 65, 9876, row0=0)
    b = o.sample_negatives(s[24:].contiguous(), l[24:].contiguous(), 100, 1, 65, 9876, row0=24)
    assert torch.equal(torch.cat([a, b]), whole)
    assert torch.equal(o.sample_negatives(None, l, 100, 1, 65, 9876), o.sample_negatives(s[:, :0].contiguous(), l, 100, 1, 65, 9876))
    from easydgl_amd import _lib
    with pytest.raises(_lib.EdglError, match="2 \\(T \\+ 1\\)"):
        o.sample_negatives(s, l, 100, 1, 16, 9876)


# ---- (f) ---------------------------------------------------------------------------------------------------------------------------
def _easydgl(B):
    prob = make_problem(seed=3, batch=B, num_items=300, seqslen=20, num_units=32, num_heads=2, num_blocks=1)
    m = build_model(prob, "f32")
    return m, to_dev(prob["efeats"]), torch.as_tensor(prob["elabels"]).cuda()


def _ctsma(B):
    from tests.test_gpu_ctsma import _model, _problem
    prob = _problem(7, B=B, T=20, C=32, h=2, E=4, I=300, nb=1)
    return _model(prob, "f32"), to_dev(prob["feats"]), torch.as_tensor(prob["tokens"]).cuda()


def _tgat(B):
    from tests.test_gpu_tgat import _model, _problem
    prob = _problem(11, B=B, T=12, C=32, h=2, I=300, nb=2)
    return _model(prob, "f32"), to_dev(prob["feats"]), torch.as_tensor(prob["tokens"]).cuda()


def _tisasrec(B):
    from tests.test_gpu_tisasrec import _model, _problem
    prob = _problem(80, B=B, T=12, C=32, h=2, I=300, nb=1, timelen=32)
    return _model(prob, "bf16"), to_dev(prob["feats"]), torch.as_tensor(prob["tokens"]).cuda()


MODELS = {"EasyDGL": _easydgl, "CTSMA": _ctsma, "TGAT": _tgat, "TiSASRec": _tisasrec}
KEYS = ("H1", "H5", "H10", "N1", "N5", "N10", "MRR")


def _cut(feats, labels, lo, hi):
    return {k: v[lo:hi].contiguous() for k, v in feats.items()}, labels[lo:hi].contiguous()


@pytest.mark.parametrize("name", sorted(MODELS))
def test_models_score_and_rank_their_candidates(name):
    m, feats, labels = MODELS[name](32)
    B, N = 32, 40
    I = m.num_items
    with torch.no_grad():
        out = m.encoder(feats, False, m._gather_pos(feats, False) if name == "EasyDGL" else m._last_pos(feats["seqs_i"]))
    rows = (out[0] if isinstance(out, tuple) else out).reshape(B, -1)
    C = rows.shape[1]
    tab = m.compute(m.item_embs.lookup_table)
    assert rows.dtype == tab.dtype
    y = labels[:, -1].contiguous()
    rng = np.random.default_rng(2)
    cand = rng.integers(0, I, size=(B, N))
    cand[rng.random((B, N)) < 0.05] = -1
    cand[:, 0] = y.cpu().numpy()
    cand[:, 1] = feats["seqs_i"][:, -2].cpu().numpy()                    # an id of the history
    c = torch.tensor(cand, dtype=torch.int32).cuda()
    for mask_seen in (True, False):
        seen = feats["seqs_i"].cpu().numpy() if mask_seen else None
        sc, lv, _, mg, lm = CR.reference(_f64(rows), _f64(tab), _f64(m.output_bias.detach()), cand, seen, y.cpu().numpy())
        lo, hi = CR.rank_bracket(sc, mg, lv, lm, cand, y.cpu().numpy(), C)
        rank = m.eval_candidates(feats, labels, candidates=c, mask_seen=mask_seen).cpu().numpy()
        assert rank.dtype == np.int32 and ((lo <= rank) & (rank <= hi)).all(), (mask_seen, lo, rank, hi)
        assert (hi - lo).sum() <= B // 4                                     # (the bracket is tight: the check is not vacuous)
        got = m.score_candidates(feats, c, mask_seen=mask_seen)
        assert got.shape == (B, N) and got.dtype == torch.float32
        _within_bound(got.cpu().numpy(), sc, mg, C)
    # sampled negatives: never the history, never the label, from [1, hi) with the MASK row left out
    hi_id = m.mask if name == "EasyDGL" else m.num_items
    want = ops().sample_negatives(feats["seqs_i"], y, 20, 1, hi_id, 5, 0, 3)
    r1 = m.eval_candidates(feats, labels, num_negatives=20, seed=5, row0=3)
    r2 = m.eval_candidates(feats, labels, candidates=want)
    assert torch.equal(r1, r2) and int(r1.max()) <= 20
    # a split in batches of 8 and of 32: identical metrics
    res = []
    for bs in (8, 32):
        m.reset_metrics((1, 5, 10))
        for lo_ in range(0, B, bs):
            f, l = _cut(feats, labels, lo_, lo_ + bs)
            m.eval_step(f, l, negatives=20, neg_seed=5, row0=lo_)
        res.append(m.metrics())
    assert tuple(res[0]) == KEYS and res[0] == res[1], res
    assert res[0]["H1"] <= res[0]["H5"] <= res[0]["H10"] <= 1.0 and 0.0 < res[0]["MRR"] <= 1.0
    # one accumulation holds one kind of step
    with pytest.raises(RuntimeError):
        m.eval_step(feats, labels)
    m.reset_metrics()
    m.eval_step(feats, labels)
    with pytest.raises(RuntimeError):
        m.eval_step(feats, labels, negatives=20)
    with pytest.raises(RuntimeError):
        m.eval_step(feats, labels, candidates=c)
    # the defaults are the full ranking, as before
    m.reset_metrics()
    m.eval_step(feats, labels)
    assert tuple(m.metrics()) == ("H10", "H50", "H100", "N10", "N50", "N100")


# ---- (g) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_name,extra", [("TiSASREC", []), ("EasyDGL", ["--device_data"])])
def test_driver_with_sampled_negatives(tmp_path, model_name, extra):
    sp = pytest.importorskip("scipy.sparse")
    from easydgl_amd import data as D
    from easydgl_amd import formats as F
    from easydgl_amd import train as TR
    num_items, seqslen, E = 300, 20, 4
    ids, ts = D.synthetic_batch(num_items, seqslen, 200, seed=3)

    def dump(name, lo, hi):
        F.write_tfrecord(str(tmp_path / name), [F.encode_example({"seqs_i": ids[i], "seqs_t": ts[i]}) for i in range(lo, hi)])
    dump("train000.tfrec", 0, 140); dump("validation.tfrec", 140, 170); dump("test.tfrec", 170, 200)
    with open(tmp_path / "mark.pkl", "wb") as f:
        pickle.dump(sp.csr_matrix(D.synthetic_mark_table(num_items, E).astype(np.int64)), f)
    res = TR.main(["--model", model_name, "--timelen", "32", "--train", str(tmp_path / "train*.tfrec"), "--valid",
                   str(tmp_path / "validation.tfrec"), "--test", str(tmp_path / "test.tfrec"), "--num_items", str(num_items),
                   "--num_units", "32", "--num_heads", "2", "--num_blocks", "1", "--seqslen", str(seqslen), "--masklen", "4",
                   "--time_scale", "86400", "--mark", str(tmp_path / "mark.pkl"), "--ct_reg", "1e-7", "--batch_size", "64",
                   "--num_epochs", "1", "--learning_rate", "1e-3", "--l2_reg", "1e-4", "--mask_seen", "--dtype", "f32",
                   "--ckpt_dir", str(tmp_path / "ckpt"), "--eval_negatives", "20", "--eval_neg_seed", "3"] + extra)
    assert set(res) == set(KEYS)
    assert all(0.0 <= v <= 1.0 and math.isfinite(v) for v in res.values())
    assert res["H1"] <= res["H5"] <= res["H10"]


def test_driver_evaluate_does_not_depend_on_the_batch_size():
    from easydgl_amd import train
    prob = make_problem(seed=6, batch=20, num_items=300, seqslen=20, num_units=32, num_heads=2, num_blocks=1)
    m = build_model(prob, "f32")
    ids, ts = np.asarray(prob["ids"]), np.asarray(prob["ts"], dtype=np.float32)
    a = train.evaluate(m, ids, ts, 8, True, negatives=20, neg_seed=1)
    b = train.evaluate(m, ids, ts, 20, True, negatives=20, neg_seed=1)
    assert tuple(a) == KEYS and a == b
    assert tuple(train.evaluate(m, ids, ts, 8, True)) == ("H10", "H50", "H100", "N10", "N50", "N100")
