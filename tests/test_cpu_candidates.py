"""Evaluation on candidate lists, the parts that need no GPU: the argument checks of the two entry points fail before
any launch, the driver knows the flag, and the numpy replica of the sampler's specification (tests/_cand_ref.py — what the GPU tests
hold the kernel to) is uniform and leaves no slot empty at the shapes those tests use."""
import inspect

import numpy as np

from tests import _cand_ref as CR

ONE = 16      # any non-null, 16-byte aligned address: the checks below fail before a pointer is dereferenced


def _score(L, rows=ONE, table=ONE, bias=ONE, cand=ONE, seen=None, T=0, labels=ONE, R=4, C=64, I=100, N=10, scores=ONE, label_val=ONE,
           count=ONE, dtype=1):
    return L.edgl_score_candidates(rows, table, bias, cand, seen, T, labels, R, C, I, N, scores, label_val, count, dtype, None)


def test_score_candidates_argument_checks_before_any_launch():
    from easydgl_amd import _lib
    L = _lib.lib
    assert _score(L, rows=None) == -4 and b"null" in L.edgl_last_error()
    assert _score(L, table=None) == -4 and _score(L, bias=None) == -4 and _score(L, cand=None) == -4
    assert _score(L, T=7) == -4 and b"seen" in L.edgl_last_error()                     # T > 0 without seen ids
    assert _score(L, labels=None) == -4                                                # count / label_val without labels
    assert _score(L, scores=None, label_val=None, count=None) == -4                    # nothing wanted
    assert _score(L, C=24) == -1 and b"multiple of 16" in L.edgl_last_error()
    assert _score(L, C=8) == -1 and _score(L, C=528) == -1 and b"512" in L.edgl_last_error()
    assert _score(L, dtype=7) == -2
    assert _score(L, seen=ONE, T=1025) == -1 and b"1024" in L.edgl_last_error()
    assert _score(L, R=0) == -1 and _score(L, N=0) == -1
    assert _score(L, R=1 << 20, N=1 << 11) == -1 and b"2^31" in L.edgl_last_error()     # R (N + 1) >= 2^31
    assert _score(L, rows=8) == -1 and b"aligned" in L.edgl_last_error()
    # the chunk query: whole steps of the workgroup, at most 1024, -1 for a shape not taken
    assert L.edgl_score_candidates_chunk(512, 128, 100, 1) == 64
    assert L.edgl_score_candidates_chunk(33, 16, 16500, 1) == 1024
    assert L.edgl_score_candidates_chunk(8, 256, 4096, 1) == 64
    assert L.edgl_score_candidates_chunk(8, 24, 4096, 1) == -1 and L.edgl_score_candidates_chunk(8, 64, 10, 7) == -1


def test_sample_negatives_argument_checks_before_any_launch():
    from easydgl_amd import _lib
    L = _lib.lib

    def call(seen=ONE, T=7, labels=ONE, R=5, n=100, lo=1, hi=65, I=65, cand=ONE, row0=0):
        return L.edgl_sample_negatives(seen, T, labels, R, n, lo, hi, I, 9876, 0, row0, cand, None)
    assert call(cand=None) == -4 and b"null" in L.edgl_last_error()
    assert call(seen=None) == -4
    assert call(T=40) == -1                                                            # 2 (T + 1) = 82 > 64
    msg = L.edgl_last_error()
    assert b"82" in msg and b"64" in msg, msg
    assert call(lo=0) == -1 and call(hi=66) == -1 and call(lo=65) == -1
    assert call(T=1025, hi=4000, I=4000) == -1 and b"1024" in L.edgl_last_error()
    assert call(R=0) == -1 and call(n=0) == -1 and call(row0=-1) == -1


def test_driver_knows_the_flag_and_evaluate_defaults_to_the_full_ranking():
    from easydgl_amd import train
    base = ["--train", "a", "--valid", "b", "--test", "c", "--model", "TiSASREC", "--num_items", "100"]
    a = train.args(base)
    assert a.eval_negatives == 0 and a.eval_neg_seed == 0
    a = train.args(base + ["--eval_negatives", "100", "--eval_neg_seed", "7"])
    assert a.eval_negatives == 100 and a.eval_neg_seed == 7
    par = inspect.signature(train.evaluate).parameters
    assert par["negatives"].default == 0 and par["neg_seed"].default == 0 and par["by_rank"].default is False
    assert list(par)[:7] == ["model", "ids", "ts", "batch_size", "mask_seen", "loader", "by_rank"]


def test_model_methods_exist_on_every_model():
    from easydgl_amd.model.base import Sequential
    for name in ("score_candidates", "eval_candidates", "_last_rows", "_negatives_hi"):
        assert hasattr(Sequential, name), name
    par = inspect.signature(Sequential.eval_step).parameters
    for name in ("candidates", "negatives", "neg_seed", "row0"):
        assert par[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert par["negatives"].default == 0 and par["candidates"].default is None


def test_sampler_replica_is_uniform():
    """chi^2 over 50 bins of 200 000 draws at (seed 9876, step 0) across (row, slot): below the 99.9 % quantile 85.35 of chi^2_49."""
    k = CR.sampler_key(9876, 0)
    rows, slots = np.meshgrid(np.arange(2000), np.arange(100), indexing="ij")
    ids = CR.draw(k, rows.ravel(), slots.ravel(), 0, 1, 51)
    assert ids.min() >= 1 and ids.max() <= 50
    x2 = CR.chi2_uniform(ids, 1, 51, 50)
    print("chi2 (row, slot):", x2)
    assert x2 <= 85.35, x2
    # ... and across attempts of a few (row, slot) pairs
    rows, atts = np.meshgrid(np.arange(6250), np.arange(32), indexing="ij")
    x2 = CR.chi2_uniform(CR.draw(k, rows.ravel(), 3, atts.ravel(), 1, 51), 1, 51, 50)
    print("chi2 (row, attempt):", x2)
    assert x2 <= 85.35, x2
    # another key gives another stream
    assert not np.array_equal(CR.draw(CR.sampler_key(9876, 1), np.arange(64), 0, 0, 1, 51), CR.draw(k, np.arange(64), 0, 0, 1, 51))
    assert not np.array_equal(CR.draw(CR.sampler_key(9877, 0), np.arange(64), 0, 0, 1, 51), CR.draw(k, np.arange(64), 0, 0, 1, 51))
    assert CR.sampler_key(9876 + (1 << 32), 0) != k                                     # the high word of the seed counts


def test_sampler_replica_leaves_no_slot_empty_at_the_gpu_test_shapes():
    for R, T, n, lo, hi in ((5, 7, 100, 1, 65), (33, 100, 100, 1, 809), (64, 7, 100, 1, 65)):
        rng = np.random.default_rng(R)
        seen = rng.integers(0, hi, size=(R, T))
        labels = rng.integers(1, hi, size=R)
        cand, worst = CR.sample_negatives(seen, labels, n, lo, hi, 9876, 0, 0)
        assert (cand >= lo).all() and (cand < hi).all() and worst <= 32, (R, worst)
        for r in range(R):
            assert not np.isin(cand[r], seen[r]).any() and labels[r] not in cand[r]
