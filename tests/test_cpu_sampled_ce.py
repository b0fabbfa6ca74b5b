"""Sampled-softmax training, the parts that need no GPU: the fp64 reference the GPU tests hold the kernels to
(tests/_cand_ce_ref.py) is checked against finite differences of its own loss and against a plain full-catalogue softmax, dead slots
contribute exactly nothing, the entry points refuse bad shapes before any launch, and the driver refuses --graph at parse time."""
import numpy as np
import pytest

from tests import _cand_ce_ref as CE

ONE = 16      # any non-null, 16-byte aligned address: the checks below fail before a pointer is dereferenced


def _problem(R, C, I, N, seed, label0=True):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((R, C)) * 0.5
    table = rng.standard_normal((I, C)) * 0.5
    bias = rng.standard_normal(I - 1) * 0.3
    cand = rng.integers(1, I, size=(R, N))
    labels = rng.integers(1, I, size=R)
    if label0:
        labels[R - 1] = 0
    return rows, table, bias, cand, labels


def test_reference_gradients_match_finite_differences():
    R, C, I, N = 3, 16, 12, 5
    rows, table, bias, cand, labels = _problem(R, C, I, N, 1, label0=False)
    cand[0, 1] = -1                   # empty slot
    cand[0, 2] = labels[0]            # accidental hit
    cand[1, 0] = 0                    # item 0: the zero row with bias -1000
    cand[1, 3] = I + 2                # past the table
    cand[2, 1] = cand[2, 4]           # a repeated id
    ref = CE.reference(rows, table, bias, cand, labels)
    h = 1e-6

    def fd(arr, idx):
        old = arr[idx]
        arr[idx] = old + h
        up = CE.loss_only(rows, table, bias, cand, labels)
        arr[idx] = old - h
        dn = CE.loss_only(rows, table, bias, cand, labels)
        arr[idx] = old
        return (up - dn) / (2 * h)

    g_rows = np.array([[fd(rows, (r, c)) for c in range(C)] for r in range(R)])
    g_table = np.array([[fd(table, (i, c)) for c in range(C)] for i in range(I)])
    g_bias = np.array([fd(bias, (i,)) for i in range(I - 1)])
    for got, want, what in ((ref["d_rows"], g_rows, "d_rows"), (ref["d_table"], g_table, "d_table"), (ref["d_bias"], g_bias, "d_bias")):
        # central differences of an fp64 loss of O(1): truncation h^2 and rounding 1e-16 / h, both far below 1e-7
        assert np.abs(got - want).max() <= 1e-7 * max(1.0, np.abs(want).max()), what
    assert np.all(g_table[0] == 0.0) and np.all(ref["d_table"][0] == 0.0)      # item 0's row is no parameter
    assert np.abs(ref["d_rows"]).max() > 1e-3 and np.abs(ref["d_table"]).max() > 1e-3


def test_full_list_equals_the_full_catalogue_softmax():
    R, C, I = 9, 16, 50
    rows, table, bias, _, labels = _problem(R, C, I, 1, 2)
    rng = np.random.default_rng(5)
    cand = np.stack([rng.permutation(np.setdiff1d(np.arange(I), [y])) if y else np.arange(1, I) for y in labels]).astype(np.int64)
    assert cand.shape == (R, I - 1)
    a = CE.reference(rows, table, bias, cand, labels)
    b = CE.full_softmax(rows, table, bias, labels)
    assert abs(a["loss"] - b["loss"]) <= 1e-12 * abs(b["loss"])
    for k in ("d_rows", "d_table", "d_bias"):
        assert np.abs(a[k] - b[k]).max() <= 1e-12 * np.abs(b[k]).max(), k


def test_dead_slots_and_weightless_rows_contribute_nothing():
    R, C, I, N = 6, 16, 30, 7
    rows, table, bias, cand, labels = _problem(R, C, I, N, 3)
    base = CE.reference(rows, table, bias, cand, labels)
    wide = np.full((R, N + 4), -1, dtype=np.int64)
    wide[:, 0:N:2] = cand[:, 0:N:2]                       # the live slots, spread out ...
    wide[:, N + 3] = cand[:, 1]
    wide[:, N + 2] = cand[:, 3]
    wide[:, N + 1] = cand[:, 5]
    wide[:, 1] = labels                                   # ... between accidental hits,
    wide[:, 3] = I + np.arange(R)                         # ids at or past I
    wide[:, 5] = -1                                       # and empty slots
    wide[R - 1] = np.arange(N + 4)                        # the row of label 0: whatever it lists
    got = CE.reference(rows, table, bias, wide, labels)
    assert got["loss"] == pytest.approx(base["loss"], rel=1e-14)
    for k in ("d_rows", "d_table", "d_bias", "lse"):
        assert np.abs(got[k] - base[k]).max() <= 1e-14 * max(1e-30, np.abs(base[k]).max()), k
    assert np.all(got["d_rows"][R - 1] == 0.0) and got["terms"][R - 1] == 0.0 and got["weight"] == R - 1
    # ... and a row of label 0 does not enter the denominator: dropping it changes nothing
    cut = CE.reference(rows[:R - 1], table, bias, cand[:R - 1], labels[:R - 1])
    assert cut["loss"] == pytest.approx(base["loss"], rel=1e-14)
    assert np.abs(cut["d_table"] - base["d_table"]).max() <= 1e-14 * np.abs(base["d_table"]).max()


def _fwd(L, rows=ONE, table=ONE, R=4, C=64, I=100, N=10, dtype=1, vals=ONE):
    return L.edgl_cand_ce_fwd(rows, table, ONE, ONE, ONE, R, C, I, N, vals, ONE, ONE, dtype, None)


def _bwd(L, table=ONE, R=4, C=64, I=100, N=10, dtype=1, d_table=ONE, d_bias=ONE):
    return L.edgl_cand_ce_bwd(ONE, table, ONE, ONE, ONE, ONE, ONE, ONE, None, R, C, I, N, ONE, ONE, d_table, d_bias, dtype, None)


def _det(L, R=4, C=64, I=100, N=10, dtype=1, plan=ONE):
    return L.edgl_cand_ce_table_det(ONE, ONE, ONE, ONE, R, C, I, N, ONE, ONE, ONE, plan, dtype, None)


def test_entry_points_refuse_bad_shapes_before_any_launch():
    from easydgl_amd import _lib
    L = _lib.lib
    for call in (_fwd, _bwd, _det):
        assert call(L, C=24) == -1 and b"multiple of 16" in L.edgl_last_error()
        assert call(L, C=528) == -1 and b"512" in L.edgl_last_error()
        assert call(L, N=0) == -1 and b"1 <= N <= 8192" in L.edgl_last_error()
        assert call(L, N=8193) == -1 and b"1 <= N <= 8192" in L.edgl_last_error()
        assert call(L, R=0) == -1 and call(L, I=1) == -1
        assert call(L, R=1 << 20, N=1 << 11) == -1 and b"2^31" in L.edgl_last_error()
        assert call(L, dtype=7) == -2
    assert _fwd(L, table=8) == -1 and b"aligned" in L.edgl_last_error()
    assert _fwd(L, rows=8) == -1 and _bwd(L, table=8) == -1
    assert _fwd(L, vals=None) == -4 and b"null" in L.edgl_last_error()
    assert _bwd(L, d_table=None) == -4 and b"go together" in L.edgl_last_error()      # d_table without d_bias
    assert _det(L, plan=None) == -4


def test_driver_refuses_graph_with_train_negatives_at_parse_time(capsys):
    from easydgl_amd import train
    base = ["--train", "a", "--valid", "b", "--test", "c", "--model", "TiSASREC", "--num_items", "100"]
    a = train.args(base)
    assert a.train_negatives == 0 and a.train_neg_seed == 0
    a = train.args(base + ["--train_negatives", "5", "--train_neg_seed", "7", "--deterministic"])
    assert a.train_negatives == 5 and a.train_neg_seed == 7
    with pytest.raises(SystemExit):
        train.args(base + ["--graph", "--train_negatives", "5"])
    assert "train_step" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.args(base + ["--train_negatives", "-1"])


def test_models_take_candidates_and_the_engine_names_the_autograd_path():
    import inspect

    from easydgl_amd import engine
    from easydgl_amd.model.base import Sequential
    from easydgl_amd.model.ctsma import CTSMA
    from easydgl_amd.model.easydgl import EasyDGL
    from easydgl_amd.model.tgat import TGAT
    from easydgl_amd.model.tisasrec import TiSASRec
    for cls in (EasyDGL, CTSMA, TGAT, TiSASRec):
        par = inspect.signature(cls.train_loss).parameters
        assert par["candidates"].kind is inspect.Parameter.KEYWORD_ONLY and par["candidates"].default is None
    assert hasattr(Sequential, "_score_ce")
    assert "model.train_step" in inspect.getsource(engine.TrainEngine.__init__)
