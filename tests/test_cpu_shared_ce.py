"""Shared-negative sampled softmax without a device: the flag plumbing of the driver and the models, the shape rule
of the C entry points (checked before any pointer is read), and the fp64 reference on a broadcast list."""
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import easydgl_oracle as O
from tests import _cand_ce_ref as CE

ONE = 16      # any non-null, 16-byte aligned address: the checks below fail before a pointer is dereferenced
BASE = ["--train", "a", "--valid", "b", "--test", "c", "--model", "EasyDGL", "--num_items", "100"]


def test_driver_flag_parses_and_conflicts(capsys):
    from easydgl_amd import train
    a = train.args(BASE)
    assert a.shared_negatives == 0
    a = train.args(BASE + ["--shared_negatives", "1024", "--train_neg_seed", "7", "--deterministic"])
    assert a.shared_negatives == 1024 and a.train_negatives == 0 and a.train_neg_seed == 7
    a = train.args(BASE + ["--shared_negatives", "16", "--lazy_adam"])          # the lazy mode takes either estimator
    assert a.lazy_adam is True and a.shared_negatives == 16
    with pytest.raises(SystemExit):
        train.args(BASE + ["--shared_negatives", "16", "--train_negatives", "5"])
    assert "one estimator per run" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.args(BASE + ["--shared_negatives", "16", "--graph"])
    assert "train_step" in capsys.readouterr().err
    for bad in ("-1", "8193"):
        with pytest.raises(SystemExit):
            train.args(BASE + ["--shared_negatives", bad])
    with pytest.raises(SystemExit):
        train.args(BASE + ["--lazy_adam"])
    err = capsys.readouterr().err
    assert "--train_negatives" in err and "--shared_negatives" in err


def _flags(model, **kw):
    F = SimpleNamespace(model=model, num_items=50, num_units=32, num_heads=2, num_blocks=1, seqslen=8, masklen=2, timelen=32,
                        time_scale=86400.0, learning_rate=1e-3, l2_reg=0.0, ct_reg=0.0, hidden_dropout_rate=0.0,
                        attention_probs_dropout_rate=0.0, mark_table=O.synthetic_mark_table(50, 4), compute_dtype="f32",
                        num_train_steps=None, num_warmup_steps=None)
    for k, v in kw.items():
        setattr(F, k, v)
    return F


def test_models_take_the_flag_and_refuse_two_estimators():
    import inspect

    import easydgl_amd
    from easydgl_amd import engine
    from easydgl_amd.model.base import Sequential
    for name in ("EasyDGL", "CTSMA", "TGAT", "TiSASREC"):
        m = easydgl_amd.ranking(_flags(name))
        assert m.shared_negatives == 0                           # absent: off
        m = easydgl_amd.ranking(_flags(name, shared_negatives=16, train_neg_seed=3))
        assert m.shared_negatives == 16 and m.train_negatives == 0 and m.train_neg_seed == 3 and m.neg_step == 0
        par = inspect.signature(type(m).train_loss).parameters
        assert par["shared"].kind is inspect.Parameter.KEYWORD_ONLY and par["shared"].default is None
        with pytest.raises(ValueError, match="one estimator per run"):
            easydgl_amd.ranking(_flags(name, shared_negatives=16, train_negatives=5))
        for bad in (-1, 8193):
            with pytest.raises(ValueError, match="shared_negatives"):
                easydgl_amd.ranking(_flags(name, shared_negatives=bad))
        with pytest.raises(ValueError, match="train_step"):
            m.graphed_train_step({}, None)
    assert list(inspect.signature(Sequential._score_ce).parameters)[-2:] == ["candidates", "shared"]
    assert "shared_negatives" in inspect.getsource(engine.TrainEngine.__init__)
    # lazy_adam: either estimator, EasyDGL only
    assert easydgl_amd.ranking(_flags("EasyDGL", shared_negatives=16, lazy_adam=True)).lazy_adam
    with pytest.raises(ValueError, match="dense table gradient"):
        easydgl_amd.ranking(_flags("EasyDGL", lazy_adam=True))
    with pytest.raises(ValueError, match="overwrites d_item"):
        easydgl_amd.ranking(_flags("TGAT", shared_negatives=16, lazy_adam=True))


def _fwd(L, rows=ONE, table=ONE, R=4, C=64, I=100, S=10, dtype=1, vals=ONE):
    return L.edgl_shared_ce_fwd(rows, table, ONE, ONE, ONE, None, R, C, I, S, vals, ONE, ONE, dtype, None)


def _bwd(L, table=ONE, R=4, C=64, I=100, S=10, dtype=1, ws=ONE, keys=None, plan=None):
    return L.edgl_shared_ce_bwd(ONE, table, ONE, ONE, ONE, ONE, ONE, ONE, None, None, R, C, I, S, ONE, ONE, ONE, ws, keys, plan, dtype, None)


def test_entry_points_refuse_bad_shapes_before_any_launch():
    from easydgl_amd import _lib
    L = _lib.lib
    for call in (_fwd, _bwd):
        assert call(L, C=20) == -1 and b"multiple of 8" in L.edgl_last_error()             # bf16
        assert call(L, C=18, dtype=0) == -1 and b"multiple of 4" in L.edgl_last_error()    # f32
        assert call(L, C=528) == -1 and b"16 <= C <= 512" in L.edgl_last_error()
        assert call(L, C=8) == -1
        assert call(L, S=0) == -1 and b"1 <= S <= 8192" in L.edgl_last_error()
        assert call(L, S=8193) == -1 and b"1 <= S <= 8192" in L.edgl_last_error()
        assert call(L, R=0) == -1 and call(L, I=1) == -1
        assert call(L, R=1 << 20, S=1 << 11) == -1 and b"2^31" in L.edgl_last_error()
        assert call(L, dtype=7) == -2
    assert _fwd(L, table=8) == -1 and b"aligned" in L.edgl_last_error()
    assert _fwd(L, vals=None) == -4 and b"null" in L.edgl_last_error()
    assert _bwd(L, ws=None) == -5 and b"edgl_shared_ce_workspace" in L.edgl_last_error()
    assert _bwd(L, keys=ONE) == -4 and b"go together" in L.edgl_last_error()
    assert L.edgl_shared_ce_workspace(4, 20, 10, 1) == -1 and L.edgl_shared_ce_workspace(4, 64, 0, 1) == -1
    # dv [R, 16] + W_S [16, C] (bf16: half a float each), the slab [16, C], the bias sums, two floats per row, the GEMM's own
    assert L.edgl_shared_ce_workspace(4, 64, 10, 1) >= (4 * 16 + 16 * 64) // 2 + 16 * 64 + 16 + 8


def test_reference_on_a_broadcast_list_touches_labels_and_live_slots_only():
    R, C, I = 6, 8, 40
    rng = np.random.default_rng(0)
    rows, table, bias = rng.standard_normal((R, C)), rng.standard_normal((I, C)), rng.standard_normal(I - 1)
    labels = np.array([3, 0, 17, 3, 29, 11])
    shared = np.array([5, -1, 17, 0, I + 2, 5, 22, 9, 38])       # empty, a label, item 0, past I, a repeat
    ref = CE.reference(rows, table, bias, np.broadcast_to(shared, (R, len(shared))), labels)
    live = shared[(shared >= 1) & (shared < I)]
    want = np.zeros(I, dtype=bool)
    want[live] = True
    want[labels[labels > 0]] = True
    assert np.array_equal(np.abs(ref["d_table"]).sum(axis=1) > 0, want)
    assert np.array_equal(np.abs(ref["d_bias"]) > 0, want[1:])
    assert not ref["d_rows"][1].any() and ref["weight"] == 5
    # row 2's label sits in the list: the slot is dead for that row alone — dropping it from ITS list changes nothing
    cand = np.broadcast_to(shared, (R, len(shared))).copy()
    cand[2, 2] = -1
    cut = CE.reference(rows, table, bias, cand, labels)
    assert cut["loss"] == ref["loss"] and np.array_equal(cut["d_table"], ref["d_table"])
