"""Lazy row-wise Adam, the parts that need no GPU: the fp64 reference the GPU tests hold edgl_adam_rows to
(tests/_lazy_adam_ref.py) against the plain TF-form formula, the touched-set rules, the entry point's refusals before any launch,
the models' refusals at construction and the driver's at parse time."""
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import easydgl_oracle as O
from tests import _lazy_adam_ref as LA

ONE = 16      # any non-null, 16-byte aligned address: the checks below fail before a pointer is dereferenced


def _state(I, C, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((I, C)), rng.standard_normal((I, C)) * 0.1, rng.standard_normal((I, C)) * 0.05,
            rng.random((I, C)) * 0.01)


def test_every_row_listed_is_the_plain_adam_formula():
    I, C = 23, 8
    w, g, m, v = _state(I, C, 0)
    for l2 in (0.0, 1e-2):
        got = LA.adam_rows(w, g, m, v, 3, 1e-2, ids=np.arange(I), l2=l2)
        # the formula written out once more, element by element, with O.adam_tf for the l2-free case
        gg = g + l2 * w
        mm = 0.9 * m + 0.1 * gg
        vv = 0.999 * v + 0.001 * gg * gg
        ww = w - 1e-2 * np.sqrt(1 - 0.999 ** 3) / (1 - 0.9 ** 3) * mm / (np.sqrt(vv) + 1e-8)
        assert got[4][1:].all() and not got[4][0]
        for a, b in zip(got[:3], (ww, mm, vv)):
            assert np.abs(a[1:] - b[1:]).max() <= 1e-15 * max(1.0, np.abs(b).max())
        assert np.array_equal(got[0][0], w[0]) and np.array_equal(got[1][0], m[0]) and np.array_equal(got[3][0], g[0])   # row 0: never
        assert np.all(got[3][1:] == 0.0)
    wt, mt, vt = O.adam_tf(w.copy(), g, m.copy(), v.copy(), 3, 1e-2)
    got = LA.adam_rows(w, g, m, v, 3, 1e-2, ids=np.arange(I))
    assert np.abs(got[0][1:] - wt[1:]).max() <= 1e-14 and np.abs(got[1][1:] - mt[1:]).max() <= 1e-15


def test_unlisted_rows_are_untouched_and_listing_is_idempotent():
    I, C = 40, 4
    w, g, m, v = _state(I, C, 1)
    ids = np.array([[3, 5, 0], [5, 5, I], [I + 3, -2, 7]])
    labels = np.array([9, 0, 3, I + 1])
    cand = np.array([[11, -1, 9], [20, 21, 22], [3, 3, 12], [30, 31, 32]])
    a = LA.adam_rows(w, g, m, v, 2, 1e-3, ids, labels, cand, l2=1e-2)
    want = np.zeros(I, dtype=bool)
    want[[3, 5, 7, 9, 11, 12]] = True          # 20..22: the list of the label-0 row; 30..32: of the row whose label is past I
    assert np.array_equal(a[4], want)
    for k, src in enumerate((w, m, v, g)):
        assert np.array_equal(a[k][~want], src[~want]), k
    assert np.all(a[3][want] == 0.0) and np.all(a[0][want] != w[want])
    # the same set, listed once each through one source, or many times through all three: the same result
    b = LA.adam_rows(w, g, m, v, 2, 1e-3, ids=np.array([12, 11, 9, 7, 5, 3]), l2=1e-2)
    c = LA.adam_rows(w, g, m, v, 2, 1e-3, np.tile(ids, 3), np.array([3, 3, 5]), np.array([[7, 9], [11, 12], [12, 12]]), l2=1e-2)
    for k in range(5):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    # nothing listed: nothing moves
    n = LA.adam_rows(w, g, m, v, 2, 1e-3)
    assert not n[4].any() and np.array_equal(n[0], w) and np.array_equal(n[3], g)


def _rows(L, C=64, I=100, R=4, N=10, n_ids=8, table=ONE, ids=ONE, stamp=ONE, shadow=None):
    return L.edgl_adam_rows(table, ONE, ONE, ONE, shadow, I, C, ids, n_ids, ONE, ONE, R, N, stamp, 0.9, 0.999, 1e-8, ONE, 0.0, None)


def test_entry_point_refuses_bad_shapes_before_any_launch():
    from easydgl_amd import _lib
    L = _lib.lib
    assert _rows(L, C=6) == -1 and b"multiple of 4" in L.edgl_last_error()
    assert _rows(L, C=516) == -1 and b"512" in L.edgl_last_error()
    assert _rows(L, C=0) == -1
    assert _rows(L, I=1) == -1 and b"I > 1" in L.edgl_last_error()
    assert _rows(L, R=1 << 20, N=1 << 11) == -1 and b"2^31" in L.edgl_last_error()
    assert _rows(L, n_ids=-1) == -1
    assert _rows(L, table=8) == -1 and b"aligned" in L.edgl_last_error()
    assert _rows(L, shadow=8) == -1 and b"aligned" in L.edgl_last_error()
    assert _rows(L, stamp=None) == -4 and b"null" in L.edgl_last_error()
    assert _rows(L, ids=None) == -4 and b"null list" in L.edgl_last_error()
    # the shape rule comes first: a bad width is named even when every pointer is null
    assert L.edgl_adam_rows(None, None, None, None, None, 100, 6, None, 0, None, None, 0, 0, None, 0.9, 0.999, 1e-8, None, 0.0, None) == -1
    # nothing listed: nothing to launch
    assert _rows(L, R=0, N=0, n_ids=0, ids=None) == 0


def _flags(model, **kw):
    F = SimpleNamespace(model=model, num_items=50, num_units=32, num_heads=2, num_blocks=1, seqslen=8, masklen=2, timelen=32,
                        time_scale=86400.0, learning_rate=1e-3, l2_reg=0.0, ct_reg=0.0, hidden_dropout_rate=0.0,
                        attention_probs_dropout_rate=0.0, mark_table=O.synthetic_mark_table(50, 4), compute_dtype="f32",
                        num_train_steps=None, num_warmup_steps=None, train_negatives=5, lazy_adam=True)
    for k, v in kw.items():
        setattr(F, k, v)
    return F


def test_models_refuse_what_the_lazy_mode_cannot_run():
    import easydgl_amd
    m = easydgl_amd.ranking(_flags("EasyDGL"))
    assert m.lazy_adam and m.train_negatives == 5
    assert not easydgl_amd.ranking(_flags("EasyDGL", lazy_adam=False)).lazy_adam          # off by default ...
    F = _flags("EasyDGL")
    del F.lazy_adam
    assert not easydgl_amd.ranking(F).lazy_adam                                            # ... and when the flag is absent
    with pytest.raises(ValueError, match="dense table gradient"):
        easydgl_amd.ranking(_flags("EasyDGL", train_negatives=0))
    for name in ("CTSMA", "TGAT", "TiSASREC"):
        with pytest.raises(ValueError, match="overwrites d_item"):
            easydgl_amd.ranking(_flags(name))
    with pytest.raises(ValueError, match="channel-padded"):
        easydgl_amd.ranking(_flags("EasyDGL", num_units=40))          # head dim 20 runs padded at 32
    assert easydgl_amd.ranking(_flags("EasyDGL", num_units=40, lazy_adam=False)).pad == (32, 20)


def test_driver_refuses_lazy_adam_without_train_negatives_at_parse_time(capsys):
    from easydgl_amd import train
    base = ["--train", "a", "--valid", "b", "--test", "c", "--model", "EasyDGL", "--num_items", "100"]
    assert train.args(base).lazy_adam is False
    a = train.args(base + ["--train_negatives", "5", "--lazy_adam", "--deterministic"])
    assert a.lazy_adam is True and a.train_negatives == 5
    with pytest.raises(SystemExit):
        train.args(base + ["--lazy_adam"])
    assert "--train_negatives" in capsys.readouterr().err
