"""TimelyREC, the parts that need no GPU: construction through util.ranking, the variable table against the float64
restatement's names and shapes, the window formula, the refused flags, the calendar fields of formats.py and the argument
validation of the new entry points."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _timelyrec_ref as TR


def _flags(**kw):
    base = dict(model="TimelyREC", num_items=50, num_units=32, num_heads=2, num_blocks=2, seqslen=10, learning_rate=1e-3, l2_reg=1e-3,
                hidden_dropout_rate=0.0, attention_probs_dropout_rate=0.0, compute_dtype="f32", num_train_steps=None,
                num_warmup_steps=None, time_scale=86400.0)
    base.update(kw)
    return SimpleNamespace(**base)


def test_ranking_constructs_the_model_with_the_reference_names():
    import easydgl_amd
    from easydgl_amd.model import TimelyREC
    m = easydgl_amd.ranking(_flags())
    assert isinstance(m, TimelyREC) and m.window_ratio == 0.2 and m.static_engine_ok is False
    want = TR.timelyrec_shapes(50, 10, 32, 0.2)
    got = m._tf_map()
    assert set(got) == set(want), set(got) ^ set(want)
    vals = m.tf_values()
    for k, sh in want.items():
        assert tuple(vals[k].shape) == tuple(sh), (k, vals[k].shape, sh)
    assert "TimelyREC/attention/TimelyREC/Atttention/multihead_attention/dense/kernel" in got
    assert "TimelyREC/mate/daymate/dense/kernel" in got
    assert float(vals["TimelyREC/te_weight"]) == 1.0
    assert m.l2_param_names() == ["item_embs.lookup_table", "pcoding.pembs.lookup_table", "month_embs.lookup_table",
                                  "day_embs.lookup_table", "weekday_embs.lookup_table", "hour_embs.lookup_table"]
    assert m.adam_hparams == (0.9, 0.999, 1e-8) and m.clip_norm is None


def test_tf_variables_round_trip():
    import easydgl_amd
    m = easydgl_amd.ranking(_flags())
    m._shadow = None        # (not finalised: no device copies to refresh)
    params = TR.init_from_shapes(TR.timelyrec_shapes(50, 10, 32), np.random.default_rng(0))
    m.load_tf_variables(params)
    back = m.tf_values()
    assert set(back) == set(params)
    for k, v in params.items():
        assert np.array_equal(back[k], v.astype(np.float32)), k
    # the four user projections are the column blocks of ONE [C, 4C] parameter, in the order month | day | weekday | hour
    for j, scope in enumerate(("month_mate", "daymate", "weekday_mate", "hour_mate")):
        blk = m.mate.kernel.detach().numpy()[:, 32 * j:32 * (j + 1)]
        assert np.array_equal(blk, params[f"TimelyREC/mate/{scope}/dense/kernel"].astype(np.float32))


@pytest.mark.parametrize("ratio,want", [(0.05, (2, 3, 2, 2)), (0.2, (3, 7, 2, 6)), (0.5, (7, 17, 5, 13))])
def test_window_sizes_follow_the_formula(ratio, want):
    from easydgl_amd import _lib, ops
    assert ops.mate_windows(ratio) == want
    assert want == tuple(TR.window_size(m, ratio) for m in (12, 31, 7, 24))
    assert _lib.lib.edgl_mate_saved_floats(*want) == sum(w + 1 for w in want) + 4


@pytest.mark.parametrize("kw,word", [(dict(window_ratio=0.0), "window_ratio"), (dict(window_ratio=0.6), "window_ratio"),
                                     (dict(num_units=48, num_heads=2), "num_heads"), (dict(seqslen=200), "seqslen")])
def test_unsupported_flags_are_refused_by_name(kw, word):
    import easydgl_amd
    with pytest.raises(ValueError, match=word):
        easydgl_amd.ranking(_flags(**kw))


def test_calendar_from_timestamps_on_fixed_epochs():
    from easydgl_amd.formats import calendar_from_timestamps
    ts = np.array([[0.0,              # 1970-01-01 00:00:00 Thursday
                    951782400.0,      # 2000-02-29 00:00:00 Tuesday (leap day)
                    1709251199.0,     # 2024-02-29 23:59:59 Thursday
                    1704067199.0,     # 2023-12-31 23:59:59 Sunday (year boundary)
                    1704067200.0,     # 2024-01-01 00:00:00 Monday
                    1136239445.5]])   # 2006-01-02 22:04:05.5 Monday
    month, day, weekday, hour = calendar_from_timestamps(ts)
    assert month.tolist() == [[1, 2, 2, 12, 1, 1]]
    assert day.tolist() == [[1, 29, 29, 31, 1, 2]]
    assert weekday.tolist() == [[3, 1, 3, 6, 0, 0]]
    assert hour.tolist() == [[0, 0, 23, 23, 0, 22]]
    assert all(a.dtype == np.int64 and a.shape == ts.shape for a in (month, day, weekday, hour))
    ids = np.array([[0, 5, 0, 7, 8, 9]])
    for a, full in zip(calendar_from_timestamps(ts, ids), (month, day, weekday, hour)):
        assert a.tolist() == (full * (ids != 0)).tolist()


def test_calendar_fields_round_trip_through_the_record_formats(tmp_path):
    from easydgl_amd import formats as F
    rng = np.random.default_rng(3)
    T1 = 7
    recs = []
    for _ in range(5):
        ids = rng.integers(1, 40, size=T1)
        ids[:2] = 0
        ts = (1.6e9 + np.cumsum(rng.integers(1, 10 ** 6, size=T1))).astype(np.float32)
        cal = F.calendar_from_timestamps(ts, ids)
        recs.append(dict(seqs_i=ids, seqs_t=ts, **dict(zip(F.CALENDAR_FIELDS, cal))))
    ex = F.parse_example(F.encode_example(recs[0]))
    for name in F.CALENDAR_FIELDS:
        assert np.array_equal(ex[name], recs[0][name])
    path = str(tmp_path / "part.tfrec")
    F.write_tfrecord(path, [F.encode_example(r) for r in recs])
    got = F.load_calendar(path, T1 - 1)
    for a, name in zip(got, F.CALENDAR_FIELDS):
        assert a.dtype == np.int64 and np.array_equal(a, np.stack([r[name] for r in recs]))
    # convert: the fields are written on request only, and read back from the .npz
    F.convert(path, T1 - 1, str(tmp_path / "plain.npz"))
    assert sorted(np.load(str(tmp_path / "plain.npz")).files) == ["seqs_i", "seqs_t"]
    F.convert(path, T1 - 1, str(tmp_path / "cal.npz"), calendar=True)
    for a, b in zip(F.load_calendar(str(tmp_path / "cal.npz"), T1 - 1), got):
        assert np.array_equal(a, b)
    with pytest.raises(KeyError):
        F.load_calendar(str(tmp_path / "plain.npz"), T1 - 1)


def test_new_entry_points_validate_arguments_without_gpu():
    from easydgl_amd import _lib
    L, one = _lib.lib, 1      # `one`: any non-null address — the checks fail before a pointer is dereferenced
    w = (3, 7, 2, 6)
    assert L.edgl_mate_fwd(None, one, one, one, one, one, one, 2, 8, 32, *w, one, None, 0, None) == -4
    assert b"null" in L.edgl_last_error()
    ok = lambda **k: L.edgl_mate_fwd(one, one, one, one, one, one, one, k.get("B", 2), k.get("T", 8), k.get("C", 32),
                                     *k.get("w", w), one, None, k.get("dtype", 0), None)
    assert ok(T=129) == -1 and b"T=129" in L.edgl_last_error()
    assert ok(T=0) == -1 and ok(C=48) == -1 and ok(C=16) == -1 and ok(C=1024) == -1
    assert ok(w=(3, 18, 2, 6)) == -1 and b"window" in L.edgl_last_error()       # day window past ratio 0.5
    assert ok(w=(1, 7, 2, 6)) == -1 and ok(w=(9, 7, 2, 6)) == -1
    assert ok(dtype=7) == -2
    assert L.edgl_mate_bwd(one, one, one, one, one, one, one, one, one, 2, 8, 32, *w, one, one, one, None, 0, None) == -4
    assert L.edgl_mate_bwd(one, one, one, one, one, one, one, one, one, 2, 200, 32, *w, one, one, one, one, 0, None) == -1
    assert L.edgl_mate_bwd_workspace(2, 8, 32, *w) == 2 * 8 * 26 + 2 * 74 * 32
    assert L.edgl_mate_bwd_workspace(2, 8, 40, *w) == -1 and L.edgl_mate_saved_floats(3, 7, 2, 20) == -1
    assert L.edgl_tahe_fwd(None, one, 2, 8, 32, one, 0, None) == -4
    assert L.edgl_tahe_fwd(one, one, 2, 129, 32, one, 0, None) == -1 and b"T=129" in L.edgl_last_error()
    assert L.edgl_tahe_fwd(one, one, 2, 8, 96, one, 0, None) == -1 and L.edgl_tahe_fwd(one, one, 2, 8, 32, one, 3, None) == -2
    assert L.edgl_tahe_bwd(one, one, None, 2, 8, 32, one, one, 0, None) == -4
    assert L.edgl_tahe_bwd(one, one, one, 0, 8, 32, one, one, 0, None) == -1
    assert L.edgl_tahe_mix_fwd(one, one, None, one, 16, 32, one, 0, None) == -4
    assert L.edgl_tahe_mix_bwd(one, one, one, 0, 32, one, one, one, 0, None) == -1
    assert L.edgl_tahe_mix_bwd_workspace(130) == 3 and L.edgl_tahe_mix_bwd_workspace(0) == -1
    assert L.edgl_cat3(one, one, None, 4, 32, one, 0, 0, None) == -4 and L.edgl_cat3(one, one, one, 4, 32, one, 0, 9, None) == -2


def test_ops_and_encoders_refuse_cpu_tensors_and_distinct_keys():
    from easydgl_amd import _lib, ops
    from easydgl_amd.module.sequential import TAHEncoder
    x = torch.zeros(2, 4, 32)
    with pytest.raises(_lib.EdglError):
        ops.TaheFn.apply(x, x)
    with pytest.raises(_lib.EdglError):
        ops.MateFn.apply(torch.zeros(4, 2, 4, dtype=torch.int64), *[torch.zeros(m, 32) for m in ops.MATE_RANGES] * 2,
                         torch.zeros(2, 4, 128), x, (3, 7, 2, 6))
    with pytest.raises(ValueError):
        TAHEncoder()(x, x.clone(), x)
