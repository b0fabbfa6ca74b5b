"""TGREC, the parts that need no GPU: the factory key, the variable table against the float64 restatement's names and
shapes, the refused widths, the driver's timestamp-order check and the argument validation of the new entry points."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _seq_baselines_ref as SR
from tests import _tgrec_ref as TG


def _flags(**kw):
    base = dict(model="TGREC", num_items=50, num_units=32, num_heads=2, num_blocks=2, seqslen=10, learning_rate=1e-3, l2_reg=1e-3,
                hidden_dropout_rate=0.1, attention_probs_dropout_rate=0.1, compute_dtype="f32", num_train_steps=None,
                num_warmup_steps=None, time_scale=86400.0)
    base.update(kw)
    return SimpleNamespace(**base)


def test_ranking_builds_tgrec_and_its_variables_round_trip():
    import easydgl_amd
    m = easydgl_amd.ranking(_flags())
    assert type(m).__name__ == "TGREC" and m.static_engine_ok is False
    want = TG.tgrec_shapes(50, 10, 32, 2)
    got = m.tf_values()
    assert set(got) == set(want), set(got) ^ set(want)
    for k, sh in want.items():
        assert tuple(got[k].shape) == tuple(sh), k
    assert m.l2_param_names() == ["item_embs.lookup_table", "pcoding.pembs.lookup_table"]
    assert m.adam_hparams == (0.9, 0.999, 1e-8) and m.clip_norm is None
    np.testing.assert_array_equal(got["TGREC/tcoding/basis_freq"], np.linspace(0, 9, 32).astype(np.float32))
    m._shadow = None        # (not finalised: no device copies to refresh)
    vals = SR.init_from_shapes(want, np.random.default_rng(0))
    m.load_tf_variables(vals)
    back = m.tf_values()
    for k, v in vals.items():
        np.testing.assert_array_equal(back[k], v.astype(np.float32))
    # K | V are the column blocks of ONE [2C, 2C] parameter; rows: x half, time half
    kv = m.layers[1].attention.kv_kernel.detach().numpy()
    np.testing.assert_array_equal(kv[:, 32:], vals["num_blocks_1/attention/TgMultiHeadAttention/dense_2/kernel"].astype(np.float32))


@pytest.mark.parametrize("kw,word", [(dict(num_units=256, num_heads=2), "num_units"), (dict(num_units=48, num_heads=3), "num_units"),
                                     (dict(num_units=64, num_heads=8), "num_heads"), (dict(seqslen=2000), "seqslen")])
def test_unsupported_flags_are_refused_by_name(kw, word):
    import easydgl_amd
    with pytest.raises(ValueError, match=word):
        easydgl_amd.ranking(_flags(**kw))


def test_decreasing_timestamps_raise_in_the_driver(tmp_path):
    """Every position of the row counts, the zeros under the left padding included: a real time below its predecessor raises."""
    from easydgl_amd import train
    T = 6
    ids = np.tile(np.arange(1, T + 2), (4, 1))
    ts = np.tile(np.arange(1, T + 2, dtype=np.float32) * 100.0, (4, 1))
    ts[2, 3] = 50.0
    path = str(tmp_path / "d.npz")
    np.savez(path, seqs_i=ids, seqs_t=ts)
    argv = ["--train", path, "--valid", path, "--test", path, "--model", "TGREC", "--num_items", "10", "--num_units", "32",
            "--num_heads", "2", "--seqslen", str(T)]
    with pytest.raises(ValueError, match="timestamps decrease"):
        train.run(train.args(argv))


def test_entry_points_validate_arguments_without_gpu():
    from easydgl_amd import _lib
    L, one = _lib.lib, 1      # `one`: any non-null address — the checks fail before a pointer is dereferenced
    fwd = lambda q=one, B=2, T=8, H=2, C=32, dt=0, rate=0.0: L.edgl_tgattn_fwd(q, one, one, one, T, one, one, one, B, T, H, C, 0.25, 1.0,
                                                                               rate, None, 0, one, one, None, None, dt, None)
    assert fwd(q=None) == -4 and b"null" in L.edgl_last_error()
    assert fwd(C=256) == -1 and b"C=256" in L.edgl_last_error()
    assert fwd(T=1025) == -1 and fwd(T=0) == -1 and fwd(H=4) == -1 and fwd(C=48, H=3) == -1
    assert fwd(dt=7) == -2 and fwd(rate=0.3) == -4
    assert L.edgl_tgattn_bwd(one, one, one, one, 8, one, one, one, one, one, one, one, None, 2, 8, 2, 32, 0.25, 1.0, 0.0, None, 0,
                             one, one, one, one, one, one, 0, None) == -4
    assert L.edgl_tgattn_saved_bytes(2, 8, 2) == 3 * 64 * 4 and L.edgl_tgattn_saved_bytes(0, 8, 2) == -1
    assert L.edgl_tgattn_bwd_workspace(2, 16, 2, 32) == 2 * 16 * 2 * 128 + 2 * 1 * 64 + 1 * 32
