"""NARM without a GPU: factory key, variable table and its round trip, the refusals of the three edgl_addattn entry
points in front of any launch, the refused width and driver flags."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _narm_ref as NR

OK = dict(B=2, T=20, C=64, dtype=0)


def _model(**kw):
    import easydgl_amd
    base = dict(model="NARM", num_items=50, num_units=32, num_heads=1, num_blocks=2, seqslen=7, learning_rate=1e-3, l2_reg=1e-3,
                compute_dtype="bf16", num_train_steps=None, num_warmup_steps=None)
    return easydgl_amd.ranking(SimpleNamespace(**{**base, **kw}))


def _calls(B, T, C, dtype, p=64):
    """(name, return code) of the three entry points on a shape, one call at a time; `p`: the value of every pointer (never
    dereferenced)."""
    from easydgl_amd._lib import lib
    yield "edgl_addattn_fwd", lib.edgl_addattn_fwd(p, p, p, p, B, T, C, p, C, None, dtype, None)
    yield "edgl_addattn_bwd", lib.edgl_addattn_bwd(p, p, p, p, p, C, None, B, T, C, p, p, p, p, dtype, None)
    yield "edgl_addattn_bwd_workspace", lib.edgl_addattn_bwd_workspace(B, T, C)


def test_ranking_builds_the_model():
    m = _model()
    assert type(m).__name__ == "NARM" and len(m.layers) == 2 and all(g.wide for g in m.layers)
    assert m.adam_hparams == (0.9, 0.98, 1e-9) and m.clip_norm == 5.0 and m.static_engine_ok is False


def test_variable_names_shapes_and_round_trip():
    m = _model()
    m._shadow = None        # (not finalised: no device copies to refresh)
    shapes, vals = NR.narm_shapes(50, 32, 2), m.tf_values()
    assert {k: v.shape for k, v in vals.items()} == shapes and len(shapes) == 6 + 2 * 12
    assert not np.allclose(vals[NR.A1], vals[NR.A2]) and np.abs(vals[NR.V]).max() <= (6.0 / 33) ** 0.5 and vals[NR.V].any()
    new = NR.narm_params(50, 32, 2, np.random.default_rng(3))
    m.load_tf_variables(new)
    back = m.tf_values()
    assert all(np.array_equal(back[k], new[k].astype(np.float32)) for k in shapes)


@pytest.mark.parametrize("bad,code,text", [(dict(C=24), -1, "[16, 512]"), (dict(C=528), -1, "[16, 512]"), (dict(T=0), -1, "T <= 1024"),
                                           (dict(T=1025), -1, "T <= 1024"), (dict(B=0), -1, "B >= 1"), (dict(dtype=7), -2, "dtype"),
                                           (dict(p=None), -4, "null")])
def test_entry_points_refuse_before_a_launch(bad, code, text):
    from easydgl_amd._lib import lib
    for name, rc in _calls(**{**OK, **bad}):
        if name.endswith("workspace"):
            assert rc == (-1 if code == -1 else 2 * 2 * 64)
        else:
            assert rc == code and text in lib.edgl_last_error().decode(), (name, rc, lib.edgl_last_error())


@pytest.mark.parametrize("kw,flag", [(dict(num_units=50), "--num_units"), (dict(num_units=1024), "--num_units"), (dict(num_blocks=0), "--num_blocks")])
def test_refused_shapes_name_the_flag(kw, flag):
    with pytest.raises(ValueError, match=flag):
        _model(**kw)


@pytest.mark.parametrize("flag", ["device_data", "graph", "lazy_adam"])
def test_the_driver_refuses_what_is_not_built_by_flag_name(flag):
    from easydgl_amd import train
    with pytest.raises(ValueError, match=f"--{flag} with --model NARM"):
        train.run(SimpleNamespace(model="NARM", seed=1, **{flag: True}))
