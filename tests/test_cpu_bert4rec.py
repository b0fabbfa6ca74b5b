"""BERT4REC, the parts that need no GPU: the factory key, the variable table with the reference's names, the
initialisers and the round trip through load_tf_variables / tf_values."""
from types import SimpleNamespace

import numpy as np

from tests import _bert4rec_ref as BR


def _model():
    import easydgl_amd
    F = SimpleNamespace(model="BERT4REC", num_items=50, num_units=32, num_heads=2, num_blocks=2, seqslen=9, masklen=2,
                        learning_rate=1e-3, l2_reg=1e-3, compute_dtype="f32")
    return easydgl_amd.ranking(F)


def test_ranking_builds_bert4rec_with_the_reference_variable_names_and_initialisers():
    m = _model()
    assert type(m).__name__ == "BERT4REC" and m.static_engine_ok is False
    assert (m.num_items, m.mask, m.seqslen) == (52, 50, 10)
    got = m.tf_values()
    assert {k: tuple(v.shape) for k, v in got.items()} == {k: tuple(s) for k, s in BR.bert4rec_shapes(52, 10, 32, 2).items()}
    for k, v in got.items():
        if "/BERTAttention/" in k and k.endswith("kernel"):       # truncated normal, sigma 0.02, cut at two sigma
            assert 0.015 < v.std() < 0.02 and np.abs(v).max() <= 0.04
        elif k.endswith("bias") or k.endswith("beta"):
            assert not v.any()
        elif k.endswith("gamma"):
            assert (v == 1).all()


def test_load_tf_variables_and_tf_values_round_trip_every_value():
    m = _model()
    m._shadow = None        # (not finalised: no device copies to refresh)
    rng = np.random.default_rng(0)
    vals = {k: rng.standard_normal(s).astype(np.float32) for k, s in BR.bert4rec_shapes(52, 10, 32, 2).items()}
    m.load_tf_variables(vals)
    back = m.tf_values()
    assert set(back) == set(vals) and all(np.array_equal(back[k], vals[k]) for k in vals)
