"""GRU4REC without a GPU: factory key, variable table, initialisers, optimizer attributes, refusals, the restatement's GRU."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _gru4rec_ref as GR
from tests import _seq_baselines_ref as SR


def _model(**kw):
    import easydgl_amd
    base = dict(model="GRU4REC", num_items=50, num_units=32, num_heads=1, num_blocks=2, seqslen=7, learning_rate=1e-3, l2_reg=1e-3,
                compute_dtype="bf16", num_train_steps=None, num_warmup_steps=None)
    return easydgl_amd.ranking(SimpleNamespace(**{**base, **kw}))


def test_ranking_builds_the_model_and_the_bare_namespace_is_still_refused():
    import easydgl_amd
    m = _model()
    assert type(m).__name__ == "GRU4REC" and len(m.layers) == 2 and all(g.wide for g in m.layers)
    assert m.adam_hparams == (0.9, 0.98, 1e-9) and m.clip_norm == 5.0 and m.static_engine_ok is False
    with pytest.raises(NotImplementedError):
        easydgl_amd.ranking(SimpleNamespace(model="GRU4REC"))


def test_reference_names_shapes_initialisers_and_round_trip():
    m = _model()
    m._shadow = None        # (not finalised: no device copies to refresh)
    shapes, vals = GR.gru4rec_shapes(50, 32, 2), m.tf_values()
    assert {k: v.shape for k, v in vals.items()} == shapes and len(shapes) == 2 + 2 * 12
    mats = [vals[GR.GRU_SCOPE + f"{l}/{k}_{g}"] for l in range(2) for k in "wr" for g in SR.GRU_GATES]
    assert all(np.abs(a.T @ a - np.eye(32)).max() < 1e-5 for a in mats)                             # orthogonal, each of the 6 L
    assert all(not np.allclose(mats[i], mats[j]) for i in range(12) for j in range(i))              # ... drawn on its own
    assert all(not v.any() for k, v in vals.items() if "/b_" in k)
    new = SR.init_from_shapes(shapes, np.random.default_rng(3))
    m.load_tf_variables(new)
    back = m.tf_values()
    assert all(np.array_equal(back[k], new[k].astype(np.float32)) for k in shapes)


@pytest.mark.parametrize("kw,flag", [(dict(num_units=50), "--num_units"), (dict(num_units=1024), "--num_units"),
                                     (dict(num_units=16), "--num_units"), (dict(num_blocks=0), "--num_blocks")])
def test_refused_shapes_name_the_flag(kw, flag):
    with pytest.raises(ValueError, match=flag):
        _model(**kw)


@pytest.mark.parametrize("flag", ["device_data", "graph", "lazy_adam"])
def test_the_driver_refuses_what_is_not_built_by_flag_name(flag):
    from easydgl_amd import train
    with pytest.raises(ValueError, match=f"--{flag} with --model GRU4REC"):
        train.run(SimpleNamespace(model="GRU4REC", seed=1, **{flag: True}))


@pytest.mark.parametrize("L", [1, 2, 3])
def test_the_restatements_stacked_gru_is_torch_nn_gru(L):
    rng = np.random.default_rng(L)
    p = {k: torch.tensor(rng.standard_normal(sh) * 0.5) for k, sh in GR.gru4rec_shapes(9, 6, L).items()}
    ref = torch.nn.GRU(6, 6, num_layers=L, batch_first=True).double()
    with torch.no_grad():
        for l in range(L):      # torch keeps [3C, in] blocks in the order r | z | n: the [in, out] parts transposed
            for name, v in zip(("weight_ih", "bias_ih", "weight_hh", "bias_hh"), GR.layer_parts(p, l)):
                getattr(ref, f"{name}_l{l}").copy_(v.t() if v.dim() == 2 else v)
    x = torch.tensor(rng.standard_normal((3, 5, 6)))
    assert (GR.stacked_gru(p, x, L) - ref(x)[0]).abs().max() < 1e-12
