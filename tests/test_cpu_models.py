"""The four models' host side without a GPU (f32 models construct, finalize("cpu"), load and read variables on the CPU): initial
parameters bit-identical to the recorded digests, the variable table of each model (model/base.py) against its oracle's names and
reference shapes, and the load / read round trip — unpadded (32 / 2 heads) and channel-padded (20 / 2 heads: 10 -> 16, 48 / 1
head: 48 -> 64)."""
import json

import numpy as np
import pytest
import torch

from oracle import baselines_ref as BR
from oracle import ctsma_ref as CR
from oracle import easydgl_oracle as O
from tests.golden import make_init_digests as D

CASES = [(model, C, h) for model in D.MODELS for C, h in D.WIDTHS]


def _build(model, C, h):
    import easydgl_amd
    return easydgl_amd.ranking(D.flags(model, C, h))


def _oracle_params(model, C, h):
    """The oracle's variables at the TRUE width."""
    f, rng = D.FIXED, np.random.default_rng(0)
    I, T, E, nb = f["num_items"], f["seqslen"], f["num_events"], f["num_blocks"]
    if model == "EasyDGL":
        return O.init_params(O.Config(num_items=I, seqslen=T, num_units=C, num_heads=h, num_blocks=nb, num_events=E), rng)
    if model == "CTSMA":
        return CR.init_params(I, T, C, h, E, nb, rng)
    if model == "TGAT":
        return BR.tgat_init_params(I, T, C, nb, rng)
    return BR.tisasrec_init_params(I, f["timelen"], C, nb, rng)


def _np(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v


@pytest.mark.parametrize("model,C,h", CASES)
def test_initial_parameters_match_the_recorded_digests(model, C, h):
    want = json.load(open(D.PATH))["digests"][D.key(model, C, h)]
    assert D.model_digests(model, C, h) == want


@pytest.mark.parametrize("model,C,h", CASES)
def test_variable_names_and_reference_shapes(model, C, h):
    m = _build(model, C, h)
    dh = C // h
    assert m.width_true == C and m.pad == ((0, 0) if dh in (16, 32, 64, 128) else (next(d for d in (16, 32, 64, 128) if d >= dh), dh))
    want = _oracle_params(model, C, h)
    got = m.tf_values()
    assert set(got) == set(want)
    for k, v in got.items():
        assert tuple(v.shape) == want[k].shape, k
        if model == "EasyDGL":      # tensors, copies
            assert isinstance(v, torch.Tensor) and v.dtype == torch.float32
        else:
            assert isinstance(v, np.ndarray) and v.dtype == np.float32, k
    if model == "EasyDGL":
        vm = m.tf_variable_map()
        assert list(vm) == list(got) and all(isinstance(p, torch.nn.Parameter) for p in vm.values())
        assert all(v.data_ptr() != vm[k].data_ptr() for k, v in got.items())


@pytest.mark.parametrize("model,C,h", CASES)
def test_load_and_read_round_trip_on_the_cpu(model, C, h):
    m = _build(model, C, h).finalize("cpu")
    assert m.padded_leak() == 0.0
    new = {k: (_np(v) + 0.01).astype(np.float32) for k, v in m.tf_values().items()}
    m.load_tf_variables(new)
    assert m.padded_leak() == 0.0
    back = m.tf_values()
    assert set(back) == set(new)
    for k in new:
        assert np.array_equal(_np(back[k]), new[k]), k
    for k, v in m._padded_values(False).items():
        assert isinstance(v, torch.Tensor) and np.array_equal(v.numpy(), new[k]), k
    bad = dict(new)
    k0 = next(k for k in new if k.endswith("item_embs/lookup_table"))
    bad[k0] = np.zeros((new[k0].shape[0], new[k0].shape[1] + 16), np.float32)
    with pytest.raises(ValueError):
        m.load_tf_variables(bad)
