"""tf_gradients() of the regressive models (derived from the variable table, model/base.py) hands the gradients of a backward out
under the reference's names: the K | V (| T_) projections that are stored as ONE matrix come back as the reference's dense_1 ..
dense_3, every other variable is its parameter's gradient — all bit for bit.  Unpadded CTSMA and TGAT in f32 at the smallest shape
that has every kind of variable."""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import baselines_ref as BR
from oracle import ctsma_ref as CR
from oracle import easydgl_oracle as O
from tests._util import to_dev

pytestmark = pytest.mark.gpu

B, T, I, E, C, H = 2, 8, 30, 4, 32, 2


@pytest.mark.parametrize("model", ["CTSMA", "TGAT"])
def test_gradients_under_the_reference_names(model):
    import easydgl_amd
    F = SimpleNamespace(model=model, num_items=I, num_units=C, num_heads=H, num_blocks=1, seqslen=T, timelen=64, time_scale=86400.0,
                        learning_rate=1e-3, l2_reg=1e-4, ct_reg=1e-3, hidden_dropout_rate=0.0, attention_probs_dropout_rate=0.0,
                        mark_table=O.synthetic_mark_table(I, E, multi_hot=True), compute_dtype="f32", num_train_steps=None,
                        num_warmup_steps=None)
    m = easydgl_amd.ranking(F).finalize("cuda")
    assert m.pad == (0, 0)
    rng = np.random.default_rng(11)
    tokens = rng.integers(1, I, size=(B, T + 1))
    tokens[0, :2] = 0
    ts = (9.5e8 + np.cumsum(rng.exponential(0.3 * 86400.0, size=(B, T + 1)), axis=1)).astype(np.float32)
    feats, labels = to_dev({"seqs_i": tokens[:, :-1].copy(), "seqs_t": ts}), torch.as_tensor(tokens[:, 1:].copy()).cuda()
    m.zero_grad_arena()
    m.train_loss(feats, labels).backward()
    got = m.tf_gradients()
    want_names = CR.init_params(I, T, C, H, E, 1, rng) if model == "CTSMA" else BR.tgat_init_params(I, T, C, 1, rng)
    assert set(got) == set(want_names)
    att = m.layers[0].attention
    fused_k, fused_b, blocks = (att.kvt_kernel, att.kvt_bias, 3) if model == "CTSMA" else (att.kv_kernel, att.kv_bias, 2)
    assert fused_k.shape[1] == blocks * C and float(fused_k.grad.abs().max()) > 0.0
    seen = 0
    for name, p, _, _ in m._pad_specs():
        g = got[name]
        assert isinstance(g, np.ndarray) and g.dtype == np.float32, name
        k = re.search(r"/dense_(\d)/(kernel|bias)$", name)
        if k:      # the k-th column block of the fused projection
            src = fused_k if k.group(2) == "kernel" else fused_b
            assert p is src, name
            want = src.grad[..., (int(k.group(1)) - 1) * C:int(k.group(1)) * C]
            seen += 1
        else:
            assert p is not fused_k and p is not fused_b, name
            want = p.grad
        assert np.array_equal(g, want.detach().cpu().numpy()), name
    assert seen == 2 * blocks
    # the table covers every parameter entry exactly once
    assert sum(g.size for g in got.values()) == sum(p.numel() for p in m.parameters())
