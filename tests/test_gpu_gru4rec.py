"""GRU4REC against the float64 restatement tests/_gru4rec_ref.py: training and evaluation logits (one sample ends on id 0), loss,
every gradient; 1 and 2 layers; 32 units (R LDS-resident: the existing kernels) and 256 (streamed in both dtypes: csrc/k_gru_wide.hip).
Bounds: f32 1e-4 (logits, loss) and GRAD_TOL["f32"], as the other model tests; bf16 3e-2 (logits), LOSS_TOL and GRAD_TOL["bf16"]."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _gru4rec_ref as GR
from tests import _seq_baselines_ref as SR
from tests._util import GRAD_TOL, LOSS_TOL, assert_close, grad_errors, to_dev

pytestmark = pytest.mark.gpu
B, T, N = 5, 7, 50


def _flags(mode, C, nb, **kw):
    return SimpleNamespace(model="GRU4REC", num_items=N, num_units=C, num_heads=1, num_blocks=nb, seqslen=T, learning_rate=1e-3,
                           l2_reg=1e-3, compute_dtype=mode, num_train_steps=None, num_warmup_steps=None, **kw)


def _batch(rng):
    tokens = torch.tensor(rng.integers(1, N, size=(B, T + 1)))
    tokens[0, :3], tokens[2, 5:] = 0, 0          # (left padding; a sample whose last input id is 0)
    return {"seqs_i": tokens[:, :-1].contiguous()}, tokens[:, 1:].contiguous()


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("C", [32, 256])
@pytest.mark.parametrize("nb", [1, 2])
def test_model_logits_loss_and_gradients_match_float64(nb, C, mode):
    import easydgl_amd
    rng = np.random.default_rng(31 + nb + C)
    params = SR.init_from_shapes(GR.gru4rec_shapes(N, C, nb), rng)
    if mode == "bf16":
        params = {k: torch.tensor(v).bfloat16().double().numpy() for k, v in params.items()}
    feats, labels = _batch(rng)
    m = easydgl_amd.ranking(_flags(mode, C, nb)).finalize("cuda")
    m.load_tf_variables(params)
    p64 = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    ref, ref_tlog, ref_elog = GR.gru4rec_train(p64, feats, labels, C, nb, 1e-3)
    ref.backward()
    ftol = 1e-4 if mode == "f32" else 3e-2
    with torch.no_grad():
        tlog, elog = (m(to_dev(feats), training).float().cpu().numpy() for training in (True, False))
    assert tlog.shape == (B * T, N) and elog.shape == (B, N) and (elog[:, 0] == -1000.0).all() and int(feats["seqs_i"][2, -1]) == 0
    assert_close(tlog[:, 1:], ref_tlog.detach().numpy()[:, 1:], ftol, "training logits")
    assert_close(elog[:, 1:], ref_elog.detach().numpy()[:, 1:], ftol, "eval logits")
    m.zero_grad_arena()
    loss = m.train_loss(to_dev(feats), labels.cuda())
    loss.backward()
    grads = m.tf_gradients()
    errs = {k: grad_errors(g, p64[k].grad.numpy()) for k, g in grads.items()}
    e_loss = abs(loss.item() - ref.item()) / abs(ref.item())
    print(f"gru4rec {mode} C={C} nb={nb}: loss err {e_loss:.2e}; (rel-L2, max) {errs}")
    assert set(grads) == set(p64) and e_loss <= LOSS_TOL[mode]
    assert all(l2 <= GRAD_TOL[mode][0] and mx <= GRAD_TOL[mode][1] for l2, mx in errs.values()), errs


def test_deterministic_train_step_twice_gives_the_same_weights():
    import easydgl_amd
    feats, labels = _batch(np.random.default_rng(5))
    arenas = []
    for _ in range(2):
        m = easydgl_amd.ranking(_flags("bf16", 256, 2, deterministic=True, hidden_dropout_rate=0.2, seed=11)).finalize("cuda")
        m.train_step(to_dev(feats), labels.cuda())
        arenas.append(m._arena.clone())
    assert torch.equal(arenas[0], arenas[1])
