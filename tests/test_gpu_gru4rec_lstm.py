"""GRU4REC with rnn_cell="lstm"  against the float64 model tests/_gru4rec_lstm_ref.py (torch.nn.LSTM(num_layers=L).double()):
training and evaluation logits, loss, every gradient, on the batch of tests/test_gpu_gru4rec.py (left padding, one sample ending on id 0).
Bounds as there: f32 1e-4 (logits, loss) and GRAD_TOL["f32"]; bf16 3e-2 (logits), LOSS_TOL and GRAD_TOL["bf16"]."""
import numpy as np
import pytest
import torch

from tests import _gru4rec_lstm_ref as LR
from tests import _seq_baselines_ref as SR
from tests._util import GRAD_TOL, LOSS_TOL, assert_close, grad_errors, to_dev
from tests.test_gpu_gru4rec import B, N, T, _batch, _flags

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("C", [32, 256])
@pytest.mark.parametrize("nb", [1, 2])
def test_lstm_model_logits_loss_and_gradients_match_float64(nb, C, mode):
    import easydgl_amd
    rng = np.random.default_rng(47 + nb + C)
    params = SR.init_from_shapes(LR.shapes(N, C, nb), rng)
    if mode == "bf16":
        params = {k: torch.tensor(v).bfloat16().double().numpy() for k, v in params.items()}
    feats, labels = _batch(rng)
    m = easydgl_amd.ranking(_flags(mode, C, nb, rnn_cell="lstm")).finalize("cuda")
    m.load_tf_variables(params)
    p64 = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    ref, ref_tlog, ref_elog = LR.train(p64, feats, labels, C, nb, 1e-3)
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
    print(f"gru4rec lstm {mode} C={C} nb={nb}: loss err {e_loss:.2e}; (rel-L2, max) {errs}")
    assert set(grads) == set(p64) and e_loss <= LOSS_TOL[mode]
    assert all(l2 <= GRAD_TOL[mode][0] and mx <= GRAD_TOL[mode][1] for l2, mx in errs.values()), errs
