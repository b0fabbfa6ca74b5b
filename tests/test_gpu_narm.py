"""NARM against the float64 restatement tests/_narm_ref.py: training and evaluation logits, loss and every gradient, at
(32 units, 1 GRU layer) and (64, 2), f32 and bf16; one epoch through the driver.  Bounds as tests/test_gpu_gru4rec.py: f32 1e-4
(logits, loss) and GRAD_TOL["f32"]; bf16 3e-2 (logits), LOSS_TOL and GRAD_TOL["bf16"]."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _narm_ref as NR
from tests._util import GRAD_TOL, LOSS_TOL, assert_close, grad_errors, to_dev

pytestmark = pytest.mark.gpu
B, T, N = 4, 9, 50


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("C,nb", [(32, 1), (64, 2)])
def test_model_logits_loss_and_gradients_match_float64(C, nb, mode):
    import easydgl_amd
    rng = np.random.default_rng(17 + C)
    params = NR.narm_params(N, C, nb, rng)
    if mode == "bf16":
        params = {k: torch.tensor(v).bfloat16().double().numpy() for k, v in params.items()}
    tokens = torch.tensor(rng.integers(1, N, size=(B, T + 1)))
    tokens[0, :3], tokens[1, 4], tokens[2, 7:] = 0, 0, 0      # (left padding; a zero inside; a sample whose last input id is 0)
    feats, labels = {"seqs_i": tokens[:, :-1].contiguous()}, tokens[:, 1:].contiguous()
    m = easydgl_amd.ranking(SimpleNamespace(model="NARM", num_items=N, num_units=C, num_heads=1, num_blocks=nb, seqslen=T,
                                            learning_rate=1e-3, l2_reg=1e-3, compute_dtype=mode, num_train_steps=None,
                                            num_warmup_steps=None)).finalize("cuda")
    m.load_tf_variables(params)
    ref, ref_tlog, ref_elog, ref_grads = NR.narm_train(params, feats, labels, C, nb, 1e-3)
    ftol = 1e-4 if mode == "f32" else 3e-2
    with torch.no_grad():
        tlog, elog = (m(to_dev(feats), training).float().cpu().numpy() for training in (True, False))
    assert tlog.shape == (B * T, N) and elog.shape == (B, N) and (elog[:, 0] == -1000.0).all()
    assert_close(tlog[:, 1:], ref_tlog[:, 1:], ftol, "training logits")
    assert_close(elog[:, 1:], ref_elog[:, 1:], ftol, "eval logits")
    m.zero_grad_arena()
    loss = m.train_loss(to_dev(feats), labels.cuda())
    loss.backward()
    grads = m.tf_gradients()
    errs = {k: grad_errors(g, ref_grads[k]) for k, g in grads.items()}
    e_loss = abs(loss.item() - ref) / abs(ref)
    print(f"narm {mode} C={C} nb={nb}: loss err {e_loss:.2e}; (rel-L2, max) {errs}")
    assert set(grads) == set(ref_grads) and e_loss <= LOSS_TOL[mode]
    assert all(l2 <= GRAD_TOL[mode][0] and mx <= GRAD_TOL[mode][1] for l2, mx in errs.values()), errs


def test_driver_runs_one_epoch(tmp_path):
    from easydgl_amd import data as D
    from easydgl_amd import formats as F
    from easydgl_amd import train as TR
    num_items, seqslen = 300, 20
    ids, ts = D.synthetic_batch(num_items, seqslen, 200, seed=3)

    def dump(name, lo, hi):
        F.write_tfrecord(str(tmp_path / name), [F.encode_example({"seqs_i": ids[i], "seqs_t": ts[i]}) for i in range(lo, hi)])
    dump("train000.tfrec", 0, 140); dump("validation.tfrec", 140, 170); dump("test.tfrec", 170, 200)
    res = TR.main(["--model", "NARM", "--train", str(tmp_path / "train*.tfrec"), "--valid", str(tmp_path / "validation.tfrec"),
                   "--test", str(tmp_path / "test.tfrec"), "--num_items", str(num_items), "--num_units", "32", "--num_blocks", "1",
                   "--seqslen", str(seqslen), "--batch_size", "64", "--num_epochs", "1", "--learning_rate", "1e-3", "--l2_reg", "1e-4",
                   "--hidden_dropout_rate", "0.1", "--mask_seen", "--dtype", "bf16", "--ckpt_dir", str(tmp_path / "ckpt")])
    assert set(res) == {"H10", "H50", "H100", "N10", "N50", "N100"}
    assert all(0.0 <= v <= 1.0 and math.isfinite(v) for v in res.values())
