"""EasyDGL at sequence lengths beyond the in-register BiMAU kernels (the key-streamed kernels of csrc/k_bimau_stream.hip): the static
training engine, the autograd path, evaluation and the train driver, after the procedures of tests/test_gpu_engine.py,
tests/test_gpu_model.py and tests/test_train_driver.py."""
import math
import pickle

import numpy as np
import pytest
import torch

from oracle import easydgl_oracle as O
from oracle import torch_ref as R
from tests._util import GRAD_TOL, LOSS_TOL, build_model, grad_ok, make_problem, rel_err, to_dev

pytestmark = pytest.mark.gpu

CASES = [dict(num_units=32, num_heads=2, num_blocks=2, seqslen=224, masklen=10, num_events=4, num_items=50),       # head dim 16, T = 225
         dict(num_units=128, num_heads=2, num_blocks=1, seqslen=140, masklen=8, num_events=16, num_items=300),     # head dim 64, T = 141
         dict(num_units=32, num_heads=2, num_blocks=1, seqslen=224, masklen=6, num_events=24, num_items=80)]       # mark groups 16 + 8
L2_TABLES = ("CSTMA/item_embs/lookup_table", "CSTMA/mark_embs/lookup_table", "CSTMA/spatial_embs/embedding/lookup_table")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_engine_gradients_match_oracle_at_long_sequences(mode, case):
    from easydgl_amd import _lib
    from easydgl_amd.engine import TrainEngine
    prob = make_problem(seed=40 + case, batch=4, **CASES[case])
    cfg = prob["cfg"]
    assert _lib.lib.edgl_bimau_form(cfg.T, cfg.num_units, cfg.num_heads, _lib.BF16 if mode == "bf16" else _lib.F32, 0) == 1
    m = build_model(prob, mode)
    eng = TrainEngine(m, 4, use_graph=False)
    assert not eng.fused_tpp and not eng.fused_tail          # neither form exists at this T
    eng.load_batch(to_dev(prob["feats"]), torch.as_tensor(prob["labels"]).cuda())
    m._grad_arena.fill_(float("nan"))          # every gradient must be (over)written by the engine
    eng._issue()
    p64 = R.to_torch_params(prob["params"])
    ref, _ = R.train_loss(cfg, p64, prob["mark_table"], prob["feats"], prob["labels"])
    ref.backward()
    print(f"loss {float(eng.loss):.6f} oracle {float(ref):.6f}")
    assert abs(float(eng.loss) - float(ref)) <= LOSS_TOL[mode] * abs(float(ref))
    bad = {}
    for name, p in m.tf_variable_map().items():
        want = p64[name].grad.numpy().copy()
        if name in L2_TABLES:
            want -= cfg.l2_reg * prob["params"][name]      # the engine folds the l2 gradient into the Adam kernel
        ok, e = grad_ok(p.grad.cpu().numpy(), want, mode)
        if not ok:
            bad[name] = e
    assert not bad, (bad, GRAD_TOL[mode])


def test_engine_trajectory_eager_and_graph_at_long_sequences():
    """Three optimizer steps, eager launch sequence vs its HIP-graph capture: the same weights, and the oracle's Adam trajectory"""
    from easydgl_amd.engine import TrainEngine
    prob = make_problem(seed=50, batch=6, **CASES[0])
    cfg = prob["cfg"]
    feats, labels = to_dev(prob["feats"]), torch.as_tensor(prob["labels"]).cuda()
    p64 = R.to_torch_params(prob["params"])
    opt = R.TFAdam(p64, cfg.learning_rate)
    ref_losses = []
    for _ in range(3):
        ref, _ = R.train_loss(cfg, p64, prob["mark_table"], prob["feats"], prob["labels"])
        ref.backward()
        opt.step()
        ref_losses.append(float(ref))
    weights = []
    for use_graph in (False, True):
        m = build_model(prob, "f32")
        eng = TrainEngine(m, 6, use_graph=use_graph)
        losses = [float(eng.step(feats, labels)) for _ in range(3)]
        for a, b in zip(losses, ref_losses):
            assert abs(a - b) <= 2e-4 * abs(b), (use_graph, losses, ref_losses)
        for name, p in m.tf_variable_map().items():
            d = np.abs(p.detach().cpu().numpy() - p64[name].detach().numpy()).max()
            assert d < 3e-4, (use_graph, name, d)
        weights.append({n: p.detach().cpu().numpy() for n, p in m.tf_variable_map().items()})
    for n in weights[0]:
        assert np.abs(weights[0][n] - weights[1][n]).max() < 1e-5, n   # eager and replay: the same trajectory


def test_engine_with_dropout_matches_autograd_path_bf16_at_long_sequences():
    """Same (seed, step, op-id) -> same dropout masks in model.train_loss (autograd path) and the engine -> same loss and gradients"""
    from easydgl_amd import ops
    from easydgl_amd.engine import TrainEngine
    prob = make_problem(seed=51, batch=4, **CASES[0])
    feats, labels = to_dev(prob["feats"]), torch.as_tensor(prob["labels"]).cuda()
    m1 = build_model(prob, "bf16", hidden_drop=0.1, att_drop=0.1)
    m2 = build_model(prob, "bf16", hidden_drop=0.1, att_drop=0.1)
    eng = TrainEngine(m2, 4, use_graph=False)
    eng.load_batch(feats, labels)
    eng._issue()
    ops.rng_advance(m1._rng_state)
    m1.zero_grad_arena()
    loss = m1.train_loss(feats, labels)
    loss.backward()
    assert abs(float(loss) - float(eng.loss)) < 2e-3 * abs(float(loss))
    l2 = m1.l2_reg
    for (n1, p1), (n2, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        g1 = p1.grad.float().cpu().numpy()
        if n1 in m1.l2_param_names():
            g1 = g1 - l2 * p1.detach().cpu().numpy()
        assert rel_err(p2.grad.float().cpu().numpy(), g1) < 3e-2, n1


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_eval_metrics_and_topk_at_long_sequences(mode):
    """tests/test_gpu_model.py::test_eval_metrics_and_topk at the first long shape (600 items instead of 50: a top-100 list)"""
    prob = make_problem(seed=3, batch=8, **dict(CASES[0], num_items=600))
    cfg = prob["cfg"]
    m = build_model(prob, mode)
    ef, el = to_dev(prob["efeats"]), torch.as_tensor(prob["elabels"]).cuda()
    val, idx = m.eval_topk(ef, mask_seen=True)
    want_metrics, want_idx = O.evaluate(cfg, prob["params"], prob["mark_table"], prob["efeats"], prob["elabels"])
    got = idx.cpu().numpy()
    if mode == "f32":
        agree = (got == want_idx).mean()
        assert agree > 0.98, agree
    else:
        overlap = np.mean([len(set(got[r, :50]) & set(want_idx[r, :50])) / 50 for r in range(got.shape[0])])
        assert overlap > 0.9, overlap
    seen = prob["efeats"]["seqs_i"]
    for r in range(got.shape[0]):
        assert not (set(got[r]) & set(seen[r]))
    m.reset_metrics()
    m.eval_step(ef, el)
    mets = m.metrics()
    per = O.ranking_metrics(got, prob["elabels"][:, -1])
    for k in mets:
        assert abs(mets[k] - per[k].mean()) < 1e-5
    if mode == "f32":
        for k in mets:
            assert abs(mets[k] - want_metrics[k]) <= 1.0 / 8 + 1e-6


def test_driver_runs_two_steps_at_seqslen_224(tmp_path):
    """easydgl_amd/train.py on tiny synthetic .npz files with --seqslen 224: two optimizer steps of the engine and the evaluations"""
    sp = pytest.importorskip("scipy.sparse")
    from easydgl_amd import data as D
    from easydgl_amd import train as TR
    num_items, seqslen, E = 120, 224, 4
    ids, ts = D.synthetic_batch(num_items, seqslen, 48, seed=3)

    def dump(name, lo, hi):
        np.savez(str(tmp_path / name), seqs_i=np.asarray(ids[lo:hi], dtype=np.int64), seqs_t=np.asarray(ts[lo:hi], dtype=np.float32))
    dump("train.npz", 0, 32); dump("validation.npz", 32, 40); dump("test.npz", 40, 48)
    with open(tmp_path / "mark.pkl", "wb") as f:
        pickle.dump(sp.csr_matrix(D.synthetic_mark_table(num_items, E).astype(np.int64)), f)
    res = TR.main(["--model", "EasyDGL", "--train", str(tmp_path / "train.npz"), "--valid", str(tmp_path / "validation.npz"),
                   "--test", str(tmp_path / "test.npz"), "--num_items", str(num_items), "--num_units", "32", "--num_heads", "2",
                   "--num_blocks", "1", "--seqslen", str(seqslen), "--masklen", "10", "--time_scale", "86400", "--mark",
                   str(tmp_path / "mark.pkl"), "--ct_reg", "1e-7", "--batch_size", "16", "--num_epochs", "1", "--learning_rate",
                   "1e-3", "--l2_reg", "1e-4", "--mask_seen", "--dtype", "bf16", "--ckpt_dir", str(tmp_path / "ckpt")])
    assert set(res) == {"H10", "H50", "H100", "N10", "N50", "N100"}
    assert all(0.0 <= v <= 1.0 and math.isfinite(v) for v in res.values())
    assert res["H10"] <= res["H50"] <= res["H100"]
