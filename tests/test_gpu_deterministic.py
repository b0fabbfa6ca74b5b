"""Deterministic training mode: two runs from the same seed give the same bits — engine (eager and HIP graph),
autograd path and the driver — and the mode computes what the default mode computes (fp64 oracle)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import torch_ref as R
from tests._util import GRAD_TOL, LOSS_TOL, build_model, grad_ok, make_problem, to_dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (problem, batch, dtype): strip scoring (the deferred one-hot term) / generic scoring / wide strip / no block / a channel-padded
# model on a 12-item catalogue at batch 48 (>= 2 sort blocks, every id repeated hundreds of times: segments that cross windows)
HEAD = dict(num_units=128, num_heads=8, num_blocks=1, seqslen=100, masklen=20, num_events=16, num_items=2000)
CASES = [(HEAD, 4, "bf16"),
         (HEAD, 4, "f32"),
         (dict(num_units=256, num_heads=8, num_blocks=1, seqslen=40, masklen=8, num_events=16, num_items=1500), 4, "bf16"),
         (dict(num_units=64, num_heads=2, num_blocks=0, seqslen=30, masklen=6, num_events=7, num_items=300), 4, "bf16"),
         (dict(num_units=50, num_heads=1, num_blocks=1, seqslen=30, masklen=6, num_events=4, num_items=12), 48, "bf16")]


def _batches(case, n=3):
    kw, batch, _ = CASES[case]
    probs = [make_problem(seed=900 + 10 * case + i, batch=batch, **kw) for i in range(n)]
    return probs[0], [(to_dev(p["feats"]), torch.as_tensor(p["labels"]).cuda()) for p in probs]


def _state(m):
    m.settle_state()
    return {"arena": m._arena.detach().clone(), "adam_m": m._adam_m.clone(), "adam_v": m._adam_v.clone()}


def _diff_names(m, a, b):
    """names of the tensors that differ between two states (parameters by name, then the moments)"""
    out = []
    for name, p in m.named_parameters():
        o = m._offsets[name]
        for k in a:
            if not torch.equal(a[k][o:o + p.numel()], b[k][o:o + p.numel()]):
                out.append(f"{k}:{name}")
    return out


def _run_engine(case, batches, use_graph, prob):
    from easydgl_amd.engine import TrainEngine
    m = build_model(prob, CASES[case][2], hidden_drop=0.1, att_drop=0.1)
    eng = TrainEngine(m, CASES[case][1], use_graph=use_graph, deterministic=True)
    assert eng.deterministic and not eng._label_fused and eng._pending_label is None
    traj = []
    for feats, labels in batches:
        loss = eng.step(feats, labels).clone()
        torch.cuda.synchronize()
        traj.append((loss, _state(m)))
        assert not eng._label_fused and eng._pending_label is None
    return m, traj


def _assert_same(m, ta, tb, what):
    for step, ((la, sa), (lb, sb)) in enumerate(zip(ta, tb)):
        bad = _diff_names(m, sa, sb)
        if bad:
            print(f"{what}, step {step}: differing tensors: {bad}")
        assert not bad, (what, step, bad)
        assert torch.equal(la, lb), (what, step, float(la), float(lb))


@pytest.mark.parametrize("case", range(len(CASES)))
def test_engine_twice_gives_the_same_bits(case):
    prob, batches = _batches(case)
    m, t1 = _run_engine(case, batches, False, prob)
    _, t2 = _run_engine(case, batches, False, prob)
    _assert_same(m, t1, t2, "eager / eager")
    assert all(np.isfinite(float(l)) for l, _ in t1)
    assert not torch.equal(t1[0][1]["arena"], t1[2][1]["arena"])      # the steps moved the weights


def test_engine_graph_replay_gives_the_same_bits():
    """The first case under use_graph=True: replay against replay, and replay against the eager launch sequence."""
    prob, batches = _batches(0)
    m, te = _run_engine(0, batches, False, prob)
    _, g1 = _run_engine(0, batches, True, prob)
    _, g2 = _run_engine(0, batches, True, prob)
    _assert_same(m, g1, g2, "graph / graph")
    _assert_same(m, g1, te, "graph / eager")


@pytest.mark.parametrize("case", [0, 1])
def test_deterministic_engine_gradients_match_oracle(case):
    """tests/test_gpu_engine.py test_engine_gradients_match_oracle, in deterministic mode."""
    from easydgl_amd.engine import TrainEngine
    kw, batch, mode = CASES[case]
    ltol = LOSS_TOL[mode]
    prob = make_problem(seed=940 + case, batch=batch, **kw)
    cfg = prob["cfg"]
    m = build_model(prob, mode)
    eng = TrainEngine(m, batch, use_graph=False, deterministic=True)
    eng.load_batch(to_dev(prob["feats"]), torch.as_tensor(prob["labels"]).cuda())
    m._grad_arena.fill_(float("nan"))          # every gradient must be (over)written by the engine
    eng._issue()
    p64 = R.to_torch_params(prob["params"])
    ref, _ = R.train_loss(cfg, p64, prob["mark_table"], prob["feats"], prob["labels"])
    ref.backward()
    assert abs(float(eng.loss) - float(ref)) <= ltol * abs(float(ref))
    bad = {}
    for name, p in m.tf_variable_map().items():
        want = p64[name].grad.numpy().copy()
        if name in ("CSTMA/item_embs/lookup_table", "CSTMA/mark_embs/lookup_table", "CSTMA/spatial_embs/embedding/lookup_table"):
            want -= cfg.l2_reg * prob["params"][name]      # the engine folds the l2 gradient into the Adam kernel
        ok, e = grad_ok(p.grad.cpu().numpy(), want, mode)
        if not ok:
            bad[name] = e
    assert not bad, (bad, GRAD_TOL[mode])


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_autograd_path_twice_gives_the_same_bits_and_matches_oracle(mode):
    prob, batches = _batches(0)
    trajs = []
    for _ in range(2):
        m = build_model(prob, mode, hidden_drop=0.1, att_drop=0.1)
        m.deterministic = True
        t = []
        for feats, labels in batches:
            loss = m.train_step(feats, labels).clone()
            t.append((loss, _state(m)))
        trajs.append(t)
    _assert_same(m, trajs[0], trajs[1], "train_step / train_step")
    # gradients of the mode against the fp64 oracle (dropout off)
    m = build_model(prob, mode)
    m.deterministic = True
    m.zero_grad_arena()
    loss = m.train_loss(*batches[0])
    loss.backward()
    cfg = prob["cfg"]
    p64 = R.to_torch_params(prob["params"])
    ref, _ = R.train_loss(cfg, p64, prob["mark_table"], prob["feats"], prob["labels"])
    ref.backward()
    assert abs(float(loss) - float(ref)) <= LOSS_TOL[mode] * abs(float(ref))
    bad = {}
    for name, p in m.tf_variable_map().items():
        ok, e = grad_ok(p.grad.cpu().numpy(), p64[name].grad.numpy(), mode)
        if not ok:
            bad[name] = e
    assert not bad, (bad, GRAD_TOL[mode])


def test_default_mode_is_unchanged():
    """deterministic=False: the one-hot term rides in the embedding scatter's launch (bf16, C = 128) or on the side stream
    (wide strip) exactly as before, and no plan buffer exists."""
    from easydgl_amd.engine import TrainEngine
    prob, batches = _batches(0)
    m = build_model(prob, "bf16", hidden_drop=0.1, att_drop=0.1)
    assert m.deterministic is False
    eng = TrainEngine(m, 4, use_graph=False)
    assert eng.deterministic is False and eng.plan_emb is None and eng.plan_lab is None
    eng.step(*batches[0])
    assert eng._label_fused and eng._pending_label is None


def test_driver_twice_gives_the_same_checkpoint(tmp_path):
    """python -m easydgl_amd.train --deterministic, twice, each in a fresh process: two epochs over a set the batch size does not
    divide (full batches through the engine, the remainder through train_step) leave byte-identical parameters in the
    checkpoint the driver writes.  EarlyStopping saves when the validation H100 does not fall: on a 60-item catalogue without
    --mask_seen every label is among the top 100, H100 is 1 at both evaluations, and the second one — behind the last training
    step — writes EasyDGL.pt."""
    import re
    from easydgl_amd import data as D
    num_items, seqslen, E = 60, 20, 4
    ids, ts = D.synthetic_batch(num_items, seqslen, 200, seed=3)
    for name, lo, hi in (("train", 0, 150), ("valid", 150, 175), ("test", 175, 200)):
        np.savez(tmp_path / f"{name}.npz", seqs_i=ids[lo:hi], seqs_t=ts[lo:hi])
    np.save(tmp_path / "mark.npy", D.synthetic_mark_table(num_items, E))
    runs = []
    for run in range(2):
        ck = tmp_path / f"ckpt{run}"
        cmd = [sys.executable, "-m", "easydgl_amd.train",
               "--model", "EasyDGL", "--train", str(tmp_path / "train.npz"), "--valid", str(tmp_path / "valid.npz"),
               "--test", str(tmp_path / "test.npz"), "--num_items", str(num_items), "--num_units", "32", "--num_heads", "2",
               "--num_blocks", "1", "--seqslen", str(seqslen), "--masklen", "4", "--time_scale", "86400", "--mark",
               str(tmp_path / "mark.npy"), "--ct_reg", "1e-7", "--batch_size", "64", "--num_epochs", "2", "--learning_rate", "1e-3",
               "--l2_reg", "1e-4", "--hidden_dropout_rate", "0.1", "--attention_probs_dropout_rate", "0.1",
               "--deterministic", "--ckpt_dir", str(ck)]
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        losses = re.findall(r"Loss=([0-9.eE+-]+|nan)", r.stderr)
        assert len(losses) == 2, r.stderr[-3000:]
        assert (ck / "EasyDGL.pt").exists(), "the driver wrote no checkpoint:\n" + r.stderr[-3000:]
        ckp = torch.load(ck / "EasyDGL.pt", map_location="cpu")
        assert int(ckp["adam_state"][0]) == 6      # written behind the last step: 2 epochs x (2 engine steps + the remainder batch)
        runs.append((ckp["arena"].numpy().tobytes(), ckp["adam_m"].numpy().tobytes(), ckp["adam_v"].numpy().tobytes(), losses))
    assert runs[0][0] == runs[1][0], "parameter bytes differ between two --deterministic runs"
    assert runs[0][1:3] == runs[1][1:3], "Adam moments differ between two --deterministic runs"
    assert runs[0][3] == runs[1][3], (runs[0][3], runs[1][3])
