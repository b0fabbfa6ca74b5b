"""TrainEngine fed by the resident-split loader (attach_loader) against the same engine fed by the host path
(numpy indexing + data.device_mask_random + step(feats, labels)): same batches, same draws, hence — in deterministic mode —
the same bits, eager and as a captured graph; and the driver's --device_data / --device_data --graph runs against its plain run."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._util import build_model, make_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 4
NSEQ = 4 * B + 2        # four full batches and a remainder nobody draws here
SEED = 4711
# the head case of tests/test_gpu_deterministic.py, with one and with two blocks
HEAD = dict(num_units=128, num_heads=8, seqslen=100, masklen=20, num_events=16, num_items=2000)


def _problem(blocks):
    prob = make_problem(seed=970 + blocks, batch=NSEQ, num_blocks=blocks, **HEAD)
    ids, ts = np.asarray(prob["ids"], dtype=np.int64), np.asarray(prob["ts"], dtype=np.float32)
    perm = np.random.default_rng(5).permutation(NSEQ)
    return prob, ids, ts, perm


def _host_batches(m, ids, ts, perm, n):
    """The driver's host path: batch k = rows perm[k*B : (k+1)*B], masked on the device from (seed, k)."""
    from easydgl_amd import data as D
    mask_state = torch.tensor([SEED, 0], dtype=torch.int64, device="cuda")
    out = []
    for k in range(n):
        idx = perm[k * B:(k + 1) * B]
        tok, tim = torch.as_tensor(ids[idx]).cuda(), torch.as_tensor(ts[idx]).cuda()
        out.append(D.device_mask_random(tok, tim, m.mask, HEAD["masklen"], mask_state))
        mask_state[1] += 1
    return out


def _loader(m, ids, ts, perm):
    from easydgl_amd import data as D
    ld = D.DeviceLoader(D.DeviceSplit(ids, ts), B, "mask_random", m.mask, HEAD["masklen"], SEED)
    ld.set_epoch(perm)
    return ld


def _state(m):
    m.settle_state()
    torch.cuda.synchronize()
    return m._arena.detach().clone(), m._adam_m.clone(), m._adam_v.clone()


def _engine(prob, mode, deterministic, use_graph=False):
    from easydgl_amd.engine import TrainEngine
    m = build_model(prob, mode, hidden_drop=0.1, att_drop=0.1)
    return m, TrainEngine(m, B, use_graph=use_graph, deterministic=deterministic)


@pytest.mark.parametrize("mode,blocks", [("f32", 1), ("bf16", 1), ("f32", 2), ("bf16", 2)])
def test_loader_fed_engine_gives_the_bits_of_the_host_path(mode, blocks):
    prob, ids, ts, perm = _problem(blocks)
    ma, ea = _engine(prob, mode, True)
    for feats, labels in _host_batches(ma, ids, ts, perm, 3):
        ea.step(feats, labels)
    mb, eb = _engine(prob, mode, True)
    ld = _loader(mb, ids, ts, perm)
    eb.attach_loader(ld)
    for _ in range(3):
        eb.step()
    sa, sb = _state(ma), _state(mb)
    for name, a, b in zip(("arena", "adam_m", "adam_v"), sa, sb):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    assert ld.state.tolist() == [SEED, 3, 3 * B, 0] and ld.remaining() == NSEQ - 3 * B
    assert not torch.equal(sa[0], build_model(prob, mode)._arena)      # the steps moved the weights


def test_default_mode_agrees_within_the_atomics_order():
    """deterministic=False: the f32 atomics of the embedding scatter may land in another order — the bound
    tests/test_train_driver.py uses for exactly that (1e-6 relative on the loss, 1e-6 absolute on the weights)."""
    prob, ids, ts, perm = _problem(1)
    ma, ea = _engine(prob, "bf16", False)
    feats, labels = _host_batches(ma, ids, ts, perm, 1)[0]
    la = float(ea.step(feats, labels))
    mb, eb = _engine(prob, "bf16", False)
    eb.attach_loader(_loader(mb, ids, ts, perm))
    lb = float(eb.step())
    assert torch.equal(eb.ids, feats["seqs_i"]) and torch.equal(eb.labels, labels)
    sa, sb = _state(ma), _state(mb)
    print(f"loss host {la!r} loader {lb!r}; max |d arena| {float((sa[0] - sb[0]).abs().max()):.3e}")
    assert math.isfinite(la) and abs(la - lb) <= 1e-6 * abs(la)
    assert float((sa[0] - sb[0]).abs().max()) <= 1e-6
    # step(features, labels) still works with a loader attached (eager engine), and draws nothing
    eb.step(feats, labels)
    assert eb.loader.state.tolist() == [SEED, 1, B, 0]


def test_captured_step_draws_its_batches_on_the_device():
    """use_graph=True: the warm-up step (a real step) and three replays consume batches 0..3 of the epoch."""
    prob, ids, ts, perm = _problem(1)
    runs = {}
    for use_graph in (False, True):
        m, eng = _engine(prob, "bf16", True, use_graph=use_graph)
        eng.accumulate_loss = True
        ld = _loader(m, ids, ts, perm)
        eng.attach_loader(ld)
        losses = []
        for _ in range(4):
            loss = eng.step()
            torch.cuda.synchronize()
            losses.append(loss.clone())
        runs[use_graph] = (m, eng, ld, losses, _state(m))
    m, eng, ld, losses, sg = runs[True]
    assert eng.graph is not None and eng._graph_feeds
    for name, a, b in zip(("arena", "adam_m", "adam_v"), runs[False][4], sg):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    for k, (a, b) in enumerate(zip(runs[False][3], losses)):
        assert torch.equal(a, b), (k, float(a), float(b))
    assert ld.cursor() == 4 * B and ld.state.tolist() == [SEED, 4, 4 * B, 0] and ld.remaining() == NSEQ - 4 * B
    host = _host_batches(m, ids, ts, perm, 4)
    assert torch.equal(eng.ids, host[3][0]["seqs_i"]) and torch.equal(eng.ts, host[3][0]["seqs_t"])
    assert torch.equal(eng.mpos, host[3][0]["masked_positions"]) and torch.equal(eng.labels, host[3][1])
    want = torch.zeros(1, device="cuda", dtype=torch.float64)
    for l in losses:
        want += l.double()
    assert torch.equal(eng.loss_sum, want), (float(eng.loss_sum), float(want))
    with pytest.raises(Exception, match="takes no batch"):
        eng.step(*host[0])


def test_attach_loader_refusals():
    from easydgl_amd._lib import EdglError
    from easydgl_amd import data as D
    from easydgl_amd.engine import TrainEngine
    prob, ids, ts, perm = _problem(1)
    m = build_model(prob, "bf16")
    ld = _loader(m, ids, ts, perm)
    with pytest.raises(EdglError, match="process_group"):
        TrainEngine(m, B, use_graph=False, process_group=object()).attach_loader(ld)
    eng = TrainEngine(m, B, use_graph=False)
    with pytest.raises(EdglError, match="mask_random"):
        eng.attach_loader(D.DeviceLoader(ld.split, B, "mask_last", m.mask))
    with pytest.raises(EdglError, match="does not match"):
        eng.attach_loader(D.DeviceLoader(ld.split, B + 1, "mask_random", m.mask, HEAD["masklen"], SEED))


# ---- the driver, fresh processes: the set of tests/test_gpu_deterministic.py::test_driver_twice_gives_the_same_checkpoint ----
def _tiny_files(tmp_path, num_items, seqslen, E):
    from easydgl_amd import data as D
    ids, ts = D.synthetic_batch(num_items, seqslen, 200, seed=3)
    for name, lo, hi in (("train", 0, 150), ("valid", 150, 175), ("test", 175, 200)):
        np.savez(tmp_path / f"{name}.npz", seqs_i=ids[lo:hi], seqs_t=ts[lo:hi])
    np.save(tmp_path / "mark.npy", D.synthetic_mark_table(num_items, E))


def _driver_args(tmp_path, model, num_items, seqslen, ck):
    return ["--model", model, "--train", str(tmp_path / "train.npz"), "--valid", str(tmp_path / "valid.npz"),
            "--test", str(tmp_path / "test.npz"), "--num_items", str(num_items), "--num_units", "32", "--num_heads", "2",
            "--num_blocks", "1", "--seqslen", str(seqslen), "--masklen", "4", "--time_scale", "86400", "--mark",
            str(tmp_path / "mark.npy"), "--ct_reg", "1e-7", "--batch_size", "64", "--num_epochs", "2", "--learning_rate", "1e-3",
            "--l2_reg", "1e-4", "--hidden_dropout_rate", "0.1", "--attention_probs_dropout_rate", "0.1", "--ckpt_dir", str(ck)]


def test_driver_device_data_runs_give_the_plain_run(tmp_path):
    """150 training sequences at batch 64 (two engine steps + the remainder batch per epoch), --deterministic: the plain run, the
    --device_data run and the --device_data --graph run leave the same parameter / moment bytes in EasyDGL.pt, log the same
    Loss= strings and the same six summary metrics."""
    num_items, seqslen, E = 60, 20, 4
    _tiny_files(tmp_path, num_items, seqslen, E)
    runs = []
    for run, extra in enumerate(([], ["--device_data"], ["--device_data", "--graph"])):
        ck = tmp_path / f"ckpt{run}"
        cmd = [sys.executable, "-m", "easydgl_amd.train"] + _driver_args(tmp_path, "EasyDGL", num_items, seqslen, ck) + \
            ["--deterministic"] + extra
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        losses = re.findall(r"Loss=([0-9.eE+-]+|nan)", r.stderr)
        assert len(losses) == 2, r.stderr[-3000:]
        summary = re.findall(r"SUMMARY: (\{.*\})", r.stderr)
        assert len(summary) == 1 and len(re.findall(r"'[HN]\d+': '[0-9.]+'", summary[0])) == 6, r.stderr[-3000:]
        assert ("resident on the device" in r.stderr) == bool(extra)
        assert (ck / "EasyDGL.pt").exists(), "the driver wrote no checkpoint:\n" + r.stderr[-3000:]
        ckp = torch.load(ck / "EasyDGL.pt", map_location="cpu")
        assert int(ckp["adam_state"][0]) == 6      # 2 epochs x (2 engine steps + the remainder batch)
        runs.append((ckp["arena"].numpy().tobytes(), ckp["adam_m"].numpy().tobytes(), ckp["adam_v"].numpy().tobytes(), losses,
                     summary[0]))
    for other, what in ((runs[1], "--device_data"), (runs[2], "--device_data --graph")):
        assert runs[0][0] == other[0], f"parameter bytes differ: plain / {what}"
        assert runs[0][1:3] == other[1:3], f"Adam moments differ: plain / {what}"
        assert runs[0][3] == other[3], (what, runs[0][3], other[3])
        assert runs[0][4] == other[4], (what, runs[0][4], other[4])


@pytest.mark.parametrize("model,extra", [("CTSMA", ["--device_data"]), ("TGAT", ["--device_data", "--graph"])])
def test_driver_device_data_regressive_models(tmp_path, model, extra):
    """The regressive models take loader.next() into train_step / graphed_train_step (these models keep f32 atomics: no bitwise
    claim here; the loader's equality in their modes is tests/test_gpu_loader.py)."""
    from easydgl_amd import train as TR
    num_items, seqslen, E = 60, 20, 4
    _tiny_files(tmp_path, num_items, seqslen, E)
    res = TR.main(_driver_args(tmp_path, model, num_items, seqslen, tmp_path / "ckpt") + ["--timelen", "32"] + extra)
    assert set(res) == {"H10", "H50", "H100", "N10", "N50", "N100"}
    assert all(math.isfinite(v) and 0.0 <= v <= 1.0 for v in res.values()), res
    assert res["H10"] <= res["H50"] <= res["H100"], res


def test_driver_refuses_splits_that_do_not_fit(tmp_path, monkeypatch):
    """--device_data never falls back to the host path: splits larger than the free device memory are refused, byte count named."""
    from easydgl_amd import train as TR
    num_items, seqslen, E = 60, 20, 4
    _tiny_files(tmp_path, num_items, seqslen, E)
    need = 200 * (seqslen + 1) * 12 + 200 * 4            # ids int64 + times f32 of the three splits, + an int32 order each
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (need - 1, 1 << 40))
    with pytest.raises(RuntimeError, match=rf"need {need} bytes of device memory, {need - 1} bytes are free"):
        TR.main(_driver_args(tmp_path, "EasyDGL", num_items, seqslen, tmp_path / "ckpt") + ["--device_data"])
