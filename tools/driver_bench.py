"""On the GPU box: ms per optimizer step of the DRIVER's training loop (easydgl_amd/train.py, one epoch, no evaluation) — what a
user of `python -m easydgl_amd.train` gets — against the resident-batch step that bench.py times.  DESIGN 4.10.

Workload: synthetic data at the headline shape of BASELINE.json (100 x 512 sequences, seqslen 100, 128 units, 20 001 items, masklen
20, 16 marks, dropout 0.1 / 0.1, bf16).  Legs, each with a model and an engine of its own:
    host          train.py's loop as it is without --device_data: numpy fancy-index of the split, two pageable host-to-device
                  copies, device_mask_random, the mask counter's increment, engine.step(feats, labels)
    device        --device_data: DeviceLoader attached to the engine, engine.step()
    device+graph  --device_data --graph: the same with use_graph=True (an epoch = 100 replays)
    floor         engine.step() on one resident batch, no data work and no loss read-back
The three driver legs keep the driver's loss read-back (join_loss + float(loss_sum) every 10 batches).  A host clock around the
epoch, ending in a device synchronise; the legs alternate inside one process, `--reps` repeats after a warm-up epoch each; per leg
the median ms per step and the spread (max - min) of the repeats.
The host and floor legs use only API that exists without the loader: this file, copied into an older checkout, runs there (the
device legs are then reported as absent) — that run is the baseline of the comparison.
    python tools/driver_bench.py [--batches 100] [--reps 3] [--out profiles/device_loader.txt] [--tag NAME]"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from easydgl_amd import data as D  # noqa: E402
from easydgl_amd.engine import TrainEngine  # noqa: E402

HAVE_LOADER = hasattr(D, "DeviceLoader") and hasattr(TrainEngine, "attach_loader")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _engine(bench, c, dev, use_graph):
    model, feats, labels = bench.make_model_and_batch(c, "bf16", dev, 9876)
    eng = TrainEngine(model, c["batch"], use_graph=use_graph)
    eng.sync_loss = False          # train.py: the loss is read at the logging points only
    eng.accumulate_loss = True
    return model, eng, feats, labels


def _readback(eng, nb, n):
    """train.py's logging point: every 10 batches and at the end of the epoch."""
    if nb % 10 == 0 or nb == n:
        eng.join_loss()
        return float(eng.loss_sum) / nb
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the report to this file")
    ap.add_argument("--tag", default="", help="a label for the report's heading (e.g. which checkout ran it)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    bench = _bench_module()
    c = dict(bench.HEADLINE)
    bs, n = c["batch"], a.batches
    dev = torch.device("cuda", 0)
    tr_i, tr_t = D.synthetic_batch(c["num_items"], c["seqslen"], n * bs, seed=9876)
    rng = np.random.default_rng(9876)
    legs = {}

    # ---- host: the loop of train.py:213-236 --------------------------------------------------------------------------------
    model, eng, _, _ = _engine(bench, c, dev, False)
    mask_state = torch.tensor([9876, 0], dtype=torch.int64, device="cuda")

    def host_epoch(model=model, eng=eng, mask_state=mask_state):
        order = rng.permutation(len(tr_i))
        eng.join_loss()
        eng.loss_sum.zero_()
        nb = 0
        for lo in range(0, len(order), bs):
            idx = order[lo:lo + bs]
            tok = torch.as_tensor(tr_i[idx]).cuda()
            tim = torch.as_tensor(tr_t[idx]).cuda()
            feats, labels = D.device_mask_random(tok, tim, model.mask, c["masklen"], mask_state)
            mask_state[1] += 1
            eng.step(feats, labels)
            nb += 1
            _readback(eng, nb, n)
    legs["host"] = host_epoch

    # ---- device / device+graph ------------------------------------------------------------------------------------------------
    if HAVE_LOADER:
        split = D.DeviceSplit(tr_i, tr_t)
        for name, use_graph in (("device", False), ("device+graph", True)):
            model, eng, _, _ = _engine(bench, c, dev, use_graph)
            loader = D.DeviceLoader(split, bs, "mask_random", model.mask, c["masklen"], 9876)
            eng.attach_loader(loader)

            def device_epoch(eng=eng, loader=loader):
                order = rng.permutation(len(tr_i))
                eng.join_loss()
                eng.loss_sum.zero_()
                loader.set_epoch(order)
                for nb in range(1, n + 1):
                    eng.step()
                    _readback(eng, nb, n)
            legs[name] = device_epoch

    # ---- floor: the resident-batch step ------------------------------------------------------------------------------------------
    model, eng, feats, labels = _engine(bench, c, dev, False)
    eng.accumulate_loss = False
    eng.bind_batch(feats, labels)

    def floor_epoch(eng=eng):
        for _ in range(n):
            eng.step()
        eng.join_loss()
    legs["floor"] = floor_epoch

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n

    for name, fn in legs.items():        # warm-up epoch (the graph leg captures in its first step)
        timed(fn)
    ms = {name: [] for name in legs}
    for _ in range(a.reps):               # the legs alternate within a repeat
        for name, fn in legs.items():
            ms[name].append(timed(fn))
    lines = [f"driver_bench {a.tag}: {n} batches of {bs}, seqslen {c['seqslen']}, {c['num_units']} units, {c['num_items'] + 1} items, "
             f"masklen {c['masklen']}, bf16; {a.reps} repeats after a warm-up epoch, host clock, ms per step",
             f"device: {torch.cuda.get_device_name(0)}"]
    out = {"tag": a.tag, "batches": n, "reps": a.reps}
    for name in ("host", "device", "device+graph", "floor"):
        if name not in ms:
            lines.append(f"  {name:13s}  absent in this checkout")
            continue
        v = ms[name]
        out[name] = dict(median=statistics.median(v), min=min(v), max=max(v), spread=max(v) - min(v))
        lines.append(f"  {name:13s}  median {out[name]['median']:.4f}  min {min(v):.4f}  max {max(v):.4f}  spread {max(v) - min(v):.4f}"
                     f"  repeats {' '.join(f'{x:.4f}' for x in v)}")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n\n")


if __name__ == "__main__":
    main()
