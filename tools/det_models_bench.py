"""On the GPU box: ms per train_step of CTSMA, TGAT and TiSASRec, default mode against deterministic mode, at
B = 512, L = 100, C = 128, 8 heads, I = 20 001, bf16, dropout 0.1 / 0.1, Zipf ids (CTSMA: 16 mark types, one block; TiSASRec:
timelen 256).  The two modes alternate within every repeat; device events around `iters` steps after a warm-up; `reps` repeats,
median and min / max printed (the spread).  `--modes default` times the default mode alone — the form that also runs on a tree
from before the mode existed, for reading the default path's numbers against its parent's.
    python tools/det_models_bench.py [--iters 20] [--reps 3] [--batch 512] [--modes default,deterministic] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from easydgl_amd import data as D  # noqa: E402
from easydgl_amd.util import ranking  # noqa: E402

L, C, H, I, E = 100, 128, 8, 20001, 16


def build(model, deterministic, batch, dev):
    F = SimpleNamespace(model=model, num_items=I, num_units=C, num_heads=H, num_blocks=1, seqslen=L, timelen=256, time_scale=86400.0,
                        learning_rate=1e-3, l2_reg=1e-4, ct_reg=1e-7, hidden_dropout_rate=0.1, attention_probs_dropout_rate=0.1,
                        compute_dtype="bf16", num_train_steps=None, num_warmup_steps=None, seed=9876,
                        mark_table=D.synthetic_mark_table(I, E), deterministic=deterministic)
    m = ranking(F).finalize(dev)
    batches = []
    for k in range(4):
        ids, ts = D.synthetic_batch(I, L, batch, seed=100 + k)
        tok, tim = torch.as_tensor(ids).to(dev), torch.as_tensor(ts).to(dev)
        batches.append(({"seqs_i": tok[:, :-1].contiguous(), "seqs_t": tim}, tok[:, 1:].contiguous()))
    return m, batches


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--modes", default="default,deterministic")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    modes = a.modes.split(",")
    out = {"shape": dict(batch=a.batch, seqslen=L, num_units=C, num_heads=H, num_items=I), "iters": a.iters, "reps": a.reps}
    for model in ("CTSMA", "TGAT", "TiSASREC"):
        steps = {}
        for mode in modes:
            m, batches = build(model, mode == "deterministic", a.batch, dev)
            state = dict(k=0)

            def step(m=m, batches=batches, state=state):
                m.train_step(*batches[state["k"] % len(batches)])
                state["k"] += 1
            for _ in range(5):
                step()
            steps[mode] = step
        torch.cuda.synchronize()
        ms = {mode: [] for mode in modes}
        for _ in range(a.reps):              # the modes alternate within a repeat
            for mode in modes:
                ms[mode].append(timed(steps[mode], a.iters))
        for mode in modes:
            v = ms[mode]
            out[f"{model}_step_ms_{mode}"] = dict(median=statistics.median(v), min=min(v), max=max(v))
            print(f"{model:9s} train_step, {mode:13s}: {statistics.median(v):8.3f} ms  (min {min(v):.3f}, max {max(v):.3f})", flush=True)
        del steps
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
