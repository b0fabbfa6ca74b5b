"""On the GPU box: ms per optimizer step of the static engine, default mode against deterministic mode, at the
headline shape (B = 512, T = 101, C = 128, I = 20 001, bf16, dropout 0.1 / 0.1, Zipf ids) — the two modes alternate within every
repeat — and the time of the deterministic mode's own launches alone: the two plans (the sort) and the two ordered sums.
Device events around `iters` steps / calls after a warm-up; `reps` repeats, median and min / max printed (the spread).
    python tools/det_step_bench.py [--iters 50] [--reps 5] [--batch 512] [--json out.json]"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from easydgl_amd import _lib, ops  # noqa: E402
from easydgl_amd.engine import TrainEngine  # noqa: E402

lib = _lib.lib


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    bench = _bench_module()
    c = dict(bench.HEADLINE, batch=a.batch)
    dev = torch.device("cuda", 0)
    engines, nb = {}, 4
    for mode in ("default", "deterministic"):
        model, batches = bench.make_model_and_batch(c, "bf16", dev, 9876, nbatch=nb)
        eng = TrainEngine(model, c["batch"], use_graph=False, deterministic=(mode == "deterministic"))
        eng.sync_loss = False
        state = dict(k=0)

        def step(eng=eng, batches=batches, state=state):
            eng.bind_batch(*batches[state["k"] % nb])
            state["k"] += 1
            eng.step()
        for _ in range(10):
            step()
        eng.join_loss()
        engines[mode] = (eng, step)
    torch.cuda.synchronize()
    ms = {m: [] for m in engines}
    for _ in range(a.reps):              # the modes alternate within a repeat
        for m, (eng, step) in engines.items():
            ms[m].append(timed(step, a.iters))
            eng.join_loss()
    out = {"shape": {k: c[k] for k in ("batch", "seqslen", "num_units", "num_items", "masklen")}, "iters": a.iters, "reps": a.reps}
    for m in ms:
        out[f"step_ms_{m}"] = stats(ms[m])
        s = out[f"step_ms_{m}"]
        print(f"step, {m:13s}: {s['median']:.4f} ms  (min {s['min']:.4f}, max {s['max']:.4f})", flush=True)
    # the deterministic mode's own launches on the operands of the last step (C ABI calls, as the engine issues them)
    eng = engines["deterministic"][0]
    m = eng.m
    P, st = ops._ptr, None
    B, T, C, E, I, R, code = eng.B, eng.T, eng.C, eng.E, eng.I, eng.R, eng.code
    tab = m.item_embs.lookup_table
    d_item, d_bias = torch.zeros_like(tab.grad), torch.zeros_like(m.output_bias.grad)
    d_pos, d_mk = torch.zeros_like(m.pcoding.pembs.lookup_table.grad), torch.zeros_like(m.mark_embs.lookup_table.grad)
    ws = torch.empty(lib.edgl_encode_bwd_workspace(B, T, C), device=dev)
    ids = eng.ids.reshape(-1)
    calls = {
        "plan_embedding_us": lambda: lib.edgl_segsum_plan(P(ids), B * T, None, I, 0, I, P(eng.plan_emb), st),
        "plan_labels_us": lambda: lib.edgl_segsum_plan(P(eng.labels_c), R, P(eng.nvalid), I, 0, I, P(eng.plan_lab), st),
        "label_term_det_us": lambda: lib.edgl_score_flash_label_term_det(P(eng.hrows_c), P(eng.labels_c), P(eng.coef), None, R, C, I, 0, I,
                                                                         P(eng.nvalid), P(d_item), P(d_bias), P(eng.plan_lab), code, st),
        "encode_bwd_det_us": lambda: lib.edgl_encode_bwd_add_det(P(eng.ids), P(eng.marks), P(eng.G3c), P(eng.G1), P(eng.G2), B, T, C, E, I, 0.1,
                                                                 P(m._rng_state), 1, P(d_item), P(d_pos), P(d_mk), P(ws), eng.c_true,
                                                                 P(eng.plan_emb), code, st),
        "encode_bwd_atomic_us": lambda: lib.edgl_encode_bwd_add_ct(P(eng.ids), P(eng.marks), P(eng.G3c), P(eng.G1), P(eng.G2), B, T, C, E, I,
                                                                   0.1, P(m._rng_state), 1, P(d_item), P(d_pos), P(d_mk), P(ws), eng.c_true,
                                                                   code, st),
        "label_term_atomic_us": lambda: lib.edgl_score_flash_label_term(P(eng.hrows_c), P(eng.labels_c), P(eng.coef), None, R, C, I, 0, I,
                                                                        P(eng.nvalid), P(d_item), P(d_bias), code, st),
    }
    for name, fn in calls.items():
        def checked(fn=fn, name=name):
            _lib.check(fn(), name)
        for _ in range(5):
            checked()
        torch.cuda.synchronize()
        v = [1e3 * timed(checked, a.iters) for _ in range(a.reps)]
        out[name] = stats(v)
        print(f"{name:22s}: {out[name]['median']:8.1f} us  (min {out[name]['min']:.1f}, max {out[name]['max']:.1f})", flush=True)
    print("(the _det calls build their plan first: label_term_det = plan_labels + the ordered sum, encode_bwd_det = the position / "
          "mark stage + plan_embedding + the ordered sum; back-to-back calls, launch gaps included)")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
