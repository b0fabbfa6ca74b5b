"""On the GPU box: forward + backward time of the BiMAU unit (bf16, C ABI calls, attention dropout 0.1) in its two kernel families.
  (a) in-register vs forced key-streamed (EDGL_MAU_STREAM) at shapes both take, alternating the two forms within every repeat;
  (b) key-streamed alone beyond the in-register bounds.
Device events around `iters` calls after a warm-up of every shape and form; `reps` repeats, median and min / max printed (the spread).
    python tools/bimau_stream_bench.py [--iters 20] [--reps 5] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from easydgl_amd import _lib, ops  # noqa: E402
from oracle import easydgl_oracle as O  # noqa: E402

lib = _lib.lib
BOTH = [(512, 201, 256, 8, 16), (512, 128, 512, 8, 16)]
LONG = [(64, 513, 128, 8, 16), (64, 257, 512, 8, 16)]


class Unit:
    """the operands of one shape; call(flags) runs one forward + backward through the C ABI"""

    def __init__(self, B, T, C, H, E, seed=0):
        self.shape = (B, T, C, H, E)
        dh = C // H
        rng = np.random.default_rng(seed)
        bf = torch.bfloat16
        self.qkvt = torch.tensor(rng.standard_normal((B, T, 4 * C)) * 0.4, dtype=bf).cuda()
        self.resid = torch.tensor(rng.standard_normal((B, T, C)), dtype=bf).cuda()
        self.spans = torch.tensor(rng.uniform(0, 5, size=(B, T)), dtype=torch.float32).cuda()
        W1 = torch.tensor(rng.standard_normal((dh + 1, dh * E)) * 0.2, dtype=torch.float32).cuda()
        b1 = torch.zeros(dh * E, device="cuda")
        w = torch.tensor(rng.standard_normal((E, dh)) * 0.3, dtype=torch.float32).cuda()
        sc = torch.zeros(E, device="cuda")
        self.d_out = torch.tensor(rng.standard_normal((B, T, C)), dtype=bf).cuda()
        self.code = ops._code(self.qkvt)
        self.pack = torch.empty(lib.edgl_bimau_pack_bytes(C, H, E, self.code), device="cuda", dtype=torch.uint8)
        _lib.check(lib.edgl_bimau_pack(W1.data_ptr(), b1.data_ptr(), w.data_ptr(), sc.data_ptr(), C, H, E, self.pack.data_ptr(), self.code, None), "pack")
        self.state = ops.make_rng_state("cuda", seed=1)
        ops.rng_advance(self.state)
        ids = rng.integers(1, 30, size=(B, T))
        for b in range(B):                      # the benchmark's own lengths: U{5..T}, left-padded
            ids[b, :T - rng.integers(5, T + 1)] = 0
        self.ids = torch.tensor(ids).cuda()
        self.marks = torch.tensor(O.synthetic_mark_table(30, E, multi_hot=False)[ids].astype(np.uint8)).cuda()
        self.out = torch.empty((B, T, C), device="cuda", dtype=bf)
        self.lam = torch.empty((H * B, T, E), device="cuda")
        self.d_lam = torch.zeros((H * B, T, E), device="cuda")
        self.dq = torch.empty_like(self.qkvt)
        self.g = torch.empty((dh + 3) * dh * E + E, device="cuda")
        self.n = ((dh + 1) * dh * E, dh * E, E * dh)
        self.bufs = {}

    def call(self, flags):
        B, T, C, H, E = self.shape
        if flags not in self.bufs:
            self.bufs[flags] = (torch.empty(lib.edgl_bimau_saved_bytes_ex(B, T, C, H, self.code, flags), device="cuda", dtype=torch.uint8),
                                torch.empty(lib.edgl_bimau_bwd_workspace_ex(B, T, C, H, E, self.code, flags), device="cuda", dtype=torch.uint8))
        saved, ws = self.bufs[flags]
        n1, n2, n3 = self.n
        g = self.g
        _lib.check(lib.edgl_bimau_fwd_db(self.qkvt.data_ptr(), self.resid.data_ptr(), C, self.ids.data_ptr(), self.spans.data_ptr(), self.marks.data_ptr(),
                                         self.pack.data_ptr(), B, T, C, H, E, 0.1, self.state.data_ptr(), 10, None, 0.0, self.out.data_ptr(),
                                         self.lam.data_ptr(), saved.data_ptr(), None, flags, self.code, None), "fwd")
        _lib.check(lib.edgl_bimau_bwd_db(self.qkvt.data_ptr(), self.ids.data_ptr(), self.spans.data_ptr(), self.marks.data_ptr(), self.pack.data_ptr(),
                                         self.d_out.data_ptr(), self.d_lam.data_ptr(), self.lam.data_ptr(), saved.data_ptr(), B, T, C, H, E, 0.1,
                                         self.state.data_ptr(), 10, None, 0.0, self.dq.data_ptr(), g.data_ptr(), g[n1:].data_ptr(),
                                         g[n1 + n2:].data_ptr(), g[n1 + n2 + n3:].data_ptr(), ws.data_ptr(), flags, self.code, None), "bwd")


def timed(u, flags, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        u.call(flags)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rows = []
    for shape, forms in [(s, (0, _lib.MAU_STREAM)) for s in BOTH] + [(s, (0,)) for s in LONG]:
        B, T, C, H, E = shape
        u = Unit(*shape)
        for f in forms:                      # warm-up: code objects, buffers
            for _ in range(3):
                u.call(f)
        torch.cuda.synchronize()
        ms = {f: [] for f in forms}
        for _ in range(a.reps):              # the forms alternate within a repeat
            for f in forms:
                ms[f].append(timed(u, f, a.iters))
        for f in forms:
            form = lib.edgl_bimau_form(T, C, H, u.code, f)
            r = dict(shape=list(shape), form="streamed" if form == 1 else "in-register", ms_median=statistics.median(ms[f]), ms_min=min(ms[f]),
                     ms_max=max(ms[f]), iters=a.iters, reps=a.reps)
            rows.append(r)
            print(f"(B,T,C,H,E)={shape}  {r['form']:11s}  fwd+bwd {r['ms_median']:8.3f} ms  (min {r['ms_min']:.3f}, max {r['ms_max']:.3f})", flush=True)
        del u
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
