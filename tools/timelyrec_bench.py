"""On the GPU box: what the two TimelyREC kernels (csrc/k_mate.hip, csrc/k_tahe.hip) and the model's step cost.

  * ops.MateFn and ops.TaheFn, forward and forward plus backward, at B = 512, T in {30, 100}, C in {128, 512}, f32 and bf16; beside
    each a plain torch-op composition of the same math on the same device (the literal form: [B,T,W,C] slots, a cumsum over the
    sequence axis, a [B,T,T] weight matrix) — in this tool, not in the package;
  * a lower bound from shapes next to each: the bytes that must move (operands, result, saved set; with the gradients for the
    backward) at the HBM rate, and for TaheFn the dense MFMA work of its two (forward) / six (forward + backward) T x T x C products
    at the dense rate of the dtype;
  * one optimizer step (train_step) of TimelyREC at the published flags (runme.sh:98-105: 512 units, 4 heads, batch 512, seqslen 30,
    17 771 items) beside SASREC's, S2PNM's, TGAT's and TiSASRec's from the SAME run.

Warm-up, device events around `iters` calls, `reps` repeats, median and min / max printed.
    python tools/timelyrec_bench.py [--iters 10] [--reps 5] [--json out.json] [--skip-models]"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from easydgl_amd import data as D  # noqa: E402
from easydgl_amd import formats as F  # noqa: E402
from easydgl_amd import ops  # noqa: E402
from easydgl_amd.util import ranking  # noqa: E402

B = 512
RATIO = 0.2
HBM_BYTES_PER_S = 6.3e12                                   # achievable HBM rate of one MI355X
MFMA_FLOP_PER_S = {"bf16": 2.5e15, "f32": 2.5e15 / 16}     # dense rate; the exact-f32 MFMA runs at 1/16 of bf16


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def spread(fn, iters, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    v = [timed(fn, iters) for _ in range(reps)]
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))


# ---- the torch compositions (the literal form of TimelyREC.py:57-77,126-135 and sequential.py:220-265) -----------------------
def torch_mate(idx, tabs, u, pq):
    C = pq.shape[-1]
    Bn, T = idx.shape[1], idx.shape[2]
    periods = []
    for g, (M, tab) in enumerate(zip(ops.MATE_RANGES, tabs)):
        W = ops.mate_windows(RATIO)[g]
        f = idx[g]
        ok = ((f >= 0) & (f < M)).unsqueeze(-1).to(tab.dtype)
        e = (tab[f.clamp(0, M - 1)] * ok).unsqueeze(2)
        delta = torch.arange(1, W + 1, device=f.device).reshape(1, 1, W)
        win = torch.remainder(f.unsqueeze(-1) + torch.cat([delta, -delta], dim=2), M).reshape(Bn, T, 2, W)
        slots = torch.cumsum(tab[win].sum(dim=2), dim=1)
        den = (torch.arange(1, W + 1, device=f.device, dtype=torch.float32) * 2.0 + 1.0).to(tab.dtype).reshape(1, W, 1)
        keys = torch.cat([e, (e + slots) / den], dim=2)
        ug = u[..., g * C:(g + 1) * C].unsqueeze(2)
        Q, K = e * ug, keys * ug
        p = torch.softmax(Q @ K.transpose(2, 3) / (C ** 0.5), dim=-1)
        periods.append((p @ K).squeeze(2))
    keys = torch.stack(periods, dim=2)
    a = torch.sigmoid(pq.unsqueeze(2) @ keys.transpose(2, 3))
    return (a @ keys).squeeze(2)


def torch_tahe(R, Hs):
    n = R * torch.rsqrt(torch.clamp((R.float() ** 2).sum(-1, keepdim=True), min=1e-12)).to(R.dtype)
    S = (1.0 + n @ n.transpose(1, 2)) / 2.0
    return torch.tril(S) @ Hs


def mate_case(T, C, dt, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(s, device=dev, generator=gen)
    idx = torch.stack([torch.randint(0, M, (B, T), device=dev, generator=gen) for M in ops.MATE_RANGES]).contiguous()
    masters = [(0.2 * rnd(M, C)).requires_grad_(True) for M in ops.MATE_RANGES]
    u, pq = (0.5 * rnd(B, T, 4 * C)).to(dt).requires_grad_(True), (0.5 * rnd(B, T, C)).to(dt).requires_grad_(True)
    d_out = rnd(B, T, C).to(dt)
    w = ops.mate_windows(RATIO)
    leaves = masters + [u, pq]

    def clear():
        for t in leaves:
            t.grad = None

    def ours(bwd):
        def f():
            with torch.set_grad_enabled(bwd):
                out = ops.MateFn.apply(idx, *masters, *[m.detach().to(dt) for m in masters], u, pq, w)
            if bwd:
                out.backward(d_out)
                clear()
        return f

    def comp(bwd):
        def f():
            with torch.set_grad_enabled(bwd):
                out = torch_mate(idx, [m.to(dt) for m in masters], u, pq)
            if bwd:
                out.backward(d_out)
                clear()
        return f
    e = 4 if dt == torch.float32 else 2
    nsv = sum(x + 1 for x in w) + 4
    fwd_bytes = B * T * (4 * 8 + 6 * C * e + nsv * 4)                    # idx, u, pq, R, saved
    bwd_bytes = B * T * (4 * 8 + 6 * C * e + 2 * nsv * 4 + 6 * C * e)    # + d_R, d_u, d_pq and the coefficients once more
    return ours, comp, dict(fwd_us=fwd_bytes / HBM_BYTES_PER_S * 1e6, fwd_bwd_us=(fwd_bytes + bwd_bytes) / HBM_BYTES_PER_S * 1e6)


def tahe_case(T, C, dt, dev, nm):
    gen = torch.Generator(device=dev).manual_seed(2)
    rnd = lambda *s: torch.randn(s, device=dev, generator=gen)
    R, Hs = rnd(B, T, C).to(dt).requires_grad_(True), (0.3 * rnd(B, T, C)).to(dt).requires_grad_(True)
    d_out = rnd(B, T, C).to(dt)

    def run(fn, bwd):
        def f():
            with torch.set_grad_enabled(bwd):
                out = fn(R, Hs)
            if bwd:
                out.backward(d_out)
                R.grad = Hs.grad = None
        return f
    e = 4 if dt == torch.float32 else 2
    byt = lambda n: n * B * T * C * e / HBM_BYTES_PER_S * 1e6
    flop = lambda n: n * 2.0 * B * T * T * C / MFMA_FLOP_PER_S[nm] * 1e6
    bounds = dict(fwd_us=max(byt(3), flop(2)), fwd_bwd_us=max(byt(3 + 5), flop(2 + 6)), fwd_bytes_us=byt(3), fwd_mfma_us=flop(2))
    return (lambda bwd: run(ops.TaheFn.apply, bwd)), (lambda bwd: run(torch_tahe, bwd)), bounds


def model_step(name, heads, blocks, dev):
    I, T, C = 17771, 30, 512
    drop = 0.2 if name == "S2PNM" else (0.0 if name == "SASREC" else 0.1)
    Fl = SimpleNamespace(model=name, num_items=I, num_units=C, num_heads=heads, num_blocks=blocks, seqslen=T, timelen=256,
                         time_scale=86400.0, window_ratio=RATIO, learning_rate=1e-3 if name == "TimelyREC" else 1e-4, l2_reg=1e-4,
                         hidden_dropout_rate=drop, attention_probs_dropout_rate=drop, compute_dtype="bf16", num_train_steps=None,
                         num_warmup_steps=None, seed=9876)
    m = ranking(Fl).finalize(dev)
    batches = []
    for k in range(4):
        ids, ts = D.synthetic_batch(I, T, B, seed=100 + k)
        tok, tim = torch.as_tensor(ids).to(dev), torch.as_tensor(ts).to(dev)
        feats = {"seqs_i": tok[:, :-1].contiguous(), "seqs_t": tim}
        if name == "TimelyREC":
            for key, a in zip(F.CALENDAR_FIELDS, F.calendar_from_timestamps(ts, ids)):
                feats[key] = torch.as_tensor(np.ascontiguousarray(a[:, :-1])).to(dev)
        batches.append((feats, tok[:, 1:].contiguous()))
    state = dict(k=0)

    def step():
        m.train_step(*batches[state["k"] % len(batches)])
        state["k"] += 1
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-models", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    out = {"batch": B, "iters": a.iters, "reps": a.reps, "window_ratio": RATIO, "ops": [], "models": {}}
    fmt = lambda r: f"{r['median_ms']:8.3f} ms ({r['min_ms']:.3f} - {r['max_ms']:.3f})"
    for T in (30, 100):
        for C in (128, 512):
            for dt, nm in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
                for op, case in (("MateFn", mate_case(T, C, dt, dev)), ("TaheFn", tahe_case(T, C, dt, dev, nm))):
                    ours, comp, bounds = case
                    row = dict(op=op, T=T, C=C, dtype=nm, bounds=bounds)
                    row["fwd"], row["fwd_bwd"] = spread(ours(False), a.iters, a.reps), spread(ours(True), a.iters, a.reps)
                    try:
                        row["torch_fwd"], row["torch_fwd_bwd"] = spread(comp(False), a.iters, a.reps), spread(comp(True), a.iters, a.reps)
                        tail = f"torch composition fwd {fmt(row['torch_fwd'])}, fwd+bwd {fmt(row['torch_fwd_bwd'])}"
                    except Exception as e:       # (e.g. out of memory at the largest shape: said, not hidden)
                        row["torch_error"] = f"{type(e).__name__}: {str(e)[:160]}"
                        tail = f"torch composition did not run: {row['torch_error']}"
                        torch.cuda.empty_cache()
                    out["ops"].append(row)
                    print(f"{op} B={B} T={T:3d} C={C:3d} {nm:4s}: fwd {fmt(row['fwd'])}, fwd+bwd {fmt(row['fwd_bwd'])}; bound fwd "
                          f"{bounds['fwd_us']:.1f} us, fwd+bwd {bounds['fwd_bwd_us']:.1f} us; {tail}", flush=True)
    if not a.skip_models:
        for name, heads, blocks in (("TimelyREC", 4, 1), ("SASREC", 8, 2), ("S2PNM", 1, 1), ("TGAT", 1, 3), ("TiSASREC", 8, 2)):
            r = spread(model_step(name, heads, blocks, dev), a.iters, a.reps)
            out["models"][name] = r
            print(f"{name:9s} train_step B={B} T=30 C=512 H={heads} blocks={blocks} bf16: {fmt(r)}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
