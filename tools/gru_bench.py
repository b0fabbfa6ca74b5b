"""On the GPU box: what the GRU recurrence (csrc/k_gru.hip) and the two time-independent baselines cost.

  * the GRU op, forward plus backward (ops.GruSeqFn over a ready xp: the two recurrence kernels, their two pack launches and the
    dR / db_R GEMM) at B = 512, T in {30, 100}, C in {128, 512}, f32 and bf16; beside it torch.nn.GRU (the vendor RNN) at the same
    shapes on the same device, forward plus backward, where it runs — otherwise the line says so;
  * the per-step lower bounds of the streamed path, from shapes: the matrix pipe (2 * 16 * C * 3C flop per workgroup and step at
    the bf16 16x16x32 rate of one CU) and the L2 stream (every workgroup reads the 3 C^2 elements of R each step);
  * one optimizer step (train_step) of SASREC and S2PNM at the published flags (runme.sh:39-55: 512 units, 8 heads / 1 head,
    2 blocks / 1 block, batch 512, seqslen 30, 17 771 items) beside TGAT's and TiSASRec's from the SAME run.

Warm-up, device events around `iters` calls, `reps` repeats, median and min / max printed.
    python tools/gru_bench.py [--iters 10] [--reps 5] [--json out.json] [--skip-models]"""
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
from easydgl_amd import ops  # noqa: E402
from easydgl_amd.module.sequential import GRU  # noqa: E402
from easydgl_amd.util import ranking  # noqa: E402

B = 512
MFMA_BF16_FLOP_PER_CLK_CU = 4096      # dense bf16, one CU (MI355X: ~2.5 PFLOP/s over 256 CUs at 2.4 GHz)
CLOCK_HZ = 2.4e9
L2_BYTES_PER_CLK_CU = 64              # what one CU draws from its XCD's L2


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


def gru_op(T, C, dt, dev):
    g = GRU(C, C, gen=torch.Generator().manual_seed(0)).to(dev)
    R, bR, Rc = g.r_kernel.detach().requires_grad_(True), g.r_bias.detach().requires_grad_(True), g.r_kernel.detach().to(dt)
    gen = torch.Generator(device=dev).manual_seed(1)
    xp = torch.randn((B, T, 3 * C), device=dev, generator=gen).to(dt).requires_grad_(True)
    d_h = torch.randn((B, T, C), device=dev, generator=gen).to(dt)

    def both():
        h = ops.GruSeqFn.apply(xp, R, bR, Rc)
        h.backward(d_h)
        xp.grad = R.grad = bR.grad = None

    def fwd():
        with torch.no_grad():
            ops.GruSeqFn.apply(xp, R, bR, Rc)
    return both, fwd


def vendor_gru(T, C, dt, dev):
    g = torch.nn.GRU(C, C, batch_first=True).to(dev).to(dt)
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((B, T, C), device=dev, generator=gen).to(dt).requires_grad_(True)
    d_h = torch.randn((B, T, C), device=dev, generator=gen).to(dt)

    def both():
        h, _ = g(x)
        h.backward(d_h)
        x.grad = None
        g.zero_grad(set_to_none=True)
    return both


def lower_bounds(C, elem):
    """Per step and workgroup of the streamed forward: microseconds on the matrix pipe and on the L2 stream."""
    flop = 2.0 * 16 * C * 3 * C
    return dict(mfma_us=flop / MFMA_BF16_FLOP_PER_CLK_CU / CLOCK_HZ * 1e6, l2_us=3.0 * C * C * elem / L2_BYTES_PER_CLK_CU / CLOCK_HZ * 1e6)


def model_step(name, heads, blocks, dev):
    I, T, C = 17771, 30, 512
    drop = 0.2 if name == "S2PNM" else (0.0 if name == "SASREC" else 0.1)
    F = SimpleNamespace(model=name, num_items=I, num_units=C, num_heads=heads, num_blocks=blocks, seqslen=T, timelen=256,
                        time_scale=86400.0, learning_rate=1e-4, l2_reg=1e-4, hidden_dropout_rate=drop,
                        attention_probs_dropout_rate=drop, compute_dtype="bf16", num_train_steps=None, num_warmup_steps=None, seed=9876)
    m = ranking(F).finalize(dev)
    batches = []
    for k in range(4):
        ids, ts = D.synthetic_batch(I, T, B, seed=100 + k)
        tok, tim = torch.as_tensor(ids).to(dev), torch.as_tensor(ts).to(dev)
        batches.append(({"seqs_i": tok[:, :-1].contiguous(), "seqs_t": tim}, tok[:, 1:].contiguous()))
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
    ap.add_argument("--vendor", choices=["on", "off", "only"], default="on",
                    help="torch.nn.GRU beside the op: on, off, or only (the vendor RNN alone, e.g. in a process of its own)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    out = {"batch": B, "iters": a.iters, "reps": a.reps, "gru": [], "models": {}}
    for T in (30, 100):
        for C in (128, 512):
            for dt, nm in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
                row = dict(T=T, C=C, dtype=nm, resident=int(ops.lib.edgl_gru_seq_resident(C, ops._DT[dt])),
                           bounds=lower_bounds(C, 4 if nm == "f32" else 2), vendor_fwd_bwd=None, vendor_error="not run")
                if a.vendor != "off":
                    try:
                        row["vendor_fwd_bwd"] = spread(vendor_gru(T, C, dt, dev), a.iters, a.reps)
                    except Exception as e:       # (the vendor RNN does not run at this dtype / on this box: said, not hidden)
                        row["vendor_error"] = f"{type(e).__name__}: {str(e)[:200]}"
                v = row["vendor_fwd_bwd"]
                if a.vendor == "only":
                    out["gru"].append(row)
                    print(f"torch.nn.GRU B={B} T={T:3d} C={C:3d} {nm:4s}: fwd+bwd "
                          + (f"{v['median_ms']:8.3f} ms ({v['min_ms']:.3f} - {v['max_ms']:.3f})" if v else f"did not run: {row['vendor_error']}"), flush=True)
                    continue
                both, fwd = gru_op(T, C, dt, dev)
                row.update(fwd_bwd=spread(both, a.iters, a.reps), fwd=spread(fwd, a.iters, a.reps))
                out["gru"].append(row)
                print(f"GRU B={B} T={T:3d} C={C:3d} {nm:4s} {'LDS' if row['resident'] else 'L2 '}: fwd+bwd {row['fwd_bwd']['median_ms']:8.3f} ms "
                      f"({row['fwd_bwd']['min_ms']:.3f} - {row['fwd_bwd']['max_ms']:.3f}), fwd {row['fwd']['median_ms']:8.3f} ms, "
                      f"per step >= {row['bounds']['mfma_us']:.2f} us MFMA / {row['bounds']['l2_us']:.2f} us L2; torch.nn.GRU fwd+bwd "
                      + (f"{v['median_ms']:8.3f} ms ({v['min_ms']:.3f} - {v['max_ms']:.3f})" if v else f"did not run: {row['vendor_error']}"), flush=True)
    if not a.skip_models and a.vendor != "only":
        for name, heads, blocks in (("SASREC", 8, 2), ("S2PNM", 1, 1), ("TGAT", 1, 3), ("TiSASREC", 8, 2)):
            r = spread(model_step(name, heads, blocks, dev), a.iters, a.reps)
            out["models"][name] = r
            print(f"{name:9s} train_step B={B} T=30 C=512 H={heads} blocks={blocks} bf16: {r['median_ms']:8.3f} ms ({r['min_ms']:.3f} - {r['max_ms']:.3f})",
                  flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
