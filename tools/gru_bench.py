"""On the GPU box: what the GRU recurrence (csrc/k_gru.hip) and the two time-independent baselines cost.

  * the GRU op, forward plus backward (ops.GruSeqFn over a ready xp: the two recurrence kernels, their two pack launches and the
    dR / db_R GEMM) at B = 512, T in {30, 100}, C in {128, 512}, f32 and bf16; beside it torch.nn.GRU (the vendor RNN) at the same
    shapes on the same device, forward plus backward, where it runs — otherwise the line says so;
  * the per-step lower bounds of the streamed path, from shapes: the matrix pipe (2 * 16 * C * 3C flop per workgroup and step at
    the bf16 16x16x32 rate of one CU) and the L2 stream (every workgroup reads the 3 C^2 elements of R each step);
  * one optimizer step (train_step) of SASREC and S2PNM at the published flags (runme.sh:39-55: 512 units, 8 heads / 1 head,
    2 blocks / 1 block, batch 512, seqslen 30, 17 771 items) beside TGAT's and TiSASRec's from the SAME run.

  * --wide (profiles/gru_wide.txt): the pipelined stream (ops.GruSeqFn(..., wide=True), csrc/k_gru_wide.hip) beside the
    existing path at B = 512, T in {30, 100}, C in {256, 512}, f32 and bf16 — the two ALTERNATE repeat by repeat in one process,
    in the same device-event windows; forward microseconds per step against the L2 bound; whether h and the three gradients of
    the two paths are bit-identical; and one GRU4REC train_step (T = 30, 17 771 items, 1 block) beside S2PNM's.

  * --cell lstm (profiles/lstm_seq.txt): module.sequential.LSTM as a layer (input GEMM, csrc/k_lstm.hip, dR GEMM) beside
    torch.nn.LSTM at the --wide shapes, alternating repeat by repeat, forward alone and forward plus backward; the recurrence's
    forward microseconds per step against its L2 bound (4 C^2 elements per step); one GRU4REC train_step with each cell.

Warm-up, device events around `iters` calls, `reps` repeats, median and min / max printed.
    python tools/gru_bench.py [--iters 10] [--reps 5] [--json out.json] [--skip-models] [--wide] [--cell lstm]"""
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
from easydgl_amd.module.sequential import GRU, LSTM  # noqa: E402
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


def gru_op(T, C, dt, dev, wide=False):
    g = GRU(C, C, gen=torch.Generator().manual_seed(0)).to(dev)
    R, bR, Rc = g.r_kernel.detach().requires_grad_(True), g.r_bias.detach().requires_grad_(True), g.r_kernel.detach().to(dt)
    gen = torch.Generator(device=dev).manual_seed(1)
    xp = torch.randn((B, T, 3 * C), device=dev, generator=gen).to(dt).requires_grad_(True)
    d_h = torch.randn((B, T, C), device=dev, generator=gen).to(dt)

    def both(keep=False):
        h = ops.GruSeqFn.apply(xp, R, bR, Rc, wide)
        h.backward(d_h)
        out = (h.detach(), xp.grad, R.grad, bR.grad) if keep else None
        xp.grad = R.grad = bR.grad = None
        return out

    def fwd():
        with torch.no_grad():
            ops.GruSeqFn.apply(xp, R, bR, Rc, wide)
    return both, fwd


def spread_pair(fa, fb, iters, reps):
    """Two callables timed alternately, repeat by repeat, in the same device-event windows."""
    for _ in range(3):
        fa()
        fb()
    torch.cuda.synchronize()
    va, vb = [], []
    for _ in range(reps):
        va.append(timed(fa, iters))
        vb.append(timed(fb, iters))
    return tuple(dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for v in (va, vb))


def wide_rows(a, dev, out):
    fmt = lambda r: f"{r['median_ms']:8.3f} ms ({r['min_ms']:.3f} - {r['max_ms']:.3f})"
    for T in (30, 100):
        for C in (256, 512):
            for dt, nm in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
                old_both, old_fwd = gru_op(T, C, dt, dev)
                new_both, new_fwd = gru_op(T, C, dt, dev, wide=True)
                same = all(torch.equal(x, y) for x, y in zip(old_both(keep=True), new_both(keep=True)))
                ob, nb = spread_pair(old_both, new_both, a.iters, a.reps)
                of, nf = spread_pair(old_fwd, new_fwd, a.iters, a.reps)
                bounds = lower_bounds(C, 4 if nm == "f32" else 2)
                row = dict(T=T, C=C, dtype=nm, bounds=bounds, bit_identical=same, fwd_bwd=ob, fwd=of, wide_fwd_bwd=nb, wide_fwd=nf)
                out["wide"].append(row)
                print(f"GRU B={B} T={T:3d} C={C:3d} {nm:4s}: fwd+bwd existing {fmt(ob)} wide {fmt(nb)}; fwd existing {fmt(of)} wide {fmt(nf)}; "
                      f"fwd per step existing {of['median_ms'] / T * 1e3:6.2f} us wide {nf['median_ms'] / T * 1e3:6.2f} us >= "
                      f"{bounds['mfma_us']:.2f} us MFMA / {bounds['l2_us']:.2f} us L2; h, d_xp, dR, db_R bit-identical: {'yes' if same else 'NO'}",
                      flush=True)
    for name, heads, blocks in (("GRU4REC", 1, 1), ("S2PNM", 1, 1)):
        r = spread(model_step(name, heads, blocks, dev), a.iters, a.reps)
        out["models"][name] = r
        print(f"{name:9s} train_step B={B} T=30 C=512 H={heads} blocks={blocks} bf16: {fmt(r)}", flush=True)


def lstm_layer(T, C, dt, dev):
    """module.sequential.LSTM as a layer, x -> h (the input GEMM, csrc/k_lstm.hip, the dR GEMM), and the recurrence alone."""
    m = LSTM(C, C, gen=torch.Generator().manual_seed(0)).to(dev)
    m.compute = lambda p: p.detach().to(dt)
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((B, T, C), device=dev, generator=gen).to(dt).requires_grad_(True)
    xp = torch.randn((B, T, 4 * C), device=dev, generator=gen).to(dt)
    d_h = torch.randn((B, T, C), device=dev, generator=gen).to(dt)
    Rc = m.r_kernel.detach().to(dt)

    def both():
        m(x).backward(d_h)
        x.grad = None
        m.zero_grad(set_to_none=True)

    def fwd():
        with torch.no_grad():
            m(x)

    def rec():
        with torch.no_grad():
            ops.LstmSeqFn.apply(xp, m.r_kernel, m.r_bias, Rc)
    return both, fwd, rec


def vendor_lstm(T, C, dt, dev):
    g = torch.nn.LSTM(C, C, batch_first=True).to(dev).to(dt)
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((B, T, C), device=dev, generator=gen).to(dt).requires_grad_(True)
    d_h = torch.randn((B, T, C), device=dev, generator=gen).to(dt)

    def both():
        g(x)[0].backward(d_h)
        x.grad = None
        g.zero_grad(set_to_none=True)

    def fwd():
        with torch.no_grad():
            g(x)
    return both, fwd


def lstm_rows(a, dev, out):
    """--cell lstm (profiles/lstm_seq.txt): the LSTM layer beside torch.nn.LSTM, alternating repeat by repeat."""
    fmt = lambda r: f"{r['median_ms']:8.3f} ms ({r['min_ms']:.3f} - {r['max_ms']:.3f})"
    for T in (30, 100):
        for C in (256, 512):
            for dt, nm in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
                both, fwd, rec = lstm_layer(T, C, dt, dev)
                l2_us = 4.0 * C * C * (4 if nm == "f32" else 2) / L2_BYTES_PER_CLK_CU / CLOCK_HZ * 1e6
                row = dict(T=T, C=C, dtype=nm, l2_us=l2_us, vendor_error=None)
                try:
                    vboth, vfwd = vendor_lstm(T, C, dt, dev)
                    row["fwd_bwd"], row["vendor_fwd_bwd"] = spread_pair(both, vboth, a.iters, a.reps)
                    row["fwd"], row["vendor_fwd"] = spread_pair(fwd, vfwd, a.iters, a.reps)
                except Exception as e:       # (the vendor RNN does not run at this dtype / on this box: said, not hidden)
                    row["vendor_error"] = f"{type(e).__name__}: {str(e)[:200]}"
                    row["fwd_bwd"], row["fwd"] = spread(both, a.iters, a.reps), spread(fwd, a.iters, a.reps)
                row["rec_fwd"] = spread(rec, a.iters, a.reps)
                out["lstm"].append(row)
                v = (f"torch.nn.LSTM fwd+bwd {fmt(row['vendor_fwd_bwd'])} fwd {fmt(row['vendor_fwd'])}" if row["vendor_error"] is None
                     else f"torch.nn.LSTM did not run: {row['vendor_error']}")
                print(f"LSTM B={B} T={T:3d} C={C:3d} {nm:4s}: layer fwd+bwd {fmt(row['fwd_bwd'])} fwd {fmt(row['fwd'])}; {v}; recurrence fwd per "
                      f"step {row['rec_fwd']['median_ms'] / T * 1e3:6.2f} us >= {l2_us:.2f} us L2", flush=True)
    for cell in ("gru", "lstm"):
        r = spread(model_step("GRU4REC", 1, 1, dev, rnn_cell=cell), a.iters, a.reps)
        out["models"]["GRU4REC " + cell] = r
        print(f"GRU4REC --rnn_cell {cell:4s} train_step B={B} T=30 C=512 blocks=1 bf16: {fmt(r)}", flush=True)


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


def model_step(name, heads, blocks, dev, **extra):
    I, T, C = 17771, 30, 512
    drop = 0.2 if name == "S2PNM" else (0.0 if name == "SASREC" else 0.1)
    F = SimpleNamespace(model=name, num_items=I, num_units=C, num_heads=heads, num_blocks=blocks, seqslen=T, timelen=256,
                        time_scale=86400.0, learning_rate=1e-4, l2_reg=1e-4, hidden_dropout_rate=drop,
                        attention_probs_dropout_rate=drop, compute_dtype="bf16", num_train_steps=None, num_warmup_steps=None, seed=9876, **extra)
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
    ap.add_argument("--wide", action="store_true", help="the pipelined stream beside the existing path (DESIGN 4.23), and nothing else")
    ap.add_argument("--cell", choices=["gru", "lstm"], default="gru",
                    help="lstm: the LSTM layer (DESIGN 4.25) beside torch.nn.LSTM and GRU4REC's train_step with each cell, and nothing else")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    out = {"batch": B, "iters": a.iters, "reps": a.reps, "gru": [], "wide": [], "lstm": [], "models": {}}
    if a.wide or a.cell == "lstm":
        (lstm_rows if a.cell == "lstm" else wide_rows)(a, dev, out)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
        return
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
