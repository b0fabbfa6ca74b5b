"""Times of the additive-attention kernel pair (csrc/k_addattn.hip) and of the NARM optimizer step beside GRU4REC's.
Device events, median (min - max) over `--reps` windows of `--iters` calls after a warm-up.  Beside each kernel time: the issue-time
floor of its transcendentals (two per (pair, channel) over the causal half; the backward recomputes them in both sweeps) at
`--trans_cycles` cycles per wave instruction and `--ghz`, and the same expression in PyTorch eager at the largest B <= the
kernel's that fits `--eager_gib` of [B,T,T,C] f32.

    python tools/addattn_bench.py --out profiles/addattn.txt"""
import argparse
import os
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return f"{statistics.median(out):9.3f} ms ({min(out):.3f} - {max(out):.3f})", statistics.median(out)


def eager(h, a12, v, ids):
    C, T = h.shape[-1], h.shape[1]
    e = (torch.sigmoid(a12[:, :, None, :C] + a12[:, None, :, C:]) * v).sum(-1)
    return (e * (torch.tril(torch.ones(T, T, dtype=torch.bool, device=h.device)) & (ids != 0)[:, None, :])) @ h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=512)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--widths", default="128,512")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trans_cycles", type=float, default=8.2, help="issue cycles of v_exp_f32 / v_rcp_f32 per wave (DESIGN 7: tools/ubench)")
    ap.add_argument("--ghz", type=float, default=2.4)
    ap.add_argument("--simds", type=int, default=1024)
    ap.add_argument("--eager_gib", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import easydgl_amd
    from easydgl_amd import ops
    B, T = a.B, a.T
    lines = [f"tools/addattn_bench.py (iters {a.iters}, reps {a.reps}: median (min - max)); B = {B}, T = {T}, bf16, no padding; floor = "
             f"2 transcendentals per (pair, channel) of the causal half at {a.trans_cycles} cycles per wave instruction, {a.simds} SIMDs, {a.ghz} GHz"]
    for C in (int(w) for w in a.widths.split(",")):
        g = torch.Generator().manual_seed(C)
        h, a12, d_out = (torch.randn(B, T, w, generator=g).bfloat16().cuda() for w in (C, 2 * C, C))
        v = (torch.randn(C, generator=g) / C ** 0.5).cuda()
        ids = torch.randint(1, 1000, (B, T), generator=g).cuda()
        hg, ag, vg = (x.clone().requires_grad_() for x in (h, a12, v))
        fwd, fwd_ms = timed(lambda: ops.AddAttnFn.apply(h, a12, v, ids), a.iters, a.reps)

        def both():
            ops.AddAttnFn.apply(hg, ag, vg, ids).backward(d_out)
            hg.grad = ag.grad = vg.grad = None
        fb, fb_ms = timed(both, a.iters, a.reps)
        floor = B * T * (T + 1) / 2 * C * 2 / 64 * a.trans_cycles / a.simds / (a.ghz * 1e6)      # ms, forward
        Be = max(1, min(B, int(a.eager_gib * 2 ** 30 / (T * T * C * 4 * 3))))
        ef, _ = timed(lambda: eager(h[:Be].float(), a12[:Be].float(), v, ids[:Be]), 2, 3)
        lines.append(f"addattn B={B} T={T} C={C:3d} bf16: fwd {fwd} (floor {floor:.3f} ms, {floor / fwd_ms:.0%}); fwd+bwd {fb} (floor "
                     f"{3 * floor:.3f} ms, {3 * floor / fb_ms:.0%}); eager f32 fwd at B={Be}: {ef}")
    for model in ("GRU4REC", "NARM"):
        F = SimpleNamespace(model=model, num_items=20000, num_units=512, num_heads=1, num_blocks=1, seqslen=T, learning_rate=1e-3,
                            l2_reg=0.0, compute_dtype="bf16", num_train_steps=None, num_warmup_steps=None)
        m = easydgl_amd.ranking(F).finalize("cuda")
        tok = torch.randint(1, 20000, (B, T + 1), generator=torch.Generator().manual_seed(1)).cuda()
        feats, labels = {"seqs_i": tok[:, :-1].contiguous()}, tok[:, 1:].contiguous()
        st, _ = timed(lambda: m.train_step(feats, labels), a.iters, a.reps)
        lines.append(f"{model:7s} train_step B={B} T={T} C=512 blocks=1 bf16 (20000 items): {st}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
