"""Evaluation by label rank against the top-K path, in ONE process, alternating:

    python tools/eval_rank_bench.py [--rounds 5] [--steps 20] [--out profiles/eval_rank.txt]

Per shape (512 sequences): EasyDGL.eval_step with and without by_rank, and the scoring op alone (ops.score_topk against
ops.score_label_rank on the encoder's rows).  Each round times `steps` calls of one form, then of the other, between device events
after a warm-up of both; the table gives the median and the spread (min .. max) over the rounds.  The baseline is the top-K path as
it stands, run in the same process.  Both forms are checked against each other before they are timed (H sums equal).  Needs a GPU:
there is no fallback."""
import argparse
import os
import statistics
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import easydgl_amd  # noqa: E402
from easydgl_amd import data as D  # noqa: E402
from easydgl_amd import ops  # noqa: E402

SHAPES = [(20000, 128), (1000000, 256), (20000, 512)]      # (items, channels): headline, config 3, the published recipe's width


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def ab(f_base, f_new, rounds, steps):
    for _ in range(3):
        f_base(); f_new()
    torch.cuda.synchronize()
    tb, tn = [], []
    for r in range(rounds):
        for which in ((0, 1) if r % 2 == 0 else (1, 0)):       # alternating order
            (tb if which == 0 else tn).append(timed(f_base if which == 0 else f_new, steps))
    return tb, tn


def fmt(ts):
    return f"{statistics.median(ts):8.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "eval_rank.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_rank_bench.py: needs a GPU")
    lines = [f"evaluation by label rank vs the top-K path: ms per call, median (min .. max) of {args.rounds} rounds x {args.steps} calls, "
             f"alternating order, one process; 512 sequences, bf16, mask_seen", ""]
    for num_items, C in SHAPES:
        L = 100 if C == 128 else 200
        F = SimpleNamespace(model="EasyDGL", num_items=num_items, num_units=C, num_heads=8, num_blocks=1, seqslen=L, masklen=L // 5,
                            time_scale=86400.0, learning_rate=5e-4, l2_reg=1e-4, ct_reg=1e-7, hidden_dropout_rate=0.1,
                            attention_probs_dropout_rate=0.1, mark_table=D.synthetic_mark_table(num_items, 16), compute_dtype="bf16",
                            num_train_steps=None, num_warmup_steps=None, seed=9876)
        model = easydgl_amd.ranking(F).finalize("cuda")
        ids, ts = D.synthetic_batch(num_items, L, 512, seed=9876)
        feats, labels = D.device_mask_last(torch.tensor(ids, device="cuda"), torch.tensor(ts, device="cuda"), model.mask)
        # same results first
        model.reset_metrics(); model.eval_step(feats, labels); base = model.metrics()
        model.reset_metrics(); model.eval_step(feats, labels, by_rank=True); by = model.metrics()
        same = all(base[k] == by[k] for k in ("H10", "H50", "H100"))
        with torch.no_grad():
            rows, _ = model.encoder(feats, False, model._gather_pos(feats, False))
        tab, bias, seen, lab = model.compute(model.item_embs.lookup_table), model.output_bias, feats["seqs_i"], labels[:, -1].contiguous()
        I, T = tab.shape[0], seen.shape[1]
        fused = bool(easydgl_amd._lib.lib.edgl_score_rank_supported(512, C, min(I, ops.RANK_FUSED_ITEMS), T, 1))
        # (one accumulation holds one kind of step: each form is timed on its own accumulation)
        model.reset_metrics()
        t_base, t_rank = [], []
        for _ in range(3):
            model.eval_step(feats, labels)
        model.reset_metrics()
        for _ in range(3):
            model.eval_step(feats, labels, by_rank=True)
        torch.cuda.synchronize()
        for r in range(args.rounds):
            for which in ((0, 1) if r % 2 == 0 else (1, 0)):
                model.reset_metrics()
                torch.cuda.synchronize()
                if which == 0:
                    t_base.append(timed(lambda: model.eval_step(feats, labels), args.steps))
                else:
                    t_rank.append(timed(lambda: model.eval_step(feats, labels, by_rank=True), args.steps))
        o_base, o_rank = ab(lambda: ops.score_topk(rows, tab, bias, seen, 100, 0, I), lambda: ops.score_label_rank(rows, tab, bias, seen, lab),
                            args.rounds, args.steps)
        lines += [f"512 x {I} x {C}  (T = {T}; rank form: {'fused sweep' if fused else 'logits tiles'}; H sums equal: {same})",
                  f"  eval_step   top-K {fmt(t_base)}   by rank {fmt(t_rank)}   ratio {statistics.median(t_rank) / statistics.median(t_base):.3f}",
                  f"  scoring op  top-K {fmt(o_base)}   by rank {fmt(o_rank)}   ratio {statistics.median(o_rank) / statistics.median(o_base):.3f}",
                  ""]
        print("\n".join(lines[-4:]), flush=True)
        del model, rows, tab
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
