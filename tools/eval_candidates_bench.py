"""Evaluation on candidate lists against the full-catalogue rank sweep, in ONE process, alternating:

    python tools/eval_candidates_bench.py [--rounds 5] [--steps 20] [--out profiles/eval_candidates.txt]

Per shape (sequences x items x channels, N candidates; bf16): the scoring op alone — ops.score_candidates (count only) against
ops.score_label_rank on the same rows, table, seen ids and labels — with the gather's R (N + 1) C 2 bytes over its time, and
EasyDGL.eval_step both ways (sampled negatives against by_rank).  Each round times `steps` calls of one form, then of the other,
between device events after a warm-up of both; the table gives the median and the spread (min .. max) over the rounds.  The lists are
drawn by ops.sample_negatives once, outside the timed region of the op rows (eval_step draws its own inside).  Needs a GPU: there
is no fallback."""
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

# (sequences, items, channels, candidates): headline, config 3 at the published protocol's N and at a long list, re-ranking
SHAPES = [(512, 20000, 128, 100), (512, 1000000, 256, 100), (512, 1000000, 256, 1000), (8, 1000000, 256, 4096)]


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def ab(f_base, f_new, rounds, steps, before=None):
    for _ in range(3):
        f_base(); f_new()
    torch.cuda.synchronize()
    tb, tn = [], []
    for r in range(rounds):
        for which in ((0, 1) if r % 2 == 0 else (1, 0)):       # alternating order
            if before is not None:
                before()
                torch.cuda.synchronize()
            (tb if which == 0 else tn).append(timed(f_base if which == 0 else f_new, steps))
    return tb, tn


def fmt(ts):
    return f"{statistics.median(ts):8.4f} ({min(ts):.4f} .. {max(ts):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "eval_candidates.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_candidates_bench.py: needs a GPU")
    lines = [f"evaluation on candidate lists vs the full rank sweep: ms per call, median (min .. max) of {args.rounds} rounds x "
             f"{args.steps} calls, alternating order, one process; bf16, mask_seen", ""]
    model = None
    for B, num_items, C, N in SHAPES:
        L = 100 if C == 128 else 200
        if model is None or model.num_items != num_items + 1 or model.num_units != C:
            del model
            torch.cuda.empty_cache()
            F = SimpleNamespace(model="EasyDGL", num_items=num_items, num_units=C, num_heads=8, num_blocks=1, seqslen=L,
                                masklen=L // 5, time_scale=86400.0, learning_rate=5e-4, l2_reg=1e-4, ct_reg=1e-7,
                                hidden_dropout_rate=0.1, attention_probs_dropout_rate=0.1,
                                mark_table=D.synthetic_mark_table(num_items, 16), compute_dtype="bf16", num_train_steps=None,
                                num_warmup_steps=None, seed=9876)
            model = easydgl_amd.ranking(F).finalize("cuda")
        ids, ts = D.synthetic_batch(num_items, L, B, seed=9876)
        feats, labels = D.device_mask_last(torch.tensor(ids, device="cuda"), torch.tensor(ts, device="cuda"), model.mask)
        with torch.no_grad():
            rows = model._last_rows(feats)
        tab, bias, seen, lab = model.compute(model.item_embs.lookup_table), model.output_bias, feats["seqs_i"], labels[:, -1].contiguous()
        I, T = tab.shape[0], seen.shape[1]
        cand = ops.sample_negatives(seen, lab, N, 1, model.mask, 9876)
        # the two forms agree where they must: the list's count can only be <= the catalogue's
        full = ops.score_label_rank(rows, tab, bias, seen, lab)
        part = ops.score_candidates(rows, tab, bias, cand, seen, lab, want_scores=False)[2]
        ok = bool((part <= full).all())
        o_full, o_cand = ab(lambda: ops.score_label_rank(rows, tab, bias, seen, lab),
                            lambda: ops.score_candidates(rows, tab, bias, cand, seen, lab, want_scores=False), args.rounds, args.steps)
        o_sc = [timed(lambda: ops.score_candidates(rows, tab, bias, cand, seen), args.steps) for _ in range(args.rounds)]
        e_full, e_cand = ab(lambda: model.eval_step(feats, labels, by_rank=True), lambda: model.eval_step(feats, labels, negatives=N),
                            args.rounds, args.steps, before=model.reset_metrics)
        gb = B * (N + 1) * C * 2 / 1e9
        med = statistics.median(o_cand)
        chunk = easydgl_amd._lib.lib.edgl_score_candidates_chunk(B, C, N, 1)
        lines += [f"{B} x {I} x {C}, N = {N}  (T = {T}; {chunk} slots per workgroup; gathered rows of {2 * C} B, {gb * 1e3:.2f} MB; "
                  f"count <= full count: {ok})",
                  f"  scoring op  full sweep {fmt(o_full)}   candidates (count) {fmt(o_cand)}   ratio {med / statistics.median(o_full):.4f}"
                  f"   gather {gb / (med * 1e-3) / 1e3:.3f} TB/s",
                  f"              candidates (scores only, re-ranking) {fmt(o_sc)}",
                  f"  eval_step   by rank    {fmt(e_full)}   sampled negatives  {fmt(e_cand)}   ratio "
                  f"{statistics.median(e_cand) / statistics.median(e_full):.4f}",
                  ""]
        print("\n".join(lines[-5:]), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
