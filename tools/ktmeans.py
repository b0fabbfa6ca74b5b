"""Means over the last steps of a traced bench run in a rocprofv3 rocpd database (tools/ktimeline.py prints ONE step, the last, whose
gaps are not typical: DESIGN rule 80): per launch of the step (by position) its mean duration and the mean / median / maximum gap in
front of it; the span from the first strip kernel's start to tail2_bwd's start; span and busy time of the step.
python tools/ktmeans.py DIR/NAME_results.db [name of the first kernel of a step, default encode_prep]"""
import sqlite3
import statistics as st
import sys


def main():
    db = sqlite3.connect(sys.argv[1])
    first = sys.argv[2] if len(sys.argv) > 2 else "encode_prep"
    rows = db.execute('select name, start, "end" from kernels order by start').fetchall()
    starts = [i for i, r in enumerate(rows) if first in r[0]]
    if len(starts) < 3:
        print("no step boundary found")
        return
    steps = [(rows[a:b], rows[b][1]) for a, b in zip(starts[:-1], starts[1:])][-20:]     # (launches, start of the next step)
    n = st.mode(len(s) for s, _ in steps)
    steps = [(s, nxt) for s, nxt in steps if len(s) == n]
    print(f"# means over {len(steps)} steps of {n} launches: dur_us | gap_before_us: mean (median, max) | kernel")
    for i in range(n):
        dur = st.mean((s[i][2] - s[i][1]) / 1e3 for s, _ in steps)
        # against the latest end among ALL earlier launches of the step (side-stream launches overlap)
        gs = [(s[i][1] - max(x[2] for x in s[:i])) / 1e3 if i else 0.0 for s, _ in steps]
        print(f"{dur:8.2f} | {st.mean(gs):7.2f} (median {st.median(gs):6.2f} max {max(gs):6.2f}) | {steps[0][0][i][0][:70]}")

    def at(s, key):
        return next(r for r in s if key in r[0])
    try:
        span = [(at(s, "tail2_bwd")[1] - at(s, "strip_kernel")[1]) / 1e3 for s, _ in steps]
        print(f"# strip span (first strip start -> tail2_bwd start): mean {st.mean(span):.2f} median {st.median(span):.2f} "
              f"min {min(span):.2f} max {max(span):.2f}")
    except StopIteration:
        pass
    tot = [(nxt - s[0][1]) / 1e3 for s, nxt in steps]
    busy = [sum(r[2] - r[1] for r in s) / 1e3 for s, _ in steps]
    print(f"# step span (start -> next step's start): mean {st.mean(tot):.2f} median {st.median(tot):.2f}; busy mean {st.mean(busy):.2f}")


if __name__ == "__main__":
    main()
