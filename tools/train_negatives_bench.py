"""Sampled-softmax training against the full-catalogue softmax, in ONE process:

    python tools/train_negatives_bench.py [--rounds 5] [--steps 20] [--models EasyDGL,TiSASREC] [--sections full,lazy,shared]
                                          [--out profiles/train_negatives.txt] [--parent TREE]

Per shape (sequences x positions x channels x items; bf16) and model: `model.train_step` with train_negatives N in {0, 100, 1000} —
N = 0 is the full softmax (ops.ScoreCEFn), the path every step took before sampled training existed — and the loss op alone,
forward + backward on the model's scored rows: ops.ScoreCEFn against ops.SampledCEFn (atomic and ordered table gradient), with
the atomic bytes R_w (N + 1) C 4 of the table gradient (R_w weighted rows) over the chip-wide rate of 1.3 TB/s beside it.  Each
round times `steps` calls between device events after a warm-up; the table gives the median and the spread (min .. max) over the
rounds.
Section `lazy` (EasyDGL): `train_step` with N in {10, 100} sampled negatives, the dense sampled step against
FLAGS.lazy_adam, with the distinct rows the step touches and the byte model beside them: touched rows x 8.5 C 4 bytes (w, g, m, v read;
w, m, v, zeros and the bf16 shadow written) against the dense path's 14.5 I C 4 (two zero fills, their sum, the copy into the arena
and the dense Adam; the l2 term's dense gradient, which the lazy mode also drops, is not counted).  `--sections lazy` keeps the
part of --out in front of the section's heading and replaces the rest.
Section `shared`: `train_step` with ONE list of S in {128, 1024, 8192} negatives per step (FLAGS.shared_negatives)
beside two baselines timed in the same session — the per-row step at N = 100 and the full softmax (N = 0), both from the tree
`--parent TREE` names (a checkout of the parent commit with its library built; a fresh child process of this tool with `--tree
TREE --sections baseline`), or from this tree when no parent is given — then, EasyDGL, shared + lazy_adam against the parent's lazy
step at N = 100, and the loss op alone (ops.SharedCEFn forward + backward, atomic and deterministic) beside its byte model: (R_w + S) C 4
bytes of f32 atomics plus the [R, S] traffic (f32 values written and read, dv in bf16 written and read twice).  `--sections shared`
replaces the part of --out from the section's heading on and keeps the rest.
Sections `popularity` and `metrics` (`--sections popularity,metrics`, which keeps what stands in front of them):
per shape the per-row step at N = 100 and the shared step at S = 1024 — the parent's (`--parent TREE`), this tree's with the flags
unset and this tree's with FLAGS.neg_sampler = popularity (counts = bincount of the batch's Zipf ids) — then the uniform against
the alias draw and the loss forward without / with the gathered logq; `metrics`: H10 / N10 on the synthetic Zipf task of
tests/metric_parity.py after `--metric_steps` equal steps under uniform negatives, popularity with log-Q and popularity without.
Section `losses` (`--sections losses`, which keeps what stands in front of it): per shape of the shared section and
model, `train_step` under FLAGS.sampled_loss = softmax / bce / bpr at N = 100 per row and at S = 1024 shared, the loss op alone
(forward + backward on the model's scored rows), and H10 / N10 of the three objectives on the synthetic Zipf task after
`--metric_steps` equal steps.  Nothing is gated on these numbers.
Needs a GPU: there is no fallback."""
import argparse
import os
import statistics
import sys
from types import SimpleNamespace

# --tree TREE: the package of another checkout (the parent commit's, with its own library) instead of this file's
_TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(_TREE))
import torch  # noqa: E402

import easydgl_amd  # noqa: E402
from easydgl_amd import data as D  # noqa: E402
from easydgl_amd import ops  # noqa: E402

# (sequences, positions, channels, items): the headline and a config-3-shaped case (BASELINE.json configs[2])
SHAPES = [(512, 100, 128, 20000), (512, 200, 256, 1000000)]
NEGATIVES = (0, 100, 1000)
LAZY_NEGATIVES = (10, 100)
LAZY_HEADING = "lazy row-wise Adam for the item table (DESIGN 4.14)"
SHARED_SIZES = (128, 1024, 8192)
SHARED_HEADING = "one negative list per step, shared by every row (DESIGN 4.15)"
POP_HEADING = "popularity-weighted negatives with the log-Q correction (DESIGN 4.16)"
METRIC_HEADING = "ranking metrics under the three samplers (DESIGN 4.16)"
POP_N, POP_S = 100, 1024
LOSS_HEADING = "objectives over the sampled negatives: softmax, bce, bpr (DESIGN 4.19)"
LOSS_FORMS = ("softmax", "bce", "bpr")
HBM_RATE = 5.0e12         # bytes per second of streamed reads / writes (a round figure for the [R, S] traffic's floor)
ATOMIC_RATE = 1.3e12      # bytes of f32 atomic adds per second, chip-wide


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def rounds_of(fn, rounds, steps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    return [timed(fn, steps) for _ in range(rounds)]


def fmt(ts):
    return f"{statistics.median(ts):9.4f} ({min(ts):.4f} .. {max(ts):.4f})"


def build(name, B, L, C, num_items, negatives=0, lazy=False, shared=0):
    F = SimpleNamespace(train_negatives=negatives, lazy_adam=lazy, shared_negatives=shared,
                        model=name, num_items=num_items, num_units=C, num_heads=8, num_blocks=1, seqslen=L, masklen=L // 5,
                        timelen=256, time_scale=86400.0, learning_rate=5e-4, l2_reg=1e-4, ct_reg=1e-7, hidden_dropout_rate=0.1,
                        attention_probs_dropout_rate=0.1, compute_dtype="bf16", num_train_steps=None, num_warmup_steps=None, seed=9876)
    if name == "EasyDGL":
        F.mark_table = D.synthetic_mark_table(num_items, 16)
    model = easydgl_amd.ranking(F).finalize("cuda")
    ids, ts = D.synthetic_batch(num_items, L, B, seed=9876)
    tok, tim = torch.tensor(ids, device="cuda"), torch.tensor(ts, device="cuda")
    if name == "EasyDGL":
        state = torch.tensor([9876, 0], dtype=torch.int64, device="cuda")
        feats, labels = D.device_mask_random(tok, tim, model.mask, L // 5, state)
    else:
        feats, labels = {"seqs_i": tok[:, :-1].contiguous(), "seqs_t": tim}, tok[:, 1:].contiguous()
    return model, feats, labels


def scored_rows(name, model, feats):
    with torch.no_grad():
        out = model.encoder(feats, False, model._gather_pos(feats, True) if name == "EasyDGL" else None)
    rows = out[0] if isinstance(out, tuple) else out
    return rows.reshape(-1, model.num_units).contiguous()


def op_call(model, rows, labels, cand, det):
    tab = model.item_embs.lookup_table
    r = rows.detach().requires_grad_(True)
    if cand is None:
        loss = ops.ScoreCEFn.apply(r, tab, model.output_bias, model.compute(tab), labels, det)
    else:
        loss = ops.SampledCEFn.apply(r, tab, model.output_bias, model.compute(tab), labels, cand, det)
    torch.autograd.grad(loss, (r, tab, model.output_bias))


def touched_rows(model, feats, labels, N):
    """Distinct item-table rows one sampled step names: input ids, labels of weighted rows and their lists (the step's own draw)."""
    I = model.item_embs.lookup_table.shape[0]
    lab = labels.reshape(-1).contiguous()
    cand = ops.sample_negatives(None, lab, N, 1, model._negatives_hi(), model.train_neg_seed, model.neg_step, 0)
    hit = torch.zeros(I, device=lab.device, dtype=torch.bool)
    live = (lab >= 1) & (lab < I)
    for ids in (feats["seqs_i"].reshape(-1), lab[live], cand[live].reshape(-1).long()):
        hit[ids[(ids >= 1) & (ids < I)]] = True
    return int(hit.sum())


def lazy_section(args, lines):
    lines += [f"{LAZY_HEADING}: ms per `train_step`, median (min .. max) of {args.rounds} rounds x {args.steps} calls; bf16, "
              f"dropout 0.1 / 0.1, l2 1e-4; dense = the sampled step with the flag unset", ""]
    for B, L, C, num_items in SHAPES:
        res = {}
        for lazy in (False, True):
            model, feats, labels = build("EasyDGL", B, L, C, num_items, LAZY_NEGATIVES[0], lazy)
            I = model.item_embs.lookup_table.shape[0]
            for N in LAZY_NEGATIVES:
                model.train_negatives = N
                res[(lazy, N)] = (rounds_of(lambda: model.train_step(feats, labels), args.rounds, args.steps),
                                  touched_rows(model, feats, labels, N), int((labels != 0).sum()), I)
            model = feats = labels = None
            torch.cuda.empty_cache()
        I = res[(True, LAZY_NEGATIVES[0])][3]
        lines.append(f"EasyDGL  {B} x {L} x {C}, {I} table rows, {res[(True, LAZY_NEGATIVES[0])][2]} weighted rows; dense path "
                     f"{14.5 * I * C * 4 / 1e6:9.1f} MB per step")
        for N in LAZY_NEGATIVES:
            d, z = res[(False, N)], res[(True, N)]
            md, mz = statistics.median(d[0]), statistics.median(z[0])
            lines.append(f"  N = {N:5d}  dense {fmt(d[0])}  lazy {fmt(z[0])}  x{mz / md:6.3f} of dense   distinct rows {z[1]:8d} "
                         f"({z[1] / I:5.3f} of the table)   lazy bytes {z[1] * 8.5 * C * 4 / 1e6:9.1f} MB")
            print(lines[-1], flush=True)
        lines.append("")


def baseline_section(args):
    """The per-row step at N = 100, the full softmax and (EasyDGL) the lazy per-row step of THIS process's tree, one `BASE` line
    each on stdout: what the `shared` section of another tree's run reads."""
    for name in args.models.split(","):
        for B, L, C, num_items in SHAPES:
            modes = ((0, False), (100, False)) + (((100, True),) if name == "EasyDGL" else ())
            for N, lazy in ((POP_N, False),) if args.for_popularity else modes:
                model, feats, labels = build(name, B, L, C, num_items, N, lazy)
                ts = rounds_of(lambda: model.train_step(feats, labels), args.rounds, args.steps)
                print("BASE", name, B, L, C, num_items, N, int(lazy), *(f"{t:.6f}" for t in ts), flush=True)
                model = feats = labels = None
                torch.cuda.empty_cache()
            if args.for_popularity:      # (the shared step at S = POP_S, keyed as N = S with the mode field 2)
                model, feats, labels = build(name, B, L, C, num_items, 0, False, POP_S)
                ts = rounds_of(lambda: model.train_step(feats, labels), args.rounds, args.steps)
                print("BASE", name, B, L, C, num_items, POP_S, 2, *(f"{t:.6f}" for t in ts), flush=True)
                model = feats = labels = None
                torch.cuda.empty_cache()


def parent_baselines(args, for_popularity=False):
    """{(model, B, L, C, items, N, lazy): [ms per round]} of the tree args.parent names, measured by a fresh child process."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--tree", args.parent, "--sections", "baseline", "--rounds", str(args.rounds),
           "--steps", str(args.steps), "--models", args.models] + (["--for_popularity"] if for_popularity else [])
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
    res = {}
    for ln in out.split("\n"):
        w = ln.split()
        if w and w[0] == "BASE":
            res[(w[1],) + tuple(int(x) for x in w[2:8])] = [float(x) for x in w[8:]]
    return res


def shared_op_call(model, rows, labels, shared, det):
    tab = model.item_embs.lookup_table
    r = rows.detach().requires_grad_(True)
    loss = ops.SharedCEFn.apply(r, tab, model.output_bias, model.compute(tab), labels, shared, det)
    torch.autograd.grad(loss, (r, tab, model.output_bias))


def shared_section(args, lines):
    src = "a checkout of the parent commit built from its own sources" if args.parent else "this tree with the flag unset (no --parent given)"
    lines += [f"{SHARED_HEADING}: ms per call, median (min .. max) of {args.rounds} rounds x {args.steps} calls; bf16, dropout 0.1 / "
              f"0.1; baselines (per-row N = 100, full softmax N = 0) from {src}, timed in the same session", ""]
    if args.parent:
        base = parent_baselines(args)
    for name in args.models.split(","):
        for B, L, C, num_items in SHAPES:
            if not args.parent:
                base = {}
                for N, lazy in ((0, False), (100, False)) + (((100, True),) if name == "EasyDGL" else ()):
                    model, feats, labels = build(name, B, L, C, num_items, N, lazy)
                    base[(name, B, L, C, num_items, N, int(lazy))] = rounds_of(lambda: model.train_step(feats, labels), args.rounds,
                                                                               args.steps)
                    model = feats = labels = None
                    torch.cuda.empty_cache()
            b0, b100 = base[(name, B, L, C, num_items, 0, 0)], base[(name, B, L, C, num_items, 100, 0)]
            model, feats, labels = build(name, B, L, C, num_items, 0, False, SHARED_SIZES[0])
            lab = labels.reshape(-1).contiguous()
            rows = scored_rows(name, model, feats)
            R, Rw, I = rows.shape[0], int((lab != 0).sum()), model.item_embs.lookup_table.shape[0]
            lines.append(f"{name}  {B} x {L} x {C}, {I} table rows: {R} scored rows, {Rw} weighted")
            lines.append(f"  parent   N = 0   train_step {fmt(b0)}      N = 100   train_step {fmt(b100)}   spread of N = 100 "
                         f"{max(b100) - min(b100):.4f}")
            m100 = statistics.median(b100)
            for S in SHARED_SIZES:
                model.shared_negatives = S
                step = rounds_of(lambda: model.train_step(feats, labels), args.rounds, args.steps)
                sh = model.draw_shared_negatives(lab.device)
                op = rounds_of(lambda: shared_op_call(model, rows, lab, sh, False), args.rounds, args.steps)
                det = rounds_of(lambda: shared_op_call(model, rows, lab, sh, True), args.rounds, args.steps)
                med = statistics.median(step)
                ab, tb = (Rw + S) * C * 4, Rw * S * (4 + 4 + 2 + 2 + 2)
                lines.append(f"  S = {S:5d}  train_step {fmt(step)}  x{med / m100:6.3f} of N = 100 (saves {m100 - med:+.4f} ms)  x"
                             f"{med / statistics.median(b0):6.3f} of N = 0   loss op fwd + bwd {fmt(op)}   deterministic {fmt(det)}   "
                             f"atomic bytes {ab / 1e6:7.1f} MB = {ab / ATOMIC_RATE * 1e3:6.3f} ms, [R, S] traffic {tb / 1e6:8.1f} MB = "
                             f"{tb / HBM_RATE * 1e3:6.3f} ms at 5 TB/s")
                print(lines[-1], flush=True)
            model = feats = labels = rows = None
            torch.cuda.empty_cache()
            if name == "EasyDGL":
                bl = base[(name, B, L, C, num_items, 100, 1)]
                lines.append(f"  parent   N = 100 + lazy_adam   train_step {fmt(bl)}")
                for S in SHARED_SIZES:
                    model, feats, labels = build(name, B, L, C, num_items, 0, True, S)
                    step = rounds_of(lambda: model.train_step(feats, labels), args.rounds, args.steps)
                    lines.append(f"  S = {S:5d} + lazy_adam   train_step {fmt(step)}  x{statistics.median(step) / statistics.median(bl):6.3f} "
                                 f"of the parent's lazy step")
                    print(lines[-1], flush=True)
                    model = feats = labels = None
                    torch.cuda.empty_cache()
            lines.append("")


def set_popularity(model, feats):
    """FLAGS.neg_sampler = popularity on a built model, the counts from the batch's own (Zipf) item ids."""
    hi = model._negatives_hi()
    ids = feats["seqs_i"].reshape(-1)
    counts = torch.bincount(ids[(ids >= 0) & (ids < hi)], minlength=hi).cpu().numpy()
    model.neg_sampler = "popularity"
    model.set_negative_weights(ops.neg_weights("popularity", hi, 1, hi, counts, model.neg_alpha))


def popularity_section(args, lines):
    """per shape the per-row step at N = 100 and the shared step at S = 1024 — the parent's, this tree's with the flags
    unset (the same launches) and this tree's with the popularity sampler; then the draw and the loss forward alone."""
    src = "a checkout of the parent commit built from its own sources" if args.parent else "not measured (no --parent given)"
    lines += [f"{POP_HEADING}: ms per call, median (min .. max) of {args.rounds} rounds x {args.steps} calls; bf16, dropout 0.1 / "
              f"0.1; N = {POP_N} per row, S = {POP_S} shared; counts = bincount of the batch's item ids, alpha 0.75; parent: {src}", ""]
    base = parent_baselines(args, True) if args.parent else {}
    for name in args.models.split(","):
        for B, L, C, num_items in SHAPES:
            lines.append(f"{name}  {B} x {L} x {C}, {num_items} items")
            for tag, N, S, key in ((f"N = {POP_N}", POP_N, 0, (POP_N, 0)), (f"S = {POP_S}", 0, POP_S, (POP_S, 2))):
                model, feats, labels = build(name, B, L, C, num_items, N, False, S)
                uni = rounds_of(lambda: model.train_step(feats, labels), args.rounds, args.steps)
                set_popularity(model, feats)
                pop = rounds_of(lambda: model.train_step(feats, labels), args.rounds, args.steps)
                par = base.get((name, B, L, C, num_items) + key)
                line = f"  {tag:9s} "
                if par:
                    mp, sp = statistics.median(par), max(par) - min(par)
                    line += (f"parent {fmt(par)}  flags unset {fmt(uni)}  {statistics.median(uni) - mp:+.4f} ms of the parent's median "
                             f"(its spread {sp:.4f}: {'within' if abs(statistics.median(uni) - mp) <= sp else 'OUTSIDE'})  ")
                else:
                    line += f"flags unset {fmt(uni)}  "
                line += f"popularity {fmt(pop)}  {statistics.median(pop) - statistics.median(uni):+.4f} ms on the flags-unset step"
                lines.append(line)
                print(line, flush=True)
                # the two additions alone: the draw, and the forward with the gathered logq
                lab = labels.reshape(-1).contiguous()
                rows = scored_rows(name, model, feats)
                dist, hi = model._negative_dist(), model._negatives_hi()
                tab = model.compute(model.item_embs.lookup_table)
                logq = dist.logq_on(lab.device)
                if N:
                    du = rounds_of(lambda: ops.sample_negatives(None, lab, N, 1, hi, 0), args.rounds, args.steps)
                    dw = rounds_of(lambda: ops.sample_negatives(None, lab, N, 1, hi, 0, dist=dist), args.rounds, args.steps)
                    cand = ops.sample_negatives(None, lab, N, 1, hi, 0, dist=dist)
                    fu = rounds_of(lambda: ops.cand_ce_fwd(rows, tab, model.output_bias, cand, lab), args.rounds, args.steps)
                    fq = rounds_of(lambda: ops.cand_ce_fwd(rows, tab, model.output_bias, cand, lab, logq), args.rounds, args.steps)
                else:
                    one = torch.zeros(1, device=lab.device, dtype=torch.int64)
                    du = rounds_of(lambda: ops.sample_negatives(None, one, S, 1, hi, 0), args.rounds, args.steps)
                    dw = rounds_of(lambda: ops.sample_negatives(None, one, S, 1, hi, 0, dist=dist), args.rounds, args.steps)
                    sh = ops.sample_negatives(None, one, S, 1, hi, 0, dist=dist).reshape(-1)
                    fu = rounds_of(lambda: ops.shared_ce_fwd(rows, tab, model.output_bias, sh, lab), args.rounds, args.steps)
                    fq = rounds_of(lambda: ops.shared_ce_fwd(rows, tab, model.output_bias, sh, lab, logq), args.rounds, args.steps)
                line = (f"            draw: uniform {fmt(du)}  alias table ({(hi - 1) * 8 / 1e6:.1f} MB) {fmt(dw)}    loss forward on the "
                        f"weighted lists: plain {fmt(fu)}  with logq ({logq.numel() * 4 / 1e6:.1f} MB) {fmt(fq)}")
                lines.append(line)
                print(line, flush=True)
                model = feats = labels = rows = tab = None
                torch.cuda.empty_cache()
            lines.append("")


def metrics_section(args, lines):
    """H10 / N10 on the synthetic Zipf task of tests/metric_parity.py (full-catalogue ranking of held-out sequences, seen items
    masked) after equal steps: uniform negatives, popularity with the log-Q correction, popularity without it."""
    import numpy as np
    from oracle import easydgl_oracle as O
    from tests import metric_parity as MP
    num_items, seqslen, batch, steps, n_eval, S = 400, 20, 128, args.metric_steps, 2048, 32
    cfg = O.Config(num_items=num_items, seqslen=seqslen, num_units=32, num_heads=2, num_blocks=1, masklen=4, time_scale=86400.0,
                   ct_reg=1e-3, l2_reg=1e-4, learning_rate=2e-3, num_events=4)
    rng = np.random.default_rng(11)
    params0 = O.init_params(cfg, rng)
    mt = O.synthetic_mark_table(cfg.num_items, cfg.num_events, multi_hot=True)
    tr_i, tr_t = MP.make_sequences(cfg, batch * steps, rng)
    ev_i, ev_t = MP.make_sequences(cfg, n_eval, rng)
    batches = [O.mask_random(cfg, tr_i[s * batch:(s + 1) * batch], tr_t[s * batch:(s + 1) * batch],
                             O.draw_masked_positions(cfg, batch, rng)) for s in range(steps)]
    efeats, elabels = O.mask_last(cfg, ev_i, ev_t)
    lines += [f"{METRIC_HEADING}: EasyDGL f32, {num_items} items, {steps} steps of {batch} sequences, shared_negatives = {S}, "
              f"full-catalogue ranking of {n_eval} held-out sequences; counts = bincount of the training ids, alpha 0.75", ""]
    for tag in ("uniform", "popularity with log-Q", "popularity without log-Q"):
        F = SimpleNamespace(model="EasyDGL", num_items=cfg.num_items, num_units=cfg.num_units, num_heads=cfg.num_heads,
                            num_blocks=cfg.num_blocks, seqslen=cfg.seqslen, masklen=cfg.masklen, time_scale=cfg.time_scale,
                            learning_rate=cfg.learning_rate, l2_reg=cfg.l2_reg, ct_reg=cfg.ct_reg, hidden_dropout_rate=0.0,
                            attention_probs_dropout_rate=0.0, mark_table=mt, compute_dtype="f32", num_train_steps=None,
                            num_warmup_steps=None, shared_negatives=S, train_neg_seed=1,
                            neg_sampler="uniform" if tag == "uniform" else "popularity")
        m = easydgl_amd.ranking(F).finalize("cuda")
        m.load_tf_variables(params0)
        if tag != "uniform":
            hi = m._negatives_hi()
            m.set_negative_weights(ops.neg_weights("popularity", hi, 1, hi, np.bincount(tr_i.reshape(-1), minlength=hi), 0.75))
            if tag.endswith("without log-Q"):
                m._negative_dist().logq[:] = 0.0         # (before the first draw: the device copy is made from this array)
        for feats, labels in batches:
            f = {k: torch.as_tensor(np.asarray(v)).cuda().contiguous() for k, v in feats.items()}
            loss = m.train_step(f, torch.as_tensor(labels).cuda())
        m.reset_metrics()
        for lo in range(0, n_eval, 256):
            ef = {k: torch.as_tensor(np.asarray(v[lo:lo + 256])).cuda().contiguous() for k, v in efeats.items()}
            m.eval_step(ef, torch.as_tensor(elabels[lo:lo + 256]).cuda(), mask_seen=True)
        got = m.metrics()
        lines.append(f"  {tag:26s} H10 {got['H10']:.4f}  N10 {got['N10']:.4f}  H50 {got['H50']:.4f}  N50 {got['N50']:.4f}  last loss "
                     f"{float(loss):.4f}")
        print(lines[-1], flush=True)
    lines.append("")


def form_op_call(model, rows, labels, lists, form):
    tab = model.item_embs.lookup_table
    r = rows.detach().requires_grad_(True)
    fn = ops.SharedCEFn if lists.dim() == 1 else ops.SampledCEFn
    loss = fn.apply(r, tab, model.output_bias, model.compute(tab), labels, lists, False, None, None, form)
    torch.autograd.grad(loss, (r, tab, model.output_bias))


def losses_section(args, lines):
    """the step and the loss op under the three objectives, per-row lists at N = 100 and one shared list of S = 1024, all
    in this session of this tree; then the ranking metrics of the three objectives after equal steps."""
    import numpy as np
    from oracle import easydgl_oracle as O
    from tests import metric_parity as MP
    lines += [f"{LOSS_HEADING}: ms per call, median (min .. max) of {args.rounds} rounds x {args.steps} calls, one session of this tree; "
              f"bf16, dropout 0.1 / 0.1; N = {POP_N} per row, S = {POP_S} shared; uniform negatives, atomic table gradient", ""]
    for name in args.models.split(","):
        for B, L, C, num_items in SHAPES:
            lines.append(f"{name}  {B} x {L} x {C}, {num_items} items")
            for tag, N, S in ((f"N = {POP_N}", POP_N, 0), (f"S = {POP_S}", 0, POP_S)):
                model, feats, labels = build(name, B, L, C, num_items, N, False, S)
                lab = labels.reshape(-1).contiguous()
                rows = scored_rows(name, model, feats)
                lists = (model._sample(None, lab, N, model.train_neg_seed, 0, 0, None) if N else model.draw_shared_negatives(lab.device))
                for form in LOSS_FORMS:
                    model.sampled_loss = form
                    step = rounds_of(lambda: model.train_step(feats, labels), args.rounds, args.steps)
                    op = rounds_of(lambda: form_op_call(model, rows, lab, lists, form), args.rounds, args.steps)
                    lines.append(f"  {tag:9s} {form:8s} train_step {fmt(step)}   loss op fwd + bwd {fmt(op)}")
                    print(lines[-1], flush=True)
                model = feats = labels = rows = lists = None
                torch.cuda.empty_cache()
            lines.append("")
    num_items, seqslen, batch, steps, n_eval, S = 400, 20, 128, args.metric_steps, 2048, 32
    cfg = O.Config(num_items=num_items, seqslen=seqslen, num_units=32, num_heads=2, num_blocks=1, masklen=4, time_scale=86400.0,
                   ct_reg=1e-3, l2_reg=1e-4, learning_rate=2e-3, num_events=4)
    rng = np.random.default_rng(11)
    params0 = O.init_params(cfg, rng)
    mt = O.synthetic_mark_table(cfg.num_items, cfg.num_events, multi_hot=True)
    tr_i, tr_t = MP.make_sequences(cfg, batch * steps, rng)
    ev_i, ev_t = MP.make_sequences(cfg, n_eval, rng)
    batches = [O.mask_random(cfg, tr_i[s * batch:(s + 1) * batch], tr_t[s * batch:(s + 1) * batch],
                             O.draw_masked_positions(cfg, batch, rng)) for s in range(steps)]
    efeats, elabels = O.mask_last(cfg, ev_i, ev_t)
    lines += [f"ranking metrics of the three objectives: EasyDGL f32, {num_items} items, {steps} steps of {batch} sequences, "
              f"shared_negatives = {S}, uniform negatives, full-catalogue ranking of {n_eval} held-out sequences", ""]
    for form in LOSS_FORMS:
        F = SimpleNamespace(model="EasyDGL", num_items=cfg.num_items, num_units=cfg.num_units, num_heads=cfg.num_heads,
                            num_blocks=cfg.num_blocks, seqslen=cfg.seqslen, masklen=cfg.masklen, time_scale=cfg.time_scale,
                            learning_rate=cfg.learning_rate, l2_reg=cfg.l2_reg, ct_reg=cfg.ct_reg, hidden_dropout_rate=0.0,
                            attention_probs_dropout_rate=0.0, mark_table=mt, compute_dtype="f32", num_train_steps=None,
                            num_warmup_steps=None, shared_negatives=S, train_neg_seed=1, sampled_loss=form)
        m = easydgl_amd.ranking(F).finalize("cuda")
        m.load_tf_variables(params0)
        for feats, labels in batches:
            f = {k: torch.as_tensor(np.asarray(v)).cuda().contiguous() for k, v in feats.items()}
            loss = m.train_step(f, torch.as_tensor(labels).cuda())
        m.reset_metrics()
        for lo in range(0, n_eval, 256):
            ef = {k: torch.as_tensor(np.asarray(v[lo:lo + 256])).cuda().contiguous() for k, v in efeats.items()}
            m.eval_step(ef, torch.as_tensor(elabels[lo:lo + 256]).cuda(), mask_seen=True)
        got = m.metrics()
        lines.append(f"  {form:8s} H10 {got['H10']:.4f}  N10 {got['N10']:.4f}  H50 {got['H50']:.4f}  N50 {got['N50']:.4f}  last loss "
                     f"{float(loss):.4f}")
        print(lines[-1], flush=True)
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--metric_steps", type=int, default=300, help="section metrics: training steps of every run")
    ap.add_argument("--for_popularity", action="store_true", help="section baseline: the two steps the popularity section compares")
    ap.add_argument("--tree", default=None, help="run against the package of this checkout (read before the imports)")
    ap.add_argument("--parent", default=None, help="section shared: a checkout of the parent commit, library built, for the baselines")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--models", default="EasyDGL,TiSASREC")
    ap.add_argument("--sections", default="full,lazy")
    ap.add_argument("--out", default=os.path.join("profiles", "train_negatives.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_negatives_bench.py: needs a GPU")
    sections = args.sections.split(",")
    if sections == ["baseline"]:
        return baseline_section(args)
    if sections == ["losses"]:      # keep what stands in front of the losses section
        lines = []
        if os.path.exists(args.out):
            old = open(args.out).read().split("\n")
            lines = old[:next((i for i, ln in enumerate(old) if ln.startswith(LOSS_HEADING)), len(old))]
            while lines and not lines[-1]:
                lines.pop()
            lines.append("")
        losses_section(args, lines)
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines))
        print("wrote", args.out)
        return
    if set(sections) <= {"popularity", "metrics"}:      # keep what stands in front of the first section asked for, replace the rest
        lines = []
        if os.path.exists(args.out):
            old = open(args.out).read().split("\n")
            head = POP_HEADING if "popularity" in sections else METRIC_HEADING
            lines = old[:next((i for i, ln in enumerate(old) if ln.startswith(head)), len(old))]
            while lines and not lines[-1]:
                lines.pop()
            lines.append("")
        if "popularity" in sections:
            popularity_section(args, lines)
        if "metrics" in sections:
            metrics_section(args, lines)
        with open(args.out, "w") as f:
            f.write("\n".join(lines))
        print("wrote", args.out)
        return
    if sections == ["shared"]:      # keep what stands in front of the shared section
        lines = []
        if os.path.exists(args.out):
            old = open(args.out).read().split("\n")
            lines = old[:next((i for i, ln in enumerate(old) if ln.startswith(SHARED_HEADING)), len(old))]
            while lines and not lines[-1]:
                lines.pop()
            lines.append("")
        shared_section(args, lines)
        with open(args.out, "w") as f:
            f.write("\n".join(lines))
        print("wrote", args.out)
        return
    lines = []
    if "full" not in sections and os.path.exists(args.out):      # keep what stands in front of the lazy section
        old = open(args.out).read().split("\n")
        cut = next((i for i, ln in enumerate(old) if ln.startswith(LAZY_HEADING)), len(old))
        lines = old[:cut]
        while lines and not lines[-1]:
            lines.pop()
        lines.append("")
    if "full" in sections:
        full_section(args, lines)
    if "lazy" in sections:
        lazy_section(args, lines)
    if "shared" in sections:
        shared_section(args, lines)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


def full_section(args, lines):
    lines += [f"sampled-softmax training vs the full softmax: ms per call, median (min .. max) of {args.rounds} rounds x {args.steps} "
             f"calls, one process; bf16, dropout 0.1 / 0.1; N = 0 is the full-catalogue softmax (ops.ScoreCEFn)", ""]
    for name in args.models.split(","):
        for B, L, C, num_items in SHAPES:
            try:
                model, feats, labels = build(name, B, L, C, num_items)
                lab = labels.reshape(-1).contiguous()
                rows = scored_rows(name, model, feats)
                R, Rw, I = rows.shape[0], int((lab != 0).sum()), model.item_embs.lookup_table.shape[0]
                lines.append(f"{name}  {B} x {L} x {C}, {I} table rows: {R} scored rows, {Rw} weighted")
                base = None
                for N in NEGATIVES:
                    model.train_negatives = N
                    step = rounds_of(lambda: model.train_step(feats, labels), args.rounds, args.steps)
                    cand = ops.sample_negatives(None, lab, N, 1, model._negatives_hi(), 0) if N else None
                    op = rounds_of(lambda: op_call(model, rows, lab, cand, False), args.rounds, args.steps)
                    med = statistics.median(step)
                    base = med if base is None else base
                    line = f"  N = {N:5d}  train_step {fmt(step)}  x{med / base:6.3f} of N = 0   loss op fwd + bwd {fmt(op)}"
                    if N:
                        det = rounds_of(lambda: op_call(model, rows, lab, cand, True), args.rounds, args.steps)
                        ab = Rw * (N + 1) * C * 4
                        line += (f"   ordered {fmt(det)}   atomic bytes {ab / 1e6:9.1f} MB = {ab / ATOMIC_RATE * 1e3:7.3f} ms "
                                 f"at 1.3 TB/s")
                    lines.append(line)
                    print(lines[-1], flush=True)
                    del cand
                    torch.cuda.empty_cache()
            except (RuntimeError, easydgl_amd._lib.EdglError) as e:      # (a shape a model does not take: say so, go on)
                lines.append(f"{name}  {B} x {L} x {C}, {num_items + 1} items: not measured ({type(e).__name__}: {str(e)[:200]})")
                print(lines[-1], flush=True)
            lines.append("")
            model = feats = labels = rows = None
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
