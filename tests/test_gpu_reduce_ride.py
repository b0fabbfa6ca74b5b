"""Queued partial reductions as extra blocks of the embedding backward's MFMA scatter launch (edgl_reduce_ride): the same sums
from the same kernel body as the stand-alone reduction launch, only without a launch of their own.

Op level.  Every case runs three times from identical inputs: "seq" (deferred mode: scatter call, then the flush — the sequence
without riding), "ride" (the same with edgl_reduce_ride(1); "ride2": edgl_reduce_ride(2), the reduction workgroups behind the
scatter's instead of in front of them) and, for the exact draw, "now" (nothing deferred: every reduction is
the stand-alone launch of its own).  The three reduction kernels add in different orders (8 row lanes x 4 accumulators, 32 row
lanes x 1, one thread per column), so a bitwise comparison ACROSS kernels needs sums that no order can round: the "exact" draw
takes every partial from a dyadic grid (multiples of 1/8 below 8 for the synthetic jobs, of 1/16 below 2 for the bf16 gradient
rows: at most 1616 terms, below 2^24 grid steps), the "random" draw takes normal variates and is compared between "seq" and
"ride" only, where the kernel body and therefore the order is the same.
Outputs are pre-filled with NaN and read once BEFORE the flush: what rode is already final there, what did not is still NaN."""
import numpy as np
import pytest
import torch

from tests._util import GRAD_TOL, grad_ok

pytestmark = pytest.mark.gpu

C, E, I = 128, 16, 701      # (I - 1 a multiple of 4: a vector-form output can sit right behind the bias gradient)
# (P, N, ld): one block of the column form; the column form over many blocks (the row splits of a [3C + 1, C] weight gradient);
# the row-lane form with P no multiple of 32; a deep job (one partial row per sample of a LayerNorm backward)
JOBS = [(1, 4, 4), (28, 385 * 128, 385 * 128), (70, 128, 128), (512, 256, 256)]


def _inputs(B, T, nvalid, draw, seed):
    g = np.random.default_rng(seed)
    rows, R = B * T, 15
    if draw == "exact":
        perm = g.permutation(np.arange(1, I))
        ids = perm[:rows].copy()
        ids[g.permutation(rows)[:5]] = 0                   # padding rows: dropped, so they may repeat
        labels = perm[rows:rows + R].copy()                # distinct, disjoint from the ids: one add per address
        q = lambda shape, s: torch.from_numpy(g.integers(-2 * s, 2 * s + 1, shape).astype(np.float32) / s)   # noqa: E731
        dx0, add1, add2, lab_rows = q((rows, 3 * C), 16), q((rows, C), 16), q((rows, C), 16), q((R, C), 16)
        parts = [torch.from_numpy(g.integers(-63, 64, (P, ld)).astype(np.float32) / 8) for P, _, ld in JOBS]
    else:                                                  # Zipf-like: a third of the rows on one id, repeated labels
        ids = np.minimum(g.zipf(1.3, rows), I - 1)
        ids[g.random(rows) < 1.0 / 3.0] = 7
        ids[g.random(rows) < 0.05] = 0
        labels = g.integers(0, 12, R)
        n = lambda shape: torch.from_numpy(g.standard_normal(shape).astype(np.float32))   # noqa: E731
        dx0, add1, add2, lab_rows = n((rows, 3 * C)), n((rows, C)), n((rows, C)), n((R, C))
        parts = [n((P, ld)) for P, _, ld in JOBS]
    coef = g.random(R).astype(np.float32)
    coef[3] = 0.0                                          # a row without weight
    marks = (g.random((rows, E)) < 0.3).astype(np.uint8)
    dev = lambda t: t.cuda().contiguous()                  # noqa: E731
    bf = lambda t: dev(t.to(torch.bfloat16))               # noqa: E731
    return dict(B=B, T=T, R=R, ids=dev(torch.from_numpy(ids.astype(np.int64))), labels=dev(torch.from_numpy(labels.astype(np.int64))),
                dx0=bf(dx0), add1=bf(add1), add2=bf(add2), lab_rows=bf(lab_rows), coef=dev(torch.from_numpy(coef)),
                marks=dev(torch.from_numpy(marks)), nvalid=torch.tensor([nvalid], dtype=torch.int32, device="cuda"),
                parts=[dev(p) for p in parts])


def _run(inp, mode, jobs=None, extra=None):
    """mode "now" | "seq" | "ride" | "ride2".  jobs: (part, P, N, ld) queued in front of the call (default: JOBS over inp["parts"]);
    extra(d_item) -> one more such job with its output inside d_item.  Returns (final, before_flush): dicts of tensors."""
    from easydgl_amd import _lib, ops
    lib, P_ = _lib.lib, ops._ptr
    B, T, R = inp["B"], inp["T"], inp["R"]
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")   # noqa: E731
    # the bias gradient with the first job's output right behind it, as neighbours in a gradient arena are
    arena = nan(I - 1 + 4)
    d_item, d_bias = torch.zeros((I, C), device="cuda"), arena[:I - 1].zero_()
    d_pos, d_mark = nan(T, C), nan(E, C)
    ws = torch.empty(lib.edgl_encode_bwd_workspace(B, T, C), device="cuda")
    if jobs is None:
        jobs = [(p, P, N, ld) for p, (P, N, ld) in zip(inp["parts"], JOBS)]
    outs = [arena[I - 1:] if (i == 0 and N == 4) else nan(N) for i, (_, _, N, _) in enumerate(jobs)]
    targets = [(p, P, N, ld, o.data_ptr()) for (p, P, N, ld), o in zip(jobs, outs)]
    if extra is not None:
        targets.append(extra(d_item))
    st = ops._stream()
    named = lambda: dict(d_item=d_item.clone(), d_bias=d_bias.clone(), d_pos=d_pos.clone(), d_mark=d_mark.clone(),   # noqa: E731
                         **{f"job{i}": o.clone() for i, o in enumerate(outs)})
    try:
        if mode != "now":
            _lib.check(lib.edgl_reduce_defer(1, st), "edgl_reduce_defer")
        for p, P, N, ld, out in targets:
            _lib.check(lib.edgl_reduce_partials(P_(p), P, N, ld, out, 0, st), "edgl_reduce_partials")
        if mode in ("ride", "ride2"):
            _lib.check(lib.edgl_reduce_ride(2 if mode == "ride2" else 1), "edgl_reduce_ride")
        _lib.check(lib.edgl_encode_bwd_add_label(P_(inp["ids"]), P_(inp["marks"]), P_(inp["dx0"]), P_(inp["add1"]), P_(inp["add2"]), B, T,
                                                 C, E, I, 0.0, None, 1, P_(d_item), P_(d_pos), P_(d_mark), P_(ws), 0, P_(inp["lab_rows"]),
                                                 P_(inp["labels"]), P_(inp["coef"]), P_(inp["nvalid"]), R, P_(d_bias), _lib.BF16, st),
                   "edgl_encode_bwd_add_label")
        torch.cuda.synchronize()
        before = named()
        if mode != "now":
            _lib.check(lib.edgl_reduce_defer(0, st), "edgl_reduce_defer")
    except BaseException:
        lib.edgl_reduce_defer(-1, st)
        raise
    torch.cuda.synchronize()
    return named(), before


def _same_bits(a, b, what, skip=()):
    for k in a:
        if k not in skip:      # (as bit patterns: the pre-filled NaNs of an output nobody wrote yet compare equal too)
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (what, k, float((a[k] - b[k]).abs().nan_to_num(nan=1e30).max()))


def _item_reference(inp):
    """fp64 d_item / d_bias of the SAME bf16 operands: the three-way sum of the item section and coef * row are rounded to bf16
    once each (the operands of the segmented sum), everything behind them in fp64."""
    rows, R = inp["B"] * inp["T"], inp["R"]
    x = (inp["dx0"].reshape(rows, 3 * C)[:, :C].float() + inp["add1"].float() + inp["add2"].float()).to(torch.bfloat16).double()
    x = x * float(np.sqrt(np.float32(C)))
    ids = inp["ids"]
    d_item = torch.zeros((I, C), device="cuda", dtype=torch.float64).index_add_(0, ids[ids != 0], x[ids != 0])
    live = (torch.arange(R, device="cuda") < min(R, int(inp["nvalid"]))) & (inp["labels"] != 0) & (inp["coef"] != 0)
    lr = (inp["coef"][:, None] * inp["lab_rows"].float()).to(torch.bfloat16).double()
    lab = inp["labels"][live]
    d_item.index_add_(0, lab, -lr[live])
    d_bias = torch.zeros(I - 1, device="cuda", dtype=torch.float64).index_add_(0, lab - 1, -inp["coef"][live].double())
    return d_item, d_bias


@pytest.mark.parametrize("order", ["ride", "ride2"])     # reduction workgroups in front of / behind the scatter's
@pytest.mark.parametrize("draw", ["exact", "random"])
@pytest.mark.parametrize("nvalid", [9, 0])
@pytest.mark.parametrize("B,T", [(3, 37), (5, 101)])     # 111 rows: one partial scatter block; 505 rows: a partial last block
def test_queued_reductions_ride_in_the_scatter_launch(B, T, nvalid, draw, order):
    inp = _inputs(B, T, nvalid, draw, seed=100 * B + nvalid + (draw == "exact"))
    seq, seq_before = _run(inp, "seq")
    ride, ride_before = _run(inp, order)
    # without riding nothing of the queue has run behind the call; with it everything has, and the flush adds nothing
    assert all(bool(torch.isnan(seq_before[k]).all()) for k in seq if k.startswith("job") or k == "d_pos")
    _same_bits(ride_before, ride, "ride: before / behind the flush")
    assert all(bool(torch.isfinite(v).all()) for v in ride.values())
    if draw == "exact":
        _same_bits(seq, ride, "seq / ride")
        now, _ = _run(inp, "now")
        _same_bits(now, ride, "stand-alone launches / ride")
        assert float(ride["d_item"].abs().max()) > 0.0 and float(ride["d_pos"].abs().max()) > 0.0
        assert (float(ride["d_bias"].abs().max()) > 0.0) == (nvalid > 0)
    else:
        _same_bits(seq, ride, "seq / ride", skip=("d_item", "d_bias"))      # (atomics on repeated ids: order-dependent bits)
        want_item, want_bias = _item_reference(inp)
        for got, want, name in ((ride["d_item"], want_item, "d_item"), (ride["d_bias"], want_bias, "d_bias"),
                                (seq["d_item"], want_item, "d_item (seq)")):
            ok, e = grad_ok(got.cpu().numpy(), want.cpu().numpy(), "f32")
            print(f"{name} B={B} T={T} nvalid={nvalid}: rel-L2 {e[0]:.3e}, rel-max {e[1]:.3e}")
            assert ok, (name, e, GRAD_TOL["f32"])


@pytest.mark.parametrize("case", ["unaligned", "overflow", "overlap"])
def test_lists_that_do_not_ride_are_left_to_the_flush(case):
    """unaligned: a job with N = 6 takes the vector form away from the whole list — nothing rides, the flush runs everything.
    overflow: 24 queued jobs fill the queue; the call launches them by themselves (without riding: when its own first job is
    queued behind the scatter; with riding: in the hand-over, in front of the scatter) and only the call's two jobs ride.  overlap: a job that ASSIGNS a row of d_item which the scatter adds to — behind the scatter in the
    deferred sequence, so the list must not run beside it."""
    inp = _inputs(5, 101, 9, "exact", seed=7)
    g = np.random.default_rng(11)
    exact = lambda P, ld: torch.from_numpy(g.integers(-63, 64, (P, ld)).astype(np.float32) / 8).cuda()   # noqa: E731
    jobs, extra, skip_now = None, None, ()
    if case == "unaligned":
        jobs = [(p, P, N, ld) for p, (P, N, ld) in zip(inp["parts"], JOBS)] + [(exact(40, 6), 40, 6, 6)]
    elif case == "overflow":
        jobs = [(exact(3 + 5 * i, 64), 3 + 5 * i, 64, 64) for i in range(24)]
    else:
        part, row = exact(4, C), int(inp["ids"][inp["ids"] != 0][0])
        extra = lambda d_item: (part, 4, C, C, d_item.data_ptr() + 4 * row * C)   # noqa: E731
        skip_now = ("d_item",)      # (undeferred, the job runs in FRONT of the scatter: another result by contract)
    seq, seq_before = _run(inp, "seq", jobs, extra)
    ride, ride_before = _run(inp, "ride", jobs, extra)
    now, _ = _run(inp, "now", jobs, extra)
    _same_bits(seq, ride, "seq / ride")
    _same_bits(now, ride, "stand-alone launches / ride", skip=skip_now)
    assert all(bool(torch.isfinite(v).all()) for v in ride.values())
    if case == "overflow":
        _same_bits(ride_before, ride, "overflow: everything has run behind the call")
        assert bool(torch.isnan(seq_before["d_pos"]).all()) and bool(torch.isfinite(seq_before["job23"]).all())
    else:
        _same_bits(seq_before, ride_before, "nothing rode")
        assert bool(torch.isnan(ride_before["d_pos"]).all()) and bool(torch.isnan(ride_before["job0"]).all())
    if case == "overlap":      # the job's sums (exact draw: every order gives these bits) replaced what the scatter had added
        assert float(ride_before["d_item"][row].abs().max()) > 0.0
        assert torch.equal(ride["d_item"][row], part.double().sum(0).float()) and not torch.equal(ride_before["d_item"][row], ride["d_item"][row])


# ---- engine level -------------------------------------------------------------------------------------------------------------------
def _engine_problem():
    """B = 4, T = seqslen + 1 = 21: 84 rows = ONE scatter block; I = num_items + 1 = 400 table rows; item ids all distinct, labels
    from a disjoint id range: no two atomics meet."""
    from tests._util import make_problem
    prob = make_problem(seed=91, batch=4, num_units=128, num_heads=8, num_blocks=1, seqslen=20, masklen=3, num_events=16, num_items=399)
    g = np.random.default_rng(92)
    B, T, M = 4, 21, 3
    ids = (1 + g.permutation(199))[:B * T].reshape(B, T).astype(np.int64)
    labels = (200 + g.permutation(199))[:B * M].reshape(B, M).astype(np.int64)
    ts = (9.5e8 + np.cumsum(g.exponential(3 * 86400.0, size=(B, T)), axis=1)).astype(np.float32)
    mp = np.stack([g.choice(T - 1, M, replace=False) + 1 for _ in range(B)]).astype(np.int64)
    feats = dict(seqs_i=torch.from_numpy(ids).cuda(), seqs_t=torch.from_numpy(ts).cuda(), masked_positions=torch.from_numpy(mp).cuda())
    return prob, feats, torch.from_numpy(labels).cuda()


@pytest.mark.parametrize("deterministic", [False, True])
def test_engine_steps_are_bit_identical_with_and_without_riding(deterministic, monkeypatch):
    """Three step()s and a bare _issue(), switch on against switch off: the same bits.  That the reductions really rode (and in
    deterministic mode really did not) is read off the position gradient, pre-filled with NaN: with riding it is final when the
    engine leaves the deferred mode, without it the flush of that call writes it."""
    import easydgl_amd.engine as engine_mod
    from easydgl_amd.engine import TrainEngine
    from tests._util import build_model
    prob, feats, labels = _engine_problem()

    class Spy:      # engine.lib with a look at d_pos in front of every edgl_reduce_defer(0)
        def __init__(self, inner, d_pos):
            self.inner, self.d_pos, self.final_before_flush = inner, d_pos, None

        def __getattr__(self, name):
            fn = getattr(self.inner, name)
            if name != "edgl_reduce_defer":
                return fn

            def call(on, st):
                if on == 0:
                    torch.cuda.synchronize()
                    self.final_before_flush = bool(torch.isfinite(self.d_pos).all())
                return fn(on, st)
            return call

    def run(flag, bare):
        monkeypatch.setenv("EDGL_REDUCE_RIDE", flag)
        m = build_model(prob, "bf16", hidden_drop=0.1, att_drop=0.1)
        e = TrainEngine(m, 4, use_graph=False, deterministic=deterministic)
        assert e.reduce_ride == (flag == "1" and not deterministic)      # deterministic mode keeps the old launch sequence
        e.load_batch(feats, labels)
        if bare:
            d_pos = m.pcoding.pembs.lookup_table.grad
            d_pos.fill_(float("nan"))
            spy = Spy(engine_mod.lib, d_pos)
            monkeypatch.setattr(engine_mod, "lib", spy)
            try:
                e._issue()
            finally:
                monkeypatch.setattr(engine_mod, "lib", spy.inner)
            torch.cuda.synchronize()
            assert spy.final_before_flush == e.reduce_ride, (flag, deterministic, spy.final_before_flush)
            return [float(e.loss)], [m._grad_arena.clone()]
        losses = [float(e.step()) for _ in range(3)]
        torch.cuda.synchronize()
        return losses, [m._arena.clone(), m._adam_m.clone(), m._adam_v.clone()]

    for bare in (False, True):
        l0, t0 = run("0", bare)
        l1, t1 = run("1", bare)
        assert l0 == l1 and all(np.isfinite(l0)), (l0, l1)
        for a, b in zip(t0, t1):
            assert torch.equal(a, b), float((a - b).abs().max())
            assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0.0
