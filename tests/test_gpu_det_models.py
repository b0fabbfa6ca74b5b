"""Deterministic training of CTSMA / TGAT / TiSASRec: the ordered forms of the embedding scatters
(edgl_embed_pos_bwd_det, edgl_embedding_bwd_det), of the interval bins (EDGL_TATTN_ORDERED) and of the interval-table gradients
(edgl_tiattn_bwd_det) give the same bits in every call and compute what the atomic forms compute; the three models are
reproducible bit for bit with the flag set.

Bounds.  Item sums: per element (n + 2) 2^-23 sum|term| with n the segment length — tests/test_gpu_segsum.py derives it (a sum
of n products has at most n + 1 f32 roundings; the factor 2 leaves room for chunked orders) and the atomic form is held to the
same bound against the same fp64 sum.  Interval attention, ordered against default: the kernel-against-oracle tolerances of
tests/test_gpu_tisasrec.py (forward 1e-4 / 3e-2, gradients 1e-3 / 1e-1, max-norm relative).  Models against their fp64 oracles:
the tolerances and per-tensor bounds of the models' own test files, imported from there."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import baselines_ref as BR
from oracle import ctsma_ref as CR
from tests import test_gpu_ctsma as TC
from tests import test_gpu_tgat as TG
from tests import test_gpu_tisasrec as TT
from tests._util import assert_close, grad_errors, regressive_bf16_bounds, rel_err, relu_flip_err, to_dev
from tests.test_gpu_segsum import U23

pytestmark = pytest.mark.gpu

STREAM = 3      # dropout stream id of the kernel-level calls


# ---- kernel level: the item sums ------------------------------------------------------------------------------------------------
def _rand(shape, dt, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, device="cuda", dtype=torch.float32, generator=g).to(dt)


def _ids(B, T, I, seed, hot=False):
    g = np.random.default_rng(seed)
    ids = g.integers(0, I, (B, T))                      # id 0 (padding) among them
    if hot:
        ids[g.random((B, T)) < 1.0 / 3.0] = I - 1       # a third of the tokens on one id
    ids[0, :T // 3] = 0
    return torch.from_numpy(ids).cuda()


def _keep_factor(n, rate, rng):
    """f32 [n]: 0 or 1 / (1 - rate) per element index — the counter-based mask every kernel derives from (state, stream, index)"""
    from easydgl_amd import ops
    if rate == 0.0:
        return torch.ones(n, device="cuda")
    return ops.dropout(torch.ones(n, device="cuda"), ops.Drop(rate, rng, STREAM))


def _embed_pos_bwd(det, ids, dx0, C, I, pos, rate, rng, c_true):
    from easydgl_amd import _lib, ops
    lib, P = _lib.lib, ops._ptr
    B, T = ids.shape
    d_item = torch.full((I, C), float("nan"), device="cuda")         # overwritten, whatever it held
    d_pos = torch.full((T, C), float("nan"), device="cuda") if pos else None
    head = (P(ids), P(dx0), B, T, C, I, float(rate), P(rng) if rate else None, STREAM, P(d_item), P(d_pos), int(c_true))
    if det:
        plan = ops.segsum_plan_buffer(B * T, I, ids.device)
        _lib.check(lib.edgl_embed_pos_bwd_det(*head, P(plan), ops._DT[dx0.dtype], ops._stream()), "edgl_embed_pos_bwd_det")
    else:
        _lib.check(lib.edgl_embed_pos_bwd_ct(*head, ops._DT[dx0.dtype], ops._stream()), "edgl_embed_pos_bwd_ct")
    return d_item, d_pos


def _index_sums(keys, terms, rows):
    """(fp64 sum, sum of |term|, count) per key in [0, rows); keys outside are dropped"""
    keep = (keys >= 0) & (keys < rows)
    ref = torch.zeros((rows, terms.shape[1]), device="cuda", dtype=torch.float64).index_add_(0, keys[keep], terms[keep])
    S = torch.zeros_like(ref).index_add_(0, keys[keep], terms[keep].abs())
    cnt = torch.bincount(keys[keep], minlength=rows).double()
    return ref, S, cnt


def _assert_within(got, ref, S, cnt, what):
    bound = (cnt[:, None] + 2) * U23 * S
    err = (got.double() - ref).abs()
    worst = float((err - bound).max())
    print(f"{what}: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}, worst err - bound {worst:.3e}")
    assert torch.isfinite(got).all(), what
    assert worst <= 0.0, (what, worst)


EMBED_SHAPES = [(48, 30, 64, 12, 0, False),         # >= 2 sort blocks, every id hundreds of times: segments cross the 64-row windows
                (3, 12, 32, 60, 0, False),
                (4, 100, 128, 2000, 0, True),       # a third of the tokens on one id
                (2, 30, 512, 700, 0, False),
                (48, 30, 64, 12, 50, False)]        # channel-padded: the scale is sqrt(50)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rate", [0.0, 0.1])
@pytest.mark.parametrize("pos", [True, False], ids=["pos", "nopos"])
@pytest.mark.parametrize("B,T,C,I,c_true,hot", EMBED_SHAPES)
def test_embed_pos_bwd_det(B, T, C, I, c_true, hot, pos, rate, dt):
    ids = _ids(B, T, I, 7 * B + T, hot)
    ldo = 2 * C if pos else C
    dx0 = _rand((B, T, ldo), dt, 11)
    rng = torch.tensor([4242, 6], dtype=torch.int64, device="cuda")
    a_item, a_pos = _embed_pos_bwd(True, ids, dx0, C, I, pos, rate, rng, c_true)
    b_item, b_pos = _embed_pos_bwd(True, ids, dx0, C, I, pos, rate, rng, c_true)
    assert torch.equal(a_item, b_item) and (not pos or torch.equal(a_pos, b_pos))
    at_item, at_pos = _embed_pos_bwd(False, ids, dx0, C, I, pos, rate, rng, c_true)
    masked = dx0.reshape(B * T, ldo).double() * _keep_factor(B * T * ldo, rate, rng).reshape(B * T, ldo).double()
    flat = ids.reshape(-1).clone()
    flat[flat == 0] = -1                                                        # coding.py:56-57: row 0 is a constant
    ref, S, cnt = _index_sums(flat, masked[:, :C] * float(np.sqrt(np.float32(c_true if c_true else C))), I)
    if hot:
        assert int(cnt[I - 1]) >= B * T // 4
    if I == 12:
        assert int(cnt[1:].min()) > 64                                          # every segment crosses a window
    _assert_within(a_item, ref, S, cnt, "d_item (ordered)")
    _assert_within(at_item, ref, S, cnt, "d_item (atomic)")
    assert float(a_item[0].abs().max()) == 0.0
    if pos:
        tpos = torch.arange(T, device="cuda").repeat(B)
        ref, S, cnt = _index_sums(tpos, masked[:, C:], T)
        _assert_within(a_pos, ref, S, cnt, "d_pos (ordered)")
        _assert_within(at_pos, ref, S, cnt, "d_pos (atomic)")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("zero_pad", [1, 0])
@pytest.mark.parametrize("B,T,C,I,hot", [s[:4] + s[5:] for s in EMBED_SHAPES[:4]])
def test_embedding_bwd_det(B, T, C, I, hot, zero_pad, dt):
    from easydgl_amd import _lib, ops
    lib, P = _lib.lib, ops._ptr
    ids = _ids(B, T, I, 5 * B + T, hot)
    ids[-1, -1] = I + 3                                 # an index past the table reads zeros in the forward: no gradient
    n = B * T
    d_out = _rand((B, T, C), dt, 21)
    scale = float(np.float32(np.sqrt(C)))

    def run(det):
        d_table = torch.full((I, C), float("nan"), device="cuda")
        if det:
            plan = ops.segsum_plan_buffer(n, I + 1, ids.device)
            _lib.check(lib.edgl_embedding_bwd_det(P(ids), n, P(d_out), I, C, zero_pad, scale, P(d_table), P(plan), ops._DT[dt],
                                                  ops._stream()), "edgl_embedding_bwd_det")
        else:
            _lib.check(lib.edgl_embedding_bwd(P(ids), n, P(d_out), I, C, zero_pad, scale, P(d_table), ops._DT[dt], ops._stream()),
                       "edgl_embedding_bwd")
        return d_table

    a, b, at = run(True), run(True), run(False)
    assert torch.equal(a, b)
    flat = ids.reshape(-1).clone()
    if zero_pad:
        flat[flat == 0] = -1
    ref, S, cnt = _index_sums(flat, d_out.reshape(n, C).double() * scale, I)
    assert zero_pad or int(cnt[0]) > 0
    _assert_within(a, ref, S, cnt, "d_table (ordered)")
    _assert_within(at, ref, S, cnt, "d_table (atomic)")


def test_embedding_module_takes_the_flag():
    """ops.EmbeddingFn(deterministic=True) through autograd: two backward passes give the same bits, and the default's values."""
    from easydgl_amd import ops
    tab = _rand((60, 32), torch.float32, 1).requires_grad_(True)
    ids = _ids(3, 12, 60, 9)
    w = _rand((3, 12, 32), torch.float32, 2)
    grads = []
    for det in (True, True, False):
        tab.grad = None
        (ops.EmbeddingFn.apply(tab, tab.detach(), ids, True, 2.0, det) * w).sum().backward()
        grads.append(tab.grad.clone())
    assert torch.equal(grads[0], grads[1])
    assert_close(grads[0].cpu().numpy(), grads[2].cpu().numpy(), 1e-5, "EmbeddingFn d_table")


# ---- kernel level: interval attention ------------------------------------------------------------------------------------------
def _ti_operands(B, T, H, dh, timelen, dt, seed):
    C = H * dh
    g = np.random.default_rng(seed)
    mk = lambda *s, k=1.0: (torch.tensor(g.standard_normal(s) * k, dtype=torch.float32).to(dt)).cuda()
    ids = g.integers(1, 50, (B, T))
    ids[0, :T // 3] = 0                                 # left padding in one sample
    # mean gap of timelen / 3 buckets at timelen 8 (almost every pair clips into the last buckets), a few buckets otherwise
    gap = timelen / 3.0 if timelen <= 8 else timelen / T * 1.5
    ts = np.cumsum(g.exponential(gap, (B, T + 1)), axis=1).astype(np.float32)
    ts[:, :-1][ids == 0] = 0.0
    return dict(q=mk(B, T, C), kvp=mk(B, T, 2 * C), resid=mk(B, T, C), d_out=mk(B, T, C), kt=mk(timelen, C, k=0.3),
                vt=mk(timelen, C, k=0.3), ids=torch.from_numpy(ids).cuda(), ts=torch.from_numpy(ts).cuda())


def _tiattn(o, B, T, H, dh, timelen, rate, rng, ordered, det_bwd):
    """forward + backward through the C ABI; every output by name"""
    from easydgl_amd import _lib, ops
    lib, P, V = _lib.lib, ops._ptr, ops._vptr
    C = H * dh
    q, kvp = o["q"], o["kvp"]
    code = ops._code(q)
    flags = _lib.TATTN_CAUSAL | (_lib.TATTN_ORDERED if ordered else 0)
    out = torch.empty_like(q)
    saved = torch.zeros(int(lib.edgl_tattn_saved_bytes(B, T, H, dh)), device="cuda", dtype=torch.uint8)
    wbuf = torch.zeros(int(lib.edgl_tiattn_bucket_elems(B, T, H, timelen)), device="cuda", dtype=q.dtype)
    scale = 1.0 / float(dh) ** 0.5
    _lib.check(lib.edgl_tiattn_fwd(P(q), C, P(kvp), 2 * C, V(kvp[:, :, C:]), 2 * C, P(o["resid"]), C, P(o["ids"]), P(o["ts"]),
                                   P(o["kt"]), P(o["vt"]), timelen, B, T, H, dh, scale, 1.0, timelen, rate, P(rng), STREAM, P(out), C,
                                   P(saved), P(wbuf), flags, code, ops._stream()), "edgl_tiattn_fwd")
    res = {"out": out.clone(), "wbuf": wbuf.clone()}
    d_q, d_kv, dgbuf = torch.empty_like(q), torch.empty_like(kvp), torch.zeros_like(wbuf)
    d_kt = torch.full((timelen, C), float("nan"), device="cuda")
    d_vt = torch.full((timelen, C), float("nan"), device="cuda")
    head = (P(q), C, P(kvp), 2 * C, V(kvp[:, :, C:]), 2 * C, P(o["ids"]), P(o["ts"]), P(o["kt"]), P(o["vt"]), timelen, P(o["d_out"]), C,
            P(saved), P(wbuf), B, T, H, dh, scale, 1.0, timelen, rate, P(rng), STREAM, P(d_q), C, P(d_kv), 2 * C, V(d_kv[:, :, C:]),
            2 * C, P(dgbuf), P(d_kt), P(d_vt))
    if det_bwd:
        ws = torch.full((int(lib.edgl_tiattn_det_workspace(H, dh, timelen)),), float("nan"), device="cuda")
        _lib.check(lib.edgl_tiattn_bwd_det(*head, P(ws), flags, code, ops._stream()), "edgl_tiattn_bwd_det")
    else:
        _lib.check(lib.edgl_tiattn_bwd(*head, flags, code, ops._stream()), "edgl_tiattn_bwd")
    res.update(saved=saved, d_q=d_q, d_kv=d_kv, dgbuf=dgbuf, d_ktime=d_kt, d_vtime=d_vt)
    return res


@pytest.mark.parametrize("dt,ftol,gtol", [(torch.float32, 1e-4, 1e-3), (torch.bfloat16, 3e-2, 1e-1)], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,H,dh,timelen", [(2, 20, 2, 16, 8), (2, 100, 2, 64, 256), (1, 37, 1, 128, 64)])
def test_tiattn_ordered_bins_and_det_backward(B, T, H, dh, timelen, dt, ftol, gtol):
    o = _ti_operands(B, T, H, dh, timelen, dt, 100 * T + dh)
    rng = torch.tensor([77, 2], dtype=torch.int64, device="cuda")
    bk = torch.clamp(o["ts"][:, 1:, None] - o["ts"][:, None, :-1], 0, timelen).long()
    causal = torch.tril(torch.ones(T, T, dtype=torch.bool, device="cuda"))
    assert timelen > 8 or float((bk[:, causal] >= timelen - 2).float().mean()) > 0.5        # the clipped case really clips
    a = _tiattn(o, B, T, H, dh, timelen, 0.1, rng, True, True)
    b = _tiattn(o, B, T, H, dh, timelen, 0.1, rng, True, True)
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert k == "saved" or torch.isfinite(a[k].float()).all(), k
    # the flag alone on the default entry point: the same ordered sweep, the table gradients through atomics
    c = _tiattn(o, B, T, H, dh, timelen, 0.1, rng, True, False)
    for k in ("out", "wbuf", "saved", "d_q", "d_kv", "dgbuf"):
        assert torch.equal(a[k], c[k]), k
    d = _tiattn(o, B, T, H, dh, timelen, 0.1, rng, False, False)
    for k, tol in (("out", ftol), ("wbuf", ftol), ("d_q", gtol), ("d_kv", gtol), ("dgbuf", gtol), ("d_ktime", gtol), ("d_vtime", gtol)):
        e = rel_err(a[k].float().cpu().numpy(), d[k].float().cpu().numpy())
        print(f"{k}: ordered against default {e:.3e} (tolerance {tol:.0e})")
        assert e <= tol, (k, e, tol)
        if k in ("d_ktime", "d_vtime"):
            assert rel_err(c[k].cpu().numpy(), d[k].cpu().numpy()) <= tol, k
    assert float(a["wbuf"].float().abs().max()) > 0 and float(a["d_ktime"].abs().max()) > 0


# ---- model level ------------------------------------------------------------------------------------------------------------------
KINDS = {"ctsma": (TC, "CTSMA"), "tgat": (TG, "TGAT"), "tisasrec": (TT, "TiSASREC")}


def _model(kind, prob, mode, hidden_drop=0.0, att_drop=0.0, deterministic=True):
    """The `_model` of the models' own test files with FLAGS.deterministic set."""
    import easydgl_amd
    d = prob["dims"]
    F = SimpleNamespace(model=KINDS[kind][1], num_items=d["I"], num_units=d["C"], num_heads=d["h"], num_blocks=d["nb"], seqslen=d["T"],
                        time_scale=prob["kw"]["time_scale"], learning_rate=1e-3, l2_reg=1e-3, hidden_dropout_rate=hidden_drop,
                        attention_probs_dropout_rate=att_drop, compute_dtype=mode, num_train_steps=None, num_warmup_steps=None,
                        deterministic=deterministic)
    if kind == "ctsma":
        F.ct_reg, F.mark_table = 1e-2, prob["mt"]
    if kind == "tisasrec":
        F.timelen = d["timelen"]
    m = easydgl_amd.ranking(F).finalize("cuda")
    m.load_tf_variables(prob["params"])
    assert m.deterministic is deterministic
    return m


def _case(kind, name):
    """(B, T, C, I): a tiny catalogue at a batch of >= 2 sort blocks / the headline widths / the channel-padded default flags"""
    base = {"tiny": dict(B=48, T=30, C=64, h=2, I=12, nb=1), "head": dict(B=4, T=100, C=128, h=8, I=2000, nb=1),
            "padded": dict(B=8, T=30, C=50, h=1, I=300, nb=1)}[name]
    if kind == "ctsma":
        base["E"] = 16 if name == "head" else 4
    if kind == "tgat" and name == "head":
        base["h"] = 2
    if kind == "tisasrec":
        base["timelen"] = {"tiny": 32, "head": 256, "padded": 256}[name]
    return base


def _state(m):
    m.settle_state()
    return {"arena": m._arena.detach().clone(), "adam_m": m._adam_m.clone(), "adam_v": m._adam_v.clone()}


@pytest.mark.parametrize("name,mode", [("tiny", "bf16"), ("tiny", "f32"), ("head", "bf16"), ("padded", "bf16")])
@pytest.mark.parametrize("kind", list(KINDS))
def test_three_train_steps_twice_give_the_same_bits(kind, name, mode):
    mod = KINDS[kind][0]
    probs = [mod._problem(300 + i, **_case(kind, name)) for i in range(3)]
    batches = [(to_dev(p["feats"]), torch.as_tensor(p["tokens"][:, 1:].copy()).cuda()) for p in probs]
    assert probs[0]["dims"]["B"] * probs[0]["dims"]["T"] > 1024 or name != "tiny"
    trajs = []
    for _ in range(2):
        m = _model(kind, probs[0], mode, hidden_drop=0.1, att_drop=0.1)
        start = m._arena.detach().clone()
        t = []
        for feats, labels in batches:
            loss = m.train_step(feats, labels).clone()
            t.append((loss, _state(m)))
        trajs.append(t)
    for step, ((la, sa), (lb, sb)) in enumerate(zip(*trajs)):
        bad = []
        for pname, p in m.named_parameters():
            o = m._offsets[pname]
            bad += [f"{k}:{pname}" for k in sa if not torch.equal(sa[k][o:o + p.numel()], sb[k][o:o + p.numel()])]
        assert not bad, (kind, name, step, bad)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (kind, name, step, k)
        assert torch.equal(la, lb), (kind, name, step, float(la), float(lb))
        assert np.isfinite(float(la))
    assert not torch.equal(start, trajs[0][0][1]["arena"]) and not torch.equal(trajs[0][0][1]["arena"], trajs[0][2][1]["arena"])


@pytest.mark.parametrize("mode,ltol,gtol", [("f32", 1e-4, 1e-3), ("bf16", 3e-2, 1e-1)])
@pytest.mark.parametrize("kind", list(KINDS))
def test_deterministic_mode_matches_the_fp64_oracle(kind, mode, ltol, gtol):
    """CASES[1] of the model's own test file under its own seed, with the flag set: loss and every gradient tensor under the
    tolerances that file applies (bf16: tests/_util.py regressive_bf16_bounds)."""
    mod = KINDS[kind][0]
    prob = mod._problem({"ctsma": 40, "tgat": 60, "tisasrec": 80}[kind] + 1, **mod.CASES[1])
    m = _model(kind, prob, mode)
    feats = to_dev(prob["feats"])
    labels_np = prob["tokens"][:, 1:].copy()
    labels = torch.as_tensor(labels_np).cuda()
    p64 = mod._p64(prob)
    if kind == "ctsma":
        ref_loss, _ = CR.train_loss(p64, prob["mt"], prob["feats"], labels_np, ct_reg=1e-2, l2_reg=1e-3, **prob["kw"])
    elif kind == "tgat":
        ref_loss, _ = BR.tgat_train_loss(p64, prob["feats"], labels_np, l2_reg=1e-3, **prob["kw"])
    else:
        ref_loss, _ = BR.tisasrec_train_loss(p64, prob["feats"], labels_np, l2_reg=1e-3, **prob["kw"])
    m.zero_grad_arena()
    loss = m.train_loss(feats, labels)
    loss.backward()
    ref_loss.backward()
    assert_close(loss.item(), ref_loss.item(), ltol, "train loss")
    got = m.tf_gradients()
    assert set(got) == set(p64)
    kbias = "modulating_attention/dense_1/bias" if kind == "ctsma" else "timeinterval/dense_1/bias"
    bad = {}
    for name, g in got.items():
        ref = p64[name].grad.numpy()
        l2_tol, g_tol = regressive_bf16_bounds(kind, name, gtol, mod.BF16_GRAD_L2) if mode == "bf16" else (mod.BF16_GRAD_L2, gtol)
        if name.endswith(kbias):      # a bias on K shifts a whole score row: its true gradient is zero
            ref_k = p64[name.replace("bias", "kernel")].grad.numpy()
            e = float(np.abs(g).max() / np.abs(ref_k).max())
        else:
            e = rel_err(g, ref)
            if mode == "bf16" and "/Inner/" not in name and grad_errors(g, ref)[0] > l2_tol:
                bad[name + " (rel-L2)"] = grad_errors(g, ref)[0]
        if mode == "bf16" and "/Inner/" in name:
            e = relu_flip_err(g, ref, gtol)
        if e > g_tol:
            bad[name] = (e, g_tol)
    assert not bad, f"gradient mismatch (rel to max |ref|): {bad}"


def test_tisasrec_evaluation_twice_gives_the_same_list():
    """The forward bins are part of the promise: eval_topk of a deterministic model, twice, and its attention units carry the flag."""
    prob = TT._problem(5, B=32, T=20, C=64, h=4, I=400, nb=2, timelen=32)
    m = _model("tisasrec", prob, "bf16")
    assert all(blk.attention.deterministic for blk in m.layers)
    assert not any(blk.attention.deterministic for blk in _model("tisasrec", prob, "bf16", deterministic=False).layers)
    feats = to_dev(prob["feats"])
    v1, i1 = m.eval_topk(feats, mask_seen=True)
    v2, i2 = m.eval_topk(feats, mask_seen=True)
    assert torch.equal(v1, v2) and torch.equal(i1, i2)
    assert torch.isfinite(v1).all()
