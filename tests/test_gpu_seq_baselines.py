"""The time-independent baselines: module/sequential.py MultiHeadAttention and the SASREC / S2PNM model classes
against the float64 restatement tests/_seq_baselines_ref.py.

Tolerances: the f32 path meets tests/_util.py's f32 bounds (loss / logits 1e-4, gradients 1e-3 relative-L2 and max-norm).  The bf16
path starts from GRAD_TOL["bf16"] / LOSS_TOL["bf16"]; a tensor class listed in tests/golden/seq_baselines_bf16_bounds.json is held
to 2 x its error measured against the fp64 restatement instead (make_seq_baselines_bounds.py); the ReLU-gated Inner tensors keep
relu_flip_err's condition."""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _cand_ce_ref as CE
from tests import _seq_baselines_ref as SR
from tests.golden.make_seq_baselines_bounds import tensor_class
from tests._util import GRAD_TOL, LOSS_TOL, assert_close, dump_errors, grad_errors, relu_flip_err, to_dev

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- MultiHeadAttention ---------------------------------------------------------------------------------------------------
def _mha(in_mult, seed=0, rate=0.0):
    from easydgl_amd.module.sequential import MultiHeadAttention
    B, T, H, dh = 3, 10, 2, 16
    C = H * dh
    cin = in_mult * C
    rng = np.random.default_rng(seed)
    ids = rng.integers(1, 50, size=(B, T))
    ids[0, :4] = 0
    ids[1, :T - 1] = 0                  # fully padded but for its last position: rows 0..T-2 are uniform over all T keys
    keys = rng.standard_normal((B, T, cin)) * (ids != 0)[..., None]          # the models mask the keys in front of every block
    queries = rng.standard_normal((B, T, cin))
    att = MultiHeadAttention(C, H, rate, in_units=cin, gen=torch.Generator().manual_seed(seed)).cuda()
    with torch.no_grad():
        att.q_bias.add_(torch.tensor(0.1 * rng.standard_normal(C), dtype=torch.float32).cuda())
        att.kv_bias.add_(torch.tensor(0.1 * rng.standard_normal(2 * C), dtype=torch.float32).cuda())
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)
    return att, f32(queries), f32(keys), torch.tensor(ids), C


def _mha_ref(att, q, k, causal):
    C = att.num_units
    w = {n: p.detach().double().cpu().requires_grad_(True) for n, p in att.named_parameters()}
    q64, k64 = q.double().requires_grad_(True), k.double().requires_grad_(True)
    out = SR.multihead_attention(q64, k64, w["q_kernel"], w["q_bias"], w["kv_kernel"][:, :C], w["kv_bias"][:C], w["kv_kernel"][:, C:],
                                 w["kv_bias"][C:], att.num_heads, causal)
    return out, w, q64, k64


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("in_mult", [1, 2])
def test_multihead_attention_matches_float64(in_mult, causal):
    att, q, k, ids, C = _mha(in_mult)
    want, w, q64, k64 = _mha_ref(att, q, k, causal)
    rng = np.random.default_rng(5)
    d_out = torch.tensor(rng.standard_normal(want.shape), dtype=torch.float32)
    want.backward(d_out.double())
    qd, kd = q.cuda().requires_grad_(True), k.cuda().requires_grad_(True)
    got = att(qd, kd, True, causal, ids=ids.cuda())
    assert_close(got.detach().cpu().numpy(), want.detach().numpy(), 1e-4, "attention output")
    # a fully masked query row is uniform over ALL keys (the -2^32+1 replacement), not zero and not NaN
    P_uniform = (k64.detach() @ w["kv_kernel"][:, C:].detach() + w["kv_bias"][C:].detach())[1].mean(0) + q64.detach()[1, 0, :C]
    if causal:
        assert_close(got.detach().cpu().numpy()[1, 0], P_uniform.numpy(), 1e-4, "uniform row")
    got.backward(d_out.cuda())
    pairs = [("queries", qd.grad, q64.grad), ("keys", kd.grad, k64.grad)] + [(n, p.grad, w[n].grad) for n, p in att.named_parameters()]
    for name, g, ref in pairs:
        l2, mx = grad_errors(g.float().cpu().numpy(), ref.numpy())
        assert l2 <= 1e-3 and mx <= 1e-3, (name, l2, mx)


@pytest.mark.parametrize("in_mult", [1, 2])
def test_multihead_attention_dropout_uses_one_mask_forward_and_backward(in_mult):
    """With dropout the output is linear in V for a fixed mask: <out(V + dV) - out(V), d_out> == <d_kv[V block], dV> holds only if
    the backward regenerates the forward's mask (the check of tests/test_gpu_tgat.py, no finite differences)."""
    from easydgl_amd import ops
    att, q, k, ids, C = _mha(in_mult, seed=3, rate=0.3)
    q, k, ids = q.cuda(), k.cuda(), ids.cuda()
    drop = ops.Drop(0.3, ops.make_rng_state("cuda", 77), 10)
    plain = att(q, k, False, True, ids=ids, drop=drop)
    out = att(q, k, True, True, ids=ids, drop=drop)
    assert torch.equal(out, att(q, k, True, True, ids=ids, drop=drop)) and not torch.allclose(out, plain)
    g = torch.Generator(device="cuda").manual_seed(0)
    d_out = torch.randn(out.shape, device="cuda", generator=g)
    q_lin = ops.LinearFn.apply(q, att.q_kernel, att.q_bias, att.q_kernel, False)
    kv = ops.LinearFn.apply(k, att.kv_kernel, att.kv_bias, att.kv_kernel, False).detach().requires_grad_(True)
    o1 = ops.PlainAttnFn.apply(q_lin, kv, q[:, :, :C], ids, att.num_heads, drop, True)
    o1.backward(d_out)
    dV = torch.zeros_like(kv)
    dV[:, :, C:] = torch.randn(kv[:, :, C:].shape, device="cuda", generator=g)
    o2 = ops.PlainAttnFn.apply(q_lin, (kv + dV).detach(), q[:, :, :C], ids, att.num_heads, drop, True)
    lhs, rhs = float(((o2 - o1).double() * d_out.double()).sum()), float((kv.grad.double() * dV.double()).sum())
    assert abs(lhs - rhs) <= 1e-3 * max(1.0, abs(rhs)), (lhs, rhs)


# ---- the models -----------------------------------------------------------------------------------------------------------
KINDS = {
    "SASREC": dict(nb=2, shapes=lambda I, T, C, nb: SR.sasrec_shapes(I, T, C, nb),
                   loss=lambda p, f, l, C, h, nb, l2: SR.sasrec_train_loss(p, f, l, C, h, nb, l2),
                   elog=lambda p, f, C, h, nb: SR.sasrec_eval_logits(p, f, C, h, nb), adam=dict()),
    "S2PNM": dict(nb=1, shapes=lambda I, T, C, nb: SR.s2pnm_shapes(I, T, C),
                  loss=lambda p, f, l, C, h, nb, l2: SR.s2pnm_train_loss(p, f, l, C, h, l2),
                  elog=lambda p, f, C, h, nb: SR.s2pnm_eval_logits(p, f, C, h), adam=dict(beta2=0.98, eps=1e-9, clip=5.0)),
}
SMALL = dict(I=50, T=10, C=32, h=2)


def _problem(kind, seed, B=5, I=50, T=10, C=32, h=2, nb=None):
    nb = KINDS[kind]["nb"] if nb is None else nb
    rng = np.random.default_rng(seed)
    params = SR.init_from_shapes(KINDS[kind]["shapes"](I, T, C, nb), rng)
    tokens = rng.integers(1, I, size=(B, T + 1))
    tokens[0, :T // 3] = 0              # left padding of different lengths per sample
    tokens[1, :1] = 0
    if B > 2:
        tokens[2, :T - 1] = 0           # one real position: every other query row is fully masked
    feats = {"seqs_i": tokens[:, :-1].copy(), "seqs_t": np.zeros((B, T + 1), dtype=np.float32)}
    return dict(kind=kind, params=params, feats=feats, tokens=tokens, dims=dict(I=I, T=T, C=C, h=h, nb=nb))


def _model(prob, mode, l2_reg=1e-3, lr=1e-3, **extra):
    import easydgl_amd
    d = prob["dims"]
    F = SimpleNamespace(model=prob["kind"], num_items=d["I"], num_units=d["C"], num_heads=d["h"], num_blocks=d["nb"], seqslen=d["T"],
                        learning_rate=lr, l2_reg=l2_reg, hidden_dropout_rate=0.0, attention_probs_dropout_rate=0.0,
                        compute_dtype=mode, num_train_steps=None, num_warmup_steps=None, **extra)
    m = easydgl_amd.ranking(F).finalize("cuda")
    m.load_tf_variables(prob["params"])
    return m


def _p64(prob):
    return {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in prob["params"].items()}


def _ref_loss(prob, p64, l2_reg=1e-3):
    d = prob["dims"]
    return KINDS[prob["kind"]]["loss"](p64, prob["feats"], prob["tokens"][:, 1:], d["C"], d["h"], d["nb"], l2_reg)


_BOUNDS = json.load(open(os.path.join(HERE, "golden", "seq_baselines_bf16_bounds.json")))["bounds"]


def bf16_bounds(kind, name):
    """(relative-L2, max-norm) bound of one gradient tensor on the bf16 path: GRAD_TOL["bf16"], or for a listed tensor class 2 x the
    error measured against the fp64 restatement (tests/golden/seq_baselines_bf16_bounds.json, make_seq_baselines_bounds.py)."""
    return tuple(_BOUNDS.get(kind, {}).get(tensor_class(name), GRAD_TOL["bf16"]))


CASES = [("small", dict(SMALL)), ("published", dict(I=300, T=30, C=512, B=4))]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("case", [c[0] for c in CASES])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_forward_loss_and_gradients(kind, case, mode):
    cfg = dict(dict(CASES)[case])
    if case == "published":             # runme.sh:39-55: SASREC 8 heads, S2PNM one head of 512 channels
        cfg["h"] = 8 if kind == "SASREC" else 1
    prob = _problem(kind, 60 + len(kind), **cfg)
    d = prob["dims"]
    m = _model(prob, mode)
    feats = to_dev(prob["feats"])
    labels = torch.as_tensor(prob["tokens"][:, 1:].copy()).cuda()
    p64 = _p64(prob)
    ref_loss, aux = _ref_loss(prob, p64)
    ltol = LOSS_TOL[mode]
    ftol = 1e-4 if mode == "f32" else 3e-2       # logits of the bf16 path: the bound of the other regressive models' tests
    logits = m(feats, True)
    assert logits.shape == aux["logits"].shape
    e_log = float(np.abs(logits.detach().float().cpu().numpy() - aux["logits"].detach().numpy()).max() / np.abs(aux["logits"].detach().numpy()[:, 1:]).max())
    print(f"{kind} {case} {mode}: train logits err {e_log:.3e}")
    assert float((logits.detach()[:, 0] + 1000).abs().max()) == 0.0
    m.zero_grad_arena()
    loss = m.train_loss(feats, labels)
    loss.backward()
    ref_loss.backward()
    e_loss = abs(loss.item() - ref_loss.item()) / abs(ref_loss.item())
    print(f"{kind} {case} {mode}: loss {loss.item():.6f} ref {ref_loss.item():.6f} err {e_loss:.3e}")
    got = m.tf_gradients()
    assert set(got) == set(p64)
    bad, errs = {}, {}
    for name, g in got.items():
        ref = p64[name].grad.numpy()
        l2, mx = grad_errors(g, ref)
        if not name.endswith("multihead_attention/dense_1/bias"):      # (the K bias: true gradient zero, no relative error to record)
            errs[f"{kind}:{mode}:{name}"] = (l2, mx)
        print(f"{kind} {case} {mode}: {name} rel-L2 {l2:.3e} max {mx:.3e}")
        if mode == "bf16" and "/Inner/" in name:   # ReLU mask flips, see tests/_util.py:relu_flip_err (at most 5 % of columns)
            relu_flip_err(g, ref, GRAD_TOL["bf16"][1])
            continue
        t2, tm = GRAD_TOL["f32"] if mode == "f32" else bf16_bounds(kind, name)
        if name.endswith("dense_1/bias") and "multihead_attention" in name:
            # a bias on K shifts a whole score row: its true gradient is zero (rounding residue only)
            ref_k = p64[name.replace("bias", "kernel")].grad.numpy()
            assert np.abs(ref).max() < 1e-12 * max(np.abs(ref_k).max(), 1e-30)
            if np.abs(g).max() > tm * np.abs(ref_k).max():
                bad[name] = float(np.abs(g).max() / np.abs(ref_k).max())
        elif l2 > t2 or mx > tm:
            bad[name] = (l2, mx, t2, tm)
    dump_errors("seq_baselines", errs)
    assert e_log <= ftol, e_log
    assert e_loss <= ltol, e_loss
    assert not bad, f"gradient mismatch (rel-L2, max-norm, bounds): {bad}"
    elog = m(feats, False)
    want = KINDS[kind]["elog"](_p64(prob), prob["feats"], d["C"], d["h"], d["nb"])
    assert elog.shape == want.shape
    assert_close(elog.detach().float().cpu().numpy()[:, 1:], want.detach().numpy()[:, 1:], ftol, "eval logits")


def _slot_values(m, arena):
    """TF name -> the entries of a flat per-parameter arena (Adam's m or v) in the reference's shape."""
    out = {}
    for name, p, maps, _ in m._pad_specs():
        off = (p.data_ptr() - m._arena.data_ptr()) // 4
        view = arena[off:off + p.numel()].view(p.shape)
        out[name] = view[m._spec_index(view, maps)].detach().double().cpu().numpy()
    return out


def _adam_case(kind, clip, lr=1e-2, steps=3):
    """`steps` optimizer steps on DIFFERENT batches (so that the gradients, their norms and the clip factors differ from step to
    step) against the restated Adam: the loss of every step, Adam's first and second moments after every step — they carry the
    clip factor (m ~ s, v ~ s^2), beta1 and beta2 directly — and the weights, which carry epsilon where the scaled gradient is of
    its size (the clip = 1e-7 case).

    Bounds.  The f32 gradients meet 1e-3 relative-L2 (tests/_util.py), so m is held to 2e-3 and v (quadratic) to 4e-3 per tensor.
    A weight moves by lr_t * m^ / (sqrt(v^) + eps) <= about lr per step; on the entries whose gradient is within a factor 100 of
    the tensor's largest in every step so far (relative error of g <= about 1e-4 there) the moves agree to 2e-2 * lr per step;
    on the others (tiny or zero gradients, e.g. the K bias: the quotient amplifies their rounding) only |move| <= lr holds."""
    probs = [_problem(kind, 11 + 7 * k, B=5 + k) for k in range(steps)]
    for q in probs[1:]:
        q["params"] = probs[0]["params"]
    m = _model(probs[0], "f32", lr=lr)
    hp = dict(KINDS[kind]["adam"])
    if clip is not None:
        m.clip_norm = clip
    hp["clip"] = m.clip_norm
    p64 = _p64(probs[0])
    opt = SR.ClippedAdam(p64, lr, **hp)
    big = {k: np.ones(v.shape, dtype=bool) for k, v in p64.items()}
    scales = []
    for step, prob in enumerate(probs):
        feats = to_dev(prob["feats"])
        labels = torch.as_tensor(prob["tokens"][:, 1:].copy()).cuda()
        got = float(m.train_step(feats, labels))
        ref, _ = _ref_loss(prob, p64)
        ref.backward()
        for k, w in p64.items():
            g = np.abs(w.grad.detach().numpy())
            big[k] &= g > 1e-2 * g.max()
        opt.step()
        scales.append(opt.last_scale)
        assert abs(got - float(ref.detach())) <= 2e-4 * abs(float(ref.detach())), (step, got, float(ref.detach()))
        m.settle_state()
        mom, var, vals = _slot_values(m, m._adam_m), _slot_values(m, m._adam_v), m.tf_values()
        for name, w in p64.items():
            if name.endswith("multihead_attention/dense_1/bias"):      # true gradient zero: rounding residue only, no relative error
                continue
            e_m = grad_errors(mom[name], opt.m[name].numpy())[0]
            e_v = grad_errors(var[name], opt.v[name].numpy())[0]
            assert e_m <= 2e-3 and e_v <= 4e-3, (step, name, e_m, e_v)
            diff = np.abs(vals[name] - w.detach().numpy())
            assert diff[big[name]].max(initial=0.0) <= 2e-2 * lr * (step + 1), (step, name, diff[big[name]].max())
            assert diff.max() <= 1.01 * lr * (step + 1), (step, name, diff.max())
    return opt, scales


def test_sasrec_adam_steps_follow_the_restatement():
    _adam_case("SASREC", None)


@pytest.mark.parametrize("clip,active", [(0.05, True), (1e-7, True), (1e6, False)])
def test_s2pnm_adam_with_clipping_follows_the_restatement(clip, active):
    """clip_by_global_norm with Adam(beta2 = 0.98, eps = 1e-9): active (the norm above the clip; at clip = 1e-7 the scaled gradients
    are of epsilon's size, so the weights depend on it) and idle (the norm below the clip: the factor is exactly 1)."""
    opt, scales = _adam_case("S2PNM", clip)
    assert (opt.last_norm > clip) == active
    if active:
        assert max(scales) < 1.0 and len(set(scales)) == len(scales), scales      # active, and a different factor in every step
    else:
        assert scales == [1.0] * len(scales)


@pytest.mark.parametrize("n", [1000, 100003])
def test_clip_by_global_norm_against_the_definition(n):
    """ops.clip_by_global_norm on a random arena: g * clip / max(||g||, clip); bit-exact when the norm is below the clip."""
    from easydgl_amd import ops
    g = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(n))
    norm = float(g.double().norm())
    for clip in (0.25 * norm, 1e-3, 5.0):
        x = g.clone()
        ops.clip_by_global_norm(x, clip)
        want = g.double() * (clip / max(norm, clip))
        assert float((x.double() - want).abs().max()) <= 2e-6 * float(want.abs().max()), clip
    for clip in (1.5 * norm, 1e9):
        x = g.clone()
        ops.clip_by_global_norm(x, clip)
        assert torch.equal(_bits(x), _bits(g)), clip


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_eval_step_metrics_equal_the_restatement(kind):
    prob = _problem(kind, 21, B=64)
    d = prob["dims"]
    for b in range(64):                 # the label is an unseen item (a seen one is masked out of the ranking altogether)
        unseen = sorted(set(range(1, d["I"])) - set(prob["feats"]["seqs_i"][b].tolist()))
        prob["tokens"][b, -1] = unseen[b % len(unseen)]
    m = _model(prob, "f32")
    feats = to_dev(prob["feats"])
    m.reset_metrics()
    m.eval_step(feats, torch.as_tensor(prob["tokens"]).cuda(), mask_seen=True, by_rank=True)
    want = KINDS[kind]["elog"](_p64(prob), prob["feats"], d["C"], d["h"], d["nb"]).detach().numpy()
    ref = SR.ranking_metrics(want, prob["feats"]["seqs_i"], prob["tokens"][:, -1])
    got = m.metrics()
    for k, v in ref.items():
        assert abs(got[k] - v) < 1e-5, (k, got[k], v)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_sampled_losses_match_the_candidate_reference(kind):
    prob = _problem(kind, 31, B=6)
    d = prob["dims"]
    m = _model(prob, "f32", l2_reg=0.0)
    feats = to_dev(prob["feats"])
    labels = torch.as_tensor(prob["tokens"][:, 1:].copy()).cuda()
    lab = prob["tokens"][:, 1:].reshape(-1)
    rng = np.random.default_rng(1)
    _, aux = _ref_loss(prob, _p64(prob), 0.0)
    rows = aux["rows"].detach().numpy()
    tab, bias = prob["params"][f"{kind}/item_embs/lookup_table"], prob["params"][f"{kind}/output_bias"]
    cand = rng.integers(1, d["I"], size=(lab.shape[0], 8)).astype(np.int32)
    with torch.no_grad():
        got = float(m.train_loss(feats, labels, candidates=torch.tensor(cand).cuda()))
        want = CE.reference(rows, tab, bias, cand, lab)["loss"]
        assert abs(got - want) <= LOSS_TOL["f32"] * abs(want), (got, want)
        shared = rng.choice(np.arange(1, d["I"]), size=12, replace=False).astype(np.int32)
        got = float(m.train_loss(feats, labels, shared=torch.tensor(shared).cuda()))
        want = CE.reference(rows, tab, bias, np.broadcast_to(shared, (lab.shape[0], 12)), lab)["loss"]
        assert abs(got - want) <= LOSS_TOL["f32"] * abs(want), (got, want)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_deterministic_three_steps_twice_give_the_same_bits(kind):
    arenas = []
    for _ in range(2):
        prob = _problem(kind, 41, B=8)
        m = _model(prob, "bf16", deterministic=True)
        assert m.deterministic is True
        feats = to_dev(prob["feats"])
        labels = torch.as_tensor(prob["tokens"][:, 1:].copy()).cuda()
        for _ in range(3):
            m.train_step(feats, labels)
        m.settle_state()
        arenas.append((m._arena.detach().clone(), m._adam_m.clone(), m._adam_v.clone()))
    for x, y in zip(*arenas):
        assert torch.equal(_bits(x), _bits(y))


def test_s2pnm_graphed_step_replayed_twice_equals_two_eager_steps():
    prob = _problem("S2PNM", 51, B=8)
    feats = to_dev(prob["feats"])
    labels = torch.as_tensor(prob["tokens"][:, 1:].copy()).cuda()
    eager = _model(prob, "f32", deterministic=True)
    eager.clip_norm = 0.05                                    # clipping active: the scale is a device scalar, no host read
    for _ in range(3):
        eager.train_step(feats, labels)
    graphed = _model(prob, "f32", deterministic=True)
    graphed.clip_norm = 0.05
    step = graphed.graphed_train_step(feats, labels, warmup=1)     # (the warm-up step is a real optimizer step)
    for _ in range(2):
        step(feats, labels)
    torch.cuda.synchronize()
    assert torch.equal(_bits(eager._arena), _bits(graphed._arena))


@pytest.mark.parametrize("model_name", sorted(KINDS))
def test_driver_runs_one_epoch(tmp_path, model_name):
    from easydgl_amd import data as D
    from easydgl_amd import formats as F
    from easydgl_amd import train as TR
    num_items, seqslen = 300, 20
    ids, ts = D.synthetic_batch(num_items, seqslen, 200, seed=3)

    def dump(name, lo, hi):
        F.write_tfrecord(str(tmp_path / name), [F.encode_example({"seqs_i": ids[i], "seqs_t": ts[i]}) for i in range(lo, hi)])
    dump("train000.tfrec", 0, 140); dump("validation.tfrec", 140, 170); dump("test.tfrec", 170, 200)
    res = TR.main(["--model", model_name, "--train", str(tmp_path / "train*.tfrec"), "--valid", str(tmp_path / "validation.tfrec"),
                   "--test", str(tmp_path / "test.tfrec"), "--num_items", str(num_items), "--num_units", "32", "--num_heads", "2",
                   "--num_blocks", "1", "--seqslen", str(seqslen), "--batch_size", "64", "--num_epochs", "1", "--learning_rate",
                   "1e-3", "--l2_reg", "1e-4", "--hidden_dropout_rate", "0.1", "--attention_probs_dropout_rate", "0.1",
                   "--mask_seen", "--dtype", "bf16", "--ckpt_dir", str(tmp_path / "ckpt")])
    assert set(res) == {"H10", "H50", "H100", "N10", "N50", "N100"}
    assert all(0.0 <= v <= 1.0 and math.isfinite(v) for v in res.values())
    assert res["H10"] <= res["H50"] <= res["H100"]
