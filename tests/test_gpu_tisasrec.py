"""SURVEY §8 row a-15 (config 5): the TiSASRec model class — and through it the interval-bucket attention kernels (edgl_tiattn_*)
— against oracle/baselines_ref.py (float64).  The kernels themselves, through the C ABI at their edge shapes against a float64
reference on their own operands: tests/test_gpu_tiattn.py.  Tolerances: f32 path 1e-4 / 1e-3 (gradients); bf16 path 3e-2 / max-norm 1e-1 AND relative L2 8e-2 per gradient tensor."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import baselines_ref as BR
from oracle import easydgl_oracle as O
from tests._util import assert_close, grad_errors, regressive_bf16_bounds, rel_err, relu_flip_err, to_dev

# per-tensor relative L2 bound of the bf16 path beside the max-norm bound `gtol`.  These models gate their feed-forward with a
# ReLU: a pre-activation within bf16 rounding of 0 flips its mask against the fp64 reference, and the flipped unit's whole
# contribution then travels to every gradient upstream of it (measured: up to 0.058 in the first block of the two-block
# cases, 0.02-0.03 elsewhere; the GELU-gated EasyDGL path holds 2e-2: tests/_util.py GRAD_TOL)
BF16_GRAD_L2 = 8e-2

pytestmark = pytest.mark.gpu

CASES = [
    dict(B=24, T=12, C=32, h=2, I=60, nb=2, timelen=16),
    dict(B=8, T=30, C=64, h=2, I=300, nb=1, timelen=50),        # dh = 32
    dict(B=4, T=100, C=128, h=8, I=2000, nb=2, timelen=256),     # runme.sh:88-96 shape (8 heads, 2 blocks, timelen 256)
    dict(B=4, T=30, C=512, h=8, I=700, nb=2, timelen=256),       # the published recipe runme.sh:89-96 itself (dh = 64, seqslen 30)
    dict(B=32, T=30, C=50, h=1, I=300, nb=3, timelen=256),        # the reference's DEFAULT flags (main.py:35-44): head dim 50, zero-padded to 64
    dict(B=24, T=20, C=100, h=2, I=120, nb=1, timelen=40),       # two padded heads (50 -> 64 each)
]


def _problem(seed, B, T, C, h, I, nb, timelen, time_scale=3600.0 * 24):
    rng = np.random.default_rng(seed)
    params = {}
    for k, v in BR.tisasrec_init_params(I, timelen, C, nb, rng).items():
        if v.ndim == 1:
            v = v + 0.05 * rng.standard_normal(v.shape)
        params[k] = v.astype(np.float32).astype(np.float64)
    tokens = rng.integers(1, I, size=(B, T + 1))
    tokens[0, :T // 3] = 0
    tokens[1, :1] = 0
    # mean gap of a few buckets; the tail of each sequence reaches past `timelen` buckets so the clip (and the zero row) is hit
    ts = (9.5e8 + np.cumsum(rng.exponential(timelen / T * 1.5 * time_scale, size=(B, T + 1)), axis=1)).astype(np.float32)
    ts[tokens == 0] = 0.0
    feats = {"seqs_i": tokens[:, :-1].copy(), "seqs_t": ts}
    return dict(params=params, feats=feats, tokens=tokens, kw=dict(C=C, h=h, nb=nb, time_scale=time_scale, timelen=timelen),
                dims=dict(B=B, T=T, C=C, h=h, I=I, nb=nb, timelen=timelen))


def _model(prob, mode, l2_reg=1e-3, hidden_drop=0.0, att_drop=0.0, lr=1e-3):
    import easydgl_amd
    d = prob["dims"]
    F = SimpleNamespace(model="TiSASREC", num_items=d["I"], num_units=d["C"], num_heads=d["h"], num_blocks=d["nb"], seqslen=d["T"],
                        timelen=d["timelen"], time_scale=prob["kw"]["time_scale"], learning_rate=lr, l2_reg=l2_reg,
                        hidden_dropout_rate=hidden_drop, attention_probs_dropout_rate=att_drop, compute_dtype=mode,
                        num_train_steps=None, num_warmup_steps=None)
    m = easydgl_amd.ranking(F).finalize("cuda")
    m.load_tf_variables(prob["params"])
    return m


def _p64(prob):
    return {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in prob["params"].items()}


@pytest.mark.parametrize("mode,ltol,gtol", [("f32", 1e-4, 1e-3), ("bf16", 3e-2, 1e-1)])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_tisasrec_forward_loss_and_gradients(mode, ltol, gtol, case):
    prob = _problem(80 + case, **CASES[case])
    m = _model(prob, mode)
    feats = to_dev(prob["feats"])
    labels_np = prob["tokens"][:, 1:].copy()
    labels = torch.as_tensor(labels_np).cuda()
    p64 = _p64(prob)
    logits = m(feats, True)
    ref_loss, aux = BR.tisasrec_train_loss(p64, prob["feats"], labels_np, l2_reg=1e-3, **prob["kw"])
    assert logits.shape == aux["logits"].shape
    assert_close(logits.detach().float().cpu().numpy(), aux["logits"].detach().numpy(), ltol, "train logits")
    assert float((logits.detach()[:, 0] + 1000).abs().max()) == 0.0
    m.zero_grad_arena()
    loss = m.train_loss(feats, labels)
    loss.backward()
    ref_loss.backward()
    assert_close(loss.item(), ref_loss.item(), ltol, "train loss")
    got = m.tf_gradients()
    assert set(got) == set(p64)
    bad, errs = {}, {}
    for name, g in got.items():
        ref = p64[name].grad.numpy()
        # bf16: per tensor class, <= 2 x the measured errors (tests/_util.py regressive_bf16_bounds); f32: gtol on everything
        l2_tol, g_tol = regressive_bf16_bounds("tisasrec", name, gtol, BF16_GRAD_L2) if mode == "bf16" else (BF16_GRAD_L2, gtol)
        if name.endswith("timeinterval/dense_1/bias"):   # a bias on K shifts a whole score row: its true gradient is zero
            ref_k = p64[name.replace("bias", "kernel")].grad.numpy()
            assert np.abs(ref).max() < 1e-12 * max(np.abs(ref_k).max(), 1e-30)
            e = float(np.abs(g).max() / np.abs(ref_k).max())
        else:
            e = rel_err(g, ref)
            # bf16: the max-norm bound alone lets every small entry of a tensor be wrong — a relative-L2 bound beside it
            # (the ReLU-gated Inner tensors are held by relu_flip_err's own rms bound instead)
            if mode == "bf16" and "/Inner/" not in name and grad_errors(g, ref)[0] > l2_tol:
                bad[name + " (rel-L2)"] = grad_errors(g, ref)[0]
        if mode == "bf16" and "/Inner/" in name:   # ReLU mask flips, see tests/_util.py:relu_flip_err
            e = relu_flip_err(g, ref, gtol)
        errs[f"{mode}:{name}"] = (grad_errors(g, ref)[0] if np.any(ref) else 0.0, e)
        if e > g_tol:
            bad[name] = (e, g_tol)
    from tests._util import dump_errors
    dump_errors("tisasrec", errs)
    assert not bad, f"gradient mismatch (rel to max |ref|): {bad}"
    elog = m(feats, False)
    want = BR.tisasrec_eval_logits(_p64(prob), prob["feats"], **prob["kw"])
    assert_close(elog.detach().float().cpu().numpy(), want.detach().numpy(), ltol, "eval logits")


def test_tisasrec_buckets_cover_the_clip_and_the_zero_row():
    """The synthetic timestamps must exercise bucket 0, interior buckets and the clipped bucket `timelen` (zero row)."""
    prob = _problem(80, **CASES[0])
    ts32 = prob["feats"]["seqs_t"] / np.float32(prob["kw"]["time_scale"])
    d = np.clip(ts32[:, 1:, None] - ts32[:, None, :-1], 0, prob["kw"]["timelen"]).astype(np.int64)
    tril = np.tril(np.ones(d.shape[1:], dtype=bool))
    seen = set(np.unique(d[:, tril]))
    assert 0 in seen and prob["kw"]["timelen"] in seen and len(seen) > 5


def test_tisasrec_adam_steps_dropout_training_and_metrics():
    from oracle import torch_ref as R
    prob = _problem(11, B=5, T=12, C=32, h=2, I=60, nb=2, timelen=16)
    m = _model(prob, "f32")
    p64 = _p64(prob)
    opt = R.TFAdam(p64, 1e-3)
    feats = to_dev(prob["feats"])
    labels_np = prob["tokens"][:, 1:].copy()
    labels = torch.as_tensor(labels_np).cuda()
    for step in range(3):
        got = float(m.train_step(feats, labels))
        ref, _ = BR.tisasrec_train_loss(p64, prob["feats"], labels_np, l2_reg=1e-3, **prob["kw"])
        ref.backward()
        opt.step()
        assert abs(got - float(ref.detach())) <= 2e-4 * abs(float(ref.detach())), (step, got)
    prob = _problem(5, B=32, T=20, C=64, h=4, I=400, nb=2, timelen=32)
    m = _model(prob, "bf16", hidden_drop=0.1, att_drop=0.1, lr=2e-3)
    feats = to_dev(prob["feats"])
    labels = torch.as_tensor(prob["tokens"][:, 1:].copy()).cuda()
    losses = [float(m.train_step(feats, labels)) for _ in range(30)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] - 0.3, losses
    _, idx = m.eval_topk(feats, mask_seen=True)
    got = idx.cpu().numpy()
    m.reset_metrics()
    m.eval_step(feats, torch.as_tensor(prob["tokens"]).cuda())
    per = O.ranking_metrics(got, prob["tokens"][:, -1])
    for k, v in m.metrics().items():
        assert abs(v - per[k].mean()) < 1e-5


def test_tiattn_dropout_gradients_match_central_differences():
    """Same counter-based mask in the forward and both backward kernels: directional derivatives of sum(out * w) wrt q, kv and
    the interval tables against central differences (f32)."""
    from easydgl_amd import ops
    B, T, C, H, timelen = 2, 24, 32, 2, 16
    g = torch.Generator(device="cuda").manual_seed(1)
    mk = lambda *s: torch.randn(*s, device="cuda", generator=g)
    q, kv, resid, w = mk(B, T, C), mk(B, T, 2 * C), mk(B, T, C), mk(B, T, C)
    posK, posV, kt, vt = mk(T, C) * 0.3, mk(T, C) * 0.3, mk(timelen, C) * 0.3, mk(timelen, C) * 0.3
    ids = torch.randint(1, 9, (B, T), device="cuda")
    ids[0, :5] = 0
    ts = torch.cumsum(torch.rand(B, T + 1, device="cuda", generator=g) * 2.0, dim=1).float()
    rng = torch.tensor([99, 3], dtype=torch.int64, device="cuda")
    drop = ops.Drop(0.25, rng, 5)

    def run(q_, kv_, kt_, vt_):
        return ops.TiAttnFn.apply(q_, kv_, resid, posK, posV, kt_, vt_, kt_, vt_, ids, ts, H, 1.0, timelen, drop)

    leaves = [t.clone().requires_grad_(True) for t in (q, kv, kt, vt)]
    out = run(*leaves)
    (out * w).sum().backward()
    base = [q, kv, kt, vt]
    for i, name in enumerate(("q", "kv", "ktime", "vtime")):
        d = torch.randn(base[i].shape, device="cuda", generator=g)
        eps = 1e-2
        args_p = [t.clone() for t in base]
        args_m = [t.clone() for t in base]
        args_p[i] += eps * d
        args_m[i] -= eps * d
        with torch.no_grad():
            fd = float(((run(*args_p).double() - run(*args_m).double()) * w.double()).sum()) / (2 * eps)
        an = float((leaves[i].grad.double() * d.double()).sum())
        assert abs(fd - an) <= 2e-2 * max(1.0, abs(an)), (name, fd, an)
