"""float64 reference of the interval attention (edgl_tiattn_*) on already projected operands, written from the reference's
semantics — TiMultiHeadAttention.__call__ after its dense layers (temporal.py:45-104) with the interval tensor of
TiSASREC.py:49,58-62 — and not from the HIP code: it builds the two [B,T,T,C] gathers the kernel avoids.  Cross-checked against
oracle.baselines_ref.ti_attention in tests/test_cpu_tiattn_ref.py; used by tests/test_gpu_tiattn.py.

    S[q,k]  = (Q[q].K[k] + Q[q].Ktime[bucket[q,k]]) * scale          K, V: the halves of kvp (position tables already added)
    bucket  = int(clip(float32(t[q+1]/time_scale) - float32(t[k]/time_scale), 0, timelen)), a bucket >= tab_rows reads a zero row
    keys with ids == 0 -> PAD; causal: keys k > q -> PAD; softmax;   out = P V + sum_k P[q,k] Vtime[bucket[q,k]] + resid
No query mask (the reference's query mask is the identity for LayerNorm-ed queries; the kernel applies none)."""
import json
import os

import numpy as np
import torch

PAD = float(np.float32(-2 ** 32 + 1))

# the wrong forms tests/test_cpu_tiattn_ref.py runs to show that the inputs tell them from the true form (reference(wrong=...))
WRONG_FORMS = ("no_ktime", "no_vtime", "round", "plus1", "tq", "last_row", "noncausal")

# (B, T, H, dh, timelen, tab_rows) and the timestamp switches of make_inputs: the cases of tests/test_gpu_tiattn.py
CASES = [
    dict(B=1, T=1, H=1, dh=16, timelen=1, tab_rows=1),                     # one key, smallest table, NBp = 16
    dict(B=3, T=16, H=2, dh=16, timelen=15, tab_rows=15),                  # tile-exact T, NBp == timelen + 1, narrow bf16 path
    dict(B=3, T=17, H=2, dh=32, timelen=16, tab_rows=16),                  # tile + 1, NBp = 32 with 15 dead columns, DT = 2
    dict(B=2, T=33, H=8, dh=16, timelen=255, tab_rows=255),                # eight narrow heads, NBp = 256
    dict(B=3, T=37, H=2, dh=64, timelen=40, tab_rows=30, epoch=True),      # tab_rows < timelen, DT = 4, odd T
    dict(B=2, T=16, H=1, dh=128, timelen=16, tab_rows=17),                 # dh = 128; the clipped bucket is a real row
    dict(B=2, T=45, H=2, dh=128, timelen=64, tab_rows=64, days=True),      # dh = 128 over three tiles, every pair on a boundary
    dict(B=1, T=241, H=2, dh=16, timelen=256, tab_rows=256, pad0=True),    # 16th key tile partly filled, LDS above 64 KB
    dict(B=1, T=256, H=1, dh=32, timelen=256, tab_rows=256, epoch=True),   # the host-checked maximum T
    dict(B=2, T=20, H=2, dh=16, timelen=8, tab_rows=8, causal=False),      # the non-causal form (flags = 0)
]
ORDERED_CASES = (1, 4, 5)       # run again with the ordered bins and the slab backward
STRIDED_CASE = 2                # run again with wide row strides inside guarded buffers


def case_id(c):
    sw = "".join("-" + k for k in ("epoch", "days", "pad0") if c.get(k)) + ("" if c.get("causal", True) else "-noncausal")
    return f"B{c['B']}-T{c['T']}-H{c['H']}-dh{c['dh']}-tl{c['timelen']}-rows{c['tab_rows']}{sw}"


def make_inputs(B, T, H, dh, timelen, tab_rows, dtype=torch.float32, seed=0, epoch=False, days=False, pad0=False, causal=True):
    """CPU operands of one case.  Float operands are standard normal (the interval tables scaled by 0.3), rounded to `dtype`:
    the reference widens the SAME values the kernel reads.  The draws do not depend on `dtype`.
    ids: sample 0 starts with max(1, T // 3) paddings, the last sample has a padded key at T - 3 (T > 5), sample 2 is all padding
    (B >= 3).  ts [B, T+1] float32: a cumulative sum of exponential gaps with a mean of 1.5 * timelen / T buckets (the tail of a
    sequence clips); one timestamp lies below its predecessor's predecessor (T > 8: negative gaps clip to bucket 0).
    epoch: 9.5e8 + ..., time_scale 86400.  days: 86400 * n with n near 11000 — exact in float32 (86400 n = 2^7 * 675 n, 675 n <
    2^24), so every difference sits exactly on a bucket boundary.  pad0: left-padded positions carry timestamp 0, as the loader
    writes them (linkpred.py:152-153)."""
    C = H * dh
    g = np.random.default_rng(seed)
    mk = lambda *s, k=1.0: torch.tensor(g.standard_normal(s) * k, dtype=torch.float32).to(dtype)
    o = dict(q=mk(B, T, C), kvp=mk(B, T, 2 * C), resid=mk(B, T, C), d_out=mk(B, T, C), kt=mk(tab_rows, C, k=0.3),
             vt=mk(tab_rows, C, k=0.3))
    ids = g.integers(1, 50, (B, T))
    ids[0, :max(1, T // 3)] = 0
    if T > 5:
        ids[-1, T - 3] = 0
    if B >= 3:
        ids[2, :] = 0
    time_scale = 86400.0 if (epoch or days) else 1.0
    mean = 1.5 * timelen / T
    if days:
        ts = 86400.0 * (11000.0 + np.cumsum(np.floor(g.exponential(mean + 0.5, (B, T + 1))), axis=1))
    else:
        ts = (9.5e8 if epoch else 0.0) + np.cumsum(g.exponential(mean, (B, T + 1)), axis=1) * time_scale
    if T > 8:
        b, j = min(1, B - 1), (2 * T) // 3
        ts[b, j] = ts[b, j - 2] - (1.0 if days else 0.75) * time_scale
    ts = ts.astype(np.float32)
    if pad0:
        ts[:, :T][np.cumsum(ids != 0, axis=1) == 0] = 0.0
    o.update(ids=torch.from_numpy(ids), ts=torch.from_numpy(ts))
    return o, dict(H=H, scale=1.0 / float(dh) ** 0.5, time_scale=time_scale, timelen=timelen, causal=causal)


def buckets(ts, time_scale, timelen, wrong=None):
    """int64 [B,T,T]: bucket[b,q,k], exactly as oracle/baselines_ref.py:204-206 computes it (float32 throughout, truncation)."""
    x = np.asarray(ts, dtype=np.float32) / np.float32(time_scale)
    T = x.shape[1] - 1
    xq = x[:, :T] if wrong == "tq" else x[:, 1:]
    d = np.clip(xq[:, :, None] - x[:, None, :T], np.float32(0), np.float32(timelen))
    assert d.dtype == np.float32
    bk = (np.rint(d) if wrong == "round" else d).astype(np.int64)
    return bk + 1 if wrong == "plus1" else bk


def reference(o, H, scale, time_scale, timelen, causal=True, wrong=None):
    """out, and by autograd d_q / d_kvp / d_ktime / d_vtime for o["d_out"]; W [H*B, T, timelen+1] = the binned probabilities
    W[head*B + b, q, d] = sum_k P[q,k] [bucket[q,k] == d] (the kernel's wbuf; head-major as tattn_common.h get_job lays it out).
    `wrong`: one of WRONG_FORMS — a deliberately wrong restatement, for the discrimination test only."""
    assert wrong is None or wrong in WRONG_FORMS
    q, kvp, kt, vt = (o[k].double().clone().requires_grad_(True) for k in ("q", "kvp", "kt", "vt"))
    ids = o["ids"]
    B, T, C = q.shape
    dh, rows = C // H, kt.shape[0]
    bk = torch.from_numpy(buckets(o["ts"].numpy(), time_scale, timelen, wrong))
    zero = torch.zeros(1, C, dtype=torch.float64)
    idx = torch.clamp(bk, max=rows - 1 if wrong == "last_row" else rows)       # a bucket >= tab_rows looks up the zero row
    Kg, Vg = torch.cat([kt, zero])[idx], torch.cat([vt, zero])[idx]            # [B,T,T,C]
    masked = (ids == 0)[:, None, :].expand(B, T, T)
    if causal and wrong != "noncausal":
        masked = masked | ~torch.tril(torch.ones(T, T, dtype=torch.bool))[None]
    W = torch.zeros(H * B, T, timelen + 1, dtype=torch.float64)
    heads = []
    for hd in range(H):
        sl = slice(hd * dh, (hd + 1) * dh)
        S = q[:, :, sl] @ kvp[:, :, sl].transpose(1, 2)
        if wrong != "no_ktime":
            S = S + torch.einsum("bqd,bqkd->bqk", q[:, :, sl], Kg[..., sl])
        S = torch.where(masked, torch.full_like(S, PAD), S * scale)
        P = torch.softmax(S, -1)
        oh = P @ kvp[:, :, C + hd * dh:C + (hd + 1) * dh]
        if wrong != "no_vtime":
            oh = oh + torch.einsum("bqk,bqkd->bqd", P, Vg[..., sl])
        heads.append(oh)
        W[hd * B:(hd + 1) * B].scatter_add_(2, torch.clamp(bk, max=timelen), P.detach())
    out = torch.cat(heads, -1) + o["resid"].double()
    out.backward(o["d_out"].double())
    grad = lambda t: torch.zeros_like(t) if t.grad is None else t.grad         # (a wrong form that drops a table never reads it)
    return dict(out=out.detach(), d_q=q.grad, d_k=kvp.grad[:, :, :C], d_v=kvp.grad[:, :, C:], d_ktime=grad(kt), d_vtime=grad(vt), W=W)


# ---- bounds: (relative L2, max-abs-error / max-abs-reference) per tensor ----------------------------------------------------------
FORWARD, GRADS = ("out", "wbuf"), ("d_q", "d_k", "d_v", "d_ktime", "d_vtime")
F32_BOUNDS = {**{k: (1e-4, 1e-4) for k in FORWARD}, **{k: (1e-3, 1e-3) for k in GRADS}}       # tests/_util.py GRAD_TOL["f32"]


def bounds(mode):
    """f32: the project's kernel-level bounds.  bf16: tests/golden/tiattn_bf16_bounds.json — 2 x the errors measured on the GPU
    against this reference, under the caps tests/golden/make_tiattn_bounds.py states."""
    if mode == "f32":
        return dict(F32_BOUNDS)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiattn_bf16_bounds.json")
    tab = json.load(open(path))["bounds"]
    return {k: tuple(tab[k]) for k in FORWARD + GRADS}
