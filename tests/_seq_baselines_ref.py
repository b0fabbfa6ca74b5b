"""TEST INFRASTRUCTURE — float64 restatement (torch on the CPU, autograd) of the reference's time-independent baselines, written
from the reference sources:

  MultiHeadAttention  src/module/sequential.py:16-83
  SASRec              src/model/SASREC.py:20-75
  S2PNM               src/model/S2PNM.py:21-90, the GRU in cuDNN's form (compat/cudnn_rnn.py: CudnnGRU, linear input, zero initial
                      state), Adam(beta2 = 0.98, eps = 1e-9) behind clip_by_global_norm(5) (compat/extender.py)

plus LayerNorm / FeedForward / the all-position loss (src/model/Base.py:12-140) and PositionCoding's concatenation
(src/module/coding.py:72-79).  Dropout off.  Nothing here imports the package under test."""
from __future__ import annotations

import math
from typing import Dict

import numpy as np
import torch

PAD = float(np.float32(-2 ** 32 + 1))       # sequential.py:54: the value a masked score is REPLACED by


def glorot(rng, shape):
    lim = math.sqrt(6.0 / (shape[0] + shape[1]))
    return rng.uniform(-lim, lim, size=shape)


def layernorm(x, gamma, beta, eps=1e-12):    # Base.py:12-67: moments over every axis but the batch's (begin_norm_axis=1)
    axes = tuple(range(1, x.dim()))
    mean = x.mean(dim=axes, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=axes, keepdim=True)
    return (x - mean) * torch.rsqrt(var + eps) * gamma + beta


def zero_padded(tab):                        # coding.py:56-57
    return torch.cat([torch.zeros_like(tab[:1]), tab[1:]], dim=0)


# ---- GRU (cuDNN form) ----------------------------------------------------------------------------------------------------
def gru_seq(xp, R, bR):
    """h [B,T,C] from the input-side pre-activations xp [B,T,3C] = x W + b_W (gate blocks r | z | n), R [C,3C], b_R [3C]:
        r = s(xp_r + h R_r + b_Rr)   z = s(xp_z + h R_z + b_Rz)   n = tanh(xp_n + r * (h R_n + b_Rn))   h' = (1 - z) n + z h
    zero initial state; every position is a step (padding is not skipped)."""
    B, T, C3 = xp.shape
    C = C3 // 3
    h = torch.zeros(B, C, dtype=xp.dtype)
    out = []
    for t in range(T):
        hp = h @ R + bR
        r = torch.sigmoid(xp[:, t, :C] + hp[:, :C])
        z = torch.sigmoid(xp[:, t, C:2 * C] + hp[:, C:2 * C])
        n = torch.tanh(xp[:, t, 2 * C:] + r * hp[:, 2 * C:])
        h = (1 - z) * n + z * h
        out.append(h)
    return torch.stack(out, dim=1)


def gru(x, W, bW, R, bR):
    return gru_seq(x @ W + bW, R, bR)


# ---- MultiHeadAttention ---------------------------------------------------------------------------------------------------
def multihead_attention(queries, keys, Wq, bq, Wk, bk, Wv, bv, h, causal=True, keep=None):
    """sequential.py:29-83.  The key mask is read off the keys themselves (:50), as the reference does; a masked score is replaced
    by -2^32+1, so a row without a visible key is uniform over all keys.  `keep` ([h*B,T,T] of 0 / 1/(1-rate)): a dropout mask."""
    Q, K, V = queries @ Wq + bq, keys @ Wk + bk, keys @ Wv + bv
    C = Q.shape[-1]
    split = lambda x: torch.cat(torch.split(x, C // h, dim=2), dim=0)             # :39-41
    Q_, K_, V_ = split(Q), split(K), split(V)
    S = Q_ @ K_.transpose(1, 2) / ((C // h) ** 0.5)                               # :44-47
    hN, T, _ = S.shape
    km = torch.sign(keys.sum(-1).abs()).repeat(h, 1).unsqueeze(1).expand(hN, T, T)   # :50-52
    S = torch.where(km == 0, torch.full_like(S, PAD), S)                          # :54-55
    if causal:
        tril = torch.tril(torch.ones(T, T, dtype=S.dtype)).unsqueeze(0).expand(hN, T, T)
        S = torch.where(tril == 0, torch.full_like(S, PAD), S)                    # :58-63
    P = torch.softmax(S, -1)                                                      # :66
    if keep is not None:
        P = P * keep                                                              # :69
    out = P @ V_
    out = torch.cat(torch.split(out, out.shape[0] // h, dim=0), dim=2)            # :75
    return out + queries[:, :, :C]                                                # :78


def _attention(p, a, queries, keys, h, causal=True):
    return multihead_attention(queries, keys, p[a + "dense/kernel"], p[a + "dense/bias"], p[a + "dense_1/kernel"],
                               p[a + "dense_1/bias"], p[a + "dense_2/kernel"], p[a + "dense_2/bias"], h, causal)


def _feed_forward(p, pre, y):                # Base.py:70-87
    inner = torch.relu(y @ p[pre + "Inner/kernel"] + p[pre + "Inner/bias"])
    return inner @ p[pre + "Readout/kernel"] + p[pre + "Readout/bias"] + y


def _pos_concat(x, pos_tab):                 # coding.py:72-79
    B, T, _ = x.shape
    return torch.cat([x, pos_tab[:T].unsqueeze(0).expand(B, T, -1)], dim=-1)


def _logits(p, table_key, bias_key, rows):   # Base.py:106-110, SASREC.py:73-74
    bias = torch.cat([torch.full((1,), -1000.0, dtype=rows.dtype), p[bias_key]])
    return rows @ zero_padded(p[table_key]).t() + bias


def all_position_loss(logits, labels):       # Base.py:119-130
    lp = torch.log(torch.softmax(logits, -1) + 1e-5)
    lab = torch.as_tensor(np.asarray(labels).reshape(-1), dtype=torch.long)
    w = (lab != 0).to(logits.dtype)
    per = -lp[torch.arange(lab.shape[0]), lab]
    return (w * per).sum() / (w.sum() + 1e-5)


def _l2(p, keys, l2_reg):
    return sum(l2_reg * 0.5 * (p[k] ** 2).sum() for k in keys) if l2_reg else 0.0


# ---- SASRec ---------------------------------------------------------------------------------------------------------------
def sasrec_shapes(I, T, C, nb):
    s = {"SASREC/item_embs/lookup_table": (I, C), "SASREC/spatial_embs/embedding/lookup_table": (T, C),
         "SASREC/output_bias": (I - 1,), "output_ln/LayerNorm/gamma": (C,), "output_ln/LayerNorm/beta": (C,)}
    for i in range(nb):
        pre, cin = f"num_blocks_{i}/", (2 * C if i == 0 else C)
        s[pre + "attention/LayerNorm/gamma"] = s[pre + "attention/LayerNorm/beta"] = (cin,)
        for nm in ("dense", "dense_1", "dense_2"):
            s[pre + f"attention/multihead_attention/{nm}/kernel"] = (cin, C)
            s[pre + f"attention/multihead_attention/{nm}/bias"] = (C,)
        s[pre + "feedforward/LayerNorm/gamma"] = s[pre + "feedforward/LayerNorm/beta"] = (C,)
        for nm in ("Inner", "Readout"):
            s[pre + f"feedforward/{nm}/kernel"], s[pre + f"feedforward/{nm}/bias"] = (C, C), (C,)
    return s


def init_from_shapes(shapes, rng, perturb=0.05) -> Dict[str, np.ndarray]:
    """glorot matrices, gamma ones, every other vector zeros; `perturb`: noise on the vectors so that no gradient is trivial.
    Values are rounded through float32 (what the model under test stores)."""
    p = {}
    for k, sh in shapes.items():
        if len(sh) == 2:
            v = glorot(rng, sh)
        else:
            v = (np.ones(sh) if k.endswith("gamma") else np.zeros(sh)) + perturb * rng.standard_normal(sh)
        p[k] = v.astype(np.float32).astype(np.float64)
    return p


SASREC_L2 = ("SASREC/item_embs/lookup_table", "SASREC/spatial_embs/embedding/lookup_table")


def sasrec_encoder(p, seqs_i, C, h, nb):
    ids = torch.as_tensor(np.asarray(seqs_i), dtype=torch.long)
    x = zero_padded(p["SASREC/item_embs/lookup_table"])[ids] * (C ** 0.5)                  # SASREC.py:43
    x = _pos_concat(x, p["SASREC/spatial_embs/embedding/lookup_table"])                    # :44
    masks = (ids != 0).to(x.dtype).unsqueeze(-1)                                           # :50
    out = x * masks                                                                        # :53
    for i in range(nb):
        pre = f"num_blocks_{i}/"
        qn = layernorm(out, p[pre + "attention/LayerNorm/gamma"], p[pre + "attention/LayerNorm/beta"])
        out = _attention(p, pre + "attention/multihead_attention/", qn, out, h)            # :57
        y = layernorm(out, p[pre + "feedforward/LayerNorm/gamma"], p[pre + "feedforward/LayerNorm/beta"])
        out = _feed_forward(p, pre + "feedforward/", y) * masks                            # :60-61
    return layernorm(out, p["output_ln/LayerNorm/gamma"], p["output_ln/LayerNorm/beta"])  # :63-64


def sasrec_train_loss(p, features, labels, C, h, nb, l2_reg):
    out = sasrec_encoder(p, features["seqs_i"], C, h, nb)
    logits = _logits(p, SASREC_L2[0], "SASREC/output_bias", out.reshape(-1, C))
    return all_position_loss(logits, labels) + _l2(p, SASREC_L2, l2_reg), dict(logits=logits, rows=out.reshape(-1, C))


def sasrec_eval_logits(p, features, C, h, nb):
    out = sasrec_encoder(p, features["seqs_i"], C, h, nb)
    return _logits(p, SASREC_L2[0], "SASREC/output_bias", out[:, -1])


# ---- S2PNM ----------------------------------------------------------------------------------------------------------------
GRU_SCOPE = "S2PNM/Reccurency/S2PNM/GRU/opaque_kernel/"      # the opaque cuDNN blob as its twelve canonical parts
GRU_GATES = ("r", "z", "n")


def s2pnm_shapes(I, T, C):
    s = {"S2PNM/item_embs/lookup_table": (I, C), "S2PNM/spatial_embs/embedding/lookup_table": (T, C), "S2PNM/output_bias": (I - 1,)}
    for g in GRU_GATES:      # weights in tf.layers.dense orientation [in, out] (the canonical cuDNN matrices transposed)
        s[GRU_SCOPE + f"w_{g}"], s[GRU_SCOPE + f"r_{g}"] = (C, C), (C, C)
        s[GRU_SCOPE + f"b_w{g}"], s[GRU_SCOPE + f"b_r{g}"] = (C,), (C,)
    s["S2PNM/Attention/LayerNorm/gamma"] = s["S2PNM/Attention/LayerNorm/beta"] = (2 * C,)
    for nm in ("dense", "dense_1", "dense_2"):
        s[f"S2PNM/Attention/multihead_attention/{nm}/kernel"] = (2 * C, C)
        s[f"S2PNM/Attention/multihead_attention/{nm}/bias"] = (C,)
    s["S2PNM/fforward/LayerNorm/gamma"] = s["S2PNM/fforward/LayerNorm/beta"] = (C,)
    for nm in ("Inner", "Readout"):
        s[f"S2PNM/fforward/{nm}/kernel"], s[f"S2PNM/fforward/{nm}/bias"] = (C, C), (C,)
    s["S2PNM/Dictionary/LayerNorm/gamma"] = s["S2PNM/Dictionary/LayerNorm/beta"] = (4 * C,)
    s["S2PNM/Dictionary/dense/kernel"], s["S2PNM/Dictionary/dense/bias"] = (4 * C, 2 * C), (2 * C,)
    s["S2PNM/Dictionary/dense_1/kernel"], s["S2PNM/Dictionary/dense_1/bias"] = (2 * C, C), (C,)
    return s


S2PNM_L2 = ("S2PNM/item_embs/lookup_table", "S2PNM/spatial_embs/embedding/lookup_table")


def s2pnm_rows(p, seqs_i, C, h):
    """S2PNM.__call__ up to the rows that are scored (S2PNM.py:37-66): [B, T, C]."""
    ids = torch.as_tensor(np.asarray(seqs_i), dtype=torch.long)
    x = zero_padded(p["S2PNM/item_embs/lookup_table"])[ids] * (C ** 0.5)                   # :39
    masks = (ids != 0).to(x.dtype).unsqueeze(-1)
    cat = lambda pre: torch.cat([p[GRU_SCOPE + pre + g] for g in GRU_GATES], dim=-1)
    hs = gru(x, cat("w_"), cat("b_w"), cat("r_"), cat("b_r"))                              # :47-49
    u = _pos_concat(hs, p["S2PNM/spatial_embs/embedding/lookup_table"]) * masks            # :52-53
    qn = layernorm(u, p["S2PNM/Attention/LayerNorm/gamma"], p["S2PNM/Attention/LayerNorm/beta"])
    u = _attention(p, "S2PNM/Attention/multihead_attention/", qn, u, h)                    # :57
    y = layernorm(u, p["S2PNM/fforward/LayerNorm/gamma"], p["S2PNM/fforward/LayerNorm/beta"])
    g = _feed_forward(p, "S2PNM/fforward/", y)                                             # :59
    f = layernorm(torch.cat([g, hs, g - hs, g * hs], dim=-1), p["S2PNM/Dictionary/LayerNorm/gamma"],
                  p["S2PNM/Dictionary/LayerNorm/beta"])                                    # :63
    f = torch.sigmoid(f @ p["S2PNM/Dictionary/dense/kernel"] + p["S2PNM/Dictionary/dense/bias"])       # :64
    return f @ p["S2PNM/Dictionary/dense_1/kernel"] + p["S2PNM/Dictionary/dense_1/bias"] + x           # :65-66


def s2pnm_train_loss(p, features, labels, C, h, l2_reg):
    out = s2pnm_rows(p, features["seqs_i"], C, h)
    logits = _logits(p, S2PNM_L2[0], "S2PNM/output_bias", out.reshape(-1, C))
    return all_position_loss(logits, labels) + _l2(p, S2PNM_L2, l2_reg), dict(logits=logits, rows=out.reshape(-1, C))


def s2pnm_eval_logits(p, features, C, h):
    return _logits(p, S2PNM_L2[0], "S2PNM/output_bias", s2pnm_rows(p, features["seqs_i"], C, h)[:, -1])


# ---- Adam (TF form) with clip_by_global_norm --------------------------------------------------------------------------------
class ClippedAdam:
    """tf.train.AdamOptimizer(lr, beta1, beta2, eps) behind clip_by_global_norm(clip): g <- g * clip / max(||g||, clip) over every
    gradient (extender.py:50-54); clip None: plain TF Adam (Base.py:142-144)."""

    def __init__(self, params: Dict[str, torch.Tensor], lr, beta1=0.9, beta2=0.999, eps=1e-8, clip=None):
        self.p, self.lr, self.b1, self.b2, self.eps, self.clip = params, lr, beta1, beta2, eps, clip
        self.m = {k: torch.zeros_like(v) for k, v in params.items()}
        self.v = {k: torch.zeros_like(v) for k, v in params.items()}
        self.t, self.last_norm, self.last_scale = 0, None, 1.0

    @torch.no_grad()
    def step(self):
        self.t += 1
        lr_t = self.lr * math.sqrt(1 - self.b2 ** self.t) / (1 - self.b1 ** self.t)
        scale = 1.0
        if self.clip is not None:
            self.last_norm = math.sqrt(sum(float((w.grad ** 2).sum()) for w in self.p.values() if w.grad is not None))
            scale = self.clip / max(self.last_norm, self.clip)
        for k, w in self.p.items():
            if w.grad is None:
                continue
            g = w.grad * scale
            self.m[k].mul_(self.b1).add_(g, alpha=1 - self.b1)
            self.v[k].mul_(self.b2).addcmul_(g, g, value=1 - self.b2)
            w.sub_(lr_t * self.m[k] / (self.v[k].sqrt() + self.eps))
            w.grad = None
        self.last_scale = scale


# ---- ranking metrics (Base.py:150-207) --------------------------------------------------------------------------------------
def ranking_metrics(logits, seen, labels, ks=(10, 50, 100)):
    """Means of H@k / N@k over the rows: the label's place in the (logit desc, item id asc) order of the unseen catalogue."""
    logits = np.array(logits, dtype=np.float64)
    out = {f"H{k}": 0.0 for k in ks}
    out.update({f"N{k}": 0.0 for k in ks})
    out["MRR"] = 0.0
    B = logits.shape[0]
    for b in range(B):
        row = logits[b].copy()
        row[0] = -np.inf
        row[np.asarray(seen[b])] = -np.inf
        lab = int(labels[b])
        rank = int((row > row[lab]).sum() + ((row == row[lab]) & (np.arange(row.shape[0]) < lab)).sum()) if np.isfinite(row[lab]) else 10 ** 9
        out["MRR"] += 1.0 / (rank + 1) / B
        for k in ks:
            if rank < k:
                out[f"H{k}"] += 1.0 / B
                out[f"N{k}"] += 1.0 / math.log2(rank + 2) / B
    return out
