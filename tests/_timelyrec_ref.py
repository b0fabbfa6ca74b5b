"""TEST INFRASTRUCTURE — float64 restatement (torch on the CPU, autograd) of the reference's TimelyREC, written from the reference
sources:

  TimelyREC            src/model/TimelyREC.py:20-173 (timeslot :57-77, the user branch :79-101, the combination :126-135, the head
                       :149-155, the training-time logit bias :162-172)
  MATEncoder           src/module/sequential.py:210-237
  TAHEncoder           src/module/sequential.py:240-265
  TimeSinusoidCoding   src/module/coding.py:125-149

plus MultiHeadAttention / LayerNorm / FeedForward / the all-position loss / Adam from tests/_seq_baselines_ref.py.  The slots are
materialised the way the reference does it: [B,T,2,W] indices, a [B,T,W,C] lookup summed over the pair, a cumsum on axis 1.  Dropout
off.  Nothing here imports the package under test."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from tests import _seq_baselines_ref as SR

RANGES = {"month": 12, "day": 31, "weekday": 7, "hour": 24}
OFFSET = {"month": 1, "day": 1, "weekday": 0, "hour": 0}
MATE_SCOPE = {"month": "month_mate", "day": "daymate", "weekday": "weekday_mate", "hour": "hour_mate"}
U_SCOPE = "TimelyREC/attention/TimelyREC/"      # the user branch runs inside two nested scopes (TimelyREC.py:93-105)


def window_size(maxrange, ratio):                # TimelyREC.py:59
    return max(int(maxrange * ratio + 0.5), 1) + 1


def lookup(tab, idx):
    """tf.nn.embedding_lookup on the GPU: an index outside the table reads zeros."""
    ok = (idx >= 0) & (idx < tab.shape[0])
    return tab[idx.clamp(0, tab.shape[0] - 1)] * ok.unsqueeze(-1).to(tab.dtype)


def timeslot(feature, maxrange, tab, ratio):
    """TimelyREC.py:57-77: feature int64 [B,T] -> (e [B,T,1,C], slots [B,T,W+1,C])."""
    B, T = feature.shape
    W = window_size(maxrange, ratio)
    delta = torch.arange(1, W + 1, dtype=torch.long).reshape(1, 1, W)
    delta = torch.cat([delta, -delta], dim=2)                                    # :60-61
    e = lookup(tab, feature).unsqueeze(2)                                        # :64
    idx = torch.remainder(feature.unsqueeze(-1) + delta, maxrange)               # :66-67 (floor-mod)
    slots = lookup(tab, idx.reshape(B, T, 2, W)).sum(dim=2)                      # :68-69
    slots = torch.cumsum(slots, dim=1)                                           # :70 — the SEQUENCE axis
    den = torch.arange(1, W + 1, dtype=tab.dtype) * 2.0 + 1.0                    # :73
    outs = (e + slots) / den.reshape(1, W, 1)                                    # :72-75
    return e, torch.cat([e, outs], dim=2)                                        # :76


def mat_encoder(queries, keys, users_proj):
    """sequential.py:220-237 after the bias-free dense: queries [B,T,1,C], keys [B,T,W+1,C], users_proj [B,T,C]."""
    C = queries.shape[-1]
    u = users_proj.unsqueeze(2)
    Q, K = queries * u, keys * u
    p = torch.softmax(Q @ K.transpose(2, 3) / (C ** 0.5), dim=-1)                # [B,T,1,W+1]
    return (p @ K).squeeze(2)


def mate(idx, tabs, u, pq, ratio):
    """Steps 2-4 of the model as one function of the op's operands: idx {name: int64 [B,T]} (already shifted), tabs {name: [M,C]},
    u [B,T,4C] (month | day | weekday | hour), pq [B,T,C] -> R [B,T,C]."""
    C = pq.shape[-1]
    periods = []
    for j, name in enumerate(RANGES):
        q, k = timeslot(idx[name], RANGES[name], tabs[name], ratio)
        periods.append(mat_encoder(q, k, u[..., j * C:(j + 1) * C]))
    keys = torch.stack(periods, dim=2)                                           # TimelyREC.py:130-131 [B,T,4,C]
    a = torch.sigmoid(pq.unsqueeze(2) @ keys.transpose(2, 3))                    # :133-134 [B,T,1,4]
    return (a @ keys).squeeze(2)                                                 # :135


def l2_normalize(x, eps=1e-12):                  # tf.nn.l2_normalize: x * rsqrt(max(sum x^2, eps))
    return x * torch.rsqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=eps))


def tahe(queries, keys, histories):              # sequential.py:247-265
    q, k = l2_normalize(queries), l2_normalize(keys)
    S = (1.0 + q @ k.transpose(1, 2)) / 2.0
    T = S.shape[1]
    return (S * torch.tril(torch.ones(T, T, dtype=S.dtype))) @ histories


def time_sinusoid(ts, time_scale, C):
    """coding.py:125-149 on seqs_t / time_scale.  The reference computes the quotients in float32: the argument of sin / cos is
    rounded through float32 twice here as well, the functions themselves are taken in float64."""
    x = (np.asarray(ts, dtype=np.float32) / np.float32(time_scale)).astype(np.float32)
    scale = np.power(10000, np.arange(0, C, 2) * 1.0 / C).astype(np.float32)
    arg = (x[..., None] / scale).astype(np.float32).astype(np.float64)
    out = np.zeros(x.shape + (C,), dtype=np.float64)
    out[..., 0::2], out[..., 1::2] = np.sin(arg), np.cos(arg)
    return torch.tensor(out)


def timelyrec_shapes(I, T, C, ratio=0.2):
    s = {"TimelyREC/item_embs/lookup_table": (I, C), "TimelyREC/output_bias": (I - 1,),
         "TimelyREC/spatial_embs/embedding/lookup_table": (T, C), "TimelyREC/te_weight": ()}
    for name, M in RANGES.items():
        s[f"TimelyREC/{name}_embs/lookup_table"] = (M, C)
        s[f"TimelyREC/mate/{MATE_SCOPE[name]}/dense/kernel"] = (C, C)
    s["TimelyREC/mate/dense/kernel"] = (C, C)
    a = U_SCOPE + "Atttention/"
    s[a + "LayerNorm/gamma"] = s[a + "LayerNorm/beta"] = (2 * C,)
    for nm in ("dense", "dense_1", "dense_2"):
        s[a + f"multihead_attention/{nm}/kernel"], s[a + f"multihead_attention/{nm}/bias"] = (2 * C, C), (C,)
    f = U_SCOPE + "fforward/"
    s[f + "LayerNorm/gamma"] = s[f + "LayerNorm/beta"] = (C,)
    for nm in ("Inner", "Readout"):
        s[f + f"{nm}/kernel"], s[f + f"{nm}/bias"] = (C, C), (C,)
    s[U_SCOPE + "out/LayerNorm/gamma"] = s[U_SCOPE + "out/LayerNorm/beta"] = (C,)
    s["TimelyREC/prediction/dense/kernel"], s["TimelyREC/prediction/dense/bias"] = (3 * C, 2 * C), (2 * C,)
    s["TimelyREC/prediction/dense_1/kernel"], s["TimelyREC/prediction/dense_1/bias"] = (2 * C, C), (C,)
    return s


def init_from_shapes(shapes, rng, perturb=0.05) -> Dict[str, np.ndarray]:
    """glorot matrices; gamma and te_weight start at one, every other vector at zero, all of them moved by `perturb` noise so that
    no path is hidden behind its initial value.  Values are rounded through float32 (what the model under test stores)."""
    p = {}
    for k, sh in shapes.items():
        if len(sh) == 2:
            v = SR.glorot(rng, sh)
        else:
            one = k.endswith("gamma") or k.endswith("te_weight")
            v = (np.ones(sh) if one else np.zeros(sh)) + perturb * rng.standard_normal(sh)
        p[k] = np.asarray(v).astype(np.float32).astype(np.float64)
    return p


L2_KEYS = ("TimelyREC/item_embs/lookup_table", "TimelyREC/spatial_embs/embedding/lookup_table", "TimelyREC/month_embs/lookup_table",
           "TimelyREC/day_embs/lookup_table", "TimelyREC/weekday_embs/lookup_table", "TimelyREC/hour_embs/lookup_table")


def user_branch(p, seqs_i, h):
    """TimelyREC.py:79-101."""
    ids = torch.as_tensor(np.asarray(seqs_i), dtype=torch.long)
    x = SR.zero_padded(p["TimelyREC/item_embs/lookup_table"])[ids]                            # :83 (scale=False)
    x = SR._pos_concat(x, p["TimelyREC/spatial_embs/embedding/lookup_table"])                 # :84
    masks = (ids != 0).to(x.dtype).unsqueeze(-1)
    out = x * masks                                                                           # :92
    a = U_SCOPE + "Atttention/"
    out = SR._attention(p, a + "multihead_attention/", SR.layernorm(out, p[a + "LayerNorm/gamma"], p[a + "LayerNorm/beta"]), out, h)
    f = U_SCOPE + "fforward/"
    out = SR._feed_forward(p, f, SR.layernorm(out, p[f + "LayerNorm/gamma"], p[f + "LayerNorm/beta"])) * masks      # :96-97
    return SR.layernorm(out, p[U_SCOPE + "out/LayerNorm/gamma"], p[U_SCOPE + "out/LayerNorm/beta"])                 # :100


def timelyrec_rows(p, features, C, h, ratio, time_scale):
    """TimelyREC.__call__ up to the rows that are scored: (rows [B,T,C], tcodes [B,T,C])."""
    ids = torch.as_tensor(np.asarray(features["seqs_i"]), dtype=torch.long)
    U = user_branch(p, features["seqs_i"], h)
    idx = {n: torch.as_tensor(np.asarray(features["seqs_" + n]), dtype=torch.long) - OFFSET[n] for n in RANGES}
    tabs = {n: p[f"TimelyREC/{n}_embs/lookup_table"] for n in RANGES}
    u = torch.cat([U @ p[f"TimelyREC/mate/{MATE_SCOPE[n]}/dense/kernel"] for n in RANGES], dim=-1)       # sequential.py:225
    R = mate(idx, tabs, u, U @ p["TimelyREC/mate/dense/kernel"], ratio)                                   # :108-135
    tcodes = time_sinusoid(np.asarray(features["seqs_t"])[:, :-1], time_scale, C)                         # :141
    Hs = SR.zero_padded(p["TimelyREC/item_embs/lookup_table"])[ids] + p["TimelyREC/te_weight"] * tcodes   # :139-142
    Hs = Hs * torch.sign(ids).unsqueeze(2).to(Hs.dtype)                                                   # :145-146
    hist = tahe(R, R, Hs)                                                                                 # :147
    f = torch.cat([U, hist, R], dim=-1)                                                                   # :150
    f = torch.sigmoid(f @ p["TimelyREC/prediction/dense/kernel"] + p["TimelyREC/prediction/dense/bias"])  # :154
    return f @ p["TimelyREC/prediction/dense_1/kernel"] + p["TimelyREC/prediction/dense_1/bias"], tcodes  # :155


def timelyrec_train_loss(p, features, labels, C, h, ratio, time_scale, l2_reg):
    """The training graph, literally: the logits carry the per-row bias te_weight * sum_c out_c tcode_c (:162-172)."""
    out, tcodes = timelyrec_rows(p, features, C, h, ratio, time_scale)
    rows = out.reshape(-1, C)
    bias = (out * tcodes).sum(-1, keepdim=True).reshape(-1, 1)                                            # :162-163
    logits = SR._logits(p, L2_KEYS[0], "TimelyREC/output_bias", rows) + bias * p["TimelyREC/te_weight"]   # :171-172
    return SR.all_position_loss(logits, labels) + SR._l2(p, L2_KEYS, l2_reg), dict(logits=logits, rows=rows)


def timelyrec_eval_logits(p, features, C, h, ratio, time_scale):
    out, _ = timelyrec_rows(p, features, C, h, ratio, time_scale)
    return SR._logits(p, L2_KEYS[0], "TimelyREC/output_bias", out[:, -1])                                 # :168-172
