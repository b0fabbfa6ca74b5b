"""float64 torch restatement of the reference's TGREC (model/TGREC.py, module/temporal.py:204-264, coding.py:97-122,
normalize.py): the time code Phi(dt) is MATERIALISED as [B,T,T,C], with the clamp, and projected with the keys and the values.
Parameters are a dict keyed by the TF variable names."""
import numpy as np
import torch

from tests._seq_baselines_ref import _l2, _logits, all_position_loss, zero_padded

PAD = float(np.float32(-2 ** 32 + 1))
L2_KEYS = ("TGREC/item_embs/lookup_table", "TGREC/pcoding/embedding/lookup_table")


def time_code(t, omega, phi):
    """coding.py:113-122 on TGREC.py:47-50's spans: cos(max(t_q - t_k, 0) w + phi), [B,T,T,C]."""
    dt = (t[:, :, None] - t[:, None, :]).clamp(min=0.0)
    return torch.cos(dt[..., None] * omega + phi)


def tg_core(q, kvx, w_t, omega, phi, ids, t, H, keep=None):
    """temporal.py:219-258 behind the x halves of the projections: q [B,T,C]; kvx [B,T,2C] = x Wk_x + bk | x Wv_x + bv; w_t [C,2C]
    = the time-half rows of Wk | Wv.  `keep` [B,H,T,T] of 0 / 1/(1-rate): a dropout mask."""
    B, T, C = q.shape
    dh = C // H
    code = time_code(t, omega, phi)
    K = (kvx[:, None, :, :C] + code @ w_t[:, :C]).reshape(B, T, T, H, dh)
    V = (kvx[:, None, :, C:] + code @ w_t[:, C:]).reshape(B, T, T, H, dh)
    S = torch.einsum("bqhd,bqkhd->bhqk", q.reshape(B, T, H, dh), K) / dh ** 0.5
    masked = (ids == 0)[:, None, None, :] | torch.triu(torch.ones(T, T, dtype=torch.bool), 1)
    P = torch.softmax(torch.where(masked, torch.full_like(S, PAD), S), -1)
    if keep is not None:
        P = P * keep
    return torch.einsum("bhqk,bqkhd->bqhd", P, V).reshape(B, T, C)


def tg_attention(p, a, x, ids, t, H):
    """TgMultiHeadAttention.__call__ (temporal.py:204-264) with the variables under scope `a`."""
    B, T, C = x.shape
    om, ph = p["TGREC/tcoding/basis_freq"], p["TGREC/tcoding/phase"]
    xq = torch.cat([x, torch.cos(ph).expand(B, T, C)], -1)
    q = xq @ p[a + "dense/kernel"] + p[a + "dense/bias"]
    Wk, Wv = p[a + "dense_1/kernel"], p[a + "dense_2/kernel"]
    kvx = torch.cat([x @ Wk[:C] + p[a + "dense_1/bias"], x @ Wv[:C] + p[a + "dense_2/bias"]], -1)
    o = tg_core(q, kvx, torch.cat([Wk[C:], Wv[C:]], 1), om, ph, ids, t, H)
    y = o @ p[a + "dense_3/kernel"] + p[a + "dense_3/bias"] + xq
    mean = y.mean(-1, keepdim=True)
    var = ((y - mean) ** 2).mean(-1, keepdim=True)
    return p[a + "ln/gamma"] * (y - mean) / torch.sqrt(var + 1e-8) + p[a + "ln/beta"]


def tgrec_shapes(I, T, C, nb):
    s = {"TGREC/item_embs/lookup_table": (I, C), "TGREC/output_bias": (I - 1,), "TGREC/pcoding/embedding/lookup_table": (T, C),
         "TGREC/tcoding/basis_freq": (C,), "TGREC/tcoding/phase": (C,)}
    for i in range(nb):
        pre = f"num_blocks_{i}/"
        a = pre + "attention/TgMultiHeadAttention/"
        for nm in ("dense", "dense_1", "dense_2"):
            s[a + nm + "/kernel"], s[a + nm + "/bias"] = (2 * C, C), (C,)
        s[a + "dense_3/kernel"], s[a + "dense_3/bias"] = (C, 2 * C), (2 * C,)
        s[a + "ln/gamma"] = s[a + "ln/beta"] = (2 * C,)
        s[pre + "dense/kernel"], s[pre + "dense/bias"] = (3 * C, C), (C,)
        s[pre + "dense_1/kernel"], s[pre + "dense_1/bias"] = (C, C), (C,)
    return s


def tgrec_rows(p, features, C, H, nb, time_scale):
    """TGREC.py:40-68 with seqs_t[:, :T]: [B,T,C]."""
    ids = torch.as_tensor(np.asarray(features["seqs_i"]), dtype=torch.long)
    T = ids.shape[1]
    t = torch.as_tensor(np.asarray(features["seqs_t"]), dtype=torch.float64)[:, :T] / time_scale
    x = zero_padded(p[L2_KEYS[0]])[ids] + p[L2_KEYS[1]][:T]
    for i in range(nb):
        pre = f"num_blocks_{i}/"
        att = tg_attention(p, pre + "attention/TgMultiHeadAttention/", x, ids, t, H)
        inner = torch.relu(torch.cat([att, x], -1) @ p[pre + "dense/kernel"] + p[pre + "dense/bias"])
        x = inner @ p[pre + "dense_1/kernel"] + p[pre + "dense_1/bias"]
    return x


def tgrec_train_loss(p, features, labels, C, H, nb, time_scale, l2_reg):
    rows = tgrec_rows(p, features, C, H, nb, time_scale).reshape(-1, C)
    return all_position_loss(_logits(p, L2_KEYS[0], "TGREC/output_bias", rows), labels) + _l2(p, L2_KEYS, l2_reg)


def tgrec_eval_logits(p, features, C, H, nb, time_scale):
    return _logits(p, L2_KEYS[0], "TGREC/output_bias", tgrec_rows(p, features, C, H, nb, time_scale)[:, -1])
