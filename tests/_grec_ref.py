"""float64 restatement of GREC in plain torch: the dilated convolution with LayerNorm / ReLU as explicit
shift-and-matmul (no conv call), and the model's training loss / evaluation logits from a {TF name: array} dict."""
import math

import torch

EPS = 1e-8


def offsets(fw, d, causal):
    return [-(fw - 1 - j) * d if causal else j * d - ((fw - 1) * d) // 2 for j in range(fw)]


def dconv_ln(x, w, bias, gamma, beta, d, causal, r=None):
    """x [B,T,C], w [fw,C,C] (tap, in, out): z[b,t] = bias + sum_j x[b,t+o_j] @ w[j] (rows outside [0,T) are zero), then
    relu(layernorm(z)) (+ r)."""
    B, T, C = x.shape
    z = bias.expand(B, T, C).clone()
    for j, o in enumerate(offsets(w.shape[0], d, causal)):
        lo, hi = max(0, -o), min(T, T - o)          # the t with 0 <= t + o < T
        if lo < hi:
            z[:, lo:hi] = z[:, lo:hi] + x[:, lo + o:hi + o] @ w[j]
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    y = torch.relu(gamma * (z - mean) / torch.sqrt(var + EPS) + beta)
    return y if r is None else y + r


def grec_shapes(I, C, fw, dilations):
    """TF name -> shape; I = num_items + 2 classes.  The head's bias has no entry for class 0 (model/grec.py)."""
    s = {"GREC/enc_embs/lookup_table": (I, C), "GREC/decc_embs/lookup_table": (I, C),
         "projector/dense/kernel": (C, 2 * C), "projector/dense/bias": (2 * C,),
         "projector/dense_1/kernel": (2 * C, C), "projector/dense_1/bias": (C,),
         "cls/predictions/transform/dense/kernel": (C, I), "cls/predictions/transform/dense/bias": (I - 1,)}
    for scope in ("regudCNN", "maskedCNN"):
        for i in range(len(dilations)):
            for k in (0, 1):
                pre = f"block_{i}/{scope}_{i}/"
                s[pre + f"dconv{k}/weight"], s[pre + f"dconv{k}/bias"] = (fw, C, C), (C,)
                s[pre + f"ln{k}/gamma"], s[pre + f"ln{k}/beta"] = (C,), (C,)
    return s


def _unit(p, pre, x, d, causal):
    y = dconv_ln(x, p[pre + "dconv0/weight"], p[pre + "dconv0/bias"], p[pre + "ln0/gamma"], p[pre + "ln0/beta"], d, causal)
    return dconv_ln(y, p[pre + "dconv1/weight"], p[pre + "dconv1/bias"], p[pre + "ln1/gamma"], p[pre + "ln1/beta"], 2 * d, causal, x)


def _rows(p, ids_enc, ids_dec, pos, dilations):
    x, dec = p["GREC/enc_embs/lookup_table"][ids_enc], p["GREC/decc_embs/lookup_table"][ids_dec]
    for i, d in enumerate(dilations):
        x = _unit(p, f"block_{i}/regudCNN_{i}/", x, d, False)
    inp = x + dec
    h = inp @ p["projector/dense/kernel"] + p["projector/dense/bias"]
    h = 0.5 * h * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (h + 0.044715 * h ** 3)))
    x = h @ p["projector/dense_1/kernel"] + p["projector/dense_1/bias"] + inp
    for i, d in enumerate(dilations):
        x = _unit(p, f"block_{i}/maskedCNN_{i}/", x, d, True)
    rows = torch.relu(torch.gather(x, 1, pos[:, :, None].expand(-1, -1, x.shape[-1])))
    return rows.reshape(-1, x.shape[-1])


def _logits(p, rows):
    out = rows @ p["cls/predictions/transform/dense/kernel"]
    bias = torch.cat([torch.zeros(1, dtype=out.dtype), p["cls/predictions/transform/dense/bias"]])
    out = out + bias
    return torch.cat([torch.full_like(out[:, :1], -1000.0), out[:, 1:]], 1)       # class 0 sits at -1000, in training too


def grec_train_loss(p, feats, labels, dilations):
    """The project's cross-entropy (-log(p + 1e-5), the rows with a label != 0, their sum over (count + 1e-5): Base.py:119-130 as
    every model here states it) + 0.001 * mean_v sum(v^2) / 2 over every variable."""
    ids_m, ids_i, pos = (torch.as_tensor(feats[k]) for k in ("seqs_m", "seqs_i", "masked_positions"))
    logp = torch.log(torch.softmax(_logits(p, _rows(p, ids_m, ids_i, pos, dilations)), -1) + 1e-5)
    lab = torch.as_tensor(labels).reshape(-1)
    w = (lab != 0).double()
    ce = -(logp.gather(1, lab[:, None])[:, 0] * w).sum() / (w.sum() + 1e-5)
    return ce + 0.001 * sum((v ** 2).sum() / 2 for v in p.values()) / len(p)


def grec_eval_logits(p, feats, dilations):
    ids = torch.as_tensor(feats["seqs_i"])
    pos = torch.full((ids.shape[0], 1), ids.shape[1] - 1, dtype=torch.int64)
    out = _logits(p, _rows(p, ids, ids, pos, dilations))
    return torch.cat([out[:, :-1], torch.full_like(out[:, :1], -1000.0)], 1)      # GREC.py:100-102
