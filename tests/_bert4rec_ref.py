"""float64 torch restatement of BERT4REC, written from the formulas of src/module/sequential.py:111-137 and
src/model/BERT4REC.py: plain matmul / softmax / torch.where, the joint LayerNorm over (T, C) with epsilon 1e-12, erf-GELU."""
import math

import torch

from tests import _seq_baselines_ref as SR

PAD = float(-2 ** 32 + 1)
L2_KEYS = ("BERT4REC/item_embs/lookup_table", "BERT4REC/spatial_embs/embedding/lookup_table")


def bert_attention(qkv, ids, h):
    """qkv [B,T,3C] = Q | K | V, ids [B,T] -> [B,T,C]: per head softmax(where(ids[k] == 0, PAD, Q K^T / sqrt(dh))) V."""
    B, T, C3 = qkv.shape
    C = C3 // 3
    q, k, v = (qkv[:, :, i * C:(i + 1) * C].reshape(B, T, h, C // h).transpose(1, 2) for i in range(3))
    s = q @ k.transpose(2, 3) / math.sqrt(C // h)
    s = torch.where((ids == 0)[:, None, None, :], torch.full_like(s, PAD), s)
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, T, C)


def gelu(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def bert4rec_shapes(I, T, C, nb):
    """TF name -> shape; I = num_items + 2 classes, T = seqslen + 1 positions."""
    s = {L2_KEYS[0]: (I, C), L2_KEYS[1]: (T, C), "BERT4REC/output_bias": (I - 1,),
         "embeddings/LayerNorm/beta": (C,), "embeddings/LayerNorm/gamma": (C,)}
    for i in range(nb):
        pre = f"layer_{i}/"
        for n in "QKV":
            s[pre + f"attention/self/BERTAttention/{n}/kernel"], s[pre + f"attention/self/BERTAttention/{n}/bias"] = (C, C), (C,)
        for scope, (a, b) in (("attention/output/", (C, C)), ("intermediate/", (C, 2 * C)), ("output/", (2 * C, C))):
            s[pre + scope + "dense/kernel"], s[pre + scope + "dense/bias"] = (a, b), (b,)
            if scope != "intermediate/":
                s[pre + scope + "LayerNorm/beta"] = s[pre + scope + "LayerNorm/gamma"] = (C,)
    t = "cls/predictions/transform/"
    s[t + "dense/kernel"], s[t + "dense/bias"], s[t + "LayerNorm/beta"], s[t + "LayerNorm/gamma"] = (C, C), (C,), (C,), (C,)
    return s


def _rows(p, ids, pos, h, nb):
    ln = lambda x, pre: SR.layernorm(x, p[pre + "LayerNorm/gamma"], p[pre + "LayerNorm/beta"])
    dense = lambda x, pre: x @ p[pre + "dense/kernel"] + p[pre + "dense/bias"]
    C = p[L2_KEYS[0]].shape[1]
    x = SR.zero_padded(p[L2_KEYS[0]])[ids] * math.sqrt(C) + p[L2_KEYS[1]][:ids.shape[1]]
    x = ln(x, "embeddings/")
    for i in range(nb):
        pre, a = f"layer_{i}/", f"layer_{i}/attention/self/BERTAttention/"
        qkv = torch.cat([x @ p[a + n + "/kernel"] + p[a + n + "/bias"] for n in "QKV"], -1)
        att = ln(dense(bert_attention(qkv, ids, h), pre + "attention/output/") + x, pre + "attention/output/")
        x = ln(dense(gelu(dense(att, pre + "intermediate/")), pre + "output/") + att, pre + "output/")
    so = ln(gelu(dense(x, "cls/predictions/transform/")), "cls/predictions/transform/")
    return so.gather(1, pos[:, :, None].expand(-1, -1, C)).reshape(-1, C)


def bert4rec_train_loss(p, feats, labels, h, nb, l2_reg):
    ids, pos = torch.as_tensor(feats["seqs_i"]), torch.as_tensor(feats["masked_positions"])
    logits = SR._logits(p, L2_KEYS[0], "BERT4REC/output_bias", _rows(p, ids, pos, h, nb))
    return SR.all_position_loss(logits, labels) + SR._l2(p, L2_KEYS, l2_reg)


def bert4rec_eval_logits(p, feats, h, nb):
    ids = torch.as_tensor(feats["seqs_i"])
    pos = torch.full((ids.shape[0], 1), ids.shape[1] - 1, dtype=torch.int64)
    return SR._logits(p, L2_KEYS[0], "BERT4REC/output_bias", _rows(p, ids, pos, h, nb))
