"""Mirror of src/model/BERT4REC.py (Sun et al., CIKM'19, as the reference implements it) on the HIP kernels: the bidirectional
baseline EasyDGL was derived from — same masked batches, same post-LayerNorm block, same head transform, with BERT's plain
self-attention (module/sequential.py BERTAttention on csrc/k_battn.hip) where EasyDGL has its modulated one.

    m = BERT4REC(num_items, FLAGS).finalize("cuda")
    logits = m(features, is_training)          # BERT4REC.__call__ (BERT4REC.py:59-129): [B*masklen, I] (train) / [B, I] (eval)
    loss = m.train_loss(features, labels)      # BERT4REC.train (BERT4REC.py:131-139)

I = num_items + 2 classes (BERT4REC.py:44); the MASK token is ``m.mask`` = num_items, so the driver feeds the model EasyDGL's
batches (MAUPostProcessor, dataloader.py:159-206): ``seqs_i`` int64 [B, seqslen + 1] with MASK at the drawn positions (training) or
at the last one (evaluation), ``masked_positions`` [B, masklen]; ``seqs_t`` is not read.

Kept from the reference: the item table is scaled by sqrt(C) with a zero row 0; the position code is ADDED (pcoding.code); the
joint LayerNorm over (T, C) with epsilon 1e-12 (Base.layernorm) in front of the hidden dropout; the loss is the cross-entropy
weighted by ``labels != 0`` over (sum of weights + 1e-5) plus the l2 terms of the two tables; Adam with the defaults; class 0 at
-1000.  The only mask is the key mask ``seqs_i != 0``: padded QUERY rows attend like every other row.

Candidate lists, shared negatives and FLAGS.deterministic come from the shared scaffold unchanged (Sequential._score_ce; the
attention kernels use no f32 atomics, the two tables take the flag).
Not built: channel padding (widths are powers of two in [32, 512] with a head dim of 16 / 32 / 64 / 128), the static TrainEngine,
lazy_adam (refused by the constructor), and in the driver --graph and --device_data (refused there by flag name)."""
from __future__ import annotations

from typing import Dict

import torch
from torch import nn

from .. import ops
from ..module import coding as C
from ..module import sequential as S
from .base import Sequential, _Dense, _LayerNorm
from .sasrec import check_width, specs_from_map


class _Block(nn.Module):
    def __init__(self, C_, heads, att_drop, gen):
        super().__init__()
        self.attention = S.BERTAttention(C_, heads, att_drop, gen)         # layer_i/attention/self/BERTAttention
        self.att_out = _Dense(C_, C_, gen)                                 # layer_i/attention/output/dense
        self.att_ln = _LayerNorm(C_)                                       # layer_i/attention/output/LayerNorm
        self.inter = _Dense(C_, 2 * C_, gen)                               # layer_i/intermediate/dense
        self.out = _Dense(2 * C_, C_, gen)                                 # layer_i/output/dense
        self.out_ln = _LayerNorm(C_)                                       # layer_i/output/LayerNorm


class BERT4REC(Sequential):
    static_engine_ok = False      # (the static TrainEngine is EasyDGL's; this model trains through train_step)

    def __init__(self, num_items, FLAGS):
        super().__init__(num_items, FLAGS)
        self.mask = num_items                      # util.py:108: the driver feeds a model with `mask` EasyDGL's masked batches
        self.seqslen += 1                          # BERT4REC.py:43
        self.num_items += 2                        # :44
        self.masklen = FLAGS.masklen
        self.seed = int(getattr(FLAGS, "seed", 9876))
        gen = torch.Generator().manual_seed(self.seed)
        C_ = self.width_true = self.num_units
        check_width("BERT4REC", C_, self.num_heads)
        if not 1 <= FLAGS.seqslen <= 1024:
            raise ValueError(f"BERT4REC: seqslen={FLAGS.seqslen} unsupported; the HIP kernels take 1 <= seqslen <= 1024 (--seqslen)")
        ops.battn_check(self.seqslen, self.num_heads, C_ // self.num_heads, self.act_dtype, "BERT4REC")
        self.item_embs = C.Embedding(self.num_items, C_, self.l2_reg, zero_pad=True, scale=True, gen=gen,
                                     deterministic=self.deterministic)                                    # :48-49
        self.pcoding = C.PositionCoding(self.seqslen, C_, self.l2_reg, gen=gen)                           # :50
        self.pcoding.pembs.deterministic = self.deterministic
        self.output_bias = self.make_output_bias()                                                        # :51
        self.emb_ln = _LayerNorm(C_)                                                                      # embeddings/LayerNorm
        self.layers = nn.ModuleList(_Block(C_, self.num_heads, self.attention_probs_dropout_rate, gen)
                                    for _ in range(FLAGS.num_blocks))                                     # :53-57
        self.transform = _Dense(C_, C_, gen)                                                              # cls/predictions/transform/dense
        self.transform_ln = _LayerNorm(C_)                                                                # .../LayerNorm

    def _pad_specs(self):
        return specs_from_map(self._tf_map())

    def l2_param_names(self):
        return ["item_embs.lookup_table", "pcoding.pembs.lookup_table"]

    def _negatives_hi(self) -> int:
        return self.mask      # (the MASK row and the class behind it are not items)

    def encoder(self, features, is_training, gather_pos):
        """BERT4REC.py:59-124: the head's rows at gather_pos [B, M] -> [B*M, C]."""
        ids = features["seqs_i"].contiguous()
        hd = self.hidden_dropout_rate
        emb = self.item_embs(ids)                                                                          # :63
        if emb.dtype != self.act_dtype:
            emb = emb.to(self.act_dtype)
        x = ops.AddLayerNormFn.apply(emb, self.pcoding.code(ids).to(self.act_dtype), self.emb_ln.gamma, self.emb_ln.beta,
                                     ops.NO_DROP, None)                                                    # :68-69
        x = ops.dropout(x, self._drop(hd, 1, is_training))                                                 # :70
        for i, blk in enumerate(self.layers):
            att = blk.attention(x, x, ids, is_training,
                                drop=self._drop(self.attention_probs_dropout_rate, 10 + 4 * i, is_training))   # :90
            att = self._linear(att, blk.att_out)                                                           # :95
            att = ops.AddLayerNormFn.apply(att, x, blk.att_ln.gamma, blk.att_ln.beta, self._drop(hd, 11 + 4 * i, is_training),
                                           None)                                                           # :96-98
            inter = self._linear(att, blk.inter, True)                                                     # :102-103
            out = self._linear(inter, blk.out)                                                             # :107
            x = ops.AddLayerNormFn.apply(out, att, blk.out_ln.gamma, blk.out_ln.beta, self._drop(hd, 12 + 4 * i, is_training),
                                         None)                                                             # :108-110
        so = self._linear(x, self.transform, True)                                                         # :116
        return ops.AddLayerNormFn.apply(so, None, self.transform_ln.gamma, self.transform_ln.beta, ops.NO_DROP,
                                        gather_pos.contiguous())                                           # :117-124

    def _gather_pos(self, features, is_training):
        return features["masked_positions"] if is_training else self._last_pos(features["seqs_i"])

    def forward(self, features: Dict[str, torch.Tensor], is_training: bool):
        rows = self.encoder(features, is_training, self._gather_pos(features, is_training))
        tab = self.item_embs.lookup_table
        return ops.ScoreLogitsFn.apply(rows, tab, self.output_bias, self.compute(tab))                     # :127-129

    def train_loss(self, features, labels, *, candidates=None, shared=None):
        """BERT4REC.train (BERT4REC.py:131-139) with the fused scoring / cross-entropy (no [B*M, I] tensor); `candidates` /
        `shared` as in the other models (Sequential._score_ce)."""
        rows = self.encoder(features, True, features["masked_positions"])
        loss = self._score_ce(rows, labels.reshape(-1).contiguous(), candidates, shared)
        if self.l2_reg != 0.0:
            for n in self.l2_param_names():
                loss = loss + ops.L2Fn.apply(self.get_parameter(n), self.l2_reg)
        return loss

    # ---- interop with the reference's variable naming (tests / checkpoints converted from TF) ------------------------
    def _tf_map(self):
        """TF variable name -> (parameter, column slice or None); Q / K / V are column slices of the fused projection."""
        C_ = self.num_units
        m = {"BERT4REC/item_embs/lookup_table": (self.item_embs.lookup_table, None),
             "BERT4REC/spatial_embs/embedding/lookup_table": (self.pcoding.pembs.lookup_table, None),
             "BERT4REC/output_bias": (self.output_bias, None),
             "embeddings/LayerNorm/beta": (self.emb_ln.beta, None), "embeddings/LayerNorm/gamma": (self.emb_ln.gamma, None)}
        for i, blk in enumerate(self.layers):
            pre = f"layer_{i}/"
            for j, name in enumerate("QKV"):
                sl = slice(j * C_, (j + 1) * C_)
                a = pre + f"attention/self/BERTAttention/{name}/"
                m[a + "kernel"], m[a + "bias"] = (blk.attention.qkv_kernel, sl), (blk.attention.qkv_bias, sl)
            for scope, dense, ln in (("attention/output/", blk.att_out, blk.att_ln), ("output/", blk.out, blk.out_ln)):
                m[pre + scope + "dense/kernel"], m[pre + scope + "dense/bias"] = (dense.kernel, None), (dense.bias, None)
                m[pre + scope + "LayerNorm/beta"], m[pre + scope + "LayerNorm/gamma"] = (ln.beta, None), (ln.gamma, None)
            m[pre + "intermediate/dense/kernel"], m[pre + "intermediate/dense/bias"] = (blk.inter.kernel, None), (blk.inter.bias, None)
        t = "cls/predictions/transform/"
        m[t + "dense/kernel"], m[t + "dense/bias"] = (self.transform.kernel, None), (self.transform.bias, None)
        m[t + "LayerNorm/beta"], m[t + "LayerNorm/gamma"] = (self.transform_ln.beta, None), (self.transform_ln.gamma, None)
        return m
