"""Mirror of src/model/TimelyREC.py (Cho et al., WWW'21, as the reference implements it) on the HIP kernels: the calendar-conditioned
baseline of the comparison.  Three branches meet in a small sigmoid head: ONE SASRec block over the items (the "inductive user
embedding" U), the multi-aspect time encoder over month / day / weekday / hour slots (csrc/k_mate.hip) and the time-aware history
encoder, a softmax-free cosine mix of the history (csrc/k_tahe.hip).

    m = TimelyREC(num_items, FLAGS).finalize("cuda")
    logits = m(features, is_training)          # TimelyREC.__call__ (TimelyREC.py:103-173): [B*T, I] (train) / [B, I] (eval)
    loss = m.train_loss(features, labels)      # Sequential.train (Base.py:119-140)

``features`` as RegressivePostProcessor(has_datetime=True) emits them: ``seqs_i`` = tokens[:-1] int64 [B,T], ``seqs_t`` [B,T+1],
``seqs_month`` / ``seqs_day`` / ``seqs_weekday`` / ``seqs_hour`` = field[:-1] int64 [B,T] (month 1-12, day 1-31, weekday 0-6, hour
0-23; 0 in every field at padding).

Stated quirks kept from the reference:
  * the slots' running sum (tf.math.cumsum, TimelyREC.py:70) runs over the SEQUENCE axis, padded positions included;
  * at padding month and day index -1: ``e`` reads a zero row there (the reference's GPU lookup; the rule TimeIntervalCoding states
    in module/coding.py), while the window rows (-1 +- w) mod M are ordinary rows; weekday 0 and hour 0 are valid rows at padding;
  * the item embedding is NOT scaled by sqrt(C) (scale=False); PositionCoding concatenates, so the block reads 2C channels;
    FLAGS.num_blocks is not read (one block);
  * in training the reference adds te_weight * sum_c out_c tcode_c to EVERY logit of a row (:162-172).  A per-row constant leaves
    softmax, and so log(softmax + 1e-5), unchanged: loss and gradients are exactly those without it.  ``train_loss`` never computes
    it; ``forward(features, True)`` adds it for surface parity;
  * the optimizer is Base's: Adam(0.9, 0.999, 1e-8), no clipping; the l2 term acts on the six embedding tables.

Not built: channel padding (widths are powers of two in [32, 512], head dims 16 / 32 / 64 / 128), the static TrainEngine, lazy_adam,
the on-device loader and graph replay of the driver, multi-GPU."""
from __future__ import annotations

from typing import Dict

import torch
from torch import nn

from .. import ops
from ..module import coding as C
from ..module import sequential as S
from .base import Sequential, _Dense, _FeedForward, _LayerNorm
from .sasrec import check_width, specs_from_map

CALENDAR = ("month", "day", "weekday", "hour")
_OFFSET = (1, 1, 0, 0)       # pd.datetime month and day start at 1 (TimelyREC.py:111,115)


class TimelyREC(Sequential):
    static_engine_ok = False              # (the static TrainEngine is EasyDGL's; this model trains through train_step)

    def __init__(self, num_items, FLAGS):
        super().__init__(num_items, FLAGS)
        self.seed = int(getattr(FLAGS, "seed", 9876))
        gen = torch.Generator().manual_seed(self.seed)
        C_ = self.width_true = self.num_units
        check_width("TimelyREC", C_, self.num_heads)
        ratio = getattr(FLAGS, "window_ratio", None)
        self.window_ratio = 0.2 if ratio is None else float(ratio)
        if not 0.0 < self.window_ratio <= 0.5:
            raise ValueError(f"TimelyREC: window_ratio={self.window_ratio} unsupported; the HIP slot kernel takes "
                             "0 < window_ratio <= 0.5 (--window_ratio)")
        if not 1 <= self.seqslen <= 128:
            raise ValueError(f"TimelyREC: seqslen={self.seqslen} unsupported; the HIP kernels take 1 <= seqslen <= 128 (--seqslen)")
        self.time_scale = float(FLAGS.time_scale)
        # a one-element DEVICE divisor: tensor / tensor is a true float32 division as in the reference (tensor / Python scalar is
        # a multiplication by the rounded reciprocal, one ulp of a day count of 1.8e4 off — 2e-3 in the fastest sinusoid)
        self.register_buffer("time_scale_t", torch.tensor([self.time_scale], dtype=torch.float32), persistent=False)
        self.item_embs = C.Embedding(num_items, C_, self.l2_reg, zero_pad=True, scale=False, gen=gen,
                                     deterministic=self.deterministic)                                    # TimelyREC.py:26-27
        self.output_bias = self.make_output_bias()                                                        # :28
        self.pcoding = C.PositionCoding(self.seqslen, C_, self.l2_reg, gen=gen)                           # :31
        self.tcoding = C.TimeSinusoidCoding(C_)                                                           # :32
        self.te_weight = nn.Parameter(torch.ones(()))                                                     # :33
        self.att_ln = _LayerNorm(2 * C_)
        self.attention = S.MultiHeadAttention(C_, self.num_heads, self.attention_probs_dropout_rate, in_units=2 * C_, gen=gen)   # :35
        self.ff_ln = _LayerNorm(C_)
        self.ff = _FeedForward(C_, gen)                                                                   # :36
        self.out_ln = _LayerNorm(C_)
        self.month_embs = C.Embedding(12, C_, self.l2_reg, zero_pad=False, scale=False, gen=gen)          # :39-46
        self.day_embs = C.Embedding(31, C_, self.l2_reg, zero_pad=False, scale=False, gen=gen)
        self.weekday_embs = C.Embedding(7, C_, self.l2_reg, zero_pad=False, scale=False, gen=gen)
        self.hour_embs = C.Embedding(24, C_, self.l2_reg, zero_pad=False, scale=False, gen=gen)
        self.mate = S.MATEncoder(C_, self.window_ratio, gen=gen)                                          # :49-52, :127
        self.tahe = S.TAHEncoder()                                                                        # :55
        self.pred_inner = _Dense(3 * C_, 2 * C_, gen)                                                     # :154
        self.pred_out = _Dense(2 * C_, C_, gen)                                                           # :155

    def _pad_specs(self):
        specs = specs_from_map(self._tf_map())
        return [(n, p, m, "ones" if n.endswith("te_weight") else k) for n, p, m, k in specs]

    def l2_param_names(self):
        return ["item_embs.lookup_table", "pcoding.pembs.lookup_table", "month_embs.lookup_table", "day_embs.lookup_table",
                "weekday_embs.lookup_table", "hour_embs.lookup_table"]

    def _tables(self):
        return (self.month_embs, self.day_embs, self.weekday_embs, self.hour_embs)

    def _calendar_idx(self, features):
        """int64 [4,B,T]: month - 1 | day - 1 | weekday | hour (TimelyREC.py:111-123)."""
        return torch.stack([features["seqs_" + n].to(torch.int64) - o for n, o in zip(CALENDAR, _OFFSET)]).contiguous()

    def _branches(self, features, is_training):
        """(U, hist, R, tcode), each [B,T,C]: the three branches at every position and the time code of the logit bias."""
        ids = features["seqs_i"].contiguous()
        C_ = self.num_units
        emb = self.item_embs(ids)                                                                          # :83, :139 (one lookup)
        if emb.dtype != self.act_dtype:
            emb = emb.to(self.act_dtype)
        # inductive user embedding (:79-101): dropout([item | pos]) * mask — the mask and the dropout commute
        x = ops.CatPosMaskFn.apply(emb, self.pcoding.pembs.lookup_table, ids)                              # :84, :92
        x = ops.dropout(x, self._drop(self.hidden_dropout_rate, 1, is_training))                           # :87
        qn = ops.AddLayerNormFn.apply(x, None, self.att_ln.gamma, self.att_ln.beta, ops.NO_DROP, None)
        att = self.attention(qn, x, is_training, True, ids=ids,
                             drop=self._drop(self.attention_probs_dropout_rate, 10, is_training))          # :94
        y = ops.AddLayerNormFn.apply(att, None, self.ff_ln.gamma, self.ff_ln.beta, ops.NO_DROP, None)
        f = self._feed_forward(y, self.ff, 0, ids, is_training)                                            # :96-97
        U = ops.AddLayerNormFn.apply(f, None, self.out_ln.gamma, self.out_ln.beta, ops.NO_DROP, None)      # :100
        # multi-aspect time encoder and the combination (:108-135)
        R = self.mate(self._calendar_idx(features), self._tables(), U)
        # time-aware history encoder (:137-147)
        tcode = self.tcoding.code(features["seqs_t"][:, :-1].to(torch.float32) / self.time_scale_t)        # :141
        Hs = ops.TaheMixFn.apply(emb, tcode, self.te_weight, ids)                                          # :142-146
        hist = self.tahe(R, R, Hs)
        return U, hist, R, tcode

    def _head(self, U, hist, R):
        f = ops.Cat3Fn.apply(U, hist, R)                                                                   # :150 (3C wide)
        f = ops.SigmoidFn.apply(self._linear(f, self.pred_inner))                                          # :154
        return self._linear(f, self.pred_out)                                                              # :155

    def encoder(self, features, is_training, gather_pos):
        """TimelyREC.py:103-155: the rows that are scored, [B, T, C], or [B, 1, C] at gather_pos (the last position: every
        position's slots and history are needed to get there; only the head's two GEMMs run on the gathered row alone)."""
        U, hist, R, _ = self._branches(features, is_training)
        if gather_pos is not None:
            U, hist, R = (t[:, -1:, :].contiguous() for t in (U, hist, R))
        return self._head(U, hist, R)

    def forward(self, features: Dict[str, torch.Tensor], is_training: bool):
        tab = self.item_embs.lookup_table
        U, hist, R, tcode = self._branches(features, is_training)
        if not is_training:
            rows = self._head(*(t[:, -1:, :].contiguous() for t in (U, hist, R))).reshape(-1, self.num_units)
            return ops.ScoreLogitsFn.apply(rows, tab, self.output_bias, self.compute(tab))                 # :168-172
        rows = self._head(U, hist, R).reshape(-1, self.num_units)
        logits = ops.ScoreLogitsFn.apply(rows, tab, self.output_bias, self.compute(tab))
        # :162-172 the per-row constant of the training graph (surface parity only: train_loss does not need it)
        bias = (rows.float() * tcode.reshape(rows.shape).float()).sum(-1, keepdim=True) * self.te_weight
        return logits + bias

    def train_loss(self, features, labels, *, candidates=None, shared=None):
        """Sequential.train (Base.py:119-131) with the fused scoring / cross-entropy; `candidates` / `shared` as in the other models
        (Sequential._score_ce).  The training-time logit bias cancels in the softmax and is not computed."""
        rows = self.encoder(features, True, None)
        loss = self._score_ce(rows.reshape(-1, self.num_units), labels.reshape(-1).contiguous(), candidates, shared)
        if self.l2_reg != 0.0:
            for n in self.l2_param_names():
                loss = loss + ops.L2Fn.apply(self.get_parameter(n), self.l2_reg)
        return loss

    # ---- interop with the reference's variable naming (tests / checkpoints converted from TF) ------------------------
    def _tf_map(self):
        """TF variable name -> (parameter, column slice or None).  The user branch runs inside two nested scopes
        (TimelyREC.py:93-105), hence ``TimelyREC/attention/TimelyREC/Atttention/...`` with the reference's spelling."""
        C_ = self.num_units
        m = {"TimelyREC/item_embs/lookup_table": (self.item_embs.lookup_table, None),
             "TimelyREC/output_bias": (self.output_bias, None),
             "TimelyREC/spatial_embs/embedding/lookup_table": (self.pcoding.pembs.lookup_table, None),
             "TimelyREC/te_weight": (self.te_weight, None)}
        for name, tab in zip(CALENDAR, self._tables()):
            m[f"TimelyREC/{name}_embs/lookup_table"] = (tab.lookup_table, None)
        u = "TimelyREC/attention/TimelyREC/"
        a = u + "Atttention/multihead_attention/"
        m[u + "Atttention/LayerNorm/gamma"], m[u + "Atttention/LayerNorm/beta"] = (self.att_ln.gamma, None), (self.att_ln.beta, None)
        m[a + "dense/kernel"], m[a + "dense/bias"] = (self.attention.q_kernel, None), (self.attention.q_bias, None)
        for j in (1, 2):
            sl = slice((j - 1) * C_, j * C_)
            m[a + f"dense_{j}/kernel"], m[a + f"dense_{j}/bias"] = (self.attention.kv_kernel, sl), (self.attention.kv_bias, sl)
        f = u + "fforward/"
        m[f + "LayerNorm/gamma"], m[f + "LayerNorm/beta"] = (self.ff_ln.gamma, None), (self.ff_ln.beta, None)
        m[f + "Inner/kernel"], m[f + "Inner/bias"] = (self.ff.inner.kernel, None), (self.ff.inner.bias, None)
        m[f + "Readout/kernel"], m[f + "Readout/bias"] = (self.ff.readout.kernel, None), (self.ff.readout.bias, None)
        m[u + "out/LayerNorm/gamma"], m[u + "out/LayerNorm/beta"] = (self.out_ln.gamma, None), (self.out_ln.beta, None)
        for j, scope in enumerate(("month_mate", "daymate", "weekday_mate", "hour_mate")):
            m[f"TimelyREC/mate/{scope}/dense/kernel"] = (self.mate.kernel, slice(j * C_, (j + 1) * C_))
        m["TimelyREC/mate/dense/kernel"] = (self.mate.combine, None)
        d = "TimelyREC/prediction/"
        m[d + "dense/kernel"], m[d + "dense/bias"] = (self.pred_inner.kernel, None), (self.pred_inner.bias, None)
        m[d + "dense_1/kernel"], m[d + "dense_1/bias"] = (self.pred_out.kernel, None), (self.pred_out.bias, None)
        return m
