"""Mirror of src/model/TGREC.py (Fan et al., CIKM'21, as the reference implements it) on the HIP kernels: the continuous-time
collaborative transformer, whose time code is projected with the keys and with the values (module/temporal.py
TgMultiHeadAttention on csrc/k_tgattn.hip).

    m = TGREC(num_items, FLAGS).finalize("cuda")
    logits = m(features, is_training)          # TGREC.__call__ (TGREC.py:40-79): [B*T, I] (train) / [B, I] (eval)
    loss = m.train_loss(features, labels)      # Sequential.train (Base.py:119-140)

``features`` as RegressivePostProcessor emits them: ``seqs_i`` = tokens[:-1] int64 [B,T] with T = FLAGS.seqslen, ``seqs_t`` float32
[B,T+1].  The reference's model cannot run on its own reader: it subtracts [B,T+1] timestamps tiled to ``seqslen`` columns
(TGREC.py:47-49).  Here the model uses ``seqs_t[:, :T]``, the times of the input tokens, and a [B,T] ``seqs_t`` is taken as is.

Timestamps must not decrease along the WHOLE row, zeros under the left padding included: the kernel uses
cos(a - b) = cos a cos b + sin a sin b for every pair k <= q, padded keys too (a fully masked row is uniform over all keys and its
values carry the time code).  ``check_inputs()`` raises if a batch violated it.

Kept from the reference: the item embedding is NOT scaled by sqrt(C); the position code is ADDED; no LayerNorm outside the
attention unit; the merge layer is concat[att(2C), x(C)] -> dense(C, relu) -> dense(C); Adam with the defaults; the l2 term acts on
the item and position tables.

Not built: num_units above 128 (refused), channel padding, the static TrainEngine, lazy_adam."""
from __future__ import annotations

from typing import Dict

import torch
from torch import nn

from .. import ops
from ..module import coding as C
from ..module import temporal as T
from .base import Sequential, _Dense
from .sasrec import check_width, specs_from_map

WIDTHS = (32, 64, 128)      # what edgl_tgattn_* tiles: the whole width is the contraction length of the time code


class _Block(nn.Module):
    def __init__(self, C_, heads, att_drop, l2, tcoding, gen):
        super().__init__()
        self.attention = T.TgMultiHeadAttention(C_, heads, att_drop, l2, tcoding, gen)   # num_blocks_i/attention/TgMultiHeadAttention
        self.inner = _Dense(3 * C_, C_, gen)                                             # num_blocks_i/dense
        self.out = _Dense(C_, C_, gen)                                                   # num_blocks_i/dense_1


class TGREC(Sequential):
    static_engine_ok = False      # (the static TrainEngine is EasyDGL's; this model trains through train_step / graphed_train_step)

    def __init__(self, num_items, FLAGS):
        super().__init__(num_items, FLAGS)
        self.time_scale = float(FLAGS.time_scale)
        self.seed = int(getattr(FLAGS, "seed", 9876))
        gen = torch.Generator().manual_seed(self.seed)
        C_ = self.width_true = self.num_units
        if C_ not in WIDTHS:
            raise ValueError(f"TGREC: num_units={C_} unsupported; the HIP temporal-graph attention takes --num_units in {WIDTHS}")
        check_width("TGREC", C_, self.num_heads)
        if not 1 <= self.seqslen <= 1024:
            raise ValueError(f"TGREC: seqslen={self.seqslen} unsupported; the HIP kernels take 1 <= seqslen <= 1024 (--seqslen)")
        self.item_embs = C.Embedding(num_items, C_, self.l2_reg, zero_pad=True, scale=False, gen=gen,
                                     deterministic=self.deterministic)                                    # TGREC.py:25-26
        self.output_bias = self.make_output_bias()                                                        # :27
        self.pcoding = C.PositionCoding(self.seqslen, C_, self.l2_reg, gen=gen)                           # :29
        self.pcoding.pembs.deterministic = self.deterministic
        self.tcoding = C.TimeFunctionCoding(C_)                                                           # :30
        self.layers = nn.ModuleList()
        for _ in range(FLAGS.num_blocks):
            self.layers.append(_Block(C_, self.num_heads, self.attention_probs_dropout_rate, self.l2_reg, self.tcoding, gen))

    def _pad_specs(self):
        specs = specs_from_map(self._tf_map())
        return [(n, p, m, "linspace9" if n.endswith("basis_freq") else k) for n, p, m, k in specs]

    def l2_param_names(self):
        return ["item_embs.lookup_table", "pcoding.pembs.lookup_table"]

    def finalize(self, device):
        super().finalize(device)
        self._violations = torch.zeros(1, device=device, dtype=torch.int32)
        for blk in self.layers:
            blk.attention.time_scale = self.time_scale
            blk.attention.violations = self._violations
        return self

    def check_inputs(self) -> None:
        """Raises if any batch so far had a timestamp below its predecessor at ANY position of a row (one device read)."""
        n = int(self._violations.item())
        if n:
            self._violations.zero_()
            raise ValueError(f"{n} positions with decreasing timestamps: sort each sequence by time, padding first with time 0 "
                             "(see model/tgrec.py)")

    def encoder(self, features, is_training, gather_pos):
        """TGREC.py:40-74: the rows that are scored, [B, T, C], or [B, 1, C] at gather_pos (the last position)."""
        ids = features["seqs_i"].contiguous()
        ts = features["seqs_t"].to(torch.float32).contiguous()
        if ts.dim() != 2 or ts.shape[0] != ids.shape[0] or ts.shape[1] not in (ids.shape[1], ids.shape[1] + 1):
            raise ValueError(f"TGREC: seqs_t of shape {tuple(ts.shape)} against seqs_i {tuple(ids.shape)}: [B, T] or [B, T+1]")
        hd = self.hidden_dropout_rate
        emb = self.item_embs(ids)                                                                          # :45
        if emb.dtype != self.act_dtype:
            emb = emb.to(self.act_dtype)
        x = ops.add(emb, self.pcoding.code(ids).to(self.act_dtype))                                        # :46
        x = ops.dropout(x, self._drop(hd, 1, is_training))                                                 # :53
        for i, blk in enumerate(self.layers):
            att = blk.attention(x, (ids, ts), is_training, True,
                                self._drop(self.attention_probs_dropout_rate, 10 + 4 * i, is_training))    # :62
            att = ops.dropout(att, self._drop(hd, 11 + 4 * i, is_training))                                # :63
            inner = self._linear(torch.cat([att, x], dim=-1), blk.inner, "relu")                           # :66-67
            x = self._linear(inner, blk.out)                                                               # :68
        if gather_pos is not None:
            x = x[:, -1:, :].contiguous()                                                                  # :74
        return x

    def forward(self, features: Dict[str, torch.Tensor], is_training: bool):
        gp = None if is_training else self._last_pos(features["seqs_i"])
        rows = self.encoder(features, is_training, gp).reshape(-1, self.num_units)
        tab = self.item_embs.lookup_table
        return ops.ScoreLogitsFn.apply(rows, tab, self.output_bias, self.compute(tab))                     # :77-79

    def train_loss(self, features, labels, *, candidates=None, shared=None):
        """Sequential.train (Base.py:119-131) with the fused scoring / cross-entropy; `candidates` / `shared` as in the other models
        (Sequential._score_ce)."""
        rows = self.encoder(features, True, None)
        loss = self._score_ce(rows.reshape(-1, self.num_units).contiguous(), labels.reshape(-1).contiguous(), candidates, shared)
        if self.l2_reg != 0.0:
            for n in self.l2_param_names():
                loss = loss + ops.L2Fn.apply(self.get_parameter(n), self.l2_reg)
        return loss

    # ---- interop with the reference's variable naming (tests / checkpoints converted from TF) ------------------------
    def _tf_map(self):
        """TF variable name -> (parameter, column slice or None)."""
        C_ = self.num_units
        m = {"TGREC/item_embs/lookup_table": (self.item_embs.lookup_table, None),
             "TGREC/output_bias": (self.output_bias, None),
             "TGREC/pcoding/embedding/lookup_table": (self.pcoding.pembs.lookup_table, None),
             "TGREC/tcoding/basis_freq": (self.tcoding.basis_freq, None),
             "TGREC/tcoding/phase": (self.tcoding.phase, None)}
        for i, blk in enumerate(self.layers):
            pre = f"num_blocks_{i}/"
            a, att = pre + "attention/TgMultiHeadAttention/", blk.attention
            m[a + "dense/kernel"], m[a + "dense/bias"] = (att.q_kernel, None), (att.q_bias, None)
            for j in (1, 2):
                sl = slice((j - 1) * C_, j * C_)
                m[a + f"dense_{j}/kernel"], m[a + f"dense_{j}/bias"] = (att.kv_kernel, sl), (att.kv_bias, sl)
            m[a + "dense_3/kernel"], m[a + "dense_3/bias"] = (att.o_kernel, None), (att.o_bias, None)
            m[a + "ln/beta"], m[a + "ln/gamma"] = (att.ln_beta, None), (att.ln_gamma, None)
            m[pre + "dense/kernel"], m[pre + "dense/bias"] = (blk.inner.kernel, None), (blk.inner.bias, None)
            m[pre + "dense_1/kernel"], m[pre + "dense_1/bias"] = (blk.out.kernel, None), (blk.out.bias, None)
        return m
