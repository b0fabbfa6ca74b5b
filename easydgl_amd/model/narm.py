"""NARM (Li et al., "Neural Attentive Session-based Recommendation", CIKM'17) on the HIP kernels, built on GRU4REC's pattern
(model/gru4rec.py): the same item embedding, stacked cuDNN-form GRU and tied scoring, with the encoder's states re-read through
additive attention (module.sequential.AdditiveAttention on csrc/k_addattn.hip).  The reference has no such model;
the definitions are the paper's.

    m = NARM(num_items, FLAGS).finalize("cuda")
    logits = m(features, is_training)          # [B*T, I] (train) / [B, I] (eval: the last position)
    loss = m.train_loss(features, labels)      # Sequential.train (Base.py:119-140)

Every position t is a session prefix: h = GRU stack(dropout(embedding)), c_local[t] = sum_{j <= t, ids[j] != 0} alpha[t,j] h[j] with
alpha[t,j] = v^T sigmoid(A1 h[t] + A2 h[j]) (no softmax, as in the paper), c = [h | c_local] (the global encoder's last state of the
prefix is h[t] itself), rows = dropout(c) B with the bilinear decoder B [2C, C] (no bias), masked by ``seqs_i != 0`` and scored
against the item table with the output bias.  The GRU runs over the padded positions too, as in GRU4REC; padded keys carry no
attention weight.  Adam(beta2 = 0.98, epsilon = 1e-9) behind clip_by_global_norm(5), as GRU4REC.

Variables: ``NARM/item_embs/lookup_table``, ``NARM/output_bias``, ``NARM/GRU/opaque_kernel/{l}/{w,r}_{r,z,n}`` and
``.../{l}/b_{w,r}{r,z,n}`` (weights in tf.layers.dense orientation [in, out]), ``NARM/attention/A1/kernel``,
``NARM/attention/A2/kernel`` [C, C], ``NARM/attention/v`` [C], ``NARM/decoder/kernel`` [2C, C].

Not built: a softmax-normalised attention, channel padding (--num_units is a power of two in [32, 512]), the static TrainEngine,
lazy_adam and --rnn_cell lstm; in the driver --device_data, --graph and --lazy_adam are refused by flag name."""
from __future__ import annotations

from typing import Dict

import torch
from torch import nn

from .. import ops
from ..module import coding as C
from ..module import sequential as S
from .base import Sequential
from .sasrec import specs_from_map

GRU_SCOPE = "NARM/GRU/opaque_kernel/"


class NARM(Sequential):
    adam_hparams = (0.9, 0.98, 1e-9)
    clip_norm = 5.0
    static_engine_ok = False              # (the static TrainEngine is EasyDGL's; this model trains through train_step)

    def __init__(self, num_items, FLAGS):
        super().__init__(num_items, FLAGS)
        self.seed = int(getattr(FLAGS, "seed", 9876))
        gen = torch.Generator().manual_seed(self.seed)
        C_ = self.width_true = self.num_units
        if C_ > 512 or C_ & (C_ - 1) or C_ < 32:
            raise ValueError(f"NARM: num_units={C_} unsupported: the fused scoring kernels take a power of two in [32, 512] "
                             f"(--num_units; this model is not channel-padded)")
        if int(FLAGS.num_blocks) < 1:
            raise ValueError(f"NARM: num_blocks={FLAGS.num_blocks} unsupported: the number of GRU layers, at least 1 (--num_blocks)")
        self.item_embs = C.Embedding(num_items, C_, self.l2_reg, zero_pad=True, scale=True, gen=gen)
        self.layers = nn.ModuleList(S.GRU(C_, C_, gen=gen, wide=True) for _ in range(int(FLAGS.num_blocks)))
        self.attention = S.AdditiveAttention(C_, gen)
        self.decoder = nn.Parameter(C.glorot_uniform_(torch.empty(2 * C_, C_), gen))
        self.register_buffer("no_bias", torch.zeros(C_), persistent=False)                # (the decoder has no bias)
        self.output_bias = self.make_output_bias()

    def _pad_specs(self):
        return specs_from_map(self._tf_map())

    def l2_param_names(self):
        return ["item_embs.lookup_table"]

    def encoder(self, features, is_training, gather_pos):
        """The rows that are scored, [B, T, C], or [B, C] at gather_pos (evaluation: _last_pos)."""
        ids = features["seqs_i"].contiguous()
        tab = self.item_embs.lookup_table
        x = ops.EmbedFn.apply(tab, self.compute(tab), ids, ops.NO_DROP, self.act_dtype, 0, self.deterministic)
        h = ops.dropout(x, self._drop(self.hidden_dropout_rate, 1, is_training))
        for gru in self.layers:
            h = gru(h)
        c = self.attention(h, ids, cat=True)                                              # [h | c_local]
        c = ops.dropout(c, self._drop(self.hidden_dropout_rate, 2, is_training))
        rows = ops.LinearFn.apply(c, self.decoder, self.no_bias, self.compute(self.decoder), False)
        out = ops.mask_rows(rows, ids)
        return out if gather_pos is None else out[:, -1, :].contiguous()

    def forward(self, features: Dict[str, torch.Tensor], is_training: bool):
        gp = None if is_training else self._last_pos(features["seqs_i"])
        rows = self.encoder(features, is_training, gp).reshape(-1, self.num_units)
        tab = self.item_embs.lookup_table
        return ops.ScoreLogitsFn.apply(rows, tab, self.output_bias, self.compute(tab))

    def train_loss(self, features, labels, *, candidates=None, shared=None):
        """Sequential.train (Base.py:119-131) with the fused scoring / cross-entropy; `candidates` / `shared` as in the other models
        (Sequential._score_ce)."""
        rows = self.encoder(features, True, None)
        loss = self._score_ce(rows.reshape(-1, self.num_units), labels.reshape(-1).contiguous(), candidates, shared)
        if self.l2_reg != 0.0:
            for n in self.l2_param_names():
                loss = loss + ops.L2Fn.apply(self.get_parameter(n), self.l2_reg)
        return loss

    # ---- variable names (tests / checkpoints) ------------------------------------------------------------------------
    def _tf_map(self):
        """Variable name -> (parameter, column slice or None)."""
        C_ = self.num_units
        att = self.attention
        m = {"NARM/item_embs/lookup_table": (self.item_embs.lookup_table, None),
             "NARM/output_bias": (self.output_bias, None)}
        for l, gru in enumerate(self.layers):
            g = GRU_SCOPE + f"{l}/"
            for j, gate in enumerate(("r", "z", "n")):
                sl = slice(j * C_, (j + 1) * C_)
                m[g + f"w_{gate}"], m[g + f"r_{gate}"] = (gru.w_kernel, sl), (gru.r_kernel, sl)
                m[g + f"b_w{gate}"], m[g + f"b_r{gate}"] = (gru.w_bias, sl), (gru.r_bias, sl)
        m["NARM/attention/A1/kernel"], m["NARM/attention/A2/kernel"] = (att.a_kernel, slice(0, C_)), (att.a_kernel, slice(C_, 2 * C_))
        m["NARM/attention/v"] = (att.v, None)
        m["NARM/decoder/kernel"] = (self.decoder, None)
        return m
