"""Mirror of src/model/GRU4REC.py (Hidasi et al., ICLR'16, as the reference implements it) on the HIP kernels: an item embedding,
a stack of cuDNN-form GRU layers and tied scoring.  The recurrence is the whole hot path; at the published width (512 units,
runme.sh:57-64) R is not LDS-resident and the layers run on the pipelined stream (csrc/k_gru_wide.hip).

    m = GRU4REC(num_items, FLAGS).finalize("cuda")
    logits = m(features, is_training)          # GRU4REC.__call__ (GRU4REC.py:33-58): [B*T, I] (train) / [B, I] (eval)
    loss = m.train_loss(features, labels)      # Sequential.train (Base.py:119-140)

``features`` as RegressivePostProcessor emits them: ``seqs_i`` = tokens[:-1] int64 [B,T] (``seqs_t`` is not read).

Kept from the reference: the item table is scaled by sqrt(C) with a zero row 0; the hidden dropout acts on the embeddings only
(:38), there is none between the layers; CudnnGRU(num_layers=FLAGS.num_blocks) (:27-29) is FLAGS.num_blocks layers in sequence,
each reading the previous layer's UNMASKED states; the GRU runs over the padded positions too (cuDNN without sequence lengths);
the top layer's states are masked by ``seqs_i != 0`` (:47) in front of the scoring; evaluation scores the last position only
(:53).  Adam(beta2 = 0.98, epsilon = 1e-9) behind clip_by_global_norm(5) (:60-71).

The opaque cuDNN parameter blob is built under the reference's stray scope (:43) and appears as its canonical parts per layer l,
the weights in tf.layers.dense orientation [in, out]: ``S2PNM/Reccurency/GRU4REC/GRU/opaque_kernel/{l}/{w,r}_{r,z,n}`` and
``.../{l}/b_{w,r}{r,z,n}``; each of a layer's six matrices is drawn with the orthogonal initialiser, the biases are zero.

``FLAGS.rnn_cell == "lstm"`` (default "gru") swaps the layers for the LSTM of the same cuDNN layer (module.sequential.LSTM on
csrc/k_lstm.hip) and nothing else; its parts are ``.../{l}/{w,r}_{i,f,c,o}`` and ``.../{l}/b_{w,r}{i,f,c,o}`` under
the same scope (cuDNN's canonical names: ``c`` is the candidate gate g), 2 + 16 L variables in all.

Not built: channel padding (--num_units is a power of two in [32, 512]), the static TrainEngine and lazy_adam; in the driver
--device_data, --graph and --lazy_adam are refused by flag name."""
from __future__ import annotations

from typing import Dict

import torch
from torch import nn

from .. import ops
from ..module import coding as C
from ..module import sequential as S
from .base import Sequential
from .sasrec import specs_from_map

GRU_SCOPE = "S2PNM/Reccurency/GRU4REC/GRU/opaque_kernel/"


class GRU4REC(Sequential):
    adam_hparams = (0.9, 0.98, 1e-9)      # GRU4REC.py:67
    clip_norm = 5.0                       # GRU4REC.py:68
    static_engine_ok = False              # (the static TrainEngine is EasyDGL's; this model trains through train_step)

    def __init__(self, num_items, FLAGS):
        super().__init__(num_items, FLAGS)
        self.seed = int(getattr(FLAGS, "seed", 9876))
        gen = torch.Generator().manual_seed(self.seed)
        C_ = self.width_true = self.num_units
        if C_ > 512 or C_ & (C_ - 1) or C_ < 32:
            raise ValueError(f"GRU4REC: num_units={C_} unsupported: the fused scoring kernels take a power of two in [32, 512] "
                             f"(--num_units; this model is not channel-padded)")
        if int(FLAGS.num_blocks) < 1:
            raise ValueError(f"GRU4REC: num_blocks={FLAGS.num_blocks} unsupported: the number of GRU layers, at least 1 (--num_blocks)")
        self.item_embs = C.Embedding(num_items, C_, self.l2_reg, zero_pad=True, scale=True, gen=gen)     # GRU4REC.py:24-25
        self.rnn_cell = getattr(FLAGS, "rnn_cell", "gru")
        if self.rnn_cell not in ("gru", "lstm"):
            raise ValueError(f"GRU4REC: rnn_cell={self.rnn_cell!r} unsupported: gru or lstm (--rnn_cell)")
        if self.rnn_cell == "lstm":       # the CUDNN_LSTM form of the same layer (csrc/k_lstm.hip)
            self.layers = nn.ModuleList(S.LSTM(C_, C_, gen=gen) for _ in range(int(FLAGS.num_blocks)))
        else:
            self.layers = nn.ModuleList(S.GRU(C_, C_, gen=gen, wide=True) for _ in range(int(FLAGS.num_blocks)))   # :27-29
        self.output_bias = self.make_output_bias()                                                        # :31

    def _pad_specs(self):
        return specs_from_map(self._tf_map())

    def l2_param_names(self):
        return ["item_embs.lookup_table"]

    def encoder(self, features, is_training, gather_pos):
        """GRU4REC.py:34-53: the rows that are scored, [B, T, C], or [B, C] at gather_pos (evaluation: _last_pos)."""
        ids = features["seqs_i"].contiguous()
        tab = self.item_embs.lookup_table
        x = ops.EmbedFn.apply(tab, self.compute(tab), ids, ops.NO_DROP, self.act_dtype, 0, self.deterministic)       # :35
        h = ops.dropout(x, self._drop(self.hidden_dropout_rate, 1, is_training))                                      # :38-39
        for gru in self.layers:                                                                                       # :44
            h = gru(h)
        out = ops.mask_rows(h, ids)                                                                                   # :47
        return out if gather_pos is None else out[:, -1, :].contiguous()                                              # :53

    def forward(self, features: Dict[str, torch.Tensor], is_training: bool):
        gp = None if is_training else self._last_pos(features["seqs_i"])
        rows = self.encoder(features, is_training, gp).reshape(-1, self.num_units)
        tab = self.item_embs.lookup_table
        return ops.ScoreLogitsFn.apply(rows, tab, self.output_bias, self.compute(tab))                                # :56-57

    def train_loss(self, features, labels, *, candidates=None, shared=None):
        """Sequential.train (Base.py:119-131) with the fused scoring / cross-entropy; `candidates` / `shared` as in the other models
        (Sequential._score_ce)."""
        rows = self.encoder(features, True, None)
        loss = self._score_ce(rows.reshape(-1, self.num_units), labels.reshape(-1).contiguous(), candidates, shared)
        if self.l2_reg != 0.0:
            for n in self.l2_param_names():
                loss = loss + ops.L2Fn.apply(self.get_parameter(n), self.l2_reg)
        return loss

    # ---- interop with the reference's variable naming (tests / checkpoints converted from TF) ------------------------
    def _tf_map(self):
        """TF variable name -> (parameter, column slice or None)."""
        C_ = self.num_units
        m = {"GRU4REC/item_embs/lookup_table": (self.item_embs.lookup_table, None),
             "GRU4REC/output_bias": (self.output_bias, None)}
        for l, gru in enumerate(self.layers):
            g = GRU_SCOPE + f"{l}/"
            for j, gate in enumerate(("i", "f", "c", "o") if self.rnn_cell == "lstm" else ("r", "z", "n")):
                sl = slice(j * C_, (j + 1) * C_)
                m[g + f"w_{gate}"], m[g + f"r_{gate}"] = (gru.w_kernel, sl), (gru.r_kernel, sl)
                m[g + f"b_w{gate}"], m[g + f"b_r{gate}"] = (gru.w_bias, sl), (gru.r_bias, sl)
        return m
