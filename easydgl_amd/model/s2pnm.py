"""Mirror of src/model/S2PNM.py (Chen et al., TKDE'21, as the reference implements it) on the HIP kernels: the strongest
time-independent baseline of the comparison.  A GRU (the recurrence kernel csrc/k_gru.hip) in front of ONE SASRec block
(model/sasrec.py) and a small "dictionary" head over [g, h, g - h, g * h].

    m = S2PNM(num_items, FLAGS).finalize("cuda")
    logits = m(features, is_training)          # S2PNM.__call__ (S2PNM.py:37-77): [B*T, I] (train) / [B, I] (eval)
    loss = m.train_loss(features, labels)      # Sequential.train (Base.py:119-140)

``features`` as RegressivePostProcessor emits them: ``seqs_i`` = tokens[:-1] int64 [B,T] (``seqs_t`` is not read).

Stated quirks kept from the reference: the GRU runs over the padded positions too (cuDNN without sequence lengths: a zero input
row still moves the state through the biases, S2PNM.py:47-49); PositionCoding concatenates, so the block reads [h | pos] * mask
at 2C channels; the feed-forward output is NOT masked (:59); every LayerNorm takes its moments over all T positions of a sample
(Base.py:12-67), the head's over T * 4C values; the head adds the UNdropped scaled item embedding (:66); FLAGS.num_blocks is not
read (one block).  The optimizer is Adam(beta2 = 0.98, epsilon = 1e-9) behind clip_by_global_norm(5) (:79-90).

The opaque cuDNN parameter blob appears as its twelve canonical parts, the weights in tf.layers.dense orientation [in, out]:
``S2PNM/Reccurency/S2PNM/GRU/opaque_kernel/{w,r}_{r,z,n}`` and ``.../b_{w,r}{r,z,n}``.

Not built: channel padding (widths are powers of two in [32, 512]; head dims 16 / 32 / 64 / 128 or a multiple of 128), the static TrainEngine and lazy_adam."""
from __future__ import annotations

from typing import Dict

import torch

from .. import ops
from ..module import coding as C
from ..module import sequential as S
from .base import Sequential, _Dense, _FeedForward, _LayerNorm
from .sasrec import check_width, specs_from_map


class S2PNM(Sequential):
    adam_hparams = (0.9, 0.98, 1e-9)      # S2PNM.py:86
    clip_norm = 5.0                       # S2PNM.py:87
    static_engine_ok = False              # (the static TrainEngine knows neither; train_step / graphed_train_step do)

    def __init__(self, num_items, FLAGS):
        super().__init__(num_items, FLAGS)
        self.seed = int(getattr(FLAGS, "seed", 9876))
        gen = torch.Generator().manual_seed(self.seed)
        C_ = self.width_true = self.num_units
        H = self.num_heads
        check_width("S2PNM", C_, H, wide=True)       # (the published recipe is ONE head of 512 channels, runme.sh:48-55)
        self.item_embs = C.Embedding(num_items, C_, self.l2_reg, zero_pad=True, scale=True, gen=gen)     # S2PNM.py:25-26
        self.pcoding = C.PositionCoding(self.seqslen, C_, self.l2_reg, gen=gen)                           # :27
        self.gru = S.GRU(C_, C_, gen=gen)                                                                 # :29-31
        self.att_ln = _LayerNorm(2 * C_)                                                                  # S2PNM/Attention/LayerNorm
        self.attention = S.MultiHeadAttention(C_, H, self.attention_probs_dropout_rate, in_units=2 * C_, gen=gen)   # :33
        self.ff_ln = _LayerNorm(C_)                                                                       # S2PNM/fforward/LayerNorm
        self.ff = _FeedForward(C_, gen)                                                                   # :34
        self.dict_ln = _LayerNorm(4 * C_)                                                                 # S2PNM/Dictionary/LayerNorm
        self.dict_inner = _Dense(4 * C_, 2 * C_, gen)                                                     # S2PNM/Dictionary/dense
        self.dict_out = _Dense(2 * C_, C_, gen)                                                           # S2PNM/Dictionary/dense_1
        self.output_bias = self.make_output_bias()                                                        # :35

    def _pad_specs(self):
        return specs_from_map(self._tf_map())

    def l2_param_names(self):
        return ["item_embs.lookup_table", "pcoding.pembs.lookup_table"]

    def encoder(self, features, is_training, gather_pos):
        """S2PNM.py:37-66: the rows that are scored, [B, T, C], or [B * Mg, C] at gather_pos (the head's LayerNorm takes its moments
        over all positions and emits the gathered rows; the head's GEMMs then run on those alone)."""
        ids = features["seqs_i"].contiguous()
        tab = self.item_embs.lookup_table
        x = ops.EmbedFn.apply(tab, self.compute(tab), ids, ops.NO_DROP, self.act_dtype, 0, self.deterministic)       # :39 (kept)
        xd = ops.dropout(x, self._drop(self.hidden_dropout_rate, 1, is_training))                                     # :42-43
        h = self.gru(xd)                                                                                              # :47-49
        u = ops.CatPosMaskFn.apply(h, self.pcoding.pembs.lookup_table, ids)                                           # :52-53
        qn = ops.AddLayerNormFn.apply(u, None, self.att_ln.gamma, self.att_ln.beta, ops.NO_DROP, None)
        att = self.attention(qn, u, is_training, True, ids=ids,
                             drop=self._drop(self.attention_probs_dropout_rate, 10, is_training))                     # :57
        y = ops.AddLayerNormFn.apply(att, None, self.ff_ln.gamma, self.ff_ln.beta, ops.NO_DROP, None)
        g = self._feed_forward(y, self.ff, 0, None, is_training)                                                      # :59 (no row mask)
        f = ops.DictFeatFn.apply(g, h)                                                                                # :63
        f = ops.AddLayerNormFn.apply(f, None, self.dict_ln.gamma, self.dict_ln.beta, ops.NO_DROP, gather_pos)
        f = ops.SigmoidFn.apply(self._linear(f, self.dict_inner))                                                     # :64
        out = self._linear(f, self.dict_out)                                                                          # :65
        if gather_pos is not None:          # (evaluation: _last_pos, the one row per sample that is scored)
            x = x[:, -1, :].contiguous()
        return ops.add(out.reshape(x.shape), x)                                                                       # :66

    def forward(self, features: Dict[str, torch.Tensor], is_training: bool):
        gp = None if is_training else self._last_pos(features["seqs_i"])
        rows = self.encoder(features, is_training, gp).reshape(-1, self.num_units)
        tab = self.item_embs.lookup_table
        return ops.ScoreLogitsFn.apply(rows, tab, self.output_bias, self.compute(tab))                                # :74-77

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
        m = {"S2PNM/item_embs/lookup_table": (self.item_embs.lookup_table, None),
             "S2PNM/spatial_embs/embedding/lookup_table": (self.pcoding.pembs.lookup_table, None),
             "S2PNM/output_bias": (self.output_bias, None)}
        g = "S2PNM/Reccurency/S2PNM/GRU/opaque_kernel/"
        for j, gate in enumerate(("r", "z", "n")):
            sl = slice(j * C_, (j + 1) * C_)
            m[g + f"w_{gate}"], m[g + f"r_{gate}"] = (self.gru.w_kernel, sl), (self.gru.r_kernel, sl)
            m[g + f"b_w{gate}"], m[g + f"b_r{gate}"] = (self.gru.w_bias, sl), (self.gru.r_bias, sl)
        a = "S2PNM/Attention/multihead_attention/"
        m["S2PNM/Attention/LayerNorm/gamma"], m["S2PNM/Attention/LayerNorm/beta"] = (self.att_ln.gamma, None), (self.att_ln.beta, None)
        m[a + "dense/kernel"], m[a + "dense/bias"] = (self.attention.q_kernel, None), (self.attention.q_bias, None)
        for j in (1, 2):
            sl = slice((j - 1) * C_, j * C_)
            m[a + f"dense_{j}/kernel"], m[a + f"dense_{j}/bias"] = (self.attention.kv_kernel, sl), (self.attention.kv_bias, sl)
        f = "S2PNM/fforward/"
        m[f + "LayerNorm/gamma"], m[f + "LayerNorm/beta"] = (self.ff_ln.gamma, None), (self.ff_ln.beta, None)
        m[f + "Inner/kernel"], m[f + "Inner/bias"] = (self.ff.inner.kernel, None), (self.ff.inner.bias, None)
        m[f + "Readout/kernel"], m[f + "Readout/bias"] = (self.ff.readout.kernel, None), (self.ff.readout.bias, None)
        d = "S2PNM/Dictionary/"
        m[d + "LayerNorm/gamma"], m[d + "LayerNorm/beta"] = (self.dict_ln.gamma, None), (self.dict_ln.beta, None)
        m[d + "dense/kernel"], m[d + "dense/bias"] = (self.dict_inner.kernel, None), (self.dict_inner.bias, None)
        m[d + "dense_1/kernel"], m[d + "dense_1/bias"] = (self.dict_out.kernel, None), (self.dict_out.bias, None)
        return m
