"""Mirror of src/model/CTSMA.py (ICML'21 continuous-time self-modulating attention) on the HIP kernels — SURVEY §8
row f-4: the causal MAU is the BiMAU kernel with two flags, the rest is LayerNorm / dense / scoring ops that exist.

    m = CTSMA(num_items, FLAGS).finalize("cuda")
    logits = m(features, is_training)          # CTSMA.__call__ (CTSMA.py:48-93): [B*T, I] (train) / [B, I] (eval)
    loss = m.train_loss(features, labels)      # CTSMA.train (CTSMA.py:95-127)

``features`` as RegressivePostProcessor emits them (dataloader.py:88-108, keep_entire): ``seqs_i`` = tokens[:-1] int64
[B,T], ``seqs_t`` float32 [B,T+1]; labels = tokens[1:] [B,T] (training) / tokens [B,T+1] (evaluation).  Unlike EasyDGL
the model keeps T = FLAGS.seqslen positions and a [num_items, C] table (CTSMA.py:23-37).
"""
from __future__ import annotations

import pickle
from typing import Dict

import numpy as np
import torch
from torch import nn

from .. import ops
from ..module import coding as C
from ..module import temporal as T
from .base import Sequential, _FeedForward, _LayerNorm


class _Block(nn.Module):
    def __init__(self, cin, C_, heads, events, att_drop, gen):
        super().__init__()
        self.att_ln = _LayerNorm(cin)                                    # num_blocks_i/attention/LayerNorm
        self.attention = T.MAU(C_, heads, events, att_drop, in_units=cin, gen=gen)    # num_blocks_i/attention/modulating_attention
        self.ff_ln = _LayerNorm(C_)                                      # num_blocks_i/feed-forward/LayerNorm
        self.ff = _FeedForward(C_, gen)


class CTSMA(Sequential):
    def __init__(self, num_items, FLAGS):
        super().__init__(num_items, FLAGS)
        self.time_scale = float(FLAGS.time_scale)
        self.seed = int(getattr(FLAGS, "seed", 9876))
        table = getattr(FLAGS, "mark_table", None)
        if table is None:
            table = pickle.load(open(FLAGS.mark, "rb")).toarray()     # CTSMA.py:24
        table = np.asarray(table)
        if table.shape[0] < num_items or not np.isin(table, (0, 1)).all():
            raise ValueError("mark table must be a 0/1 multi-hot table with one row per item id")
        self.num_events = int(table.shape[-1])
        if not (2 <= self.num_events <= T.MAX_EVENTS):
            raise ValueError(f"num_events must be in [2, {T.MAX_EVENTS}] (more than 16 run as mark groups: temporal.modulated_attention)")
        self.register_buffer("mark_lookup_table", torch.from_numpy(table.astype(np.uint8)), persistent=False)
        self.ct_reg = float(getattr(FLAGS, "ct_reg", 0.0) or 0.0)
        gen = torch.Generator().manual_seed(self.seed)
        self._setup_channel_pad("CTSMA")      # head dims below 128 that the kernels do not tile run zero-padded (model/base.py)
        C_ = self.num_units
        self.item_embs = C.Embedding(self.num_items, C_, self.l2_reg, zero_pad=True, scale=True, gen=gen)   # CTSMA.py:30-31
        self.pcoding = C.PositionCoding(self.seqslen, C_, self.l2_reg, gen=gen)                              # :32
        self.output_bias = self.make_output_bias()                                                           # :34
        self.layers = nn.ModuleList()
        for i in range(FLAGS.num_blocks):
            self.layers.append(_Block(2 * C_ if i == 0 else C_, C_, self.num_heads, self.num_events,
                                      self.attention_probs_dropout_rate, gen))
        self.out_ln = _LayerNorm(C_)                                                                         # outln
        self._finish_pad(gen)

    def _pad_specs(self):
        """The variable table (model/base.py): (TF name, parameter, axis maps reference -> stored, initialiser).  K | V | T_ are
        one stored matrix whose column blocks are the reference's dense_1 .. dense_3."""
        Cp = self.num_units
        c = self._cmap()
        st_rows, jmap, u = self._mlp_maps()        # intensity MLP: inputs (dh channels + the span), hidden units (e, u), output u
        sp = [("CSTMA/item_embs/lookup_table", self.item_embs.lookup_table, (None, c), "glorot"),
              ("CSTMA/spatial_embs/embedding/lookup_table", self.pcoding.pembs.lookup_table, (None, c), "glorot"),
              ("CSTMA/output_bias", self.output_bias, (None,), "zeros"),
              ("outln/LayerNorm/gamma", self.out_ln.gamma, (c,), "ones"), ("outln/LayerNorm/beta", self.out_ln.beta, (c,), "zeros")]
        for i, blk in enumerate(self.layers):
            pre = f"num_blocks_{i}/"
            a = pre + "attention/modulating_attention/"
            st = a + "sequential_temporal_combined/"
            cin = self._cmap(2) if i == 0 else c                               # item | position channels of the first block's input
            att = blk.attention
            sp += [(pre + "attention/LayerNorm/gamma", blk.att_ln.gamma, (cin,), "ones"),
                   (pre + "attention/LayerNorm/beta", blk.att_ln.beta, (cin,), "zeros"),
                   (a + "dense/kernel", att.q_kernel, (cin, c), "glorot"), (a + "dense/bias", att.q_bias, (c,), "zeros")]
            for k in (1, 2, 3):
                sp += [(a + f"dense_{k}/kernel", att.kvt_kernel, (cin, c + (k - 1) * Cp), "glorot"),
                       (a + f"dense_{k}/bias", att.kvt_bias, (c + (k - 1) * Cp,), "zeros")]
            sp += [(st + "dense/kernel", att.st_kernel, (st_rows, jmap), "glorot"), (st + "dense/bias", att.st_bias, (jmap,), "zeros"),
                   (st + "weight", att.weight, (None, u), "glorot"), (st + "scaling", att.scaling, (None,), "zeros"),
                   (pre + "feed-forward/LayerNorm/gamma", blk.ff_ln.gamma, (c,), "ones"),
                   (pre + "feed-forward/LayerNorm/beta", blk.ff_ln.beta, (c,), "zeros"),
                   (pre + "feed-forward/Inner/kernel", blk.ff.inner.kernel, (c, c), "glorot"),
                   (pre + "feed-forward/Inner/bias", blk.ff.inner.bias, (c,), "zeros"),
                   (pre + "feed-forward/Readout/kernel", blk.ff.readout.kernel, (c, c), "glorot"),
                   (pre + "feed-forward/Readout/bias", blk.ff.readout.bias, (c,), "zeros")]
        return sp

    def l2_param_names(self):
        return ["item_embs.lookup_table", "pcoding.pembs.lookup_table"]

    def encoder(self, features, is_training, gather_pos):
        """CTSMA.py:48-83: (rows [B*Mg, C] of the final LayerNorm at gather_pos (None: all positions), [lambda])."""
        ids, ts = features["seqs_i"].contiguous(), features["seqs_t"].contiguous()
        tab = self.item_embs.lookup_table
        hd = self.hidden_dropout_rate
        pad = self.pad
        x, spans, marks = ops.EmbedPosFn.apply(tab, self.pcoding.pembs.lookup_table, self.compute(tab), ids, ts,
                                               self.mark_lookup_table, self.time_scale, self._drop(hd, 1, is_training),
                                               self.act_dtype, self.width_true if pad[0] else 0, self.deterministic)   # :50-58
        lams = []
        for i, blk in enumerate(self.layers):
            q_in = ops.AddLayerNormFn.apply(x, None, blk.att_ln.gamma, blk.att_ln.beta, ops.NO_DROP, None, pad)  # :70
            att, lam = blk.attention(q_in, x, ids, spans, marks, is_training, True,
                                     drop=self._drop(self.attention_probs_dropout_rate, 10 + 4 * i, is_training))
            y = ops.AddLayerNormFn.apply(att, None, blk.ff_ln.gamma, blk.ff_ln.beta, ops.NO_DROP, None, pad)     # :75
            x = self._feed_forward(y, blk.ff, i, None, is_training)                                              # Base.py:79-86
            lams.append(lam)
        rows = ops.AddLayerNormFn.apply(x, None, self.out_ln.gamma, self.out_ln.beta, ops.NO_DROP, gather_pos, pad)   # :82-83
        return rows, lams

    def forward(self, features: Dict[str, torch.Tensor], is_training: bool):
        rows, lams = self.encoder(features, is_training, None if is_training else self._last_pos(features["seqs_i"]))
        self._last_lams = lams
        rows = rows.reshape(-1, self.num_units)
        tab = self.item_embs.lookup_table
        return ops.ScoreLogitsFn.apply(rows, tab, self.output_bias, self.compute(tab))

    def train_loss(self, features, labels, *, candidates=None, shared=None):
        """CTSMA.train (CTSMA.py:95-127) with the fused scoring / cross-entropy (no [B*T, I] tensor).  `candidates` (int32 [B*T, N])
        or FLAGS.train_negatives > 0: the softmax of every position over its label and its own list (Sequential._score_ce);
        `shared` (int32 [S]) or FLAGS.shared_negatives > 0: over its label and the step's ONE list."""
        rows, lams = self.encoder(features, True, None)
        loss = self._score_ce(rows.reshape(-1, self.num_units), labels.reshape(-1).contiguous(), candidates, shared)
        if self.l2_reg != 0.0:
            for p in (self.item_embs.lookup_table, self.pcoding.pembs.lookup_table):
                loss = loss + ops.L2Fn.apply(p, self.l2_reg)
        if self.ct_reg != 0.0:                                                                     # :101-112
            for lam in lams:
                loss = loss + ops.TppFn.apply(lam, None, labels.contiguous(), features["seqs_t"].contiguous(),
                                              self.mark_lookup_table, self.num_heads, self.ct_reg)
        return loss
