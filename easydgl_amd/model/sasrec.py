"""Mirror of src/model/SASREC.py (Kang & McAuley, ICDM'18, as the reference re-implements it) on the HIP kernels: the
time-independent baseline of the comparison.  TGAT's block wiring (model/tgat.py) around S.MultiHeadAttention, the plain-head case
of the generic masked attention kernel.

    m = SASRec(num_items, FLAGS).finalize("cuda")
    logits = m(features, is_training)          # SASRec.__call__ (SASREC.py:39-75): [B*T, I] (train) / [B, I] (eval)
    loss = m.train_loss(features, labels)      # Sequential.train (Base.py:119-140)

``features`` as RegressivePostProcessor emits them (dataloader.py:95-108): ``seqs_i`` = tokens[:-1] int64 [B,T] with
T = FLAGS.seqslen (``seqs_t`` is not read); labels = tokens[1:] (training) / tokens (evaluation).

Stated quirks kept from the reference: PositionCoding CONCATENATES (coding.py:72-74), so the first block reads 2C channels — its
LayerNorm, Q and K | V projections are [2C]-wide and its residual is the first C channels of the normalised input
(sequential.py:78); the input dropout covers the position half too (SASREC.py:48).

Not built: channel padding (the reference's default --num_units 50 is refused; widths are powers of two in [32, 512] with a head
dim of 16 / 32 / 64 / 128), the static TrainEngine and lazy_adam."""
from __future__ import annotations

from typing import Dict

import torch
from torch import nn

from .. import ops
from ..module import coding as C
from ..module import sequential as S
from .base import Sequential, _FeedForward, _LayerNorm


def check_width(who, num_units, num_heads, wide=False):
    """The widths SASRec / S2PNM run at, refused with the flag names (no channel padding for these two models).  Head dims: what
    the attention kernel tiles, 16 / 32 / 64 / 128; `wide` (S2PNM): also a whole multiple of 128 through the kernel's sliced form —
    its published single head of 512 channels (runme.sh:48-55)."""
    dh = num_units // num_heads if num_heads > 0 and num_units % num_heads == 0 else 0
    if not (dh in (16, 32, 64, 128) or (wide and dh > 128 and dh % 128 == 0)):
        raise ValueError(f"{who}: head dim num_units/num_heads = {num_units}/{num_heads} unsupported; the HIP attention kernel "
                         f"takes 16 / 32 / 64 / 128{' or a multiple of 128' if wide else ''} (--num_units / --num_heads, e.g. "
                         f"--num_units=512 --num_heads={1 if wide else 8})")
    if num_units > 512 or num_units & (num_units - 1) or num_units < 32:
        raise ValueError(f"{who}: num_units={num_units} unsupported: the fused scoring kernels take a power of two in [32, 512] "
                         f"(--num_units; these models are not channel-padded)")


def specs_from_map(tf_map):
    """The variable table (model/base.py _pad_specs) of an unpadded model from its {TF name: (parameter, column slice or None)}."""
    specs = []
    for name, (param, sl) in tf_map.items():
        leaf = name.rsplit("/", 1)[-1]
        kind = {"lookup_table": "glorot", "kernel": "glorot", "gamma": "ones"}.get(leaf, "zeros")
        maps = [None] * param.dim()
        if sl is not None:
            maps[-1] = torch.arange(sl.start, sl.stop)
        specs.append((name, param, tuple(maps), kind))
    return specs


class _Block(nn.Module):
    def __init__(self, cin, C_, heads, att_drop, gen):
        super().__init__()
        self.att_ln = _LayerNorm(cin)                                                       # num_blocks_i/attention/LayerNorm
        self.attention = S.MultiHeadAttention(C_, heads, att_drop, in_units=cin, gen=gen)   # .../attention/multihead_attention
        self.ff_ln = _LayerNorm(C_)                                                         # num_blocks_i/feedforward/LayerNorm
        self.ff = _FeedForward(C_, gen)


class SASRec(Sequential):
    static_engine_ok = False      # (the static TrainEngine is EasyDGL's; this model trains through train_step / graphed_train_step)

    def __init__(self, num_items, FLAGS):
        super().__init__(num_items, FLAGS)
        self.seed = int(getattr(FLAGS, "seed", 9876))
        gen = torch.Generator().manual_seed(self.seed)
        C_ = self.width_true = self.num_units
        check_width("SASREC", C_, self.num_heads)
        self.item_embs = C.Embedding(num_items, C_, self.l2_reg, zero_pad=True, scale=True, gen=gen)     # SASREC.py:24-25
        self.pcoding = C.PositionCoding(self.seqslen, C_, self.l2_reg, gen=gen)                           # :26
        self.output_bias = self.make_output_bias()                                                        # :28
        self.layers = nn.ModuleList()
        for i in range(FLAGS.num_blocks):
            self.layers.append(_Block(2 * C_ if i == 0 else C_, C_, self.num_heads, self.attention_probs_dropout_rate, gen))
        self.out_ln = _LayerNorm(C_)                                                                      # output_ln

    def _pad_specs(self):
        return specs_from_map(self._tf_map())

    def l2_param_names(self):
        return ["item_embs.lookup_table", "pcoding.pembs.lookup_table"]

    def encoder(self, features, is_training, gather_pos):
        """SASREC.py:39-64: rows of the final LayerNorm at gather_pos (None: all positions)."""
        ids = features["seqs_i"].contiguous()
        tab = self.item_embs.lookup_table
        x = ops.EmbedCatFn.apply(tab, self.pcoding.pembs.lookup_table, self.compute(tab), ids,
                                 self._drop(self.hidden_dropout_rate, 1, is_training), self.act_dtype, self.deterministic)   # :43-49
        x = ops.mask_rows(x, ids)                                                                          # :53 (the position half)
        for i, blk in enumerate(self.layers):
            qn = ops.AddLayerNormFn.apply(x, None, blk.att_ln.gamma, blk.att_ln.beta, ops.NO_DROP, None)   # :57
            att = blk.attention(qn, x, is_training, True, ids=ids,
                                drop=self._drop(self.attention_probs_dropout_rate, 10 + 4 * i, is_training))
            y = ops.AddLayerNormFn.apply(att, None, blk.ff_ln.gamma, blk.ff_ln.beta, ops.NO_DROP, None)    # :60
            x = self._feed_forward(y, blk.ff, i, ids, is_training)                                         # Base.py:79-86, :61
        return ops.AddLayerNormFn.apply(x, None, self.out_ln.gamma, self.out_ln.beta, ops.NO_DROP, gather_pos)   # :63-70

    def forward(self, features: Dict[str, torch.Tensor], is_training: bool):
        gp = None if is_training else self._last_pos(features["seqs_i"])
        rows = self.encoder(features, is_training, gp).reshape(-1, self.num_units)
        tab = self.item_embs.lookup_table
        return ops.ScoreLogitsFn.apply(rows, tab, self.output_bias, self.compute(tab))                     # :72-75

    def train_loss(self, features, labels, *, candidates=None, shared=None):
        """Sequential.train (Base.py:119-131) with the fused scoring / cross-entropy (no [B*T, I] tensor).  `candidates` (int32
        [B*T, N]) or FLAGS.train_negatives > 0: the softmax of every position over its label and its own list (Sequential._score_ce);
        `shared` (int32 [S]) or FLAGS.shared_negatives > 0: over its label and the step's ONE list."""
        rows = self.encoder(features, True, None)
        loss = self._score_ce(rows.reshape(-1, self.num_units), labels.reshape(-1).contiguous(), candidates, shared)
        if self.l2_reg != 0.0:
            for n in self.l2_param_names():
                loss = loss + ops.L2Fn.apply(self.get_parameter(n), self.l2_reg)
        return loss

    # ---- interop with the reference's variable naming (tests / checkpoints converted from TF) ------------------------
    def _tf_map(self):
        """TF variable name -> (parameter, column slice or None)."""
        m = {"SASREC/item_embs/lookup_table": (self.item_embs.lookup_table, None),
             "SASREC/spatial_embs/embedding/lookup_table": (self.pcoding.pembs.lookup_table, None),
             "SASREC/output_bias": (self.output_bias, None),
             "output_ln/LayerNorm/gamma": (self.out_ln.gamma, None), "output_ln/LayerNorm/beta": (self.out_ln.beta, None)}
        C_ = self.num_units
        for i, blk in enumerate(self.layers):
            pre = f"num_blocks_{i}/"
            a = pre + "attention/multihead_attention/"
            m[pre + "attention/LayerNorm/gamma"] = (blk.att_ln.gamma, None)
            m[pre + "attention/LayerNorm/beta"] = (blk.att_ln.beta, None)
            m[a + "dense/kernel"], m[a + "dense/bias"] = (blk.attention.q_kernel, None), (blk.attention.q_bias, None)
            for j in (1, 2):
                sl = slice((j - 1) * C_, j * C_)
                m[a + f"dense_{j}/kernel"], m[a + f"dense_{j}/bias"] = (blk.attention.kv_kernel, sl), (blk.attention.kv_bias, sl)
            m[pre + "feedforward/LayerNorm/gamma"] = (blk.ff_ln.gamma, None)
            m[pre + "feedforward/LayerNorm/beta"] = (blk.ff_ln.beta, None)
            m[pre + "feedforward/Inner/kernel"], m[pre + "feedforward/Inner/bias"] = (blk.ff.inner.kernel, None), (blk.ff.inner.bias, None)
            m[pre + "feedforward/Readout/kernel"], m[pre + "feedforward/Readout/bias"] = (blk.ff.readout.kernel, None), (blk.ff.readout.bias, None)
        return m
