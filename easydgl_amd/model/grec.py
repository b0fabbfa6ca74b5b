"""Mirror of src/model/GREC.py (Yuan et al., WWW'20, as the reference implements it) on the HIP kernels: the gap-filling
encoder / decoder of dilated convolutions.  Every convolution runs with its LayerNorm, ReLU and residual in one kernel
(module/sequential.py MaskedCNN on csrc/k_dconv.hip).

    m = GREC(num_items, FLAGS).finalize("cuda")
    logits = m(features, is_training)          # GREC.__call__ (GREC.py:57-103): [B*masklen, I] (train) / [B, I] (eval)
    loss = m.train_loss(features, labels)      # GREC.train (GREC.py:105-116)

I = num_items + 2 classes (GREC.py:38); the MASK token is ``m.mask_id`` = num_items.  ``features`` as GRECPostProcessor emits them
(dataloader.py:111-156; data.grec_mask_random): training ``seqs_i`` [B, seqslen + 1] the tokens, ``seqs_m`` the tokens with MASK at
the drawn positions, ``masked_positions`` [B, masklen] = those positions - 1 (the row that predicts a masked token), labels the
tokens there; evaluation ``seqs_i`` = tokens[:-1] [B, seqslen] (``seqs_m`` is not read), scored at the last position.

Kept from the reference: two unscaled item tables without a zero row (id 0 has a learned embedding, nothing masks the padding);
the projector dense(2C, tanh-GELU) -> dense(C) with a residual; the regulariser 0.001 * mean over ALL trainable variables of
sum(v^2) / 2 (GREC.py:115); Adam with the defaults; evaluation puts -1000 at class 0 and at the last class (GREC.py:100-102).

Two differences, the project's conventions in every other model (the scoring kernels are shared):
  1. class 0 sits at -1000 in training as well (the reference gives it a learned bias there): the head's bias has I - 1 entries,
     row 0 of the head's kernel takes no gradient from the cross-entropy;
  2. a row whose label is 0 carries no weight, the loss is the mean over the other rows (the reference: a plain mean).
The reference seeds every convolution weight with seed=1, which gives identical draws in all of them; that is not reproduced.

The head's kernel is stored [I, C] so that the scoring ops read it as a table: it is this model's ``item_embs`` for the shared
loss / evaluation scaffold of Sequential; tf_values() / tf_gradients() / load_tf_variables() speak the reference's [C, I].

No f32 atomics in the convolution kernels (there is no second form for FLAGS.deterministic); the two tables take the flag.
Not built: channel padding, a device loader, the static TrainEngine, a captured step, lazy_adam, a kernel that fuses both
convolutions of a unit."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch
from torch import nn

from .. import ops
from ..module import coding as C
from ..module import sequential as S
from ..module.coding import glorot_uniform_
from .base import Sequential, _Dense
from .sasrec import specs_from_map

HEAD_KERNEL = "cls/predictions/transform/dense/kernel"
L2_COEF = 0.001                  # GREC.py:115


def parse_dilations(text) -> list:
    """--dilations "1,2,2,4" -> [1, 2, 2, 4] (GREC.py:41)."""
    out = [int(v) for v in str(text).split(",") if v.strip()]
    if not out or min(out) < 1:
        raise ValueError(f"--dilations {text!r}: a comma-separated list of integers >= 1")
    return out


class _Head(nn.Module):
    """cls/predictions/transform/dense: the kernel stored [I, C] (a table for the scoring kernels), glorot over (C, I)."""

    def __init__(self, num_classes, num_units, gen):
        super().__init__()
        self.lookup_table = nn.Parameter(glorot_uniform_(torch.empty(num_classes, num_units), gen))


class GREC(Sequential):
    static_engine_ok = False

    def __init__(self, num_items, FLAGS):
        super().__init__(num_items, FLAGS)
        self.mask_id = num_items                   # util.py:108 (not `mask`: the driver feeds a model with `mask` EasyDGL's batches)
        self.num_items += 2                        # GREC.py:38
        self.masklen = int(FLAGS.masklen)
        self.filter_width = int(getattr(FLAGS, "filter_width", 3))
        self.dilations = parse_dilations(getattr(FLAGS, "dilations", "1,2,2,4"))
        self.seed = int(getattr(FLAGS, "seed", 9876))
        gen = torch.Generator().manual_seed(self.seed)
        C_ = self.width_true = self.num_units
        if C_ > 512 or C_ < 32 or C_ & (C_ - 1):
            raise ValueError(f"GREC: num_units={C_} unsupported: the HIP kernels take a power of two in [32, 512] (--num_units; "
                             "this model is not channel-padded)")
        if not 1 <= self.seqslen <= 1024:
            raise ValueError(f"GREC: seqslen={self.seqslen} unsupported; the HIP kernels take 1 <= seqslen <= 1024 (--seqslen)")
        for d in self.dilations:                   # what the LDS image cannot hold is refused here, before any launch
            ops.dconv_check(C_, self.filter_width, 2 * d, self.act_dtype, "GREC")
        for name in ("train_negatives", "shared_negatives"):
            if int(getattr(FLAGS, name, 0) or 0) > 0:
                raise ValueError(f"GREC: {name} is not supported (the model trains on the full softmax, GREC.py:105-116)")
        self.enc_embs = C.Embedding(self.num_items, C_, self.l2_reg, zero_pad=False, scale=False, gen=gen,
                                    deterministic=self.deterministic)                                     # GREC.py:44-45
        self.decc_embs = C.Embedding(self.num_items, C_, self.l2_reg, zero_pad=False, scale=False, gen=gen,
                                     deterministic=self.deterministic)                                    # :46-47
        for emb in (self.enc_embs, self.decc_embs):
            S.truncated_normal_(emb.lookup_table.data, gen)
        self.regu = nn.ModuleList(S.MaskedCNN(self.filter_width, C_, d, False, gen) for d in self.dilations)   # :49-55
        self.masked = nn.ModuleList(S.MaskedCNN(self.filter_width, C_, d, True, gen) for d in self.dilations)
        self.proj_inner = _Dense(C_, 2 * C_, gen)                                                         # projector/dense
        self.proj_out = _Dense(2 * C_, C_, gen)                                                           # projector/dense_1
        self.item_embs = _Head(self.num_items, C_, gen)                                                   # cls/predictions/transform
        self.output_bias = self.make_output_bias()

    def _pad_specs(self):
        return specs_from_map(self._tf_map())

    def _negatives_hi(self) -> int:
        return self.mask_id   # (the MASK row and the class behind it are not items)

    def encoder(self, features, is_training, gather_pos):
        """GREC.py:57-97: relu of the rows that are scored, [B, M, C] at gather_pos [B, M]."""
        ids_dec = features["seqs_i"].contiguous()
        ids_enc = features["seqs_m"].contiguous() if is_training else ids_dec                            # :59-62
        x = self.enc_embs(ids_enc)                                                                        # :64
        dec = self.decc_embs(ids_dec)                                                                     # :65
        if x.dtype != self.act_dtype:
            x, dec = x.to(self.act_dtype), dec.to(self.act_dtype)
        for unit in self.regu:                                                                            # :68-71
            x = unit(x, is_training)
        inp = ops.add(x, dec)                                                                             # :75
        h = ops.GeluTanhFn.apply(self._linear(inp, self.proj_inner))                                      # :76
        x = ops.add(self._linear(h, self.proj_out), inp)                                                  # :77-78
        for unit in self.masked:                                                                          # :81-84
            x = unit(x, is_training)
        return ops.GatherReluFn.apply(x, gather_pos)                                                      # :87-97

    def _gather_pos(self, features, is_training):
        return features["masked_positions"] if is_training else self._last_pos(features["seqs_i"])

    def forward(self, features: Dict[str, torch.Tensor], is_training: bool):
        rows = self.encoder(features, is_training, self._gather_pos(features, is_training)).reshape(-1, self.num_units)
        tab = self.item_embs.lookup_table
        logits = ops.ScoreLogitsFn.apply(rows, tab, self.output_bias, self.compute(tab))                  # :98
        if not is_training:
            with torch.no_grad():
                logits[:, -1] = -1000.0                                                                   # :100-102 (class 0: the kernels)
        return logits

    def train_loss(self, features, labels, *, candidates=None, shared=None):
        """GREC.train (GREC.py:105-116) with the fused scoring / cross-entropy and the regulariser over every variable."""
        if candidates is not None or shared is not None:
            raise ValueError("GREC trains on the full softmax: no candidate lists")
        rows = self.encoder(features, True, features["masked_positions"])
        loss = self._score_ce(rows.reshape(-1, self.num_units).contiguous(), labels.reshape(-1).contiguous())
        params = list(self.parameters())
        for p in params:                                                                                  # :115
            loss = loss + ops.L2Fn.apply(p, L2_COEF / len(params))
        return loss

    # ---- interop with the reference's variable naming (tests / checkpoints converted from TF) ------------------------
    def _tf_map(self):
        """TF variable name -> (parameter, column slice or None).  The head's kernel is stored transposed (see _padded_values)
        and its bias has no entry for class 0."""
        m = {"GREC/enc_embs/lookup_table": (self.enc_embs.lookup_table, None),
             "GREC/decc_embs/lookup_table": (self.decc_embs.lookup_table, None),
             "projector/dense/kernel": (self.proj_inner.kernel, None), "projector/dense/bias": (self.proj_inner.bias, None),
             "projector/dense_1/kernel": (self.proj_out.kernel, None), "projector/dense_1/bias": (self.proj_out.bias, None),
             HEAD_KERNEL: (self.item_embs.lookup_table, None),
             "cls/predictions/transform/dense/bias": (self.output_bias, None)}
        for scope, units in (("regudCNN", self.regu), ("maskedCNN", self.masked)):
            for i, u in enumerate(units):
                pre = f"block_{i}/{scope}_{i}/"
                for k, conv in enumerate((u.dconv0, u.dconv1)):
                    m[pre + f"dconv{k}/weight"], m[pre + f"dconv{k}/bias"] = (conv.weight, None), (conv.bias, None)
                    m[pre + f"ln{k}/gamma"] = (getattr(u, f"ln{k}_gamma"), None)
                    m[pre + f"ln{k}/beta"] = (getattr(u, f"ln{k}_beta"), None)
        return m

    def _padded_values(self, grad: bool):
        out = super()._padded_values(grad)
        out[HEAD_KERNEL] = out[HEAD_KERNEL].t().contiguous()      # the reference's [C, I]
        return out

    @torch.no_grad()
    def load_tf_variables(self, values) -> None:
        values = dict(values)
        values[HEAD_KERNEL] = np.asarray(values[HEAD_KERNEL]).T
        super().load_tf_variables(values)
