"""Mirror of src/module/sequential.py: MultiHeadAttention (Vaswani et al., the unit of SASRec) on the generic masked attention
kernel in its plain-head form (Dq == Dv, csrc/k_tattn.hip), and the GRU layer S2PNM puts in front of it (the reference's
compat/cudnn_rnn.py CudnnGRU) on the recurrence kernel csrc/k_gru.hip."""
from __future__ import annotations

import torch
from torch import nn

from .. import ops
from .coding import glorot_uniform_, orthogonal_
from .temporal import SUPPORTED_HEAD_DIMS


class MultiHeadAttention(nn.Module):
    """sequential.py:16-83.  ``q_kernel`` [in, C] (dense), ``kv_kernel`` [in, 2C] (dense_1 | dense_2 as column blocks: K and V read
    the same input, one GEMM), each block glorot, biases zero.  ``in_units`` is the width of ``queries`` / ``keys`` (default
    ``num_units``): PositionCoding concatenates (coding.py:72-74), so the first block of a model sees 2C channels and its residual
    is the first C channels of the (normalised) queries (:78).

    ``forward(queries, keys, is_training, causality, ids=..., drop=...)`` keeps the reference's positional arguments.  The key mask
    is ``ids != 0``: the reference's sign(abs(sum(keys))) (:50) is zero exactly there, because the models multiply the keys by
    ``seqs_masks`` in front of every block (SASREC.py:53,61; S2PNM.py:53) and a real row is not all-zero.  A masked score is
    REPLACED by float32(-2^32+1) (:54-55,62-63), so a query row without a visible key is uniform over all T keys."""

    def __init__(self, num_units, num_heads, dropout_rate, in_units=None, gen=None):
        super().__init__()
        dh = num_units // num_heads if num_heads > 0 and num_units % num_heads == 0 else 0
        if not (dh in SUPPORTED_HEAD_DIMS or (dh > 128 and dh % 128 == 0)):
            raise ValueError(f"MultiHeadAttention: head dim num_units/num_heads = {num_units}/{num_heads} unsupported; the HIP "
                             f"attention kernel takes {SUPPORTED_HEAD_DIMS} or a multiple of 128 (--num_units / --num_heads)")
        self.num_units, self.num_heads, self.dropout_rate = num_units, num_heads, dropout_rate
        in_units = num_units if in_units is None else in_units
        self.q_kernel = nn.Parameter(glorot_uniform_(torch.empty(in_units, num_units), gen))        # dense
        self.q_bias = nn.Parameter(torch.zeros(num_units))
        kv = torch.cat([glorot_uniform_(torch.empty(in_units, num_units), gen) for _ in range(2)], dim=1)
        self.kv_kernel = nn.Parameter(kv)                                                             # dense_1 | dense_2
        self.kv_bias = nn.Parameter(torch.zeros(2 * num_units))
        self.compute = lambda p: p  # replaced by the owning model (bf16 shadow lookup)

    def forward(self, queries, keys, is_training, causality=True, *, ids, drop: ops.Drop = ops.NO_DROP):
        C = self.num_units
        q = ops.LinearFn.apply(queries, self.q_kernel, self.q_bias, self.compute(self.q_kernel), False)
        kv = ops.LinearFn.apply(keys, self.kv_kernel, self.kv_bias, self.compute(self.kv_kernel), False)
        return ops.PlainAttnFn.apply(q, kv, queries[:, :, :C], ids, self.num_heads, drop if is_training else ops.NO_DROP,
                                     bool(causality))


class GRU(nn.Module):
    """One unidirectional GRU layer in cuDNN's form (compat/cudnn_rnn.py: CudnnGRU, linear input, zero initial state, no
    dropout): gate order r, z, n.  ``w_kernel`` [in, 3C] / ``w_bias`` [3C] act on the input, ``r_kernel`` [C, 3C] / ``r_bias`` [3C]
    on the state; the gate blocks are column blocks, each of the six matrices drawn with the orthogonal initialiser, the six
    biases zero (cudnn_rnn.py:340-355; the opaque cuDNN blob is these twelve canonical parts).  Padded positions are NOT skipped:
    a zero input row still moves the state through the biases.  ``forward(x)``: x [B,T,in] -> h [B,T,C]."""

    def __init__(self, num_units, in_units=None, gen=None):
        super().__init__()
        if num_units % 16 or not 16 <= num_units <= 512:
            raise ValueError(f"GRU: num_units={num_units} unsupported; the HIP recurrence takes a multiple of 16 in [16, 512]")
        in_units = num_units if in_units is None else in_units
        self.num_units = num_units
        self.w_kernel = nn.Parameter(torch.cat([orthogonal_(torch.empty(in_units, num_units), gen) for _ in range(3)], dim=1))
        self.w_bias = nn.Parameter(torch.zeros(3 * num_units))
        self.r_kernel = nn.Parameter(torch.cat([orthogonal_(torch.empty(num_units, num_units), gen) for _ in range(3)], dim=1))
        self.r_bias = nn.Parameter(torch.zeros(3 * num_units))
        self.compute = lambda p: p  # replaced by the owning model (bf16 shadow lookup)

    def forward(self, x):
        xp = ops.LinearFn.apply(x, self.w_kernel, self.w_bias, self.compute(self.w_kernel), False)
        return ops.GruSeqFn.apply(xp, self.r_kernel, self.r_bias, self.compute(self.r_kernel))
