"""Mirror of src/module/sequential.py: MultiHeadAttention (Vaswani et al., the unit of SASRec) on the generic masked attention
kernel in its plain-head form (Dq == Dv, csrc/k_tattn.hip), and the GRU layer S2PNM puts in front of it (the reference's
compat/cudnn_rnn.py CudnnGRU) on the recurrence kernel csrc/k_gru.hip; TimelyREC's MATEncoder and TAHEncoder on csrc/k_mate.hip
and csrc/k_tahe.hip."""
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


class MATEncoder(nn.Module):
    """sequential.py:210-237, the multi-aspect time encoder of TimelyREC for its four calendar granularities at once.  The
    reference builds one encoder per granularity and hands it materialised slots; here the slots are never built: ``kernel``
    [C, 4C] holds the four bias-free user projections (``month_mate`` | ``daymate`` | ``weekday_mate`` | ``hour_mate`` as column
    blocks: one GEMM) and the slot attention runs inside csrc/k_mate.hip together with the gated combination of TimelyREC.py:126-135
    (``combine`` [C, C], bias-free).

    ``forward(idx, tables, users)``: idx int64 [4,B,T] (month - 1 | day - 1 | weekday | hour), tables = the four
    coding.Embedding modules, users [B,T,C] -> the combined period information [B,T,C]."""

    def __init__(self, num_units, window_ratio=0.2, gen=None):
        super().__init__()
        if not 0.0 < float(window_ratio) <= 0.5:
            raise ValueError(f"MATEncoder: window_ratio={window_ratio} unsupported; the HIP kernel takes 0 < window_ratio <= 0.5 "
                             "(--window_ratio)")
        self.num_units, self.window_ratio = num_units, float(window_ratio)
        self.windows = ops.mate_windows(window_ratio)
        self.kernel = nn.Parameter(torch.cat([glorot_uniform_(torch.empty(num_units, num_units), gen) for _ in range(4)], dim=1))
        self.combine = nn.Parameter(glorot_uniform_(torch.empty(num_units, num_units), gen))
        self.register_buffer("no_bias", torch.zeros(4 * num_units), persistent=False)     # (tf.layers.dense(use_bias=False))
        self.compute = lambda p: p  # replaced by the owning model (bf16 shadow lookup)

    def forward(self, idx, tables, users):
        C = self.num_units
        u = ops.LinearFn.apply(users, self.kernel, self.no_bias, self.compute(self.kernel), False)
        pq = ops.LinearFn.apply(users, self.combine, self.no_bias[:C], self.compute(self.combine), False)
        masters = [t.lookup_table for t in tables]
        return ops.MateFn.apply(idx, *masters, *[self.compute(m) for m in masters], u, pq, self.windows)


class TAHEncoder(nn.Module):
    """sequential.py:240-265, the time-aware history encoder of TimelyREC: ``forward(queries, keys, histories)`` with the
    reference's arguments.  The reference calls it with the same tensor twice (TimelyREC.py:147, "queries and keys are
    identical"), and that is the only form the kernel (csrc/k_tahe.hip) takes: the l2 normalisation, the cosine weights
    (1 + cos) / 2 under the causal mask (diagonal kept) and the weighted sum of the histories."""

    def forward(self, queries, keys, histories):
        if keys is not queries:
            raise ValueError("TAHEncoder: the HIP kernel takes queries is keys (TimelyREC.py:147)")
        return ops.TaheFn.apply(queries, histories)


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
