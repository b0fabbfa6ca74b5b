"""Mirror of src/module/sequential.py: MultiHeadAttention (Vaswani et al., the unit of SASRec) on the generic masked attention
kernel in its plain-head form (Dq == Dv, csrc/k_tattn.hip), and the GRU layer S2PNM puts in front of it (the reference's
compat/cudnn_rnn.py CudnnGRU) on the recurrence kernel csrc/k_gru.hip; TimelyREC's MATEncoder and TAHEncoder on csrc/k_mate.hip
and csrc/k_tahe.hip; GREC's MaskedCNN (two dilated convolutions, each with LayerNorm and ReLU, and a residual) on csrc/k_dconv.hip;
BERT4REC's BERTAttention (bidirectional, key mask only, no residual) on csrc/k_battn.hip.  Not in the reference: the LSTM form of
the GRU layer (csrc/k_lstm.hip) and NARM's AdditiveAttention over the GRU states (csrc/k_addattn.hip)."""
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
    a zero input row still moves the state through the biases.  ``forward(x)``: x [B,T,in] -> h [B,T,C].  ``wide``: where R is
    not LDS-resident at the activation dtype the recurrence runs on the pipelined stream (csrc/k_gru_wide.hip); a
    resident pack is at its LDS form already and keeps the existing kernels."""

    def __init__(self, num_units, in_units=None, gen=None, wide=False):
        super().__init__()
        if num_units % 16 or not 16 <= num_units <= 512:
            raise ValueError(f"GRU: num_units={num_units} unsupported; the HIP recurrence takes a multiple of 16 in [16, 512]")
        in_units = num_units if in_units is None else in_units
        self.num_units = num_units
        self.wide = bool(wide)
        self.w_kernel = nn.Parameter(torch.cat([orthogonal_(torch.empty(in_units, num_units), gen) for _ in range(3)], dim=1))
        self.w_bias = nn.Parameter(torch.zeros(3 * num_units))
        self.r_kernel = nn.Parameter(torch.cat([orthogonal_(torch.empty(num_units, num_units), gen) for _ in range(3)], dim=1))
        self.r_bias = nn.Parameter(torch.zeros(3 * num_units))
        self.compute = lambda p: p  # replaced by the owning model (bf16 shadow lookup)

    def forward(self, x):
        xp = ops.LinearFn.apply(x, self.w_kernel, self.w_bias, self.compute(self.w_kernel), False)
        wide = self.wide and ops.lib.edgl_gru_seq_resident(self.num_units, ops._DT[xp.dtype]) == 0
        return ops.GruSeqFn.apply(xp, self.r_kernel, self.r_bias, self.compute(self.r_kernel), wide)


class LSTM(nn.Module):
    """One unidirectional LSTM layer in cuDNN's form (compat/cudnn_rnn.py: the CUDNN_LSTM branches of _CudnnRNN; linear input,
    zero initial h and c, no forget-gate offset, no projection, no peepholes, no dropout): gate order i, f, g, o — cuDNN's and
    torch.nn.LSTM's.  ``w_kernel`` [in, 4C] / ``w_bias`` [4C] act on the input, ``r_kernel`` [C, 4C] / ``r_bias`` [4C] on the state;
    the gate blocks are column blocks, each of the eight matrices drawn with the orthogonal initialiser on its own, the biases
    zero.  Padded positions are steps like any other.  ``forward(x)``: x [B,T,in] -> h [B,T,C] on csrc/k_lstm.hip,
    one kernel family at every width."""

    def __init__(self, num_units, in_units=None, gen=None):
        super().__init__()
        if num_units % 16 or not 16 <= num_units <= 512:
            raise ValueError(f"LSTM: num_units={num_units} unsupported; the HIP recurrence takes a multiple of 16 in [16, 512]")
        in_units = num_units if in_units is None else in_units
        self.num_units = num_units
        self.w_kernel = nn.Parameter(torch.cat([orthogonal_(torch.empty(in_units, num_units), gen) for _ in range(4)], dim=1))
        self.w_bias = nn.Parameter(torch.zeros(4 * num_units))
        self.r_kernel = nn.Parameter(torch.cat([orthogonal_(torch.empty(num_units, num_units), gen) for _ in range(4)], dim=1))
        self.r_bias = nn.Parameter(torch.zeros(4 * num_units))
        self.compute = lambda p: p  # replaced by the owning model (bf16 shadow lookup)

    def forward(self, x):
        xp = ops.LinearFn.apply(x, self.w_kernel, self.w_bias, self.compute(self.w_kernel), False)
        return ops.LstmSeqFn.apply(xp, self.r_kernel, self.r_bias, self.compute(self.r_kernel))


class AdditiveAttention(nn.Module):
    """The attention of NARM (Li et al., CIKM'17, eq. 7-8) over the states of a recurrent encoder, every position a query:
    alpha[t,j] = v^T sigmoid(A1 h[t] + A2 h[j]) for the keys j <= t with ids[j] != 0, c[t] = sum_j alpha[t,j] h[j]; no softmax,
    as in the paper.  ``a_kernel`` [C, 2C] holds A1 | A2 as column blocks (each glorot uniform, no bias: both read the same
    input, one GEMM), ``v`` [C] is glorot uniform as a [C, 1] matrix.  ``forward(h, ids, cat=False)``: h [B,T,C] -> c [B,T,C], or
    [h | c] [B,T,2C] with ``cat`` (csrc/k_addattn.hip)."""

    def __init__(self, num_units, gen=None):
        super().__init__()
        if num_units % 16 or not 16 <= num_units <= 512:
            raise ValueError(f"AdditiveAttention: num_units={num_units} unsupported; the HIP kernels take a multiple of 16 in [16, 512]")
        self.num_units = num_units
        self.a_kernel = nn.Parameter(torch.cat([glorot_uniform_(torch.empty(num_units, num_units), gen) for _ in range(2)], dim=1))
        self.v = nn.Parameter(glorot_uniform_(torch.empty(num_units, 1), gen).reshape(num_units))
        self.register_buffer("no_bias", torch.zeros(2 * num_units), persistent=False)     # (tf.layers.dense(use_bias=False))
        self.compute = lambda p: p  # replaced by the owning model (bf16 shadow lookup)

    def forward(self, h, ids, cat=False):
        a12 = ops.LinearFn.apply(h, self.a_kernel, self.no_bias, self.compute(self.a_kernel), False)
        return ops.AddAttnFn.apply(h, a12, self.v, ids, cat)


def truncated_normal_(t: torch.Tensor, gen: torch.Generator, std: float = 0.02) -> torch.Tensor:
    """tf.truncated_normal_initializer(stddev=std): N(0, std), a value beyond two standard deviations is drawn again."""
    v = torch.randn(t.shape, generator=gen)
    while True:
        bad = v.abs() > 2.0
        if not bool(bad.any()):
            break
        v[bad] = torch.randn(int(bad.sum()), generator=gen)
    with torch.no_grad():
        t.copy_(v * std)
    return t


class BERTAttention(nn.Module):
    """sequential.py:86-137 (BERT's self-attention, the unit of BERT4REC).  ``qkv_kernel`` [C, 3C] / ``qkv_bias`` [3C] hold the
    reference's Q | K | V dense layers as column blocks: the three read the same input, so they run as ONE GEMM and the
    attention kernel (csrc/k_battn.hip) reads its operands as column blocks of that output.  Each block is truncated-normal with
    sigma 0.02, the biases zero.  Bidirectional: the only mask is the key mask ``ids != 0`` (BERT4REC.py:75-77), a masked score is
    REPLACED by float32(-2^32+1); no residual and no LayerNorm inside.

    ``forward(queries, keys, ids, is_training, drop=...)``: the reference's arguments with the key ids in place of the [B,T,T]
    mask it builds from them; ``queries is keys`` is the only form the reference uses (BERT4REC.py:90) and the only one taken."""

    def __init__(self, num_units, num_heads, dropout_rate, gen=None):
        super().__init__()
        dh = num_units // num_heads if num_heads > 0 and num_units % num_heads == 0 else 0
        ops.battn_check(1, num_heads, dh, torch.float32, "BERTAttention")
        self.num_units, self.num_heads, self.dropout_rate = num_units, num_heads, dropout_rate
        qkv = torch.cat([truncated_normal_(torch.empty(num_units, num_units), gen) for _ in range(3)], dim=1)
        self.qkv_kernel = nn.Parameter(qkv)                                                           # Q | K | V
        self.qkv_bias = nn.Parameter(torch.zeros(3 * num_units))
        self.compute = lambda p: p  # replaced by the owning model (bf16 shadow lookup)

    def forward(self, queries, keys, ids, is_training, *, drop: ops.Drop = ops.NO_DROP):
        if keys is not queries:
            raise ValueError("BERTAttention: the HIP path takes queries is keys (BERT4REC.py:90)")
        qkv = ops.LinearFn.apply(queries, self.qkv_kernel, self.qkv_bias, self.compute(self.qkv_kernel), False)
        return ops.BertAttnFn.apply(qkv, ids, self.num_heads, drop if is_training else ops.NO_DROP)


class Conv1D(nn.Module):
    """sequential.py:140-174, the parameters: ``weight`` [fw, in, out] (the reference's [1, fw, in, out] without the leading 1),
    truncated normal (sigma 0.02), ``bias`` zeros.  The reference seeds every weight with seed=1, i.e. draws the SAME values for
    every convolution of the model; that is not reproduced — each weight takes its own draws from the model's generator."""

    def __init__(self, filter_width, out_channels, dilation, causality, gen=None):
        super().__init__()
        self.filter_width, self.dilation, self.causality = int(filter_width), int(dilation), bool(causality)
        self.weight = nn.Parameter(truncated_normal_(torch.empty(self.filter_width, out_channels, out_channels), gen))
        self.bias = nn.Parameter(torch.zeros(out_channels))


class MaskedCNN(nn.Module):
    """sequential.py:177-207 (Yuan et al., WWW'20): dconv0 (dilation d) -> ln0 -> relu -> dconv1 (dilation 2d) -> ln1 -> relu ->
    + input, as two calls of ops.DConvLnFn (csrc/k_dconv.hip); the second adds the residual in its epilogue.  The LayerNorms are
    normalize.py's (biased variance, epsilon 1e-8).  ``forward(features, is_training)`` keeps the reference's arguments."""

    def __init__(self, filter_width, out_channels, dilation, causality, gen=None):
        super().__init__()
        self.dconv0 = Conv1D(filter_width, out_channels, dilation, causality, gen)
        self.dconv1 = Conv1D(filter_width, out_channels, 2 * dilation, causality, gen)
        self.ln0_gamma, self.ln0_beta = nn.Parameter(torch.ones(out_channels)), nn.Parameter(torch.zeros(out_channels))
        self.ln1_gamma, self.ln1_beta = nn.Parameter(torch.ones(out_channels)), nn.Parameter(torch.zeros(out_channels))
        self.compute = lambda p: p  # replaced by the owning model (bf16 shadow lookup)

    def forward(self, features, is_training=False):
        c0, c1 = self.dconv0, self.dconv1
        y = ops.DConvLnFn.apply(features, c0.weight, c0.bias, self.ln0_gamma, self.ln0_beta, self.compute(c0.weight), c0.dilation,
                                c0.causality, None)
        return ops.DConvLnFn.apply(y, c1.weight, c1.bias, self.ln1_gamma, self.ln1_beta, self.compute(c1.weight), c1.dilation,
                                   c1.causality, features)
