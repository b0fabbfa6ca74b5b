"""torch.autograd.Function wrappers over the C ABI (include/easydgl_hip.h).

PyTorch is plumbing here: it owns device memory, the stream and the autograd tape; every op body is
a call into libeasydgl_hip.so.  There is no CPU path — handing a CPU tensor to any op raises."""
from __future__ import annotations

import ctypes
import math
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import BF16, F32, check, lib

_DT = {torch.float32: F32, torch.bfloat16: BF16}


def _ptr(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.EdglError("easydgl_amd ops run on the GPU only (got a CPU tensor); there is no CPU fallback")
    if not t.is_contiguous():
        raise _lib.EdglError("easydgl_amd ops need contiguous tensors")
    return t.data_ptr()


def _vptr(t: torch.Tensor):
    """Pointer of a strided VIEW (a column block of a wider activation buffer); the row stride is passed separately."""
    if not t.is_cuda:
        raise _lib.EdglError("easydgl_amd ops run on the GPU only (got a CPU tensor); there is no CPU fallback")
    if t.stride(-1) != 1:
        raise _lib.EdglError("easydgl_amd ops need unit stride along the last axis")
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _code(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise _lib.EdglError(f"unsupported activation dtype {t.dtype}")


@dataclass
class Drop:
    """Dropout description handed to a kernel: rate, device RNG state (int64[2]: seed, step), stream id."""
    rate: float = 0.0
    state: Optional[torch.Tensor] = None
    stream_id: int = 0

    @property
    def active(self) -> bool:
        return self.rate > 0.0

    def ptr(self):
        return _ptr(self.state) if self.active else None


NO_DROP = Drop()
MAU_CAUSAL, MAU_NO_DIAG, MAU_DIAG_ZERO = _lib.MAU_CAUSAL, _lib.MAU_NO_DIAG, _lib.MAU_DIAG_ZERO
MAU_STREAM = _lib.MAU_STREAM   # host-side hint: the key-streamed kernels at a shape the in-register kernels also take


def make_rng_state(device, seed: int = 9876) -> torch.Tensor:
    """Device RNG state of the counter-based dropout generator: int64[2] = (seed, step)."""
    return torch.tensor([int(seed), 0], device=device, dtype=torch.int64)


def rng_advance(state: torch.Tensor) -> None:
    check(lib.edgl_rng_advance(_ptr(state), _stream()), "edgl_rng_advance")


# ------------------------------------------------------------------------------------------------
# plain helpers (no autograd)
# ------------------------------------------------------------------------------------------------
def gemm(A, Bm, M, N, K, lda, ldb, a_kc, b_kc, out_dtype, bias=None, aux=None, flags=0, splitk=1, ws=None,
         out=None, code=None):
    code = _code(A) if code is None else code
    if out is None:
        out = torch.empty((M, N), device=A.device, dtype=out_dtype)
    if out.dtype == torch.float32:
        flags |= _lib.EPI_OUT_F32
    if splitk > 1 and ws is None:
        ws = torch.empty(splitk * M * N, device=A.device, dtype=torch.float32)
    check(lib.edgl_gemm(_ptr(A), _ptr(Bm), _ptr(out), M, N, K, lda, ldb, out.stride(0), int(a_kc), int(b_kc),
                        _ptr(bias), _ptr(aux), flags, splitk, _ptr(ws), code, _stream()), "edgl_gemm")
    return out


def colsum(X, M, N):
    out = torch.empty(N, device=X.device, dtype=torch.float32)
    ws = torch.empty(256 * N, device=X.device, dtype=torch.float32)
    check(lib.edgl_colsum(_ptr(X), M, N, X.stride(0) if X.dim() == 2 else N, _ptr(out), 0, _ptr(ws),
                          int(X.dtype == torch.float32), _code(X) if X.dtype != torch.float32 else F32, _stream()),
          "edgl_colsum")
    return out


def cast_to(src_f32: torch.Tensor, dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if out is None:
        out = torch.empty(src_f32.shape, device=src_f32.device, dtype=dtype)
    check(lib.edgl_cast(_ptr(src_f32), _ptr(out), src_f32.numel(), _DT[dtype], _stream()), "edgl_cast")
    return out


def dense_grads(x2, dz, M, K, N):
    code = _code(x2)
    # (dW, db) in one buffer, as they sit in the flat gradient arena: the library then reduces both with one launch
    both = torch.empty((K + 1) * N, device=x2.device, dtype=torch.float32)
    dw, db = both[:K * N].view(K, N), both[K * N:]
    ws = torch.empty(lib.edgl_gemm_dw_workspace(M, K, N, code), device=x2.device, dtype=torch.float32)
    check(lib.edgl_gemm_dw(_ptr(x2), _ptr(dz), _ptr(dw), _ptr(db), M, K, N, x2.stride(0), dz.stride(0), 0, _ptr(ws), code,
                           _stream()), "edgl_gemm_dw")
    return dw, db


def _splitk_for(m_out: int, n_out: int, kc: int) -> int:
    tiles = ((m_out + 127) // 128) * ((n_out + 127) // 128)
    return int(max(1, min(kc // 256, max(1, 320 // tiles))))


# ------------------------------------------------------------------------------------------------
# deterministic item-table scatter (csrc/k_segsum.hip)
# ------------------------------------------------------------------------------------------------
def segsum_plan_buffer(n: int, I: int, device) -> torch.Tensor:
    """Device buffer for one plan over n rows (sort scratch and the partial sums of the ordered sum included)."""
    nbytes = int(lib.edgl_segsum_plan_bytes(int(n), int(I)))
    if nbytes <= 0:
        raise _lib.EdglError(f"segsum plan: bad shape n={n} I={I}")
    return torch.empty((nbytes + 3) // 4, device=device, dtype=torch.int32)


def segsum_plan(keys: torch.Tensor, I: int, nvalid: Optional[torch.Tensor] = None, i0: int = 0, i1: Optional[int] = None):
    """The sorted plan of `keys` (int64 [n]) as views into its buffer: (perm [n], seg_key [n], seg_start [n + 1], nseg [1],
    nkept [1]), all int32 on the device — perm[:nkept] are the kept rows by ascending key (ascending rows inside a key),
    seg_key[:nseg] the distinct keys, seg_start[:nseg + 1] their first positions.  For tests and tools."""
    keys = keys.reshape(-1).contiguous()
    n = keys.numel()
    buf = segsum_plan_buffer(n, I, keys.device)
    check(lib.edgl_segsum_plan(_ptr(keys), n, _ptr(nvalid), int(I), int(i0), int(I if i1 is None else i1), _ptr(buf), _stream()),
          "edgl_segsum_plan")
    n4 = (n + 3) // 4 * 4
    return buf[4:4 + n], buf[4 + n4:4 + n4 + n], buf[4 + 2 * n4:4 + 2 * n4 + n + 1], buf[0:1], buf[1:2]


# ------------------------------------------------------------------------------------------------
# K1 encode
# ------------------------------------------------------------------------------------------------
def _table_out(d_table_out, shape, who):
    """The `d_table_out` argument of EncodeFn / SampledCEFn: a contiguous f32 GPU tensor of the table's shape."""
    if d_table_out is None:
        return None
    _ptr(d_table_out)
    if d_table_out.dtype != torch.float32 or tuple(d_table_out.shape) != tuple(shape):
        raise _lib.EdglError(f"{who}: d_table_out must be f32 {tuple(shape)} (got {d_table_out.dtype} {tuple(d_table_out.shape)})")
    return d_table_out


class EncodeFn(torch.autograd.Function):
    """EasyDGL.py:70-95.  item_c is the compute copy of the item table (the f32 master itself, or its
    bf16 shadow); gradients flow to the masters."""

    @staticmethod
    def forward(ctx, item_master, pos_tab, mark_emb, item_c, ids, ts, mark_table, tscale, mask_id, time_scale,
                drop: Drop, act_dtype, pad=(0, 0), deterministic=False, d_table_out=None):
        """pad = (dh_pad, dh_true) of a channel-padded model (model/base.py), (0, 0) otherwise.  deterministic: the backward adds
        the item gradient as ordered sums over a sorted plan (edgl_encode_bwd_add_det) instead of f32 atomics.  d_table_out
        (f32 [I, C]): the backward ADDS the item gradient into it, allocates no [I, C] tensor and returns None for
        the table master."""
        B, T = ids.shape
        I, C = item_c.shape
        E = mark_table.shape[1]
        x0 = torch.empty((B, T, 3 * C), device=ids.device, dtype=act_dtype)
        spans = torch.empty((B, T), device=ids.device, dtype=torch.float32)
        marks = torch.empty((B, T, E), device=ids.device, dtype=torch.uint8)
        check(lib.edgl_encode_fwd_ct(_ptr(ids), _ptr(ts), _ptr(item_c), _ptr(pos_tab), _ptr(mark_emb), _ptr(mark_table),
                                     _ptr(tscale), B, T, C, E, I, int(mask_id), float(time_scale), float(drop.rate),
                                     drop.ptr(), drop.stream_id, _ptr(x0), _ptr(spans), _ptr(marks), int(pad[0]), int(pad[1]),
                                     _DT[act_dtype], _stream()), "edgl_encode_fwd")
        ctx.save_for_backward(ids, marks)
        ctx.c_true = (C // pad[0] * pad[1]) if pad[0] else 0
        ctx.deterministic = bool(deterministic)
        ctx.meta = (B, T, C, E, I, drop, item_master.shape, pos_tab.shape, mark_emb.shape)
        ctx.d_table_out = _table_out(d_table_out, item_master.shape, "EncodeFn")
        ctx.mark_non_differentiable(spans, marks)
        return x0, spans, marks

    @staticmethod
    def backward(ctx, dx0, _ds, _dm):
        ids, marks = ctx.saved_tensors
        B, T, C, E, I, drop, ishape, pshape, mshape = ctx.meta
        dx0 = dx0.contiguous()
        in_place = ctx.d_table_out is not None
        d_item = ctx.d_table_out if in_place else torch.zeros(ishape, device=dx0.device, dtype=torch.float32)
        d_pos = torch.zeros(pshape, device=dx0.device, dtype=torch.float32)
        d_mark = torch.empty(mshape, device=dx0.device, dtype=torch.float32)
        ws = torch.empty(lib.edgl_encode_bwd_workspace(B, T, C), device=dx0.device, dtype=torch.float32)
        if ctx.deterministic:
            plan = segsum_plan_buffer(B * T, I, dx0.device)
            check(lib.edgl_encode_bwd_add_det(_ptr(ids), _ptr(marks), _ptr(dx0), None, None, B, T, C, E, I, float(drop.rate), drop.ptr(),
                                              drop.stream_id, _ptr(d_item), _ptr(d_pos), _ptr(d_mark), _ptr(ws), int(ctx.c_true),
                                              _ptr(plan), _code(dx0), _stream()), "edgl_encode_bwd_add_det")
        else:
            check(lib.edgl_encode_bwd_add_ct(_ptr(ids), _ptr(marks), _ptr(dx0), None, None, B, T, C, E, I, float(drop.rate), drop.ptr(),
                                             drop.stream_id, _ptr(d_item), _ptr(d_pos), _ptr(d_mark), _ptr(ws), int(ctx.c_true),
                                             _code(dx0), _stream()), "edgl_encode_bwd")
        return (None if in_place else d_item, d_pos, d_mark) + (None,) * 12


def _embed_pos_bwd(deterministic, ids, dx0, B, T, C, I, drop: Drop, d_item, d_pos, c_true):
    """edgl_embed_pos_bwd_ct, or its ordered form over a plan buffer of this call's own."""
    if deterministic:
        plan = segsum_plan_buffer(B * T, I, dx0.device)
        check(lib.edgl_embed_pos_bwd_det(_ptr(ids), _ptr(dx0), B, T, C, I, float(drop.rate), drop.ptr(), drop.stream_id,
                                         _ptr(d_item), _ptr(d_pos), c_true, _ptr(plan), _code(dx0), _stream()),
              "edgl_embed_pos_bwd_det")
    else:
        check(lib.edgl_embed_pos_bwd_ct(_ptr(ids), _ptr(dx0), B, T, C, I, float(drop.rate), drop.ptr(), drop.stream_id,
                                        _ptr(d_item), _ptr(d_pos), c_true, _code(dx0), _stream()), "edgl_embed_pos_bwd")


class EmbedPosFn(torch.autograd.Function):
    """CTSMA.py:48-58: X0 = dropout(concat(item[ids]*sqrt(C), pos[0..T))), spans, marks (edgl_embed_pos_fwd/bwd)."""

    @staticmethod
    def forward(ctx, item_master, pos_tab, item_c, ids, ts, mark_table, time_scale, drop: Drop, act_dtype, c_true=0,
                deterministic=False):
        """c_true: the true width of a channel-padded model (0: = C) — coding.py:62-63's sqrt(num_units).  deterministic: the
        backward sums the item rows over a sorted plan and the position rows over b in order (edgl_embed_pos_bwd_det)."""
        B, T = ids.shape
        I, C = item_c.shape
        E = mark_table.shape[1]
        x0 = torch.empty((B, T, 2 * C), device=ids.device, dtype=act_dtype)
        spans = torch.empty((B, T), device=ids.device, dtype=torch.float32)
        marks = torch.empty((B, T, E), device=ids.device, dtype=torch.uint8)
        check(lib.edgl_embed_pos_fwd_ct(_ptr(ids), _ptr(ts), _ptr(item_c), _ptr(pos_tab), _ptr(mark_table), B, T, C, E,
                                        float(time_scale), float(drop.rate), drop.ptr(), drop.stream_id, _ptr(x0), _ptr(spans),
                                        _ptr(marks), int(c_true), _DT[act_dtype], _stream()), "edgl_embed_pos_fwd")
        ctx.save_for_backward(ids)
        ctx.c_true = int(c_true)
        ctx.deterministic = bool(deterministic)
        ctx.meta = (B, T, C, I, drop, item_master.shape, pos_tab.shape)
        ctx.mark_non_differentiable(spans, marks)
        return x0, spans, marks

    @staticmethod
    def backward(ctx, dx0, _ds, _dm):
        (ids,) = ctx.saved_tensors
        B, T, C, I, drop, ishape, pshape = ctx.meta
        dx0 = dx0.contiguous()
        d_item = torch.empty(ishape, device=dx0.device, dtype=torch.float32)
        d_pos = torch.zeros(pshape, device=dx0.device, dtype=torch.float32)
        _embed_pos_bwd(ctx.deterministic, ids, dx0, B, T, C, I, drop, d_item, d_pos, ctx.c_true)
        return (d_item, d_pos) + (None,) * 9


# ------------------------------------------------------------------------------------------------
# K2/K4 dense
# ------------------------------------------------------------------------------------------------
class LinearFn(torch.autograd.Function):
    """tf.layers.dense: y = act(x @ W + b), W [in, out] (Appendix A).  w_c is W in the activation dtype."""

    @staticmethod
    def forward(ctx, x, w_master, bias, w_c, gelu):
        """`gelu`: False / True (erf-GELU, EasyDGL.py:19-32) / "relu" (FeedForward inner layer, Base.py:73)."""
        K, N = w_c.shape
        x2 = x.reshape(-1, K).contiguous()
        M = x2.shape[0]
        relu = gelu == "relu"
        gelu = gelu is True
        flags = _lib.EPI_BIAS | (_lib.EPI_GELU | _lib.EPI_SAVE_PRE if gelu else 0) | (_lib.EPI_RELU if relu else 0)
        pre = torch.empty((M, N), device=x.device, dtype=x.dtype) if gelu else None
        y = gemm(x2, w_c, M, N, K, K, N, True, False, x.dtype, bias=bias, aux=pre, flags=flags)
        ctx.save_for_backward(x2, w_c, y if relu else pre)
        ctx.meta = (M, N, K, "relu" if relu else gelu, x.shape)
        return y.reshape(x.shape[:-1] + (N,))

    @staticmethod
    def backward(ctx, dy):
        x2, w_c, pre = ctx.saved_tensors
        M, N, K, gelu, xshape = ctx.meta
        dz = dy.reshape(M, N).contiguous()
        if gelu == "relu":
            out = torch.empty_like(dz)
            check(lib.edgl_relu_bwd(_ptr(dz), _ptr(pre), _ptr(out), dz.numel(), _code(dz), _stream()), "edgl_relu_bwd")
            dz = out
        elif gelu:
            out = torch.empty_like(dz)
            check(lib.edgl_gelu_bwd(_ptr(dz), _ptr(pre), _ptr(out), dz.numel(), _code(dz), _stream()), "edgl_gelu_bwd")
            dz = out
        # dX[M,K] = dz[M,N] . W^T : B(kk=n, nn=k) = W[k][n] -> stored [K rows][N contiguous] = k-contiguous operand
        dx = gemm(dz, w_c, M, K, N, N, N, True, True, dz.dtype)
        # dW[K,N] = X^T . dz and db = colsum(dz): contraction over the rows of two row-major operands
        dw, db = dense_grads(x2, dz, M, K, N)
        return dx.reshape(xshape), dw, db, None, None


class DualLinearFn(torch.autograd.Function):
    """Q = dense(xq, C) and K | V | T_ = dense(xk, 3C) written as the column blocks of ONE [.., 4C] operand — MAU.__call__'s four
    projections (temporal.py:352-355) in the layout the fused attention kernel reads, without a concatenation copy (forward) or
    slice copies (backward): the GEMMs take the row stride 4C of the shared buffer."""

    @staticmethod
    def forward(ctx, xq, xk, wq_master, bq, wq_c, wk_master, bk, wk_c):
        Kq, C = wq_c.shape
        Kk, C3 = wk_c.shape
        xq2, xk2 = xq.reshape(-1, Kq).contiguous(), xk.reshape(-1, Kk).contiguous()
        M = xq2.shape[0]
        out = torch.empty((M, C + C3), device=xq.device, dtype=xq.dtype)
        code, st = _code(xq2), _stream()
        for x2, w, b, K, N, col in ((xq2, wq_c, bq, Kq, C, 0), (xk2, wk_c, bk, Kk, C3, C)):
            check(lib.edgl_gemm(_ptr(x2), _ptr(w), _vptr(out[:, col:]), M, N, K, K, N, out.stride(0), 1, 0, _ptr(b), None, _lib.EPI_BIAS, 1,
                                None, code, st), "edgl_gemm")
        ctx.save_for_backward(xq2, xk2, wq_c, wk_c)
        ctx.meta = (M, C, C3, Kq, Kk, xq.shape, xk.shape)
        return out.reshape(xq.shape[:-1] + (C + C3,))

    @staticmethod
    def backward(ctx, dy):
        xq2, xk2, wq_c, wk_c = ctx.saved_tensors
        M, C, C3, Kq, Kk, qshape, kshape = ctx.meta
        dz = dy.reshape(M, C + C3).contiguous()
        code, st = _code(dz), _stream()
        res = []
        for x2, w, K, N, col in ((xq2, wq_c, Kq, C, 0), (xk2, wk_c, Kk, C3, C)):
            dzv = dz[:, col:col + N]                                   # column block, row stride 4C
            dx = torch.empty((M, K), device=dz.device, dtype=dz.dtype)
            check(lib.edgl_gemm(_vptr(dzv), _ptr(w), _ptr(dx), M, K, N, dz.stride(0), N, K, 1, 1, None, None, 0, 1, None, code, st),
                  "edgl_gemm")
            both = torch.empty((K + 1) * N, device=dz.device, dtype=torch.float32)
            ws = torch.empty(lib.edgl_gemm_dw_workspace(M, K, N, code), device=dz.device, dtype=torch.float32)
            check(lib.edgl_gemm_dw(_ptr(x2), _vptr(dzv), _ptr(both), both.data_ptr() + 4 * K * N, M, K, N, K, dz.stride(0), 0, _ptr(ws), code,
                                   st), "edgl_gemm_dw")
            res.append((dx, both[:K * N].view(K, N), both[K * N:]))
        (dxq, dwq, dbq), (dxk, dwk, dbk) = res
        return dxq.reshape(qshape), dxk.reshape(kshape), dwq, dbq, None, dwk, dbk, None


# ------------------------------------------------------------------------------------------------
# K3 BiMAU
# ------------------------------------------------------------------------------------------------
class BiMAUFn(torch.autograd.Function):
    """Fused attention of BiMAU.__call__ (temporal.py:413-447) given qkvt = dense(x)."""

    @staticmethod
    def forward(ctx, qkvt, resid, W1, b1, w, scaling, ids, spans, marks, H, drop: Drop, flags: int = 0, qk_scale: float = 0.0):
        """qk_scale: the score scale (0 = 1 / sqrt(head dim)); a channel-padded model passes 1 / sqrt(true head dim)."""
        B, T, C4 = qkvt.shape
        C = C4 // 4
        E = w.shape[0]
        code = _code(qkvt)
        # the kernel reads `ids` as B*T 64-bit words: the reference's [h*B,T,T] float mask handed through unchanged would be read
        # as garbage ids without any error (module/temporal.py key_ids_from_masks converts it)
        if ids.dtype != torch.int64 or tuple(ids.shape) != (B, T) or not ids.is_contiguous() or ids.device != qkvt.device:
            raise _lib.EdglError(f"BiMAU: key ids / mask must be a contiguous int64 [B={B}, T={T}] tensor on {qkvt.device}, got "
                                 f"{tuple(ids.shape)} {ids.dtype}")
        pack = torch.empty(lib.edgl_bimau_pack_bytes(C, H, E, code), device=qkvt.device, dtype=torch.uint8)
        check(lib.edgl_bimau_pack(_ptr(W1), _ptr(b1), _ptr(w), _ptr(scaling), C, H, E, _ptr(pack), code, _stream()),
              "edgl_bimau_pack")
        out = torch.empty((B, T, C), device=qkvt.device, dtype=qkvt.dtype)
        lam = torch.empty((H * B, T, E), device=qkvt.device, dtype=torch.float32)
        if resid.stride(-1) != 1 or resid.stride(0) != T * resid.stride(1):
            raise _lib.EdglError("BiMAU residual must be a row-strided view of a contiguous [B,T,*] tensor")
        need_grad = any(ctx.needs_input_grad)
        # head dims >= 64 and the key-streamed form (long T, or MAU_STREAM) run as scores phase -> intensity kernel -> values phase
        # and hand H rows / z (/ the softmax statistics) through `saved`
        form = lib.edgl_bimau_form(T, C, H, code, int(flags))
        need_saved = need_grad or (C // H) >= 64 or form == 1
        saved = torch.empty(max(lib.edgl_bimau_saved_bytes_ex(B, T, C, H, code, int(flags)), 0), device=qkvt.device, dtype=torch.uint8) if need_saved else None
        check(lib.edgl_bimau_fwd_db(_ptr(qkvt), resid.data_ptr(), resid.stride(1), _ptr(ids), _ptr(spans), _ptr(marks),
                                    _ptr(pack), B, T, C, H, E, float(drop.rate), drop.ptr(), drop.stream_id, None, float(qk_scale),
                                    _ptr(out), _ptr(lam), _ptr(saved), None, int(flags), code, _stream()), "edgl_bimau_fwd")
        if need_grad:
            ctx.save_for_backward(qkvt, ids, spans, marks, pack, lam, saved)
        ctx.qk_scale = float(qk_scale)
        ctx.meta = (B, T, C, H, E, drop, code, W1.shape, b1.shape, w.shape, scaling.shape, int(flags))
        return out, lam

    @staticmethod
    def backward(ctx, d_out, d_lam):
        qkvt, ids, spans, marks, pack, lam, saved = ctx.saved_tensors
        B, T, C, H, E, drop, code, s1, s2, s3, s4, flags = ctx.meta
        d_out = d_out.contiguous()
        dev = d_out.device
        d_qkvt = torch.empty_like(qkvt)
        # dW1 | db1 | dw | dscaling in one buffer (the flat-arena order): the library reduces all four with one launch
        n1, n2, n3, n4 = (int(np.prod(sh)) for sh in (s1, s2, s3, s4))
        both = torch.empty(n1 + n2 + n3 + n4, device=dev, dtype=torch.float32)
        dW1, db1 = both[:n1].view(s1), both[n1:n1 + n2].view(s2)
        dw, dsc = both[n1 + n2:n1 + n2 + n3].view(s3), both[n1 + n2 + n3:].view(s4)
        ws = torch.empty(lib.edgl_bimau_bwd_workspace_ex(B, T, C, H, E, code, flags), device=dev, dtype=torch.uint8)
        dl = d_lam.contiguous() if d_lam is not None else None
        check(lib.edgl_bimau_bwd_db(_ptr(qkvt), _ptr(ids), _ptr(spans), _ptr(marks), _ptr(pack), _ptr(d_out), _ptr(dl),
                                    _ptr(lam), _ptr(saved), B, T, C, H, E, float(drop.rate), drop.ptr(), drop.stream_id, None,
                                    ctx.qk_scale, _ptr(d_qkvt), _ptr(dW1), _ptr(db1), _ptr(dw), _ptr(dsc), _ptr(ws), flags, code,
                                    _stream()), "edgl_bimau_bwd")
        return d_qkvt, d_out, dW1, db1, dw, dsc, None, None, None, None, None, None, None


# ------------------------------------------------------------------------------------------------
# K4-LN
# ------------------------------------------------------------------------------------------------
class AddLayerNormFn(torch.autograd.Function):
    """y = layernorm_joint(dropout(x) + resid) (Base.py:12-67; EasyDGL.py:114-116,126-128,139), optionally
    emitting only the rows gather_pos [B,Mg] (EasyDGL.py:142-146)."""

    @staticmethod
    def forward(ctx, x, resid, gamma, beta, drop: Drop, gather_pos, pad=(0, 0)):
        B, T, C = x.shape
        code = _code(x)
        stats = torch.empty((B, 2), device=x.device, dtype=torch.float32)
        Mg = 0 if gather_pos is None else gather_pos.shape[1]
        y = torch.empty((B * Mg, C) if gather_pos is not None else (B, T, C), device=x.device, dtype=x.dtype)
        rptr, ld = (None, 0)
        if resid is not None:
            if resid.stride(-1) != 1 or resid.stride(0) != T * resid.stride(1):
                raise _lib.EdglError("layernorm residual must be a row-strided view of a contiguous [B,T,*] tensor")
            rptr, ld = resid.data_ptr(), resid.stride(1)
        check(lib.edgl_add_layernorm_fwd_ct(_ptr(x), rptr, ld, _ptr(gamma), _ptr(beta), B, T, C, float(drop.rate),
                                            drop.ptr(), drop.stream_id, _ptr(gather_pos), Mg, _ptr(y), _ptr(stats),
                                            int(pad[0]), int(pad[1]), code, _stream()), "edgl_add_layernorm_fwd")
        ctx.save_for_backward(x, resid, gamma, stats, gather_pos)
        ctx.pad = (int(pad[0]), int(pad[1]))
        ctx.meta = (B, T, C, drop, code, Mg)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, resid, gamma, stats, gather_pos = ctx.saved_tensors
        B, T, C, drop, code, Mg = ctx.meta
        dy = dy.contiguous()
        dsum = torch.empty_like(x)
        dxd = torch.empty_like(x) if drop.active else None
        both = torch.empty(2 * C, device=x.device, dtype=torch.float32)   # dbeta | dgamma adjacent: one reduction launch
        db, dg = both[:C], both[C:]
        ws = torch.empty(B * 2 * C, device=x.device, dtype=torch.float32)
        rptr, ld = (None, 0) if resid is None else (resid.data_ptr(), resid.stride(1))
        check(lib.edgl_add_layernorm_bwd_act_ct(_ptr(x), rptr, ld, _ptr(gamma), _ptr(stats), _ptr(dy), B, T, C,
                                                float(drop.rate), drop.ptr(), drop.stream_id, _ptr(gather_pos), Mg, None, None,
                                                _ptr(dsum), _ptr(dxd), _ptr(dg), _ptr(db), _ptr(ws), ctx.pad[0], ctx.pad[1], code,
                                                _stream()), "edgl_add_layernorm_bwd")
        dx = dxd if drop.active else dsum
        return dx, (dsum if resid is not None else None), dg, db, None, None, None


# ------------------------------------------------------------------------------------------------
# K5 scoring + CE
# ------------------------------------------------------------------------------------------------
def compact_rows(rows, labels):
    """Weighted rows (label != 0) first: returns rows_c, labels_c, perm, inv, nvalid (all on device)."""
    R, C = rows.shape
    dev = rows.device
    perm = torch.empty(R, device=dev, dtype=torch.int32)
    inv = torch.empty(R, device=dev, dtype=torch.int32)
    nvalid = torch.empty(1, device=dev, dtype=torch.int32)
    rows_c = torch.empty_like(rows)
    labels_c = torch.empty_like(labels)
    check(lib.edgl_compact_rows(_ptr(rows), _ptr(labels), R, C, _ptr(perm), _ptr(inv), _ptr(nvalid), _ptr(rows_c),
                                _ptr(labels_c), _code(rows), _stream()), "edgl_compact_rows")
    return rows_c, labels_c, perm, inv, nvalid


def score_lse(rows, table_c, out_bias, labels, i0, i1, want_logits=False, nvalid=None, want_lse=True):
    R, C = rows.shape
    I = table_c.shape[0]
    dev = rows.device
    lse = torch.empty(R, device=dev, dtype=torch.float32) if want_lse else None     # (None: the logits tile only — evaluation)
    lab_logit = torch.zeros(R, device=dev, dtype=torch.float32) if labels is not None or want_lse else None
    logits = torch.empty((R, i1 - i0), device=dev, dtype=torch.float32) if want_logits else None
    ws = torch.empty(2 * R * lib.edgl_score_chunks(R, i1 - i0), device=dev, dtype=torch.float32)
    check(lib.edgl_score_lse_fwd(_ptr(rows), _ptr(table_c), _ptr(out_bias), _ptr(labels), R, C, I, i0, i1, _ptr(nvalid),
                                 _ptr(lse), _ptr(lab_logit), _ptr(logits), _ptr(ws), _code(rows), _stream()),
          "edgl_score_lse_fwd")
    return lse, lab_logit, logits


VP_FLASH = os.environ.get("EDGL_VP_FLASH", "1") != "0"      # vocab-parallel loss through the flash / strip kernels (0: the two-pass kernels)


def vocab_parallel_ce(rows, table_c, out_bias, labels, group=None):
    """parallel.vocab_parallel_ce with the HIP scoring kernels: every rank holds the same rows [R, C] / labels [R] and scores them
    against its row shard of the (replicated, un-scaled, tied) item table over the item range [i0, i1) with the GLOBAL log-sum-exp —
    the flash form (edgl_score_flash_fwd / _bwd: the strip kernels at the bf16 widths they cover; the row finish takes the gathered
    sums) or, with EDGL_VP_FLASH=0, the two-pass kernels edgl_score_lse_fwd / edgl_score_ce_bwd.  Returns (loss, d_rows [R, C] f32, d_table [I, C] f32 — zero outside the
    rank's shard —, d_bias [I - 1] f32 — zero outside it —, (i0, i1)).  EasyDGL.py:149-155,177-185."""
    from . import parallel
    rows = rows.contiguous()
    labels = labels.reshape(-1).contiguous()
    R, C = rows.shape
    I = table_c.shape[0]
    dev, code, st = rows.device, _code(rows), _stream()
    d_table = torch.zeros((I, C), device=dev, dtype=torch.float32)
    d_bias = torch.zeros(I - 1, device=dev, dtype=torch.float32)
    if VP_FLASH:
        # the flash form over the rank's item range (the strip kernels at bf16 C = 128 / 256 / 512): ONE sweep gives the range's
        # log-sum-exp and the unnormalised row gradients, the backward call finishes them with the GLOBAL log-sum-exp (the label row
        # leaves on the rank that owns the label) and runs the table pass over the range — weighted rows first, as the training step
        rows_c, lab_c, _perm, inv, nvalid = compact_rows(rows, labels)
        state = {}

        def lse_flash(i0, i1):
            ws = torch.empty(int(lib.edgl_score_flash_workspace(R, C, I, i1 - i0, code)), device=dev, dtype=torch.float32)
            lse = torch.empty(R, device=dev, dtype=torch.float32)
            lab = torch.zeros(R, device=dev, dtype=torch.float32)
            check(lib.edgl_score_flash_fwd(_ptr(rows_c), _ptr(table_c), _ptr(out_bias), _ptr(lab_c), R, C, I, i0, i1, _ptr(nvalid), _ptr(lse),
                                           _ptr(lab), _ptr(ws), code, st), "edgl_score_flash_fwd")
            state["ws"] = ws
            own = (lab_c >= max(i0, 1)) & (lab_c < i1)
            live = torch.arange(R, device=dev) < nvalid.to(torch.long)
            # rows behind the weighted ones carry label 0 (weight 0): a finite log-sum-exp of their own keeps the gathered sums finite
            return torch.where(live, lse, torch.zeros_like(lse)), torch.where(own, lab, torch.full_like(lab, float("-inf")))

        def grad_flash(i0, i1, lse, coef):
            d_rows = torch.empty_like(rows_c)
            check(lib.edgl_score_flash_bwd(_ptr(rows_c), _ptr(table_c), _ptr(out_bias), _ptr(lab_c), _ptr(lse.contiguous()), _ptr(coef.contiguous()),
                                           None, R, C, I, i0, i1, _ptr(nvalid), _ptr(d_rows), _ptr(d_table), _ptr(d_bias), _ptr(state["ws"]), code, st),
                  "edgl_score_flash_bwd")
            return d_rows

        def ce_hip(lse, lab, labels_c):      # loss + coefficients of the merged sums in one launch (EasyDGL.py:177-185)
            loss = torch.empty(1, device=dev, dtype=torch.float32)
            coef = torch.empty(R, device=dev, dtype=torch.float32)
            check(lib.edgl_ce_loss_fwd(_ptr(lse), _ptr(lab), _ptr(labels_c), R, _ptr(loss), _ptr(coef), st), "edgl_ce_loss_fwd")
            return loss.reshape(()), coef

        loss, d_rows_c, (i0, i1) = parallel.vocab_parallel_ce(lab_c, I, lse_flash, grad_flash, group, ce_local=ce_hip)
        return loss, d_rows_c[inv.long()], d_table, d_bias, (i0, i1)

    def lse_local(i0, i1):
        lse, lab, _ = score_lse(rows, table_c, out_bias, labels, i0, i1)
        own = (labels >= i0) & (labels < i1)
        return lse, torch.where(own, lab, torch.full_like(lab, float("-inf")))

    def grad_local(i0, i1, lse, coef):
        d_rows = torch.empty_like(rows)
        ws = torch.empty(int(lib.edgl_score_bwd_workspace(R, C, I, i1 - i0, code)), device=dev, dtype=torch.float32)
        check(lib.edgl_score_ce_bwd(_ptr(rows), _ptr(table_c), _ptr(out_bias), _ptr(labels), _ptr(lse), _ptr(coef), None, R, C, I,
                                    i0, i1, None, _ptr(d_rows), _ptr(d_table), _ptr(d_bias), _ptr(ws), code, st), "edgl_score_ce_bwd")
        return d_rows

    loss, d_rows, (i0, i1) = parallel.vocab_parallel_ce(labels, I, lse_local, grad_local, group)
    return loss, d_rows, d_table, d_bias, (i0, i1)


class ScoreCEFn(torch.autograd.Function):
    """EasyDGL.py:149-155,177-185 without the [R, I] logits tensor.  Rows with label 0 carry weight 0
    (EasyDGL.py:180); they are compacted away before scoring, which changes neither loss nor gradients.
    When a gradient is wanted the forward is the flash form (edgl_score_flash_fwd): the same sweep over the item table that
    gives the row log-sum-exp also accumulates the row gradients, and the backward only finishes them."""

    @staticmethod
    def forward(ctx, rows, table_master, out_bias, table_c, labels, deterministic=False):
        """deterministic: the one-hot term of the table / bias gradient is left out of the scoring backward
        (edgl_score_flash_bwd_ex, defer_label_term = 1) and applied as ordered sums (edgl_score_flash_label_term_det)."""
        ctx.deterministic = bool(deterministic)
        rows, labels, _perm, inv, nvalid = compact_rows(rows.contiguous(), labels.reshape(-1).contiguous())
        R, C = rows.shape
        I = table_c.shape[0]
        flash = any(ctx.needs_input_grad)
        ws = None
        if flash:
            code = _code(rows)
            ws = torch.empty(int(lib.edgl_score_flash_workspace(R, C, I, I, code)), device=rows.device, dtype=torch.float32)
            lse = torch.empty(R, device=rows.device, dtype=torch.float32)
            lab_logit = torch.zeros(R, device=rows.device, dtype=torch.float32)
            check(lib.edgl_score_flash_fwd(_ptr(rows), _ptr(table_c), _ptr(out_bias), _ptr(labels), R, C, I, 0, I, _ptr(nvalid),
                                           _ptr(lse), _ptr(lab_logit), _ptr(ws), code, _stream()), "edgl_score_flash_fwd")
        else:
            lse, lab_logit, _ = score_lse(rows, table_c, out_bias, labels, 0, I, nvalid=nvalid)
        loss = torch.empty(1, device=rows.device, dtype=torch.float32)
        coef = torch.empty(R, device=rows.device, dtype=torch.float32)
        check(lib.edgl_ce_loss_fwd(_ptr(lse), _ptr(lab_logit), _ptr(labels), R, _ptr(loss), _ptr(coef), _stream()),
              "edgl_ce_loss_fwd")
        ctx.save_for_backward(rows, table_c, out_bias, labels, lse, coef, inv, nvalid, ws)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        rows, table_c, out_bias, labels, lse, coef, inv, nvalid, ws = ctx.saved_tensors
        R, C = rows.shape
        I = table_c.shape[0]
        dev = rows.device
        g = g.reshape(1).to(torch.float32).contiguous()
        d_rows_c = torch.empty_like(rows)
        d_rows = torch.empty_like(rows)
        d_table = torch.empty((I, C), device=dev, dtype=torch.float32)
        d_bias = torch.empty(I - 1, device=dev, dtype=torch.float32)
        if ctx.deterministic:
            check(lib.edgl_score_flash_bwd_ex(_ptr(rows), _ptr(table_c), _ptr(out_bias), _ptr(labels), _ptr(lse), _ptr(coef),
                                              _ptr(g), R, C, I, 0, I, _ptr(nvalid), _ptr(d_rows_c), _ptr(d_table), _ptr(d_bias),
                                              _ptr(ws), 1, _code(rows), _stream()), "edgl_score_flash_bwd")
            plan = segsum_plan_buffer(R, I, dev)
            check(lib.edgl_score_flash_label_term_det(_ptr(rows), _ptr(labels), _ptr(coef), _ptr(g), R, C, I, 0, I, _ptr(nvalid),
                                                      _ptr(d_table), _ptr(d_bias), _ptr(plan), _code(rows), _stream()),
                  "edgl_score_flash_label_term_det")
        else:
            check(lib.edgl_score_flash_bwd(_ptr(rows), _ptr(table_c), _ptr(out_bias), _ptr(labels), _ptr(lse), _ptr(coef),
                                           _ptr(g), R, C, I, 0, I, _ptr(nvalid), _ptr(d_rows_c), _ptr(d_table), _ptr(d_bias),
                                           _ptr(ws), _code(rows), _stream()), "edgl_score_flash_bwd")
        check(lib.edgl_scatter_rows(_ptr(d_rows_c), _ptr(inv), R, C, _ptr(d_rows), _code(rows), _stream()),
              "edgl_scatter_rows")
        return d_rows, d_table, d_bias, None, None, None


def _logq_arg(logq, I, device, who):
    """The `logq` argument of the sampled losses: None, or a contiguous f32 [I] GPU tensor (NegDist.logq_on)."""
    if logq is None:
        return None
    if not torch.is_tensor(logq) or logq.dtype != torch.float32 or logq.shape != (I,) or logq.device != device or not logq.is_contiguous():
        raise _lib.EdglError(f"{who}: logq must be a contiguous f32 [{I}] tensor on {device}, one term per item id (got "
                             f"{getattr(logq, 'dtype', type(logq))} {tuple(getattr(logq, 'shape', ()))})")
    return logq


LOSS_FORMS = {"softmax": _lib.LOSS_SOFTMAX, "bce": _lib.LOSS_BCE, "bpr": _lib.LOSS_BPR}


def _loss_form(form, who):
    """The code of a sampled objective: "softmax" (the default), "bce" or "bpr"."""
    if form not in LOSS_FORMS:
        raise ValueError(f"{who}: form must be one of {sorted(LOSS_FORMS)} (got {form!r})")
    return LOSS_FORMS[form]


def _apply_form(base, args, form):
    """`.apply` of SampledCEFn / SharedCEFn: the nine arguments of `forward`, then the objective — a tenth positional argument or
    `form=` ("softmax", the default, "bce", "bpr").  `forward` itself keeps its signature: the objective selects a
    variant of the function (`_form_variant`) whose forward hands it on, so a call without it is the call it always was."""
    if len(args) > 9:
        if form is not None or len(args) > 10:
            raise TypeError(f"{base.__name__}.apply: at most ten positional arguments, the last of them the form")
        args, form = args[:9], args[9]
    code = _loss_form("softmax" if form is None else form, base.__name__)
    fn = base if code == _lib.LOSS_SOFTMAX else _form_variant(base, form)
    return super(base, fn).apply(*args)


_FORM_VARIANTS = {}


def _form_variant(base, form):
    """The autograd function of `base` (SampledCEFn / SharedCEFn) under another objective: the same forward and backward bodies."""
    if (base, form) not in _FORM_VARIANTS:
        class Variant(base):
            @staticmethod
            def forward(ctx, *args):
                return base._forward(ctx, form, *args)
        Variant.__name__ = Variant.__qualname__ = f"{base.__name__}[{form}]"
        _FORM_VARIANTS[(base, form)] = Variant
    return _FORM_VARIANTS[(base, form)]


def sampled_row_loss(vals, label_val, labels, nvalid, I, form):
    """(loss f32 [1], coef f32 [R], row_aux f32 [R], row_loss f32 [R]) of the bce / bpr objective over the values a sampled forward
    wrote (edgl_sampled_row_loss + edgl_sampled_loss_finish): vals f32 [R, N + 1] with slot 0 the label (label_val None, cand_ce_fwd's)
    or vals f32 [R, S] with label_val (shared_ce_fwd's).  row_aux goes to the backward where lse went."""
    code = _loss_form(form, "sampled_row_loss")
    R = vals.shape[0]
    S = vals.shape[1] - (1 if label_val is None else 0)
    dev = vals.device
    row_loss, row_aux, row_scale, coef = (torch.empty(R, device=dev, dtype=torch.float32) for _ in range(4))
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    check(lib.edgl_sampled_row_loss(_ptr(vals), _ptr(label_val), _ptr(labels), _ptr(nvalid), R, S, I, code, _ptr(row_loss),
                                    _ptr(row_aux), _ptr(row_scale), _stream()), "edgl_sampled_row_loss")
    check(lib.edgl_sampled_loss_finish(_ptr(row_loss), _ptr(row_scale), _ptr(labels), _ptr(nvalid), R, I, _ptr(loss), _ptr(coef),
                                       _stream()), "edgl_sampled_loss_finish")
    return loss, coef, row_aux, row_loss


def cand_ce_fwd(rows, table_c, out_bias, cand, labels, logq=None):
    """(vals f32 [R, N + 1], label_val f32 [R], lse f32 [R]) of edgl_cand_ce_fwd: slot 0 is the label, slot 1 + n is cand[r, n]
    (int32 [R, N]); -inf at an empty slot, an id >= I and an accidental hit (cand[r, n] == labels[r]); rows of label 0 are skipped
    (vals -inf, label_val = lse = 0).  The values carry the bits of score_candidates.
    logq (f32 [I]): the label and every live slot read v - logq[c] (edgl_cand_ce_fwd_q); zeros give the bits of None."""
    _ptr(rows)                                               # (GPU tensors only: refused before anything else)
    R, C = rows.shape
    I = table_c.shape[0]
    if table_c.dtype != rows.dtype or table_c.dim() != 2 or table_c.shape[1] != C:
        raise _lib.EdglError(f"cand_ce: rows {rows.dtype} [{R}, {C}] against a table {table_c.dtype} {tuple(table_c.shape)}")
    if cand.dtype != torch.int32 or cand.dim() != 2 or cand.shape[0] != R:
        raise _lib.EdglError(f"cand_ce: candidates must be int32 [{R}, N], one list per scored row (got {cand.dtype} "
                             f"{tuple(cand.shape)})")
    if labels.dtype != torch.int64 or labels.shape != (R,):
        raise _lib.EdglError(f"cand_ce: labels must be int64 [{R}] (got {labels.dtype} {tuple(labels.shape)})")
    dev, N = rows.device, cand.shape[1]
    vals = torch.empty((R, N + 1), device=dev, dtype=torch.float32)
    label_val = torch.empty(R, device=dev, dtype=torch.float32)
    lse = torch.empty(R, device=dev, dtype=torch.float32)
    logq = _logq_arg(logq, I, dev, "cand_ce")
    if logq is None:
        check(lib.edgl_cand_ce_fwd(_ptr(rows), _ptr(table_c), _ptr(out_bias), _ptr(cand), _ptr(labels), R, C, I, N, _ptr(vals),
                                   _ptr(label_val), _ptr(lse), _code(rows), _stream()), "edgl_cand_ce_fwd")
    else:
        check(lib.edgl_cand_ce_fwd_q(_ptr(rows), _ptr(table_c), _ptr(out_bias), _ptr(logq), _ptr(cand), _ptr(labels), R, C, I, N,
                                     _ptr(vals), _ptr(label_val), _ptr(lse), _code(rows), _stream()), "edgl_cand_ce_fwd_q")
    return vals, label_val, lse


class SampledCEFn(torch.autograd.Function):
    """Sampled-softmax cross-entropy: ScoreCEFn's loss with the softmax of row r taken over {labels[r]} and its own list
    cand[r, :] (int32 [R, N]; -1 = empty slot) instead of the catalogue.  Same gradient contract as ScoreCEFn: d_rows in the compute
    dtype, a dense f32 d_table [I, C] (zero-filled, then scattered into) and d_bias [I - 1].  No compaction: rows of label 0 are
    skipped inside the kernels, so a row's list never depends on which other rows are weighted.
    deterministic: the table / bias gradient is summed in plan order (edgl_cand_ce_table_det) instead of with f32 atomics.
    d_table_out (f32 [I, C]): the backward ADDS the table gradient into it (both entry points add), allocates no
    [I, C] tensor and returns None for the table master; d_bias stays a dense f32 [I - 1].
    logq (f32 [I]): the log-Q correction of a weighted sampler, subtracted from the label's and every live slot's
    value in the forward; a constant, so the backward is the same code on the corrected vals / lse.
    form ("softmax", "bce", "bpr"): the objective over the same slots and values, a tenth positional argument of
    `.apply` (or `form=`; _apply_form).  bce / bpr take their loss and coef from sampled_row_loss and their dv from
    edgl_cand_ce_bwd_form; the gradient contract above holds for every form."""

    @classmethod
    def apply(cls, *args, form=None):
        return _apply_form(SampledCEFn, args, form)

    @staticmethod
    def forward(ctx, rows, table_master, out_bias, table_c, labels, cand, deterministic=False, d_table_out=None, logq=None):
        return SampledCEFn._forward(ctx, "softmax", rows, table_master, out_bias, table_c, labels, cand, deterministic, d_table_out, logq)

    @staticmethod
    def _forward(ctx, form, rows, table_master, out_bias, table_c, labels, cand, deterministic=False, d_table_out=None, logq=None):
        ctx.deterministic = bool(deterministic)
        ctx.form = _loss_form(form, "SampledCEFn")
        ctx.d_table_out = _table_out(d_table_out, table_master.shape, "SampledCEFn")
        rows, labels, cand = rows.contiguous(), labels.reshape(-1).contiguous(), cand.contiguous()
        vals, label_val, lse = cand_ce_fwd(rows, table_c, out_bias, cand, labels, logq)
        R = rows.shape[0]
        if ctx.form == _lib.LOSS_SOFTMAX:
            loss = torch.empty(1, device=rows.device, dtype=torch.float32)
            coef = torch.empty(R, device=rows.device, dtype=torch.float32)
            check(lib.edgl_ce_loss_fwd(_ptr(lse), _ptr(label_val), _ptr(labels), R, _ptr(loss), _ptr(coef), _stream()),
                  "edgl_ce_loss_fwd")
        else:
            loss, coef, lse, _ = sampled_row_loss(vals, None, labels, None, table_c.shape[0], form)      # (lse: the row auxiliary)
        ctx.save_for_backward(rows, table_c, out_bias, labels, cand, vals, lse, coef)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        rows, table_c, out_bias, labels, cand, vals, lse, coef = ctx.saved_tensors
        R, C = rows.shape
        I, N = table_c.shape[0], cand.shape[1]
        dev = rows.device
        g = g.reshape(1).to(torch.float32).contiguous()
        d_rows = torch.empty_like(rows)
        dv = torch.empty((R, N + 1), device=dev, dtype=torch.float32)
        in_place = ctx.d_table_out is not None
        d_table = ctx.d_table_out if in_place else torch.zeros((I, C), device=dev, dtype=torch.float32)
        d_bias = torch.zeros(I - 1, device=dev, dtype=torch.float32)
        det = ctx.deterministic
        if ctx.form == _lib.LOSS_SOFTMAX:
            check(lib.edgl_cand_ce_bwd(_ptr(rows), _ptr(table_c), _ptr(out_bias), _ptr(cand), _ptr(labels), _ptr(vals), _ptr(lse),
                                       _ptr(coef), _ptr(g), R, C, I, N, _ptr(d_rows), _ptr(dv), None if det else _ptr(d_table),
                                       None if det else _ptr(d_bias), _code(rows), _stream()), "edgl_cand_ce_bwd")
        else:
            check(lib.edgl_cand_ce_bwd_form(_ptr(rows), _ptr(table_c), _ptr(out_bias), _ptr(cand), _ptr(labels), _ptr(vals), _ptr(lse),
                                            _ptr(coef), _ptr(g), R, C, I, N, _ptr(d_rows), _ptr(dv), None if det else _ptr(d_table),
                                            None if det else _ptr(d_bias), ctx.form, _code(rows), _stream()), "edgl_cand_ce_bwd_form")
        if det:
            n = R * (N + 1)
            keys = torch.empty(n, device=dev, dtype=torch.int64)
            plan = segsum_plan_buffer(n, I, dev)
            check(lib.edgl_cand_ce_table_det(_ptr(rows), _ptr(cand), _ptr(labels), _ptr(dv), R, C, I, N, _ptr(d_table), _ptr(d_bias),
                                             _ptr(keys), _ptr(plan), _code(rows), _stream()), "edgl_cand_ce_table_det")
        return d_rows, None if in_place else d_table, d_bias, None, None, None, None, None, None


MAX_SHARED = 8192


def _shared_ce_check(rows, table_c, shared, labels):
    _ptr(rows)                                               # (GPU tensors only: refused before anything else)
    R, C = rows.shape
    if table_c.dtype != rows.dtype or table_c.dim() != 2 or table_c.shape[1] != C:
        raise _lib.EdglError(f"shared_ce: rows {rows.dtype} [{R}, {C}] against a table {table_c.dtype} {tuple(table_c.shape)}")
    if shared.dtype != torch.int32 or shared.dim() != 1 or not 1 <= shared.shape[0] <= MAX_SHARED:
        raise _lib.EdglError(f"shared_ce: the shared list must be int32 [S], 1 <= S <= {MAX_SHARED}, one list for every row (got "
                             f"{shared.dtype} {tuple(shared.shape)})")
    if labels.dtype != torch.int64 or labels.shape != (R,):
        raise _lib.EdglError(f"shared_ce: labels must be int64 [{R}] (got {labels.dtype} {tuple(labels.shape)})")


def _shared_ce_fwd(rows, table_c, out_bias, shared, labels, nvalid, logq=None):
    R, C = rows.shape
    I, S, dev = table_c.shape[0], shared.shape[0], rows.device
    vals = torch.empty((R, S), device=dev, dtype=torch.float32)
    label_val = torch.empty(R, device=dev, dtype=torch.float32)
    lse = torch.empty(R, device=dev, dtype=torch.float32)
    logq = _logq_arg(logq, I, dev, "shared_ce")
    if logq is None:
        check(lib.edgl_shared_ce_fwd(_ptr(rows), _ptr(table_c), _ptr(out_bias), _ptr(shared), _ptr(labels), _ptr(nvalid), R, C, I, S,
                                     _ptr(vals), _ptr(label_val), _ptr(lse), _code(rows), _stream()), "edgl_shared_ce_fwd")
    else:
        check(lib.edgl_shared_ce_fwd_q(_ptr(rows), _ptr(table_c), _ptr(out_bias), _ptr(logq), _ptr(shared), _ptr(labels), _ptr(nvalid),
                                       R, C, I, S, _ptr(vals), _ptr(label_val), _ptr(lse), _code(rows), _stream()),
              "edgl_shared_ce_fwd_q")
    return vals, label_val, lse


def shared_ce_fwd(rows, table_c, out_bias, shared, labels, logq=None):
    """(vals f32 [R, S], label_val f32 [R], lse f32 [R]) of edgl_shared_ce_fwd, in the caller's row order: vals[r, s] is the value of
    (rows[r], shared[s]) (int32 [S], one list for every row); -inf at an id < 0, an id >= I and an accidental hit (shared[s] ==
    labels[r]); label_val is the label's value; rows of label 0 are skipped (vals -inf, label_val = lse = 0).
    logq (f32 [I]): the label and every live slot read v - logq[c] (edgl_shared_ce_fwd_q); zeros give the bits of None."""
    _shared_ce_check(rows, table_c, shared, labels)
    return _shared_ce_fwd(rows.contiguous(), table_c, out_bias, shared.contiguous(), labels.contiguous(), None, logq)


class SharedCEFn(torch.autograd.Function):
    """Sampled-softmax cross-entropy on ONE negative list per call: SampledCEFn's loss with cand[r, :] = shared[:]
    (int32 [S]; an id < 0 or >= I is an empty slot, an id equal to a row's label is dead for that row) — the scoring and both
    gradient products run as dense products on MFMA (edgl_shared_ce_fwd / _bwd).  SampledCEFn's gradient contract: d_rows in the
    compute dtype, a dense f32 d_table [I, C] (zero-filled, then added into) and d_bias [I - 1].  The weighted rows are compacted
    first, as in ScoreCEFn: the list does not depend on the row, so that changes nothing but the work.
    deterministic: no float atomics — repeated ids are summed in slot order, the label term over a k_segsum.hip plan.
    d_table_out (f32 [I, C]): the backward ADDS the table gradient into it and returns None for the table master.
    logq (f32 [I]): the log-Q correction of a weighted sampler, as in SampledCEFn.
    form ("softmax", "bce", "bpr"): the objective, as in SampledCEFn: a tenth positional argument of `.apply`
    (edgl_shared_ce_bwd_form)."""

    @classmethod
    def apply(cls, *args, form=None):
        return _apply_form(SharedCEFn, args, form)

    @staticmethod
    def forward(ctx, rows, table_master, out_bias, table_c, labels, shared, deterministic=False, d_table_out=None, logq=None):
        return SharedCEFn._forward(ctx, "softmax", rows, table_master, out_bias, table_c, labels, shared, deterministic, d_table_out, logq)

    @staticmethod
    def _forward(ctx, form, rows, table_master, out_bias, table_c, labels, shared, deterministic=False, d_table_out=None, logq=None):
        ctx.deterministic = bool(deterministic)
        ctx.form = _loss_form(form, "SharedCEFn")
        ctx.d_table_out = _table_out(d_table_out, table_master.shape, "SharedCEFn")
        rows, labels, shared = rows.contiguous(), labels.reshape(-1).contiguous(), shared.contiguous()
        _shared_ce_check(rows, table_c, shared, labels)
        if lib.edgl_shared_ce_workspace(rows.shape[0], rows.shape[1], shared.shape[0], _code(rows)) < 0:     # (the shape rule, before the compaction)
            check(-1, "edgl_shared_ce_workspace")
        rows, labels, _perm, inv, nvalid = compact_rows(rows, labels)
        vals, label_val, lse = _shared_ce_fwd(rows, table_c, out_bias, shared, labels, nvalid, logq)
        R = rows.shape[0]
        if ctx.form == _lib.LOSS_SOFTMAX:
            loss = torch.empty(1, device=rows.device, dtype=torch.float32)
            coef = torch.empty(R, device=rows.device, dtype=torch.float32)
            check(lib.edgl_ce_loss_fwd(_ptr(lse), _ptr(label_val), _ptr(labels), R, _ptr(loss), _ptr(coef), _stream()),
                  "edgl_ce_loss_fwd")
        else:
            loss, coef, lse, _ = sampled_row_loss(vals, label_val, labels, nvalid, table_c.shape[0], form)   # (lse: the row auxiliary)
        ctx.save_for_backward(rows, table_c, labels, shared, vals, label_val, lse, coef, inv, nvalid)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        rows, table_c, labels, shared, vals, label_val, lse, coef, inv, nvalid = ctx.saved_tensors
        R, C = rows.shape
        I, S = table_c.shape[0], shared.shape[0]
        dev, code = rows.device, _code(rows)
        g = g.reshape(1).to(torch.float32).contiguous()
        d_rows_c = torch.empty_like(rows)
        d_rows = torch.empty_like(rows)
        in_place = ctx.d_table_out is not None
        d_table = ctx.d_table_out if in_place else torch.zeros((I, C), device=dev, dtype=torch.float32)
        d_bias = torch.zeros(I - 1, device=dev, dtype=torch.float32)
        ws = torch.empty(int(lib.edgl_shared_ce_workspace(R, C, S, code)), device=dev, dtype=torch.float32)
        keys = plan = None
        if ctx.deterministic:
            keys = torch.empty(2 * R, device=dev, dtype=torch.int64)
            plan = segsum_plan_buffer(2 * R, I, dev)
        if ctx.form == _lib.LOSS_SOFTMAX:
            check(lib.edgl_shared_ce_bwd(_ptr(rows), _ptr(table_c), _ptr(shared), _ptr(labels), _ptr(vals), _ptr(label_val), _ptr(lse),
                                         _ptr(coef), _ptr(g), _ptr(nvalid), R, C, I, S, _ptr(d_rows_c), _ptr(d_table), _ptr(d_bias),
                                         _ptr(ws), _ptr(keys), _ptr(plan), code, _stream()), "edgl_shared_ce_bwd")
        else:
            check(lib.edgl_shared_ce_bwd_form(_ptr(rows), _ptr(table_c), _ptr(shared), _ptr(labels), _ptr(vals), _ptr(label_val),
                                              _ptr(lse), _ptr(coef), _ptr(g), _ptr(nvalid), R, C, I, S, _ptr(d_rows_c), _ptr(d_table),
                                              _ptr(d_bias), _ptr(ws), _ptr(keys), _ptr(plan), ctx.form, code, _stream()),
                  "edgl_shared_ce_bwd_form")
        check(lib.edgl_scatter_rows(_ptr(d_rows_c), _ptr(inv), R, C, _ptr(d_rows), code, _stream()), "edgl_scatter_rows")
        return d_rows, None if in_place else d_table, d_bias, None, None, None, None, None, None


class ScoreLogitsFn(torch.autograd.Function):
    """Materialised logits [R, I] (EasyDGL.py:149-151) for API parity with the reference's __call__."""

    @staticmethod
    def forward(ctx, rows, table_master, out_bias, table_c):
        I = table_c.shape[0]
        _, _, logits = score_lse(rows, table_c, out_bias, None, 0, I, want_logits=True)
        ctx.save_for_backward(rows, table_c)
        return logits

    @staticmethod
    def backward(ctx, dl):
        rows, table_c = ctx.saved_tensors
        R, C = rows.shape
        I = table_c.shape[0]
        dl = dl.contiguous()
        dl[:, 0] = 0  # column 0 is the constant -1000 (Base.py:110) over a constant zero row
        dlc = dl if rows.dtype == torch.float32 else cast_to(dl, rows.dtype)
        tab = table_c.clone()
        tab[0] = 0  # coding.py:56-57
        d_rows = gemm(dlc, tab, R, C, I, I, C, True, False, rows.dtype)
        d_table = gemm(dlc, rows, I, C, R, I, C, False, False, torch.float32, splitk=_splitk_for(I, C, R))
        d_table[0] = 0
        d_bias = dl.sum(0)[1:]
        return d_rows, d_table, d_bias, None


# ------------------------------------------------------------------------------------------------
# K8 TPP regulariser, l2
# ------------------------------------------------------------------------------------------------
class TppFn(torch.autograd.Function):
    """ct_reg/h * MAU.biased_likelihood on the gathered intensities (EasyDGL.py:157-175)."""

    @staticmethod
    def forward(ctx, lam, masked_pos, labels, ts_raw, mark_table, H, coef):
        HB, T, E = lam.shape
        B, M = labels.shape if masked_pos is None else masked_pos.shape
        sums = torch.empty(lib.edgl_tpp_workspace(), device=lam.device, dtype=torch.float32)
        reg = torch.empty(1, device=lam.device, dtype=torch.float32)
        check(lib.edgl_tpp_fwd(_ptr(lam), _ptr(masked_pos), _ptr(labels), _ptr(ts_raw), _ptr(mark_table), B, T, H, E, M,
                               float(coef), _ptr(sums), _ptr(reg), 0, _stream()), "edgl_tpp_fwd")
        ctx.save_for_backward(lam, masked_pos, labels, ts_raw, mark_table, sums)
        ctx.meta = (B, T, H, E, M, coef)
        return reg.reshape(())

    @staticmethod
    def backward(ctx, g):
        lam, masked_pos, labels, ts_raw, mark_table, sums = ctx.saved_tensors
        B, T, H, E, M, coef = ctx.meta
        g = g.reshape(1).to(torch.float32).contiguous()
        d_lam = torch.empty_like(lam)
        check(lib.edgl_tpp_bwd(_ptr(lam), _ptr(masked_pos), _ptr(labels), _ptr(ts_raw), _ptr(mark_table), B, T, H, E, M,
                               float(coef), _ptr(sums), _ptr(g), _ptr(d_lam), _stream()), "edgl_tpp_bwd")
        return d_lam, None, None, None, None, None, None


_SEG_CACHE = {}


def _whole_segment(n: int, device) -> torch.Tensor:
    """[0, n] on the device, built once per (n, device): no host-to-device copy inside a step (HIP graph capture forbids it)."""
    key = (n, str(device))
    if key not in _SEG_CACHE:
        _SEG_CACHE[key] = torch.tensor([0, n], device=device, dtype=torch.int64)
    return _SEG_CACHE[key]


class L2Fn(torch.autograd.Function):
    """l2_reg * sum(w^2)/2 over one raw embedding table (coding.py:34-40).  forward_only (the lazily updated item table, DESIGN
    4.14): the term enters the loss, the backward returns no dense tensor — its gradient l2 w reaches the table as the `l2`
    argument of adam_rows, on the touched rows."""

    @staticmethod
    def forward(ctx, w, l2, forward_only=False):
        ctx.forward_only = bool(forward_only)
        seg = _whole_segment(w.numel(), w.device)
        out = torch.empty(1, device=w.device, dtype=torch.float32)
        ws = torch.empty(1024, device=w.device, dtype=torch.float32)
        check(lib.edgl_l2_loss(_ptr(w), _ptr(seg), 1, float(l2), _ptr(out), 0, _ptr(ws), _stream()), "edgl_l2_loss")
        ctx.save_for_backward(w)
        ctx.l2 = l2
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        if ctx.forward_only:
            return None, None, None
        return w * (g * ctx.l2), None, None


# ------------------------------------------------------------------------------------------------
# K6/K7 evaluation
# ------------------------------------------------------------------------------------------------
def mask_topk(logits: torch.Tensor, i0: int, seen: Optional[torch.Tensor], K: int):
    R, n = logits.shape
    val = torch.empty((R, K), device=logits.device, dtype=torch.float32)
    idx = torch.empty((R, K), device=logits.device, dtype=torch.int32)
    T = 0 if seen is None else seen.shape[1]
    check(lib.edgl_mask_topk(_ptr(logits), R, n, i0, _ptr(seen), T, K, _ptr(val), _ptr(idx), _stream()), "edgl_mask_topk")
    return val, idx


def topk_merge(cand_val: torch.Tensor, cand_idx: torch.Tensor):
    S, R, K = cand_val.shape
    val = torch.empty((R, K), device=cand_val.device, dtype=torch.float32)
    idx = torch.empty((R, K), device=cand_val.device, dtype=torch.int32)
    check(lib.edgl_topk_merge(_ptr(cand_val), _ptr(cand_idx), S, R, K, _ptr(val), _ptr(idx), _stream()), "edgl_topk_merge")
    return val, idx


EVAL_TILE_BYTES = 64 << 20   # logits staging tile of score_topk: [R, chunk] f32, sized to stay L2 / MALL resident
TOPK_REG_ITEMS = (256 * 80 - 8) // 8 * 8   # longest row of the register form of edgl_mask_topk (csrc/k_score.hip), a multiple of 8
EVAL_FUSED = os.environ.get("EDGL_EVAL_FUSED", "1") != "0"   # scoring + seen mask + top-K without a logits tile (k_eval_topk.hip)
EVAL_GEMM = True             # full item chunks of the chunked evaluation path score through edgl_gemm (tests switch it off)


EVAL_FUSED_SCRATCH_BYTES = int(os.environ.get("EDGL_EVAL_FUSED_SCRATCH_BYTES", str(512 << 20)))
_FUSED_EVAL_WS = {}


def _fused_eval_workspace(device, nbytes: int) -> torch.Tensor:
    """Grow-only workspace of the fused evaluation scoring, one per device and stream (the launches of one stream are ordered, so
    consecutive calls may share it): no allocation per call."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _FUSED_EVAL_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(int(nbytes), device=device, dtype=torch.uint8)
        _FUSED_EVAL_WS[key] = ws
    return ws


def score_topk(rows, table_c, out_bias, seen, K, i0, i1):
    """Sequential.eval's scoring + seen-mask + top-K (Base.py:150-181) over the item range [i0, i1) WITHOUT the [R, I]
    logits tensor of the reference: the range is walked in chunks whose [R, chunk] f32 logits tile is bounded by
    EVAL_TILE_BYTES (2 GB per batch at |items| = 1M otherwise); every chunk gives a local top-K with global ids and the
    merge kernel orders the candidates by (value desc, id asc) — the tie rule of tf.nn.top_k.  Returns (val, idx) [R, K]."""
    R = rows.shape[0]
    n = i1 - i0
    # the fused form (csrc/k_eval_topk.hip): no logits tile at all — two sweeps on the matrix pipe, candidates above a per-row bound,
    # one ranking launch; item ranges of <= 262 144 per call, longer catalogues in chunks + the merge kernel
    if EVAL_FUSED and K <= 128 and rows.dtype == torch.bfloat16 and i0 % 8 == 0:
        if seen is not None:
            # the sweep reads a row's seen ids as 16-byte pairs of int64 at a row stride of T (csrc/k_eval_topk.hip eval_sweep_kernel)
            if seen.dtype != torch.int64:
                raise _lib.EdglError(f"score_topk: seen ids must be int64 (got {seen.dtype})")
            seen = seen.contiguous()
            if seen.data_ptr() % 16 != 0:
                seen = seen.clone()                     # (an offset view of a larger buffer: a fresh allocation is 256-byte aligned)
        T = 0 if seen is None else seen.shape[1]
        C, code, st = rows.shape[1], _code(rows), _stream()
        fchunk = 131072 if C == 256 else 262144      # (64 item slices of <= 2048 / 4096 items: the seen bitmap's LDS)
        starts = list(range(i0, i1, fchunk))
        # (a short last chunk joins its neighbour's range when that keeps both callable: the fused form wants >= 4096 items)
        if len(starts) > 1 and (i1 - starts[-1]) < 4096:
            starts[-1] = max(starts[-2] + 8, (i1 - 4096) // 8 * 8)
        bounds = [(lo, (starts[j + 1] if j + 1 < len(starts) else i1)) for j, lo in enumerate(starts)]
        # The plan reserves an [R, items] f32 scratch for the exact fallback of rows whose candidate list overflows (almost never
        # touched): bounded by walking the rows in blocks, so that a large evaluation batch on a large catalogue holds at most
        # EVAL_FUSED_SCRATCH_BYTES of it — the unfused path it replaces is bounded by EVAL_TILE_BYTES the same way
        span = max(hi - lo for lo, hi in bounds)
        rb = R if R * span * 4 <= EVAL_FUSED_SCRATCH_BYTES else max(128, (EVAL_FUSED_SCRATCH_BYTES // (span * 4)) // 128 * 128)
        rblocks = [(r0, min(R, r0 + rb)) for r0 in range(0, R, rb)]
        rsizes = sorted({r1 - r0 for r0, r1 in rblocks})
        if all(lib.edgl_score_topk_fused_supported(rn, C, hi - lo, T, K, code) for lo, hi in bounds for rn in rsizes) \
                and (len(bounds) == 1 or K <= 512):
            wsb = max(int(lib.edgl_score_topk_fused_workspace(rn, C, hi - lo, T, K)) for lo, hi in bounds for rn in rsizes)
            ws = _fused_eval_workspace(rows.device, wsb)
            cval = torch.empty((len(bounds), R, K), device=rows.device, dtype=torch.float32)
            cidx = torch.empty((len(bounds), R, K), device=rows.device, dtype=torch.int32)
            for j, (lo, hi) in enumerate(bounds):
                for r0, r1 in rblocks:
                    check(lib.edgl_score_topk_fused(_ptr(rows[r0:r1]), _ptr(table_c), _ptr(out_bias),
                                                    None if seen is None else _ptr(seen[r0:r1]), T, r1 - r0, C, table_c.shape[0], lo, hi, K,
                                                    _ptr(cval[j, r0:r1]), _ptr(cidx[j, r0:r1]), _ptr(ws), code, st), "edgl_score_topk_fused")
            return _merge_lists(cval, cidx, R, K)
    chunk = max(1024, (EVAL_TILE_BYTES // (4 * R)) // 8 * 8)
    if K <= 128 and chunk > TOPK_REG_ITEMS >= 1024:      # rows the top-K kernel keeps in registers: one read of the tile instead of five
        chunk = TOPK_REG_ITEMS // 128 * 128              # (a multiple of 128: full chunks take the tiled GEMM below)
    if n <= chunk:
        _, _, logits = score_lse(rows, table_c, out_bias, None, i0, i1, want_logits=True, want_lse=False)
        return mask_topk(logits, i0, seen, K)
    starts = list(range(i0, i1, chunk))                  # chunk starts stay multiples of 8 (i0 is one)
    if len(starts) > 1 and K > 512:
        raise _lib.EdglError(f"score_topk: K={K} > 512 on the chunked path (the merge kernel orders up to 1024 candidates per row: "
                             f"two K-lists at least)")
    # One logits tile, one scoring workspace and the candidate lists of ALL chunks are allocated once: per chunk the loop is two
    # library calls (at 1 M items and 49 chunks the allocations and wrappers of the per-chunk form kept the GPU waiting for the host)
    C, I, dev, code, st = rows.shape[1], table_c.shape[0], rows.device, _code(rows), _stream()
    logits = torch.empty((R, chunk), device=dev, dtype=torch.float32)
    ws = torch.empty(2 * R * lib.edgl_score_chunks(R, chunk), device=dev, dtype=torch.float32)
    cval = torch.empty((len(starts), R, K), device=dev, dtype=torch.float32)
    cidx = torch.empty((len(starts), R, K), device=dev, dtype=torch.int32)
    T = 0 if seen is None else seen.shape[1]
    esz = rows.element_size()
    # bias of item z at element z (item 0, the padding item, never read through it): 16-byte aligned for every chunk start
    bias_z = torch.cat([out_bias.new_zeros(1), out_bias]) if (code == BF16 and EVAL_GEMM and len(starts) > 2) else None
    for j, lo in enumerate(starts):
        hi = min(i1, lo + chunk)
        if bias_z is not None and lo >= 1 and (hi - lo) % 128 == 0 and C % 32 == 0:
            # a full chunk behind the padding item: logits = rows . table[lo:hi]^T + bias as a plain GEMM with f32 output (the
            # weights-resident strip kernel against the scoring kernel's 45-85 us at 512 x 20 352 x 128 / 256); bias of item z is
            # out_bias[z - 1] (EasyDGL.py:149-151), the pad logit -1000 belongs to item 0 — never in these chunks
            check(lib.edgl_gemm(_ptr(rows), ctypes.c_void_p(table_c.data_ptr() + lo * C * esz), _ptr(logits), R, hi - lo, C, C, C,
                                hi - lo, 1, 1, ctypes.c_void_p(bias_z.data_ptr() + lo * 4), None,
                                _lib.EPI_BIAS | _lib.EPI_OUT_F32, 1, None, code, st), "edgl_gemm")
        else:
            check(lib.edgl_score_lse_fwd(_ptr(rows), _ptr(table_c), _ptr(out_bias), None, R, C, I, lo, hi, None, None, None,
                                         _ptr(logits), _ptr(ws), code, st), "edgl_score_lse_fwd")  # logits [R, hi - lo], row stride hi - lo
        check(lib.edgl_mask_topk(_ptr(logits), R, hi - lo, lo, _ptr(seen), T, K, _ptr(cval[j]), _ptr(cidx[j]), st), "edgl_mask_topk")
    return _merge_lists(cval, cidx, R, K)


def _merge_lists(cval, cidx, R, K):
    """[S, R, K] candidate lists -> the global top-K by (value desc, index asc): rounds of the merge kernel (<= 1024 candidates each)."""
    dev, st = cval.device, _stream()
    fan = max(2, 1024 // K)                              # the merge kernel takes up to 1024 candidates per row
    while cval.shape[0] > 1:
        n = cval.shape[0]
        ng = (n + fan - 1) // fan
        nval = torch.empty((ng, R, K), device=dev, dtype=torch.float32)
        nidx = torch.empty((ng, R, K), device=dev, dtype=torch.int32)
        for g in range(ng):
            a, b = g * fan, min(n, (g + 1) * fan)
            if b - a == 1:
                nval[g].copy_(cval[a]); nidx[g].copy_(cidx[a])
            else:
                check(lib.edgl_topk_merge(_ptr(cval[a:b]), _ptr(cidx[a:b]), b - a, R, K, _ptr(nval[g]), _ptr(nidx[g]), st),
                      "edgl_topk_merge")
        cval, cidx = nval, nidx
    return cval[0], cidx[0]


def rank_metrics(topk_idx: torch.Tensor, label: torch.Tensor, metrics: torch.Tensor) -> None:
    R, K = topk_idx.shape
    check(lib.edgl_rank_metrics(_ptr(topk_idx), R, K, _ptr(label), _ptr(metrics), _stream()), "edgl_rank_metrics")


# ---- K6r: evaluation by label rank (csrc/k_eval_rank.hip) — Base.py:150-201 without a top-K list ---------------------------------
RANK_FUSED_ITEMS = 262144    # items per call of edgl_score_rank_fused


def _aligned_seen(seen, who):
    """The sweeps read a row's seen ids as 16-byte pairs of int64 at a row stride of T."""
    if seen is None:
        return None
    if seen.dtype != torch.int64:
        raise _lib.EdglError(f"{who}: seen ids must be int64 (got {seen.dtype})")
    seen = seen.contiguous()
    return seen.clone() if seen.data_ptr() % 16 != 0 else seen


def _rank_labels(labels, R, who):
    if labels.dtype != torch.int64 or labels.shape != (R,):
        raise _lib.EdglError(f"{who}: labels must be int64 [{R}] (got {labels.dtype} {tuple(labels.shape)})")
    return labels.contiguous()


def score_label_rank(rows, table_c, out_bias, seen, labels, i0=0, i1=None):
    """int32 [R]: for every row the number of items j != y of [i0, i1) that come before its label y = labels[r] in the (logit desc,
    item id asc) order of the catalogue with the row's seen ids at -inf (Base.py:150-201).  Over the whole catalogue that is the
    label's rank: its index in score_topk's list whenever it is < K.  Counts over disjoint ranges add.
    bf16 at C in {64, 128, 256}: the fused form — the label values by the sweep's own MFMA chain, then one counting sweep per range
    of <= RANK_FUSED_ITEMS items, no logits in HBM.  Anything else: logits tiles bounded by EVAL_TILE_BYTES, scored by
    edgl_score_lse_fwd (ONE kernel for every chunk: the label's value and its duplicates elsewhere in the catalogue must be the
    same bits) — pass A takes each label's value from the chunk that holds it, pass B counts; a catalogue of one chunk is scored once."""
    R, C = rows.shape
    I = table_c.shape[0]
    i1 = I if i1 is None else i1
    _ptr(rows)                                               # (GPU tensors only: refused before anything else)
    dev, code, st = rows.device, _code(rows), _stream()
    labels = _rank_labels(labels, R, "score_label_rank")
    count = torch.zeros(R, device=dev, dtype=torch.int32)
    if i1 <= i0:                                            # (an empty table shard)
        return count
    T = 0 if seen is None else seen.shape[1]
    label_val = torch.empty(R, device=dev, dtype=torch.float32)
    if i0 % 8 == 0 and lib.edgl_score_rank_supported(R, C, min(i1 - i0, RANK_FUSED_ITEMS), T, code):
        seen = _aligned_seen(seen, "score_label_rank")
        check(lib.edgl_score_label_value(_ptr(rows), _ptr(table_c), _ptr(out_bias), _ptr(seen), T, _ptr(labels), R, C, I,
                                         _ptr(label_val), code, st), "edgl_score_label_value")
        for lo in range(i0, i1, RANK_FUSED_ITEMS):
            check(lib.edgl_score_rank_fused(_ptr(rows), _ptr(table_c), _ptr(out_bias), _ptr(seen), T, _ptr(labels), _ptr(label_val),
                                            R, C, I, lo, min(i1, lo + RANK_FUSED_ITEMS), _ptr(count), None, code, st),      # (workspace: 0 bytes)
                  "edgl_score_rank_fused")
        return count
    if seen is not None:
        seen = seen.contiguous()
    chunk = max(8, (EVAL_TILE_BYTES // (4 * R)) // 8 * 8)

    def chunks(lo, hi):
        return [(a, min(hi, a + chunk)) for a in range(lo, hi, chunk)]

    logits = torch.empty((R, min(chunk, I)), device=dev, dtype=torch.float32)
    ws = torch.empty(2 * R * lib.edgl_score_chunks(R, min(chunk, I)), device=dev, dtype=torch.float32)

    def score(lo, hi):     # logits [R, hi - lo], row stride hi - lo
        check(lib.edgl_score_lse_fwd(_ptr(rows), _ptr(table_c), _ptr(out_bias), None, R, C, I, lo, hi, None, None, None,
                                     _ptr(logits), _ptr(ws), code, st), "edgl_score_lse_fwd")

    def value(lo, hi):
        check(lib.edgl_label_value_tile(_ptr(logits), R, hi - lo, lo, _ptr(seen), T, _ptr(labels), _ptr(label_val), st),
              "edgl_label_value_tile")

    def add(lo, hi):
        check(lib.edgl_rank_count_tile(_ptr(logits), R, hi - lo, lo, _ptr(seen), T, _ptr(labels), _ptr(label_val), _ptr(count), st),
              "edgl_rank_count_tile")

    whole = chunks(0, I)             # pass A walks the whole catalogue: a label may lie outside [i0, i1) (table shards)
    if len(whole) == 1:
        score(0, I)
        value(0, I)
        if (i0, i1) != (0, I):
            score(i0, i1)
        add(i0, i1)
        return count
    for lo, hi in whole:
        score(lo, hi)
        value(lo, hi)
    for lo, hi in chunks(i0, i1):
        score(lo, hi)
        add(lo, hi)
    return count


def rank_from_logits(logits: torch.Tensor, i0: int, seen: Optional[torch.Tensor], labels: torch.Tensor) -> torch.Tensor:
    """score_label_rank for materialised f32 logits [B, n] of the items [i0, i0 + n) (the regressive models): every label must lie
    in that range.  The logits are not modified."""
    R, n = logits.shape
    _ptr(logits)                                             # (GPU tensors only: refused before anything else)
    if logits.dtype != torch.float32:
        raise _lib.EdglError(f"rank_from_logits: f32 logits (got {logits.dtype})")
    labels = _rank_labels(labels, R, "rank_from_logits")
    seen = None if seen is None else seen.contiguous()
    T = 0 if seen is None else seen.shape[1]
    st = _stream()
    label_val = torch.full((R,), float("inf"), device=logits.device, dtype=torch.float32)
    count = torch.zeros(R, device=logits.device, dtype=torch.int32)
    check(lib.edgl_label_value_tile(_ptr(logits), R, n, i0, _ptr(seen), T, _ptr(labels), _ptr(label_val), st), "edgl_label_value_tile")
    check(lib.edgl_rank_count_tile(_ptr(logits), R, n, i0, _ptr(seen), T, _ptr(labels), _ptr(label_val), _ptr(count), st),
          "edgl_rank_count_tile")
    return count


def rank_metrics_from_rank(rank: torch.Tensor, ks: torch.Tensor, sums: torch.Tensor, row_order: bool = False) -> None:
    """sums f32 [2 nk + 1] += (H@k.., N@k.., MRR) of the int32 ranks; ks int32 [nk <= 8] on the device.  `row_order`: the rows are
    added one by one instead of as the batch's tree — the sums of a split then do not depend on how it is cut into batches."""
    if rank.dtype != torch.int32 or ks.dtype != torch.int32 or sums.dtype != torch.float32 or sums.numel() != 2 * ks.numel() + 1:
        raise _lib.EdglError("rank_metrics_from_rank: rank int32 [R], ks int32 [nk], sums f32 [2 nk + 1]")
    if row_order:
        check(lib.edgl_rank_metrics_from_rank_rows(_ptr(rank), rank.shape[0], _ptr(ks), ks.numel(), _ptr(sums), _stream()),
              "edgl_rank_metrics_from_rank_rows")
        return
    check(lib.edgl_rank_metrics_from_rank(_ptr(rank), rank.shape[0], _ptr(ks), ks.numel(), _ptr(sums), _stream()),
          "edgl_rank_metrics_from_rank")


# ---- K6c: evaluation on candidate lists (csrc/k_eval_cand.hip) — sampled negatives and re-ranking -------------------
class NegDist:
    """A weighted negative distribution over the ids [lo, hi), as build_neg_dist leaves it: the alias table on the
    host (thr uint32 [n], alias int32 [n], n = hi - lo), logq f32 [I] and the number of rejected ids per row the table was checked
    for (T_reject).  The device copies — the interleaved (thr, alias) table the sampler reads and logq — are made once per device."""

    def __init__(self, lo, hi, T_reject, thr, alias, logq):
        self.lo, self.hi, self.T_reject = int(lo), int(hi), int(T_reject)
        self.thr, self.alias, self.logq = thr, alias, logq
        self._dev = {}

    def _on(self, device):
        key = str(torch.device(device))
        if key not in self._dev:
            tab = np.stack([self.thr.view(np.int32), self.alias], axis=1)        # [n, 2]: one 8-byte entry per bucket
            self._dev[key] = (torch.from_numpy(np.ascontiguousarray(tab)).to(device), torch.from_numpy(self.logq).to(device))
        return self._dev[key]

    def table_on(self, device) -> torch.Tensor:
        return self._on(device)[0]

    def logq_on(self, device) -> torch.Tensor:
        return self._on(device)[1]

    def probabilities(self) -> np.ndarray:
        """fp64 [n]: the probability of every id of [lo, hi) that the stored (thr, alias) imply for a uniform bucket."""
        n = self.hi - self.lo
        acc = np.where(self.alias == np.arange(n), 1.0, self.thr.astype(np.float64) * 2.0 ** -32)
        p = acc.copy()
        np.add.at(p, self.alias, 1.0 - acc)
        return p / n


def neg_weights(sampler, I, lo, hi, counts=None, alpha=0.75):
    """fp64 [I]: the weight presets of FLAGS.neg_sampler over the ids [lo, hi); 0 outside the range.
    popularity: (count_c + 1)^alpha — add-one smoothing, so every id of the range can be drawn and no corrected logit is +inf.
    log_uniform: log((c - lo + 2) / (c - lo + 1)) — TensorFlow's default sampler, meant for ids sorted by falling frequency."""
    w = np.zeros(int(I), dtype=np.float64)
    if sampler == "popularity":
        if counts is None:
            raise ValueError("neg_weights: the popularity sampler needs `counts` (one count per item id)")
        counts = np.asarray(counts, dtype=np.float64).reshape(-1)
        if counts.shape[0] < hi or not np.isfinite(counts[lo:hi]).all() or (counts[lo:hi] < 0).any():
            raise ValueError(f"neg_weights: counts must hold a finite count >= 0 for every id of [{lo}, {hi}) (got {counts.shape[0]} entries)")
        w[lo:hi] = (counts[lo:hi] + 1.0) ** float(alpha)
    elif sampler == "log_uniform":
        k = np.arange(hi - lo, dtype=np.float64)
        w[lo:hi] = np.log((k + 2.0) / (k + 1.0))
    else:
        raise ValueError(f"neg_weights: sampler {sampler!r} (popularity or log_uniform)")
    return w


def build_neg_dist(weights, lo, hi, T_reject=0) -> NegDist:
    """The alias table (Vose's method, fp64) and the log-Q terms of the weighted negative sampler over the ids
    [lo, hi) of `weights` (float [I]; entries outside the range are ignored).  Host work in numpy, once per run.
    Refused: a weight of the range that is not finite or not > 0, and weights whose T_reject + 1 heaviest ids hold more than half of
    the total — the weighted form of 2 (T + 1) <= hi - lo: a row rejects at most T_reject seen ids and its label, so every attempt
    is then rejected with probability <= 1/2 and a slot stays empty (-1) with probability <= 2^-32.
    Build order (fixed): p_j = w_j n / sum(w); the buckets with p_j < 1 and those with p_j >= 1 go on two stacks in ascending j; the
    tops s (small) and l (large) are popped, bucket s keeps p_s and takes alias l, p_l <- (p_l + p_s) - 1 and l goes back on the
    stack its new p_l names; what is left on either stack when one runs empty is a full bucket (alias[j] = j).  thr[j] =
    floor(p_j 2^32) < 2^32 for a bucket with an alias; a full bucket returns j on either branch, so no threshold has to be 2^32.
    logq[c] = log(w_c / sum(w)) for lo <= c < hi (fp64, rounded once to f32), 0 elsewhere."""
    w_all = np.asarray(weights)
    if w_all.ndim != 1 or w_all.dtype not in (np.float64, np.float32):
        raise ValueError(f"build_neg_dist: weights must be float64 / float32 [I] (got {w_all.dtype} {w_all.shape})")
    I, lo, hi, T_reject = w_all.shape[0], int(lo), int(hi), int(T_reject)
    if not (1 <= lo < hi <= I) or T_reject < 0:
        raise ValueError(f"build_neg_dist: range [{lo}, {hi}) of {I} ids, T_reject={T_reject} (1 <= lo < hi <= I, T_reject >= 0)")
    w = w_all[lo:hi].astype(np.float64)
    n = hi - lo
    bad = ~np.isfinite(w) | ~(w > 0.0)
    if bad.any():
        c = lo + int(np.argmax(bad))
        raise ValueError(f"build_neg_dist: weight {w[c - lo]!r} of id {c}: every weight of [{lo}, {hi}) must be finite and > 0 "
                         f"({int(bad.sum())} are not; a zero weight would make the id's corrected logit +inf)")
    total = float(w.sum())
    k = min(T_reject + 1, n)
    top = float(np.sort(w)[n - k:].sum())
    if top > 0.5 * total:
        raise ValueError(f"build_neg_dist: the T_reject + 1 = {T_reject + 1} heaviest ids of [{lo}, {hi}) hold {top / total:.4f} of "
                         "the weight, more than 1/2: a row may reject that many ids, every attempt must be rejected with "
                         "probability <= 1/2 (a slot then stays empty with probability <= 2^-32)")
    p = w * (n / total)
    small = np.flatnonzero(p < 1.0).tolist()
    large = np.flatnonzero(p >= 1.0).tolist()
    p = p.tolist()
    thr = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    alias = np.arange(n, dtype=np.int32)
    while small and large:
        s, l = small.pop(), large.pop()
        thr[s] = int(p[s] * 4294967296.0)                    # (p_s < 1 in fp64 and the product is exact: < 2^32)
        alias[s] = l
        p[l] = (p[l] + p[s]) - 1.0
        (small if p[l] < 1.0 else large).append(l)
    logq = np.zeros(I, dtype=np.float32)
    logq[lo:hi] = np.log(w / total).astype(np.float32)
    return NegDist(lo, hi, T_reject, thr, alias, logq)


def sample_negatives(seen, labels, n, lo, hi, seed, step=0, row0=0, dist=None):
    """int32 [R, n]: per row n ids drawn uniformly from [lo, hi) (with replacement between slots), never one of the row's seen ids
    (int64 [R, T] or None) and never labels[r] (int64 [R]).  Counter-based on (seed, step, row0 + r, slot): `row0` is the index of the
    batch's first sequence in its split, so a sequence's list does not depend on the batch size.  Needs 2 (T + 1) <= hi - lo.
    dist (NegDist of build_neg_dist over the same [lo, hi)): the ids are drawn by its weights instead
    (edgl_sample_negatives_alias); the table must have been checked for at least T rejected ids per row."""
    _ptr(labels)                                             # (GPU tensors only: refused before anything else)
    R = labels.shape[0]
    labels = _rank_labels(labels, R, "sample_negatives")
    if seen is not None:
        if seen.dtype != torch.int64 or seen.dim() != 2 or seen.shape[0] != R:
            raise _lib.EdglError(f"sample_negatives: seen ids must be int64 [{R}, T] (got {seen.dtype} {tuple(seen.shape)})")
        seen = seen.contiguous()
    T = 0 if seen is None else seen.shape[1]
    cand = torch.empty((R, int(n)), device=labels.device, dtype=torch.int32)
    mask64 = (1 << 64) - 1
    if dist is not None:
        if not isinstance(dist, NegDist) or (dist.lo, dist.hi) != (int(lo), int(hi)):
            raise _lib.EdglError(f"sample_negatives: dist must be a NegDist over [{int(lo)}, {int(hi)}) (got "
                                 f"{'[%d, %d)' % (dist.lo, dist.hi) if isinstance(dist, NegDist) else type(dist).__name__})")
        if T > dist.T_reject:
            raise _lib.EdglError(f"sample_negatives: {T} seen ids per row against a table checked for T_reject = {dist.T_reject} "
                                 "(build_neg_dist(..., T_reject=T): the T + 1 heaviest ids may hold at most half of the weight)")
        tab = dist.table_on(labels.device)
        check(lib.edgl_sample_negatives_alias(_ptr(seen), T, _ptr(labels), R, int(n), int(lo), int(hi), int(hi), _ptr(tab),
                                              int(seed) & mask64, int(step) & mask64, int(row0), _ptr(cand), _stream()),
              "edgl_sample_negatives_alias")
        return cand
    check(lib.edgl_sample_negatives(_ptr(seen), T, _ptr(labels), R, int(n), int(lo), int(hi), int(hi), int(seed) & mask64,
                                    int(step) & mask64, int(row0), _ptr(cand), _stream()), "edgl_sample_negatives")
    return cand


def score_candidates(rows, table_c, out_bias, cand, seen=None, labels=None, want_scores=True, count=None):
    """(scores f32 [R, N] | None, label_val f32 [R] | None, rank int32 [R] | None) of every row's OWN candidate list cand int32 [R, N]:
    scores[r, n] = rows[r] . table_c[c] + bias_used[c] for c = cand[r, n], -inf for an empty slot (c < 0) and for the row's seen ids
    (int64 [R, T] or None).  With labels (int64 [R]): label_val = the label's value by the same arithmetic and rank = the number of
    slots that come before the label in the (value desc, item id asc) order — the label's own slots are not counted, a repeated id
    counts once per slot.  `count`: an int32 [R] buffer the counts are ADDED into (the lists of one row scored in parts) instead of a
    fresh one.  A gather of R (N + 1) table rows: no sweep over the catalogue."""
    _ptr(rows)                                               # (GPU tensors only: refused before anything else)
    R, C = rows.shape
    I = table_c.shape[0]
    if table_c.dtype != rows.dtype or table_c.shape[1] != C:
        raise _lib.EdglError(f"score_candidates: rows {rows.dtype} [{R}, {C}] against a table {table_c.dtype} {tuple(table_c.shape)}")
    if cand.dtype != torch.int32 or cand.dim() != 2 or cand.shape[0] != R:
        raise _lib.EdglError(f"score_candidates: candidates must be int32 [{R}, N] (got {cand.dtype} {tuple(cand.shape)})")
    if seen is not None and (seen.dtype != torch.int64 or seen.dim() != 2 or seen.shape[0] != R):
        raise _lib.EdglError(f"score_candidates: seen ids must be int64 [{R}, T] (got {seen.dtype} {tuple(seen.shape)})")
    dev, N = rows.device, cand.shape[1]
    rows, cand = rows.contiguous(), cand.contiguous()
    seen = None if seen is None else seen.contiguous()
    T = 0 if seen is None else seen.shape[1]
    scores = torch.empty((R, N), device=dev, dtype=torch.float32) if want_scores else None
    label_val = None
    if labels is None:
        if count is not None:
            raise _lib.EdglError("score_candidates: a count buffer without labels")
    else:
        labels = _rank_labels(labels, R, "score_candidates")
        label_val = torch.empty(R, device=dev, dtype=torch.float32)
        if count is None:
            count = torch.zeros(R, device=dev, dtype=torch.int32)
        elif count.dtype != torch.int32 or count.shape != (R,):
            raise _lib.EdglError(f"score_candidates: count must be int32 [{R}] (got {count.dtype} {tuple(count.shape)})")
    check(lib.edgl_score_candidates(_ptr(rows), _ptr(table_c), _ptr(out_bias), _ptr(cand), _ptr(seen), T, _ptr(labels), R, C, I, N,
                                    _ptr(scores), _ptr(label_val), _ptr(count), _code(rows), _stream()), "edgl_score_candidates")
    return scores, label_val, count


def adam_step(param, grad, m, v, lr, state, l2, seg, shadow, beta1=0.9, beta2=0.999, eps=1e-8):
    check(lib.edgl_adam_step(_ptr(param), _ptr(grad), _ptr(m), _ptr(v), param.numel(), float(lr), beta1, beta2, eps,
                             _ptr(state), float(l2), _ptr(seg), 0 if seg is None else seg.numel() // 2, _ptr(shadow),
                             _stream()), "edgl_adam_step")


def adam_apply(param, grad, m, v, state, l2, seg, shadow, beta1=0.9, beta2=0.999, eps=1e-8):
    """The parameter update of adam_step alone: the step count and learning rate are read from `state` as the last adam_step left them."""
    check(lib.edgl_adam_apply(_ptr(param), _ptr(grad), _ptr(m), _ptr(v), param.numel(), beta1, beta2, eps, _ptr(state), float(l2),
                              _ptr(seg), 0 if seg is None else seg.numel() // 2, _ptr(shadow), _stream()), "edgl_adam_apply")


def adam_rows(table, grad, m, v, shadow, ids, labels, cand, stamp, state, l2=0.0, beta1=0.9, beta2=0.999, eps=1e-8):
    """Lazy row-wise Adam (edgl_adam_rows): the TF-form update on the rows of `table` f32 [I, C] that `ids` (int64, any
    shape, or None), `labels` (int64 [R] or None) or `cand` (int32 [R, N] or None; the lists of rows with labels != 0) name, each
    exactly once; their rows of `grad` are left at zero, every other row keeps its bits.  `stamp`: int32 [I], zero before the first
    call.  The step count and learning rate are read from `state` (advance it first: adam_step on another range)."""
    _ptr(table)                                              # (GPU tensors only: refused before anything else)
    I, C = table.shape
    for name, t in (("table", table), ("grad", grad), ("m", m), ("v", v)):
        if t.dtype != torch.float32 or tuple(t.shape) != (I, C):
            raise _lib.EdglError(f"adam_rows: {name} must be f32 [{I}, {C}] (got {t.dtype} {tuple(t.shape)})")
    if shadow is not None and (shadow.dtype != torch.bfloat16 or tuple(shadow.shape) != (I, C)):
        raise _lib.EdglError(f"adam_rows: shadow must be bf16 [{I}, {C}] (got {shadow.dtype} {tuple(shadow.shape)})")
    if stamp.dtype != torch.int32 or tuple(stamp.shape) != (I,):
        raise _lib.EdglError(f"adam_rows: stamp must be int32 [{I}] (got {stamp.dtype} {tuple(stamp.shape)})")
    n_ids = 0
    if ids is not None:
        if ids.dtype != torch.int64:
            raise _lib.EdglError(f"adam_rows: ids must be int64 (got {ids.dtype})")
        ids = ids.reshape(-1).contiguous()
        n_ids = ids.numel()
    R = N = 0
    if labels is not None:
        labels = _rank_labels(labels.reshape(-1), labels.numel(), "adam_rows")
        R = labels.numel()
    if cand is not None:
        if labels is None or cand.dtype != torch.int32 or cand.dim() != 2 or cand.shape[0] != R:
            raise _lib.EdglError(f"adam_rows: candidates must be int32 [{R}, N] beside int64 labels [{R}] (got {cand.dtype} "
                                 f"{tuple(cand.shape)})")
        cand = cand.contiguous()
        N = cand.shape[1]
    check(lib.edgl_adam_rows(_ptr(table), _ptr(grad), _ptr(m), _ptr(v), _ptr(shadow), I, C, _ptr(ids) if n_ids else None, n_ids,
                             _ptr(labels) if R else None, _ptr(cand) if R and N else None, R, N, _ptr(stamp), beta1, beta2, eps,
                             _ptr(state), float(l2), _stream()), "edgl_adam_rows")


class DropoutFn(torch.autograd.Function):
    """tf.layers.dropout as a standalone op (FeedForward, Base.py:80,83): counter-based mask, regenerated in the backward."""

    @staticmethod
    def forward(ctx, x, drop: Drop):
        x = x.contiguous()
        y = torch.empty_like(x)
        check(lib.edgl_dropout(_ptr(x), _ptr(y), x.numel(), float(drop.rate), drop.ptr(), drop.stream_id, _code(x), _stream()),
              "edgl_dropout")
        ctx.drop = drop
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        d = ctx.drop
        check(lib.edgl_dropout(_ptr(dy), _ptr(dx), dy.numel(), float(d.rate), d.ptr(), d.stream_id, _code(dy), _stream()),
              "edgl_dropout")
        return dx, None


def dropout(x, drop: Drop):
    return x if not drop.active else DropoutFn.apply(x, drop)


class AddFn(torch.autograd.Function):
    """out = a + b (edgl_add); the gradient passes to both."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        out = torch.empty_like(a)
        check(lib.edgl_add(_ptr(a), _ptr(b), _ptr(out), a.numel(), _code(a), _stream()), "edgl_add")
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g


def add(a, b):
    return AddFn.apply(a, b)


# ------------------------------------------------------------------------------------------------
# config 5 baselines: item embedding alone, row mask, K11 attention with the time feature map
# ------------------------------------------------------------------------------------------------
class EmbedFn(torch.autograd.Function):
    """x = dropout(item[ids] * sqrt(C)) with the zero-padded row 0 (TGAT.py:49-56, TiSASREC.py:52-65): edgl_embed_pos_* with
    no position table."""

    @staticmethod
    def forward(ctx, item_master, item_c, ids, drop: Drop, act_dtype, c_true=0, deterministic=False):
        B, T = ids.shape
        I, C = item_c.shape
        x0 = torch.empty((B, T, C), device=ids.device, dtype=act_dtype)
        check(lib.edgl_embed_pos_fwd_ct(_ptr(ids), None, _ptr(item_c), None, None, B, T, C, 0, 1.0, float(drop.rate), drop.ptr(),
                                        drop.stream_id, _ptr(x0), None, None, int(c_true), _DT[act_dtype], _stream()),
              "edgl_embed_pos_fwd")
        ctx.c_true = int(c_true)
        ctx.deterministic = bool(deterministic)
        ctx.save_for_backward(ids)
        ctx.meta = (B, T, C, I, drop, item_master.shape)
        return x0

    @staticmethod
    def backward(ctx, dx0):
        (ids,) = ctx.saved_tensors
        B, T, C, I, drop, ishape = ctx.meta
        dx0 = dx0.contiguous()
        d_item = torch.empty(ishape, device=dx0.device, dtype=torch.float32)
        _embed_pos_bwd(ctx.deterministic, ids, dx0, B, T, C, I, drop, d_item, None, ctx.c_true)
        return d_item, None, None, None, None, None, None


class MaskRowsFn(torch.autograd.Function):
    """y = x * (ids != 0)[..., None]  (`seqs_outs *= seqs_masks`, TGAT.py:70)."""

    @staticmethod
    def forward(ctx, x, ids):
        x = x.contiguous()
        y = torch.empty_like(x)
        check(lib.edgl_mask_rows(_ptr(x), _ptr(ids), _ptr(y), ids.numel(), x.shape[-1], _code(x), _stream()), "edgl_mask_rows")
        ctx.save_for_backward(ids)
        return y

    @staticmethod
    def backward(ctx, dy):
        (ids,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        check(lib.edgl_mask_rows(_ptr(dy), _ptr(ids), _ptr(dx), ids.numel(), dy.shape[-1], _code(dy), _stream()), "edgl_mask_rows")
        return dx, None


def mask_rows(x, ids):
    return MaskRowsFn.apply(x, ids)


class TfAttnFn(torch.autograd.Function):
    """TfMultiHeadAttention after its dense layers (temporal.py:139-184): q [B,T,C], kv [B,T,2C] (K | V column blocks),
    resid = the queries; time feature map (edgl_timefn_*) + masked causal attention (edgl_tattn_*).  `violations`: device
    int32 counter of positions whose timestamps decrease (see include/easydgl_hip.h)."""

    @staticmethod
    def forward(ctx, q, kv, resid, pos_tab, omega, phi, ids, ts, H, time_scale, drop: Drop, violations, qk_scale=0.0):
        """qk_scale: the score scale (0 = 1 / sqrt(head dim)); a channel-padded model passes 1 / sqrt(true head dim)."""
        B, T, C = q.shape
        dh = C // H
        q, kv, resid = q.contiguous(), kv.contiguous(), resid.contiguous()
        code = _code(q)
        qx = torch.empty((B, T, 3 * C), device=q.device, dtype=q.dtype)
        kx = torch.empty_like(qx)
        check(lib.edgl_timefn_fwd(_ptr(q), C, _ptr(kv), 2 * C, _ptr(pos_tab), _ptr(ts), _ptr(ids), _ptr(omega), _ptr(phi), B, T, C,
                                  H, float(time_scale), _ptr(qx), _ptr(kx), _ptr(violations), code, _stream()), "edgl_timefn_fwd")
        out = torch.empty((B, T, C), device=q.device, dtype=q.dtype)
        need = any(ctx.needs_input_grad)
        saved = torch.empty(int(lib.edgl_tattn_saved_bytes(B, T, H, dh)), device=q.device, dtype=torch.uint8) if need else None
        scale = float(qk_scale) if qk_scale else 1.0 / float(dh) ** 0.5                  # temporal.py:153
        check(lib.edgl_tattn_fwd(_ptr(qx), 3 * C, _ptr(kx), 3 * C, _vptr(kv[:, :, C:]), 2 * C, _ptr(resid), C, _ptr(ids), B, T, H,
                                 3 * dh, dh, scale, float(drop.rate), drop.ptr(), drop.stream_id, _ptr(out), C, _ptr(saved),
                                 _lib.TATTN_CAUSAL, code, _stream()), "edgl_tattn_fwd")
        ctx.save_for_backward(q, kv, qx, kx, omega, phi, ids, ts, saved)
        ctx.meta = (B, T, C, H, dh, scale, float(time_scale), drop, pos_tab.shape)
        return out

    @staticmethod
    def backward(ctx, d_out):
        q, kv, qx, kx, omega, phi, ids, ts, saved = ctx.saved_tensors
        B, T, C, H, dh, scale, time_scale, drop, pshape = ctx.meta
        d_out = d_out.contiguous()
        code = _code(q)
        d_qx, d_kx = torch.empty_like(qx), torch.empty_like(kx)
        d_kv = torch.empty_like(kv)
        check(lib.edgl_tattn_bwd(_ptr(qx), 3 * C, _ptr(kx), 3 * C, _vptr(kv[:, :, C:]), 2 * C, _ptr(ids), _ptr(d_out), C, _ptr(saved),
                                 B, T, H, 3 * dh, dh, scale, float(drop.rate), drop.ptr(), drop.stream_id, _ptr(d_qx), 3 * C,
                                 _ptr(d_kx), 3 * C, _vptr(d_kv[:, :, C:]), 2 * C, _lib.TATTN_CAUSAL, code, _stream()), "edgl_tattn_bwd")
        d_q = torch.empty_like(q)
        both = torch.empty(2 * C, device=q.device, dtype=torch.float32)   # d_omega | d_phi adjacent: one reduction launch
        d_omega, d_phi = both[:C], both[C:]
        ws = torch.empty(int(lib.edgl_timefn_bwd_workspace(C)), device=q.device, dtype=torch.float32)
        check(lib.edgl_timefn_bwd(_ptr(q), C, _ptr(ts), _ptr(omega), _ptr(phi), _ptr(d_qx), _ptr(d_kx), B, T, C, H, time_scale,
                                  _ptr(d_q), C, _ptr(d_kv), 2 * C, _ptr(d_omega), _ptr(d_phi), _ptr(ws), code, _stream()),
              "edgl_timefn_bwd")
        # d(pos_tab)[t] = sum_b dK[b,t]  (K + pos enters the score, temporal.py:143,148): column sums of d_kv seen as [B, T*2C]
        d_pos = colsum(d_kv.view(B, T * 2 * C), B, T * 2 * C).view(T, 2 * C)[:, :C].contiguous()
        if pshape[0] != T:
            full = torch.zeros(pshape, device=q.device, dtype=torch.float32)
            full[:T] = d_pos
            d_pos = full
        return d_q, d_kv, d_out, d_pos, d_omega, d_phi, None, None, None, None, None, None, None


class TiAttnFn(torch.autograd.Function):
    """TiMultiHeadAttention after its dense layers (temporal.py:45-104): q [B,T,C], kv [B,T,2C] (K | V), resid = the queries,
    position tables posK/posV f32 [>=T, C], interval tables (masters f32 + compute-dtype copies) [timelen, C]."""

    @staticmethod
    def forward(ctx, q, kv, resid, posK, posV, ktime, vtime, ktime_c, vtime_c, ids, ts, H, time_scale, timelen, drop: Drop,
                qk_scale=0.0, deterministic=False):
        """deterministic: the interval bins of the forward and of the query sweep are filled in a fixed order (TATTN_ORDERED) and
        the interval-table gradients are summed from per-split slabs (edgl_tiattn_bwd_det)."""
        B, T, C = q.shape
        dh = C // H
        q, kv, resid = q.contiguous(), kv.contiguous(), resid.contiguous()
        code = _code(q)
        flags = _lib.TATTN_CAUSAL | (_lib.TATTN_ORDERED if deterministic else 0)
        kvp = torch.empty_like(kv)
        check(lib.edgl_add_pos2(_ptr(kv), _ptr(posK), _ptr(posV), B, T, C, _ptr(kvp), code, _stream()), "edgl_add_pos2")
        out = torch.empty((B, T, C), device=q.device, dtype=q.dtype)
        need = any(ctx.needs_input_grad)
        saved = wbuf = None
        if need:
            saved = torch.empty(int(lib.edgl_tattn_saved_bytes(B, T, H, dh)), device=q.device, dtype=torch.uint8)
            wbuf = torch.empty(int(lib.edgl_tiattn_bucket_elems(B, T, H, timelen)), device=q.device, dtype=q.dtype)
        scale = float(qk_scale) if qk_scale else 1.0 / float(dh) ** 0.5
        rows = ktime_c.shape[0]
        check(lib.edgl_tiattn_fwd(_ptr(q), C, _ptr(kvp), 2 * C, _vptr(kvp[:, :, C:]), 2 * C, _ptr(resid), C, _ptr(ids), _ptr(ts),
                                  _ptr(ktime_c), _ptr(vtime_c), rows, B, T, H, dh, scale, float(time_scale), int(timelen),
                                  float(drop.rate), drop.ptr(), drop.stream_id, _ptr(out), C, _ptr(saved), _ptr(wbuf),
                                  flags, code, _stream()), "edgl_tiattn_fwd")
        ctx.save_for_backward(q, kvp, ktime_c, vtime_c, ids, ts, saved, wbuf)
        ctx.deterministic = bool(deterministic)
        ctx.meta = (B, T, C, H, dh, scale, float(time_scale), int(timelen), drop, posK.shape, posV.shape, rows)
        return out

    @staticmethod
    def backward(ctx, d_out):
        q, kvp, ktime_c, vtime_c, ids, ts, saved, wbuf = ctx.saved_tensors
        B, T, C, H, dh, scale, time_scale, timelen, drop, pk_shape, pv_shape, rows = ctx.meta
        d_out = d_out.contiguous()
        code = _code(q)
        d_q, d_kv = torch.empty_like(q), torch.empty_like(kvp)
        dgbuf = torch.empty_like(wbuf)   # binned score gradients
        d_kt = torch.empty((rows, C), device=q.device, dtype=torch.float32)
        d_vt = torch.empty_like(d_kt)
        head = (_ptr(q), C, _ptr(kvp), 2 * C, _vptr(kvp[:, :, C:]), 2 * C, _ptr(ids), _ptr(ts), _ptr(ktime_c), _ptr(vtime_c), rows,
                _ptr(d_out), C, _ptr(saved), _ptr(wbuf), B, T, H, dh, scale, time_scale, timelen, float(drop.rate), drop.ptr(),
                drop.stream_id, _ptr(d_q), C, _ptr(d_kv), 2 * C, _vptr(d_kv[:, :, C:]), 2 * C, _ptr(dgbuf), _ptr(d_kt), _ptr(d_vt))
        if ctx.deterministic:
            ws = torch.empty(int(lib.edgl_tiattn_det_workspace(H, dh, timelen)), device=q.device, dtype=torch.float32)
            check(lib.edgl_tiattn_bwd_det(*head, _ptr(ws), _lib.TATTN_CAUSAL | _lib.TATTN_ORDERED, code, _stream()),
                  "edgl_tiattn_bwd_det")
        else:
            check(lib.edgl_tiattn_bwd(*head, _lib.TATTN_CAUSAL, code, _stream()), "edgl_tiattn_bwd")
        d_pos = colsum(d_kv.view(B, T * 2 * C), B, T * 2 * C).view(T, 2 * C)     # the tables enter K and V additively
        d_pk = torch.zeros(pk_shape, device=q.device, dtype=torch.float32)
        d_pv = torch.zeros(pv_shape, device=q.device, dtype=torch.float32)
        d_pk[:T] = d_pos[:, :C]
        d_pv[:T] = d_pos[:, C:]
        return d_q, d_kv, d_out, d_pk, d_pv, d_kt, d_vt, None, None, None, None, None, None, None, None, None, None



class EmbedCatFn(torch.autograd.Function):
    """X0 = dropout(concat(item[ids] * sqrt(C), pos[0..T))) without time spans or marks (SASREC.py:43-49): edgl_embed_pos_* with
    no timestamps and no mark table.  The position half is NOT zero on padding: the caller masks the rows."""

    @staticmethod
    def forward(ctx, item_master, pos_tab, item_c, ids, drop: Drop, act_dtype, deterministic=False):
        B, T = ids.shape
        I, C = item_c.shape
        x0 = torch.empty((B, T, 2 * C), device=ids.device, dtype=act_dtype)
        check(lib.edgl_embed_pos_fwd_ct(_ptr(ids), None, _ptr(item_c), _ptr(pos_tab), None, B, T, C, 0, 1.0, float(drop.rate),
                                        drop.ptr(), drop.stream_id, _ptr(x0), None, None, 0, _DT[act_dtype], _stream()),
              "edgl_embed_pos_fwd")
        ctx.save_for_backward(ids)
        ctx.deterministic = bool(deterministic)
        ctx.meta = (B, T, C, I, drop, item_master.shape, pos_tab.shape)
        return x0

    @staticmethod
    def backward(ctx, dx0):
        (ids,) = ctx.saved_tensors
        B, T, C, I, drop, ishape, pshape = ctx.meta
        dx0 = dx0.contiguous()
        d_item = torch.empty(ishape, device=dx0.device, dtype=torch.float32)
        d_pos = torch.zeros(pshape, device=dx0.device, dtype=torch.float32)
        _embed_pos_bwd(ctx.deterministic, ids, dx0, B, T, C, I, drop, d_item, d_pos, 0)
        return (d_item, d_pos) + (None,) * 5


class PlainAttnFn(torch.autograd.Function):
    """MultiHeadAttention after its dense layers (sequential.py:39-78): q [B,T,C], kv [B,T,2C] (K | V column blocks), resid = the
    first C channels of the queries (a row-strided view); the plain-head case Dq == Dv of edgl_tattn_*."""

    @staticmethod
    def forward(ctx, q, kv, resid, ids, H, drop: Drop, causal=True):
        B, T, C = q.shape
        dh = C // H
        q, kv = q.contiguous(), kv.contiguous()
        if resid.stride(-1) != 1 or resid.stride(0) != T * resid.stride(1):
            raise _lib.EdglError("attention residual must be a row-strided view of a contiguous [B,T,*] tensor")
        if ids.dtype != torch.int64 or tuple(ids.shape) != (B, T) or not ids.is_contiguous():
            raise _lib.EdglError(f"attention key ids must be a contiguous int64 [B={B}, T={T}] tensor, got {tuple(ids.shape)} {ids.dtype}")
        code = _code(q)
        flags = _lib.TATTN_CAUSAL if causal else 0
        out = torch.empty((B, T, C), device=q.device, dtype=q.dtype)
        need = any(ctx.needs_input_grad)
        saved = torch.empty(int(lib.edgl_tattn_saved_bytes(B, T, H, dh)), device=q.device, dtype=torch.uint8) if need else None
        scale = 1.0 / float(dh) ** 0.5                                                   # sequential.py:47
        check(lib.edgl_tattn_fwd(_ptr(q), C, _ptr(kv), 2 * C, _vptr(kv[:, :, C:]), 2 * C, _vptr(resid), resid.stride(1), _ptr(ids), B,
                                 T, H, dh, dh, scale, float(drop.rate), drop.ptr(), drop.stream_id, _ptr(out), C, _ptr(saved), flags,
                                 code, _stream()), "edgl_tattn_fwd")
        ctx.save_for_backward(q, kv, ids, saved)
        ctx.meta = (B, T, C, H, dh, scale, drop, flags)
        return out

    @staticmethod
    def backward(ctx, d_out):
        q, kv, ids, saved = ctx.saved_tensors
        B, T, C, H, dh, scale, drop, flags = ctx.meta
        d_out = d_out.contiguous()
        d_q, d_kv = torch.empty_like(q), torch.empty_like(kv)
        check(lib.edgl_tattn_bwd(_ptr(q), C, _ptr(kv), 2 * C, _vptr(kv[:, :, C:]), 2 * C, _ptr(ids), _ptr(d_out), C, _ptr(saved), B, T,
                                 H, dh, dh, scale, float(drop.rate), drop.ptr(), drop.stream_id, _ptr(d_q), C, _ptr(d_kv), 2 * C,
                                 _vptr(d_kv[:, :, C:]), 2 * C, flags, _code(q), _stream()), "edgl_tattn_bwd")
        return d_q, d_kv, d_out, None, None, None, None


class GruSeqFn(torch.autograd.Function):
    """The GRU recurrence over xp = x W + b_W (edgl_gru_seq_fwd / bwd): h [B,T,C] from xp [B,T,3C], R [C,3C] (r_c: its
    compute copy), b_R [3C].  Gate order r | z | n, cuDNN's form, zero initial state.  The backward carries dh in f32 through the
    recurrence and returns d_xp; dR = H_prev^T dG_h and db_R are one dense_grads call over the B*T rows.  No atomics anywhere:
    the same bits in every call, so FLAGS.deterministic needs no second form."""

    @staticmethod
    def forward(ctx, xp, r_master, r_bias, r_c):
        B, T, C3 = xp.shape
        C = C3 // 3
        xp = xp.contiguous()
        code = _code(xp)
        if r_c.dtype != xp.dtype or tuple(r_c.shape) != (C, C3) or tuple(r_bias.shape) != (C3,) or r_bias.dtype != torch.float32:
            raise _lib.EdglError(f"GruSeqFn: R must be {xp.dtype} [{C}, {C3}] and b_R f32 [{C3}] (got {r_c.dtype} {tuple(r_c.shape)}, "
                                 f"{r_bias.dtype} {tuple(r_bias.shape)})")
        nbytes = int(lib.edgl_gru_seq_pack_bytes(C, code))
        if nbytes <= 0:
            raise _lib.EdglError(f"GruSeqFn: width C={C} unsupported (a multiple of 16 in [16, 512])")
        pack = torch.empty(nbytes, device=xp.device, dtype=torch.uint8)
        h = torch.empty((B, T, C), device=xp.device, dtype=xp.dtype)
        need = any(ctx.needs_input_grad)
        saved = torch.empty((B, T, 5 * C), device=xp.device, dtype=torch.float32) if need else None
        # the A operand of dR: in f32 mode the h_prev block of `saved` itself, else a copy in the activation dtype
        hprev = torch.empty((B, T, C), device=xp.device, dtype=xp.dtype) if need and xp.dtype != torch.float32 else None
        check(lib.edgl_gru_seq_fwd(_ptr(xp), _ptr(r_c), _ptr(r_bias), B, T, C, _ptr(h), _ptr(saved), _ptr(hprev), _ptr(pack), code,
                                   _stream()), "edgl_gru_seq_fwd")
        ctx.save_for_backward(r_c, saved, hprev)
        ctx.meta = (B, T, C, code)
        return h

    @staticmethod
    def backward(ctx, d_h):
        r_c, saved, hprev = ctx.saved_tensors
        B, T, C, code = ctx.meta
        d_h = d_h.contiguous()
        d_xp = torch.empty((B, T, 3 * C), device=d_h.device, dtype=d_h.dtype)
        d_gh = torch.empty_like(d_xp)
        pack = torch.empty(int(lib.edgl_gru_seq_pack_bytes(C, code)), device=d_h.device, dtype=torch.uint8)
        check(lib.edgl_gru_seq_bwd(_ptr(d_h), _ptr(r_c), _ptr(saved), B, T, C, _ptr(d_xp), _ptr(d_gh), _ptr(pack), code, _stream()),
              "edgl_gru_seq_bwd")
        hp = saved.view(B * T, 5 * C)[:, 4 * C:] if hprev is None else hprev.view(B * T, C)      # (row stride 5C / C)
        M, N = B * T, 3 * C
        both = torch.empty((C + 1) * N, device=d_h.device, dtype=torch.float32)
        ws = torch.empty(lib.edgl_gemm_dw_workspace(M, C, N, code), device=d_h.device, dtype=torch.float32)
        check(lib.edgl_gemm_dw(_vptr(hp), _ptr(d_gh), _ptr(both), both.data_ptr() + 4 * C * N, M, C, N, hp.stride(0), N, 0, _ptr(ws), code,
                               _stream()), "edgl_gemm_dw")
        return d_xp, both[:C * N].view(C, N), both[C * N:], None


class CatPosMaskFn(torch.autograd.Function):
    """[h | pos[0..T)] * (ids != 0) (S2PNM.py:52-53; PositionCoding concatenates): edgl_cat_pos_mask_fwd / bwd.  d_pos is summed over
    b in a fixed order, without atomics."""

    @staticmethod
    def forward(ctx, h, pos_tab, ids):
        B, T, C = h.shape
        h = h.contiguous()
        out = torch.empty((B, T, 2 * C), device=h.device, dtype=h.dtype)
        check(lib.edgl_cat_pos_mask_fwd(_ptr(h), _ptr(pos_tab), _ptr(ids), B, T, C, _ptr(out), _code(h), _stream()), "edgl_cat_pos_mask_fwd")
        ctx.save_for_backward(ids)
        ctx.meta = (B, T, C, pos_tab.shape)
        return out

    @staticmethod
    def backward(ctx, d_out):
        (ids,) = ctx.saved_tensors
        B, T, C, pshape = ctx.meta
        d_out = d_out.contiguous()
        d_h = torch.empty((B, T, C), device=d_out.device, dtype=d_out.dtype)
        d_pos = torch.zeros(pshape, device=d_out.device, dtype=torch.float32)      # (rows past T, if any, stay zero)
        check(lib.edgl_cat_pos_mask_bwd(_ptr(d_out), _ptr(ids), B, T, C, _ptr(d_h), _ptr(d_pos), _code(d_out), _stream()),
              "edgl_cat_pos_mask_bwd")
        return d_h, d_pos, None


class DictFeatFn(torch.autograd.Function):
    """[g, h, g - h, g * h] along the channels (S2PNM.py:63): edgl_dict_feat_fwd / bwd."""

    @staticmethod
    def forward(ctx, g, h):
        g, h = g.contiguous(), h.contiguous()
        C = g.shape[-1]
        rows = g.numel() // C
        out = torch.empty(g.shape[:-1] + (4 * C,), device=g.device, dtype=g.dtype)
        check(lib.edgl_dict_feat_fwd(_ptr(g), _ptr(h), rows, C, _ptr(out), _code(g), _stream()), "edgl_dict_feat_fwd")
        ctx.save_for_backward(g, h)
        return out

    @staticmethod
    def backward(ctx, d_out):
        g, h = ctx.saved_tensors
        d_out = d_out.contiguous()
        C = g.shape[-1]
        d_g, d_h = torch.empty_like(g), torch.empty_like(h)
        check(lib.edgl_dict_feat_bwd(_ptr(g), _ptr(h), _ptr(d_out), g.numel() // C, C, _ptr(d_g), _ptr(d_h), _code(g), _stream()),
              "edgl_dict_feat_bwd")
        return d_g, d_h


class SigmoidFn(torch.autograd.Function):
    """y = sigmoid(x) (the activation of tf.layers.dense(..., tf.nn.sigmoid), S2PNM.py:64): edgl_sigmoid_fwd / bwd."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y = torch.empty_like(x)
        check(lib.edgl_sigmoid_fwd(_ptr(x), _ptr(y), x.numel(), _code(x), _stream()), "edgl_sigmoid_fwd")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        check(lib.edgl_sigmoid_bwd(_ptr(dy), _ptr(y), _ptr(dx), dy.numel(), _code(dy), _stream()), "edgl_sigmoid_bwd")
        return dx


# ------------------------------------------------------------------------------------------------
# TimelyREC: the multi-aspect time encoder and the time-aware history encoder
# ------------------------------------------------------------------------------------------------
MATE_RANGES = (12, 31, 7, 24)      # month, day, weekday, hour


def mate_windows(window_ratio: float):
    """TimelyREC.py:59: W_g = max(int(M_g * window_ratio + 0.5), 1) + 1 for month, day, weekday, hour."""
    return tuple(max(int(m * float(window_ratio) + 0.5), 1) + 1 for m in MATE_RANGES)


def _seq3(name, t, B, T, C, dtype):
    if not t.is_cuda:
        raise _lib.EdglError("easydgl_amd ops run on the GPU only (got a CPU tensor); there is no CPU fallback")
    if t.dtype != dtype or tuple(t.shape) != (B, T, C) or not t.is_contiguous():
        raise _lib.EdglError(f"{name} must be a contiguous {dtype} [{B}, {T}, {C}] tensor, got {t.dtype} {tuple(t.shape)}")


class MateFn(torch.autograd.Function):
    """Calendar slots, slot attention and the gated combination of TimelyREC (TimelyREC.py:57-77,108-135; edgl_mate_fwd / bwd):
    R [B,T,C] from idx int64 [4,B,T] (month - 1 | day - 1 | weekday | hour), the four tables (masters f32 and compute copies), u
    [B,T,4C] = U [Wu_month | Wu_day | Wu_weekday | Wu_hour] and pq [B,T,C] = U Wc.  `windows`: mate_windows(window_ratio).  Saved:
    the slot probabilities and the gates; the backward recomputes the slots and returns d_u, d_pq and the table gradients, summed
    in a fixed order (no atomics): FLAGS.deterministic needs no second form."""

    @staticmethod
    def forward(ctx, idx, month, day, weekday, hour, month_c, day_c, weekday_c, hour_c, u, pq, windows):
        B, T, C = pq.shape
        u, pq = u.contiguous(), pq.contiguous()
        code = _code(pq)
        _seq3("MateFn: u", u, B, T, 4 * C, pq.dtype)
        if idx.dtype != torch.int64 or tuple(idx.shape) != (4, B, T) or not idx.is_contiguous():
            raise _lib.EdglError(f"MateFn: idx must be a contiguous int64 [4, {B}, {T}] tensor, got {idx.dtype} {tuple(idx.shape)}")
        tabs = (month_c, day_c, weekday_c, hour_c)
        for t, m in zip(tabs, MATE_RANGES):
            if t.dtype != pq.dtype or tuple(t.shape) != (m, C):
                raise _lib.EdglError(f"MateFn: a calendar table must be {pq.dtype} [{m}, {C}], got {t.dtype} {tuple(t.shape)}")
        w = tuple(int(x) for x in windows)
        nsv = int(lib.edgl_mate_saved_floats(*w))
        if nsv <= 0:
            raise _lib.EdglError(f"MateFn: windows {w} unsupported (window_ratio in (0, 0.5])")
        R = torch.empty((B, T, C), device=pq.device, dtype=pq.dtype)
        need = any(ctx.needs_input_grad)
        saved = torch.empty((B, T, nsv), device=pq.device, dtype=torch.float32) if need else None
        check(lib.edgl_mate_fwd(_ptr(idx), *[_ptr(t) for t in tabs], _ptr(u), _ptr(pq), B, T, C, *w, _ptr(R), _ptr(saved), code,
                                _stream()), "edgl_mate_fwd")
        ctx.save_for_backward(idx, month_c, day_c, weekday_c, hour_c, u, pq, saved)
        ctx.meta = (B, T, C, w, code)
        return R

    @staticmethod
    def backward(ctx, d_R):
        idx, month_c, day_c, weekday_c, hour_c, u, pq, saved = ctx.saved_tensors
        B, T, C, w, code = ctx.meta
        d_R = d_R.contiguous()
        d_u, d_pq = torch.empty_like(u), torch.empty_like(pq)
        d_tab = torch.empty((sum(MATE_RANGES), C), device=pq.device, dtype=torch.float32)
        ws = torch.empty(int(lib.edgl_mate_bwd_workspace(B, T, C, *w)), device=pq.device, dtype=torch.float32)
        check(lib.edgl_mate_bwd(_ptr(idx), _ptr(month_c), _ptr(day_c), _ptr(weekday_c), _ptr(hour_c), _ptr(u), _ptr(pq), _ptr(saved),
                                _ptr(d_R), B, T, C, *w, _ptr(d_u), _ptr(d_pq), _ptr(d_tab), _ptr(ws), code, _stream()), "edgl_mate_bwd")
        d_m, d_d, d_w, d_h = torch.split(d_tab, MATE_RANGES, dim=0)
        return None, d_m, d_d, d_w, d_h, None, None, None, None, d_u, d_pq, None


class TaheFn(torch.autograd.Function):
    """hist[q] = sum_{k <= q} ((1 + n_q . n_k) / 2) Hs[k] with n = l2_normalize(R) (sequential.py:247-265; edgl_tahe_fwd / bwd):
    R, Hs [B,T,C] -> hist [B,T,C].  R is both the queries and the keys: one d_R.  No atomics anywhere."""

    @staticmethod
    def forward(ctx, R, Hs):
        B, T, C = R.shape
        R, Hs = R.contiguous(), Hs.contiguous()
        code = _code(R)
        _seq3("TaheFn: Hs", Hs, B, T, C, R.dtype)
        hist = torch.empty_like(R)
        check(lib.edgl_tahe_fwd(_ptr(R), _ptr(Hs), B, T, C, _ptr(hist), code, _stream()), "edgl_tahe_fwd")
        ctx.save_for_backward(R, Hs)
        return hist

    @staticmethod
    def backward(ctx, d_hist):
        R, Hs = ctx.saved_tensors
        B, T, C = R.shape
        d_hist = d_hist.contiguous()
        d_R, d_Hs = torch.empty_like(R), torch.empty_like(Hs)
        check(lib.edgl_tahe_bwd(_ptr(R), _ptr(Hs), _ptr(d_hist), B, T, C, _ptr(d_R), _ptr(d_Hs), _code(R), _stream()), "edgl_tahe_bwd")
        return d_R, d_Hs


class Cat3Fn(torch.autograd.Function):
    """[a | b | c] along the channels (TimelyREC.py:150; edgl_cat3): three [.., C] tensors -> [.., 3C]."""

    @staticmethod
    def forward(ctx, a, b, c):
        a, b, c = a.contiguous(), b.contiguous(), c.contiguous()
        C = a.shape[-1]
        if b.shape != a.shape or c.shape != a.shape or b.dtype != a.dtype or c.dtype != a.dtype:
            raise _lib.EdglError("Cat3Fn: the three inputs must agree in shape and dtype")
        out = torch.empty(a.shape[:-1] + (3 * C,), device=a.device, dtype=a.dtype)
        check(lib.edgl_cat3(_ptr(a), _ptr(b), _ptr(c), a.numel() // C, C, _ptr(out), 0, _code(a), _stream()), "edgl_cat3")
        return out

    @staticmethod
    def backward(ctx, d_out):
        d_out = d_out.contiguous()
        C = d_out.shape[-1] // 3
        shape = d_out.shape[:-1] + (C,)
        da, db, dc = (torch.empty(shape, device=d_out.device, dtype=d_out.dtype) for _ in range(3))
        check(lib.edgl_cat3(_ptr(da), _ptr(db), _ptr(dc), d_out.numel() // (3 * C), C, _ptr(d_out), 1, _code(d_out), _stream()),
              "edgl_cat3")
        return da, db, dc


class TaheMixFn(torch.autograd.Function):
    """Hs = (emb + te_weight * tcode) * (ids != 0) (TimelyREC.py:139-146; edgl_tahe_mix_fwd / bwd): emb, tcode [B,T,C], te_weight
    the trainable f32 scalar.  d_te is a sum of per-workgroup partials in a fixed order."""

    @staticmethod
    def forward(ctx, emb, tcode, te_weight, ids):
        emb, tcode = emb.contiguous(), tcode.contiguous()
        C = emb.shape[-1]
        rows = emb.numel() // C
        if tcode.dtype != emb.dtype or tcode.shape != emb.shape or te_weight.dtype != torch.float32 or te_weight.numel() != 1:
            raise _lib.EdglError("TaheMixFn: tcode must match emb and te_weight must be one f32 scalar")
        if ids.dtype != torch.int64 or ids.numel() != rows or not ids.is_contiguous():
            raise _lib.EdglError("TaheMixFn: ids must be a contiguous int64 tensor with one id per row")
        out = torch.empty_like(emb)
        check(lib.edgl_tahe_mix_fwd(_ptr(emb), _ptr(tcode), _ptr(te_weight), _ptr(ids), rows, C, _ptr(out), _code(emb), _stream()),
              "edgl_tahe_mix_fwd")
        ctx.save_for_backward(tcode, ids)
        ctx.meta = (rows, C, te_weight.shape)
        return out

    @staticmethod
    def backward(ctx, d_out):
        tcode, ids = ctx.saved_tensors
        rows, C, tshape = ctx.meta
        d_out = d_out.contiguous()
        d_emb = torch.empty_like(d_out)
        d_te = torch.empty(1, device=d_out.device, dtype=torch.float32)
        ws = torch.empty(int(lib.edgl_tahe_mix_bwd_workspace(rows)), device=d_out.device, dtype=torch.float32)
        check(lib.edgl_tahe_mix_bwd(_ptr(d_out), _ptr(tcode), _ptr(ids), rows, C, _ptr(d_emb), _ptr(d_te), _ptr(ws), _code(d_out),
                                    _stream()), "edgl_tahe_mix_bwd")
        return d_emb, None, d_te.view(tshape), None


def clip_by_global_norm(grad: torch.Tensor, clip: float) -> None:
    """grad (the flat f32 gradient arena) *= clip / max(||grad||, clip), in place: tf.clip_by_global_norm over every gradient.  The
    sum of squares and the factor stay on the device (edgl_l2_loss with l2 = 2, edgl_clip_scale): no host read, graph-capturable."""
    seg = _whole_segment(grad.numel(), grad.device)
    sumsq = torch.empty(1, device=grad.device, dtype=torch.float32)
    ws = torch.empty(1024, device=grad.device, dtype=torch.float32)
    check(lib.edgl_l2_loss(_ptr(grad), _ptr(seg), 1, 2.0, _ptr(sumsq), 0, _ptr(ws), _stream()), "edgl_l2_loss")
    check(lib.edgl_clip_scale(_ptr(grad), grad.numel(), _ptr(sumsq), float(clip), _stream()), "edgl_clip_scale")


class FFTailFn(torch.autograd.Function):
    """FeedForward tail: (dropout(a) + b) * (ids != 0) in one kernel (edgl_ff_tail); ids None = no row mask."""

    @staticmethod
    def forward(ctx, a, b, ids, drop: Drop):
        a, b = a.contiguous(), b.contiguous()
        out = torch.empty_like(a)
        C = a.shape[-1]
        rows = a.numel() // C
        check(lib.edgl_ff_tail(_ptr(a), _ptr(b), _ptr(ids), rows, C, float(drop.rate), drop.ptr(), drop.stream_id, _ptr(out),
                               _code(a), _stream()), "edgl_ff_tail")
        ctx.ids, ctx.drop, ctx.meta = ids, drop, (rows, C)
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        rows, C = ctx.meta
        d, ids = ctx.drop, ctx.ids
        da = torch.empty_like(g)
        check(lib.edgl_ff_tail(_ptr(g), None, _ptr(ids), rows, C, float(d.rate), d.ptr(), d.stream_id, _ptr(da), _code(g),
                               _stream()), "edgl_ff_tail")
        if ids is None:
            db = g
        else:
            db = torch.empty_like(g)
            check(lib.edgl_mask_rows(_ptr(g), _ptr(ids), _ptr(db), rows, C, _code(g), _stream()), "edgl_mask_rows")
        return da, db, None, None


def ff_tail(a, b, ids, drop: Drop):
    return FFTailFn.apply(a, b, ids, drop)


# ------------------------------------------------------------------------------------------------
# operator-level forms of src/module/coding.py (called on their own, outside the fused model kernels)
# ------------------------------------------------------------------------------------------------
class EmbeddingFn(torch.autograd.Function):
    """Embedding.__call__ (coding.py:60-64): scale * table[ids] with the zero-padded row 0 (edgl_embedding_fwd/bwd).
    table_c is the compute copy of the table (the f32 master, or its bf16 shadow); the gradient goes to the master."""

    @staticmethod
    def forward(ctx, table_master, table_c, ids, zero_pad, scale, deterministic=False):
        """deterministic: the backward sums the rows of every index over a sorted plan (edgl_embedding_bwd_det), no f32 atomics."""
        ids = ids.contiguous()
        rows, C = table_c.shape
        out = torch.empty(tuple(ids.shape) + (C,), device=ids.device, dtype=table_c.dtype)
        check(lib.edgl_embedding_fwd(_ptr(ids), ids.numel(), _ptr(table_c), rows, C, int(bool(zero_pad)), float(scale), _ptr(out),
                                     _code(table_c), _stream()), "edgl_embedding_fwd")
        ctx.save_for_backward(ids)
        ctx.meta = (rows, C, int(bool(zero_pad)), float(scale), bool(deterministic))
        return out

    @staticmethod
    def backward(ctx, d_out):
        (ids,) = ctx.saved_tensors
        rows, C, zero_pad, scale, deterministic = ctx.meta
        d_out = d_out.contiguous()
        d_table = torch.empty((rows, C), device=d_out.device, dtype=torch.float32)
        if deterministic:
            plan = segsum_plan_buffer(ids.numel(), rows + 1, d_out.device)
            check(lib.edgl_embedding_bwd_det(_ptr(ids), ids.numel(), _ptr(d_out), rows, C, zero_pad, scale, _ptr(d_table), _ptr(plan),
                                             _code(d_out), _stream()), "edgl_embedding_bwd_det")
        else:
            check(lib.edgl_embedding_bwd(_ptr(ids), ids.numel(), _ptr(d_out), rows, C, zero_pad, scale, _ptr(d_table), _code(d_out),
                                         _stream()), "edgl_embedding_bwd")
        return d_table, None, None, None, None, None


def time_sinusoid(x: torch.Tensor, tscale: torch.Tensor, num_units: int, dtype=torch.float32) -> torch.Tensor:
    """TimeSinusoidCoding.code (coding.py:137-149): x [B,T] -> [B,T,C], sin on even / cos on odd channels."""
    x = x.to(torch.float32).contiguous()
    out = torch.empty(tuple(x.shape) + (num_units,), device=x.device, dtype=dtype)
    check(lib.edgl_time_sinusoid(_ptr(x), x.numel(), _ptr(tscale), num_units, _ptr(out), _DT[dtype], _stream()),
          "edgl_time_sinusoid")
    return out


class TimeFunctionFn(torch.autograd.Function):
    """TimeFunctionCoding.code (coding.py:113-122): cos(x[..., None] * basis_freq + phase)."""

    @staticmethod
    def forward(ctx, x, freq, phase, dtype):
        x = x.to(torch.float32).contiguous()
        C = freq.shape[0]
        out = torch.empty(tuple(x.shape) + (C,), device=x.device, dtype=dtype)
        check(lib.edgl_time_function_fwd(_ptr(x), x.numel(), _ptr(freq), _ptr(phase), C, _ptr(out), _DT[dtype], _stream()),
              "edgl_time_function_fwd")
        ctx.save_for_backward(x, freq, phase)
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, freq, phase = ctx.saved_tensors
        C = freq.shape[0]
        d_out = d_out.contiguous()
        both = torch.empty(2 * C, device=x.device, dtype=torch.float32)
        ws = torch.empty(int(lib.edgl_time_function_bwd_workspace(C)), device=x.device, dtype=torch.float32)
        check(lib.edgl_time_function_bwd(_ptr(x), x.numel(), _ptr(freq), _ptr(phase), C, _ptr(d_out), _ptr(both[:C]),
                                         _ptr(both[C:]), _ptr(ws), _code(d_out), _stream()), "edgl_time_function_bwd")
        return None, both[:C], both[C:], None
