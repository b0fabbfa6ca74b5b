// The rows around the loss (EasyDGL.py:155,177-188): what runs before and after the scoring kernels of k_score.hip.
//   compact_scan / compact_gather / scatter_rows   the weighted rows (label != 0) first, and back (scan body: batch_prep.h)
//   ce_loss_kernel                                 loss and loss coefficients from (row lse, label logit)
//   ce_loss_parts_kernel                           the loss from the per-workgroup sums the one-launch row finish left
//                                                  (edgl_score_flash_fwd_rows_wp; their number: edgl_score_ce_nparts, k_score.hip)
#include <algorithm>

#include "edgl_common.h"
#include "batch_prep.h"

namespace {

// Rows whose label is 0 (a masked position that fell on padding) have weight 0 in the loss (EasyDGL.py:180): they
// contribute nothing to the loss or to any gradient.  compact_scan orders the weighted rows first
// (perm[j] = original row of compact row j, inv[r] = compact index of row r or -1, nvalid = #weighted rows), so the
// scoring kernels can skip the rest exactly.
__global__ __launch_bounds__(1024) void compact_scan_kernel(const int64_t* labels, int R, int32_t* perm, int32_t* inv,
                                                            int32_t* nvalid, int64_t* labels_c) {
    __shared__ int wcnt[2 * 16 * 16];
    batch_prep::compact_scan_body<1024>(labels, R, perm, inv, nvalid, labels_c, wcnt);
}
template <typename T>
__global__ void compact_gather_kernel(const T* rows, const int64_t* labels, const int32_t* perm, int R, int C, T* rows_c,
                                      int64_t* labels_c) {
    const int vpr = C / ElemTraits<T>::VEC;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)R * vpr; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i / vpr), cv = (int)(i % vpr);
        const int r = perm[j];
        st16<T>(rows_c + (long)j * C + cv * ElemTraits<T>::VEC, r >= 0 ? ld16<T>(rows + (long)r * C + cv * ElemTraits<T>::VEC) : zero16<T>());
        if (cv == 0) labels_c[j] = r >= 0 ? labels[r] : 0;
    }
}
template <typename T>
__global__ void scatter_rows_kernel(const T* rows_c, const int32_t* inv, int R, int C, T* rows) {
    const int vpr = C / ElemTraits<T>::VEC;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)R * vpr; i += (long)gridDim.x * blockDim.x) {
        const int r = (int)(i / vpr), cv = (int)(i % vpr);
        const int j = inv[r];
        st16<T>(rows + (long)r * C + cv * ElemTraits<T>::VEC, j >= 0 ? ld16<T>(rows_c + (long)j * C + cv * ElemTraits<T>::VEC) : zero16<T>());
    }
}

// ---------------------------------------------------------------------------------------------
// CE loss from (lse, label logit) — EasyDGL.py:155,177-185
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void ce_loss_kernel(const float* row_lse, const float* label_logit, const int64_t* labels, int R,
                                                       float* loss_out, float* coef, const float* add_in, const float* add_in2,
                                                       const int32_t* wtotal) {
    // one workgroup; a thread keeps up to CE_KEEP of its rows' probabilities in registers between the two passes (the loads of
    // a pass are independent, so they overlap instead of paying one memory round trip per row)
    constexpr int CE_KEEP = 16;
    __shared__ float red[16];
    float py[CE_KEEP];
    float num = 0.f, den = 0.f;
    {   // all 3 * CE_KEEP loads issued before the first use (`m < R && labels[..]` is a guarded load: a branch and a wait per row
        // — 16 dependent round trips, 10 us for this kernel)
        int64_t lb[CE_KEEP];
        float lg[CE_KEEP], ls[CE_KEEP];
#pragma unroll
        for (int i = 0; i < CE_KEEP; ++i) {
            const int mc = min((int)threadIdx.x + i * 1024, R - 1);
            lb[i] = labels[mc]; lg[i] = label_logit[mc]; ls[i] = row_lse[mc];
        }
#pragma unroll
        for (int i = 0; i < CE_KEEP; ++i) asm volatile("" : "+v"(lb[i]), "+v"(lg[i]), "+v"(ls[i]));
#pragma unroll
        for (int i = 0; i < CE_KEEP; ++i) {
            const int m = threadIdx.x + i * 1024;
            const bool on = (m < R) & (lb[i] != 0);   // weight 0 (EasyDGL.py:180): lse may be undefined for such rows
            const float v = __expf(lg[i] - ls[i]);
            py[i] = on ? v : -1.f;
            num += on ? -__logf(v + 1e-5f) : 0.f;
            den += on ? 1.f : 0.f;
        }
    }
    for (int m = threadIdx.x + CE_KEEP * 1024; m < R; m += 1024) {
        if (labels[m] == 0) continue;
        num += -__logf(__expf(label_logit[m] - row_lse[m]) + 1e-5f);
        den += 1.f;
    }
    num = block_sum(num, red);
    den = block_sum(den, red);
    const float W = (wtotal ? (float)wtotal[0] : den) + 1e-5f;     // data parallel: the weighted rows of all ranks
    if (threadIdx.x == 0) loss_out[0] = num / W + (add_in ? add_in[0] : 0.f) + (add_in2 ? add_in2[0] : 0.f);   // + regularisation terms
    if (!coef) return;    // (the flash forward wrote the coefficients: edgl_score_flash_fwd_coef)
#pragma unroll
    for (int i = 0; i < CE_KEEP; ++i) {
        const int m = threadIdx.x + i * 1024;
        if (m < R) coef[m] = py[i] >= 0.f ? (1.f / W) * (py[i] / (py[i] + 1e-5f)) : 0.f;
    }
    for (int m = threadIdx.x + CE_KEEP * 1024; m < R; m += 1024) {
        float cf = 0.f;
        if (labels[m] != 0) {
            const float v = __expf(label_logit[m] - row_lse[m]);
            cf = (1.f / W) * (v / (v + 1e-5f));
        }
        coef[m] = cf;
    }
}

// ce_loss_kernel for a forward that left per-workgroup sums of -log(p_label + 1e-5) (flash_finish_lse_kernel: ce_part): the loss is
// their sum over the weighted-row count (+ the regularisation terms) — a few thousand numbers instead of three arrays of R rows,
// and nothing of the batch (labels, lse, label logits) is read: the launch may run any time before the next forward rewrites ce_part.
__global__ __launch_bounds__(1024) void ce_loss_parts_kernel(const float* ce_part, int nparts, float* loss_out,
                                                             const float* add_in, const float* add_in2, const int32_t* wtotal) {
    __shared__ float red[16];
    float num = 0.f;
    for (int i0 = threadIdx.x; i0 < nparts; i0 += 1024 * 4) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ce_part[min(i0 + j * 1024, nparts - 1)];
#pragma unroll
        for (int j = 0; j < 4; ++j) num += i0 + j * 1024 < nparts ? v[j] : 0.f;
    }
    num = block_sum(num, red);
    if (threadIdx.x != 0) return;
    const float W = (wtotal ? (float)wtotal[0] : ce_part[nparts]) + 1e-5f;     // (the count rides behind the sums)
    loss_out[0] = num / W + (add_in ? add_in[0] : 0.f) + (add_in2 ? add_in2[0] : 0.f);
}

}  // namespace

// edgl_compact_rows = edgl_compact_scan (labels only: may run as soon as the batch is known, e.g. on a side stream at the start
// of the step) + edgl_compact_gather (needs the rows)
extern "C" int edgl_compact_scan(const int64_t* labels, int R, int32_t* perm, int32_t* inv, int32_t* nvalid, void* stream) {
    EDGL_REQUIRE(labels && perm && inv && nvalid, EDGL_ERR_NULL, "edgl_compact_scan: null pointer");
    EDGL_REQUIRE(R > 0, EDGL_ERR_SHAPE, "edgl_compact_scan: bad shape R=%d", R);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, labels, R, perm, inv, nvalid, (int64_t*)nullptr);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
// The scan that also writes the compacted labels (labels_c [R]: the labels of the weighted rows first, 0 behind them) — with
// it and edgl_tail_fwd's row map the rows reach the scoring kernels without edgl_compact_gather.
extern "C" int edgl_compact_scan_labels(const int64_t* labels, int R, int32_t* perm, int32_t* inv, int32_t* nvalid,
                                        int64_t* labels_c, void* stream) {
    EDGL_REQUIRE(labels && perm && inv && nvalid && labels_c, EDGL_ERR_NULL, "edgl_compact_scan_labels: null pointer");
    EDGL_REQUIRE(R > 0, EDGL_ERR_SHAPE, "edgl_compact_scan_labels: bad shape R=%d", R);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, labels, R, perm, inv, nvalid, labels_c);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
extern "C" int edgl_compact_gather(const void* rows, const int64_t* labels, const int32_t* perm, int R, int C, void* rows_c,
                                   int64_t* labels_c, int dtype, void* stream) {
    EDGL_REQUIRE(rows && labels && perm && rows_c && labels_c, EDGL_ERR_NULL, "edgl_compact_gather: null pointer");
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_compact_gather: bad dtype %d", dtype);
    EDGL_REQUIRE(R > 0 && C % (dtype == EDGL_BF16 ? 8 : 4) == 0, EDGL_ERR_SHAPE, "edgl_compact_gather: bad shape R=%d C=%d", R, C);
    hipStream_t st = (hipStream_t)stream;
    const long nv = (long)R * C / (dtype == EDGL_BF16 ? 8 : 4);
    const unsigned nb = (unsigned)std::min<long>((nv + 255) / 256, 2048);
    if (dtype == EDGL_F32) hipLaunchKernelGGL((compact_gather_kernel<float>), dim3(nb), dim3(256), 0, st, (const float*)rows, labels, perm, R, C, (float*)rows_c, labels_c);
    else hipLaunchKernelGGL((compact_gather_kernel<bf16>), dim3(nb), dim3(256), 0, st, (const bf16*)rows, labels, perm, R, C, (bf16*)rows_c, labels_c);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
extern "C" int edgl_compact_rows(const void* rows, const int64_t* labels, int R, int C, int32_t* perm, int32_t* inv,
                                 int32_t* nvalid, void* rows_c, int64_t* labels_c, int dtype, void* stream) {
    EDGL_REQUIRE(rows && labels && perm && inv && nvalid && rows_c && labels_c, EDGL_ERR_NULL, "edgl_compact_rows: null pointer");
    const int rc = edgl_compact_scan(labels, R, perm, inv, nvalid, stream);
    return rc ? rc : edgl_compact_gather(rows, labels, perm, R, C, rows_c, labels_c, dtype, stream);
}

extern "C" int edgl_scatter_rows(const void* rows_c, const int32_t* inv, int R, int C, void* rows, int dtype, void* stream) {
    EDGL_REQUIRE(rows_c && inv && rows, EDGL_ERR_NULL, "edgl_scatter_rows: null pointer");
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_scatter_rows: bad dtype %d", dtype);
    hipStream_t st = (hipStream_t)stream;
    const long nv = (long)R * C / (dtype == EDGL_BF16 ? 8 : 4);
    const unsigned nb = (unsigned)std::min<long>((nv + 255) / 256, 2048);
    if (dtype == EDGL_F32) hipLaunchKernelGGL((scatter_rows_kernel<float>), dim3(nb), dim3(256), 0, st, (const float*)rows_c, inv, R, C, (float*)rows);
    else hipLaunchKernelGGL((scatter_rows_kernel<bf16>), dim3(nb), dim3(256), 0, st, (const bf16*)rows_c, inv, R, C, (bf16*)rows);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_ce_loss_fwd_add_w(const float* row_lse, const float* label_logit, const int64_t* labels, int R, float* loss_out,
                                      float* coef, const float* add_in, const float* add_in2, const int32_t* wtotal, void* stream) {
    EDGL_REQUIRE(row_lse && label_logit && labels && loss_out, EDGL_ERR_NULL, "edgl_ce_loss_fwd: null pointer");   // coef may be NULL
    hipLaunchKernelGGL(ce_loss_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, row_lse, label_logit, labels, R, loss_out, coef,
                       add_in, add_in2, wtotal);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
// loss (EasyDGL.py:181-188) from the sums edgl_score_flash_fwd_rows_wp left in ce_part: sum / (weighted rows + 1e-5) + add_in + add_in2
// (ce_part: edgl_score_ce_nparts(R, C) sums and, behind them, the weighted-row count — nparts + 1 floats; wtotal: the global count
// under data parallelism)
extern "C" int edgl_ce_loss_parts(const float* ce_part, int nparts, float* loss_out, const float* add_in, const float* add_in2,
                                  const int32_t* wtotal, void* stream) {
    EDGL_REQUIRE(ce_part && loss_out && nparts > 0, EDGL_ERR_NULL, "edgl_ce_loss_parts: null pointer / bad size");
    hipLaunchKernelGGL(ce_loss_parts_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, ce_part, nparts, loss_out, add_in, add_in2,
                       wtotal);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
extern "C" int edgl_ce_loss_fwd_add(const float* row_lse, const float* label_logit, const int64_t* labels, int R, float* loss_out,
                                    float* coef, const float* add_in, const float* add_in2, void* stream) {
    return edgl_ce_loss_fwd_add_w(row_lse, label_logit, labels, R, loss_out, coef, add_in, add_in2, nullptr, stream);
}
extern "C" int edgl_ce_loss_fwd(const float* row_lse, const float* label_logit, const int64_t* labels, int R,
                                float* loss_out, float* coef, void* stream) {
    return edgl_ce_loss_fwd_add(row_lse, label_logit, labels, R, loss_out, coef, nullptr, nullptr, stream);
}
