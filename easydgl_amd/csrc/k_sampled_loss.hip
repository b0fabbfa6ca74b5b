// K5e: binary cross-entropy and BPR over sampled negatives.  The slots, their liveness and their values are those of
// k_cand_ce.hip (one list per row) and k_shared_ce.hip (one list per step): the forwards of those files write vals, a dead slot reads
// -inf, and the kernels here turn the values of a row into its loss.  Row r is WEIGHTED iff 1 <= labels[r] < I and r < nvalid[0]
// (nvalid: the compacted shared path; NULL = R).  v0 is the label's value, L_r the live list slots, n_r their number, W the number of
// weighted rows.
//   softplus(x) = max(x, 0) + log1p(exp(-|x|))        sigma(x): the exponential of a non-positive argument only (sampled_dv.h)
//   bce   l_r = softplus(-v0) + sum_{s in L_r} softplus(v_s)          (negatives summed, as tf.nn.nce_loss; N = 1 is SASRec's loss)
//   bpr   l_r = (1 / n_r) sum_{s in L_r} softplus(v_s - v0)           (n_r = 0: l_r = 0 and every derivative 0)
//   loss  = sum over the weighted rows of l_r / (W + 1e-5)            (the denominator of edgl_ce_loss_fwd)
// With a log-Q term in the values bce is tf.nn.nce_loss up to its constant log N, which is not applied.
//
//   sampled_row_loss_kernel    one wave per row.  Lane l sums its slots l, l + 64, .. in ascending order, a fixed xor butterfly joins
//                              the lanes (both partners form a + b), the label's term joins last: the order is a function of the
//                              slot count alone.  No atomics; a row's outputs depend on neither R nor the other rows.  Writes
//                              row_loss = l_r, row_aux (bpr: sum_s sigma(v_s - v0), what dv_label needs; bce: 0) and row_scale
//                              (bce: 1; bpr: 1 / n_r, 0 when n_r = 0); zeros for a row of weight 0.
//   sampled_loss_finish_kernel one workgroup, ce_loss_kernel's shape: a thread adds its rows in ascending order, block_sum joins the
//                              threads.  loss = sum / (W + 1e-5), coef[r] = row_scale[r] / (W + 1e-5).
// The backward is cand_ce_bwd_kernel / shared_dv_kernel with the form as a template parameter (edgl_cand_ce_bwd_form,
// edgl_shared_ce_bwd_form): dv = g coef[r] dl_r/dv by sampled_dv.h, and everything behind dv does not know the objective.
#include "edgl_common.h"
#include "sampled_dv.h"

namespace sloss {

constexpr int MAX_S = 8192;

__device__ __forceinline__ float softplusf(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }

__device__ __forceinline__ bool weighted(const int64_t* labels, const int32_t* nvalid, int r, int R, int I) {
    const int nlive = nvalid ? min(R, max(nvalid[0], 0)) : R;
    const int64_t y = labels[r];
    return r < nlive && y >= 1 && y < I;
}

// vals: [R, ld]; the list slots of row r are vals[r ld + off .. + S) and the label's value is label_val[r] (off = 0) or vals[r ld] (off = 1)
template <int FORM>
__global__ __launch_bounds__(256) void sampled_row_loss_kernel(const float* vals, const float* label_val, const int64_t* labels,
                                                               const int32_t* nvalid, int R, int S, int I, float* row_loss,
                                                               float* row_aux, float* row_scale) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;                                               // (wave-uniform)
    if (!weighted(labels, nvalid, r, R, I)) {                         // (wave-uniform)
        if (lane == 0) { row_loss[r] = 0.0f; row_aux[r] = 0.0f; row_scale[r] = 0.0f; }
        return;
    }
    const int off = label_val ? 0 : 1;
    const float* vrow = vals + (long)r * (S + off);
    const float v0 = label_val ? label_val[r] : vrow[0];
    const float* list = vrow + off;
    float sum = 0.0f, sig = 0.0f, cnt = 0.0f;
    for (int s = lane; s < S; s += 64) {                              // this lane's slots in ascending order
        const float v = list[s];
        if (!(v > -INFINITY)) continue;                               // (the forward's test: dead slots read -inf)
        if constexpr (FORM == sdv::BCE) sum += softplusf(v);
        else {
            sum += softplusf(v - v0);
            sig += sdv::sigmoidf(v - v0);
            cnt += 1.0f;
        }
    }
    sum = wave_sum(sum);
    if constexpr (FORM == sdv::BPR) { sig = wave_sum(sig); cnt = wave_sum(cnt); }
    if (lane != 0) return;
    if constexpr (FORM == sdv::BCE) {
        row_loss[r] = sum + softplusf(-v0);                           // the label last
        row_aux[r] = 0.0f;
        row_scale[r] = 1.0f;
    } else {
        const float inv = cnt > 0.0f ? 1.0f / cnt : 0.0f;
        row_loss[r] = sum * inv;
        row_aux[r] = sig;
        row_scale[r] = inv;
    }
}

__global__ __launch_bounds__(1024) void sampled_loss_finish_kernel(const float* row_loss, const float* row_scale, const int64_t* labels,
                                                                   const int32_t* nvalid, int R, int I, float* loss_out, float* coef) {
    __shared__ float red[16];
    float num = 0.0f, den = 0.0f;
    for (int r = threadIdx.x; r < R; r += 1024) {                     // this thread's rows in ascending order
        const bool on = weighted(labels, nvalid, r, R, I);
        num += on ? row_loss[r] : 0.0f;
        den += on ? 1.0f : 0.0f;
    }
    num = block_sum(num, red);
    den = block_sum(den, red);
    const float W = den + 1e-5f;
    if (threadIdx.x == 0) loss_out[0] = num / W;
    for (int r = threadIdx.x; r < R; r += 1024) coef[r] = weighted(labels, nvalid, r, R, I) ? (1.0f / W) * row_scale[r] : 0.0f;
}

}  // namespace sloss

extern "C" int edgl_sampled_row_loss(const float* vals, const float* label_val, const int64_t* labels, const int32_t* nvalid, int R,
                                     int S, int I, int form, float* row_loss, float* row_aux, float* row_scale, void* stream) {
    EDGL_REQUIRE(form == EDGL_LOSS_BCE || form == EDGL_LOSS_BPR, EDGL_ERR_SHAPE,
                 "edgl_sampled_row_loss: form %d (bce = %d or bpr = %d; the softmax loss is edgl_ce_loss_fwd's)", form, EDGL_LOSS_BCE,
                 EDGL_LOSS_BPR);
    EDGL_REQUIRE(R >= 1 && S >= 1 && S <= sloss::MAX_S && I > 1 && (long)R * ((long)S + 8) < (1L << 31), EDGL_ERR_SHAPE,
                 "edgl_sampled_row_loss: R=%d S=%d I=%d (R >= 1, 1 <= S <= %d, I > 1, R (S + 8) < 2^31)", R, S, I, sloss::MAX_S);
    EDGL_REQUIRE(vals && labels && row_loss && row_aux && row_scale, EDGL_ERR_NULL, "edgl_sampled_row_loss: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)edgl_cdiv(R, 4));
    if (form == EDGL_LOSS_BCE)
        hipLaunchKernelGGL((sloss::sampled_row_loss_kernel<sdv::BCE>), grid, dim3(256), 0, st, vals, label_val, labels, nvalid, R, S, I,
                           row_loss, row_aux, row_scale);
    else
        hipLaunchKernelGGL((sloss::sampled_row_loss_kernel<sdv::BPR>), grid, dim3(256), 0, st, vals, label_val, labels, nvalid, R, S, I,
                           row_loss, row_aux, row_scale);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_sampled_loss_finish(const float* row_loss, const float* row_scale, const int64_t* labels, const int32_t* nvalid,
                                        int R, int I, float* loss_out, float* coef, void* stream) {
    EDGL_REQUIRE(R >= 1 && I > 1, EDGL_ERR_SHAPE, "edgl_sampled_loss_finish: R=%d I=%d (R >= 1, I > 1)", R, I);
    EDGL_REQUIRE(row_loss && row_scale && labels && loss_out && coef, EDGL_ERR_NULL, "edgl_sampled_loss_finish: null pointer");
    hipLaunchKernelGGL(sloss::sampled_loss_finish_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, row_loss, row_scale, labels,
                       nvalid, R, I, loss_out, coef);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
