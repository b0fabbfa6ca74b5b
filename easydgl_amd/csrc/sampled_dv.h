// The per-slot loss coefficient dv of the sampled objectives: ONE copy of each formula for the three places that
// form dv — the register sweep and the atomic table sweep of cand_ce_bwd_kernel (k_cand_ce.hip), which must write and use the
// same bits, and shared_dv_kernel (k_shared_ce.hip).  v is a live slot's value, v0 the label's, gc = g coef[r], a the row
// auxiliary (softmax: lse[r]; bpr: sum over the live slots of sigma(v_s - v0); bce: unused).
//   softmax   dv_s = gc exp(v - a)                 dv_0 = gc (exp(v0 - a) - 1)      coef[r] from edgl_ce_loss_fwd
//   bce       dv_s = gc sigma(v)                   dv_0 = -gc sigma(-v0)            coef[r] = 1 / (W + 1e-5)
//   bpr       dv_s = gc sigma(v - v0)              dv_0 = -gc a                     coef[r] = 1 / ((W + 1e-5) n_r), 0 when n_r = 0
// The softmax expressions are those the kernels held before the forms existed: FORM = SOFTMAX compiles to the same arithmetic.
#pragma once
#include "edgl_common.h"

namespace sdv {

constexpr int SOFTMAX = EDGL_LOSS_SOFTMAX, BCE = EDGL_LOSS_BCE, BPR = EDGL_LOSS_BPR;

// 1 / (1 + exp(-x)) with the exponential of a non-positive argument only: no overflow on either side (x = -inf gives 0)
__device__ __forceinline__ float sigmoidf(float x) {
    const float e = __expf(-fabsf(x));
    const float r = 1.0f / (1.0f + e);
    return x >= 0.0f ? r : e * r;
}

template <int FORM>
__device__ __forceinline__ float dv_slot(float gc, float v, float v0, float a) {
    if constexpr (FORM == BCE) return gc * sigmoidf(v);
    else if constexpr (FORM == BPR) return gc * sigmoidf(v - v0);
    else return gc * __expf(v - a);
}

template <int FORM>
__device__ __forceinline__ float dv_label(float gc, float v0, float a) {
    if constexpr (FORM == BCE) return -(gc * sigmoidf(-v0));          // sigma(v0) - 1 without the cancellation at a large v0
    else if constexpr (FORM == BPR) return -(gc * a);
    else return gc * (__expf(v0 - a) - 1.0f);
}

}  // namespace sdv
