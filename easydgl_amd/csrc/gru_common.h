// What the GRU recurrence kernels share (k_gru.hip: LDS-resident / plainly streamed; k_gru_wide.hip: the pipelined
// stream): the k-block geometry, the fragment-major pack of R, the shape check and the size of the pack buffer.
#pragma once
#include "edgl_common.h"

namespace {

struct GruDims { int KBN, Kp, ldo, KBN2, K2p, ldo2; };
template <typename T> __host__ __device__ inline GruDims gru_dims(int C) {
    constexpr int KB = ElemTraits<T>::KB, VEC = ElemTraits<T>::VEC;
    GruDims d;
    d.KBN = (C + KB - 1) / KB;  d.Kp = d.KBN * KB;  d.ldo = d.Kp + VEC;              // forward: K = C (zero-padded to the k-block)
    d.KBN2 = (3 * C + KB - 1) / KB;  d.K2p = d.KBN2 * KB;  d.ldo2 = d.K2p + VEC;     // backward: K = 3C
    return d;
}

// R [C, 3C] -> B-fragments.  which = 0 (forward, G = h R): tile nt of the 3C output columns, k = row of R;
// which = 1 (backward, dh = dG R^T): tile ct of the C output channels, k = column of R.
// element j of lane l of (tile, kb): k = kb * KB + (l >> 4) * VEC + j, column = tile * 16 + (l & 15); zeros past the true K.
template <typename T>
__global__ __launch_bounds__(256) void gru_pack_kernel(const T* __restrict__ R, T* __restrict__ out, int C, int which) {
    constexpr int KB = ElemTraits<T>::KB, VEC = ElemTraits<T>::VEC;
    const GruDims d = gru_dims<T>(C);
    const int kbn = which ? d.KBN2 : d.KBN, ntile = which ? C / 16 : 3 * C / 16, ktrue = which ? 3 * C : C;
    const long total = (long)ntile * kbn * 64 * VEC;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i % VEC), l = (int)((i / VEC) % 64);
        const long tk = i / (VEC * 64);
        const int kb = (int)(tk % kbn), tile = (int)(tk / kbn);
        const int k = kb * KB + (l >> 4) * VEC + j, col = tile * 16 + (l & 15);
        T v = from_f32<T>(0.f);
        if (k < ktrue) v = which ? R[(long)col * 3 * C + k] : R[(long)k * 3 * C + col];
        out[i] = v;
    }
}

template <typename T> long gru_pack_bytes_t(int C) {
    const GruDims d = gru_dims<T>(C);
    const long f = 3L * C * d.Kp, b = (long)C * d.K2p;
    return (f > b ? f : b) * (long)sizeof(T);
}

int gru_check(const char* who, int B, int T, int C, int dtype) {
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "%s: bad dtype %d", who, dtype);
    EDGL_REQUIRE(B > 0 && T > 0 && C >= 16 && C <= 512 && C % 16 == 0, EDGL_ERR_SHAPE,
                 "%s: bad shape B=%d T=%d C=%d (C a multiple of 16 up to 512, B >= 1, T >= 1)", who, B, T, C);
    EDGL_REQUIRE((double)B * T * 5.0 * C < 9.0e15 && (long)B * T < 2147483647L, EDGL_ERR_SHAPE, "%s: B*T too large", who);
    return EDGL_OK;
}

}  // namespace
