// The small element-wise kernels of S2PNM (src/model/S2PNM.py:52-66) and gradient clipping by global norm.
//   edgl_cat_pos_mask_fwd/bwd   [h | pos[t]] * (ids != 0)                     (S2PNM.py:52-53; PositionCoding concatenates)
//   edgl_dict_feat_fwd/bwd      [g, h, g - h, g * h]                          (:63, the input of the dictionary head's LayerNorm)
//   edgl_sigmoid_fwd/bwd        the activation of the head's first dense layer (:64)
//   edgl_clip_scale             g *= clip / max(||g||, clip)                  (compat/extender.py: clip_by_global_norm)
// No atomics: d_pos[t] is summed over b in ascending order by one thread per (t, c).
#include "edgl_common.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void cat_pos_mask_fwd_kernel(const T* __restrict__ h, const float* __restrict__ pos,
                                                               const int64_t* __restrict__ ids, long rows, int Tlen, int C,
                                                               T* __restrict__ out) {
    const long total = rows * 2 * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / (2 * C);
        const int c = (int)(i % (2 * C));
        float v = 0.f;
        if (ids[row] != 0) v = c < C ? to_f32(h[row * C + c]) : pos[(row % Tlen) * C + (c - C)];
        out[i] = from_f32<T>(v);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void cat_pos_mask_bwd_h_kernel(const T* __restrict__ dout, const int64_t* __restrict__ ids,
                                                                 long rows, int C, T* __restrict__ dh) {
    const long total = rows * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / C;
        const int c = (int)(i % C);
        dh[i] = ids[row] != 0 ? dout[row * 2 * C + c] : from_f32<T>(0.f);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void cat_pos_mask_bwd_pos_kernel(const T* __restrict__ dout, const int64_t* __restrict__ ids,
                                                                   int B, int Tlen, int C, float* __restrict__ dpos) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Tlen * C) return;
    const int t = i / C, c = i % C;
    float acc = 0.f;
    for (int b = 0; b < B; ++b) {                                    // ascending b: a fixed order
        const long row = (long)b * Tlen + t;
        if (ids[row] != 0) acc += to_f32(dout[row * 2 * C + C + c]);
    }
    dpos[i] = acc;
}

template <typename T>
__global__ __launch_bounds__(256) void dict_feat_fwd_kernel(const T* __restrict__ g, const T* __restrict__ h, long n, int C,
                                                            T* __restrict__ out) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long row = i / C;
        const int c = (int)(i % C);
        const float a = to_f32(g[i]), b = to_f32(h[i]);
        T* o = out + row * 4 * C + c;
        o[0] = g[i]; o[C] = h[i]; o[2 * C] = from_f32<T>(a - b); o[3 * C] = from_f32<T>(a * b);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void dict_feat_bwd_kernel(const T* __restrict__ g, const T* __restrict__ h,
                                                            const T* __restrict__ df, long n, int C, T* __restrict__ dg,
                                                            T* __restrict__ dh) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long row = i / C;
        const int c = (int)(i % C);
        const T* d = df + row * 4 * C + c;
        const float d0 = to_f32(d[0]), d1 = to_f32(d[C]), d2 = to_f32(d[2 * C]), d3 = to_f32(d[3 * C]);
        dg[i] = from_f32<T>(d0 + d2 + d3 * to_f32(h[i]));
        dh[i] = from_f32<T>(d1 - d2 + d3 * to_f32(g[i]));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void sigmoid_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        y[i] = from_f32<T>(1.0f / (1.0f + expf(-to_f32(x[i]))));
}

template <typename T>
__global__ __launch_bounds__(256) void sigmoid_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y, T* __restrict__ dx, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float s = to_f32(y[i]);
        dx[i] = from_f32<T>(to_f32(dy[i]) * s * (1.0f - s));
    }
}

__global__ __launch_bounds__(256) void clip_scale_kernel(float* __restrict__ g, long n, const float* __restrict__ sumsq, float clip) {
    const float norm = sqrtf(sumsq[0]);
    const float scale = clip / fmaxf(norm, clip);                    // exactly 1 when the norm is below the clip
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) g[i] *= scale;
}

inline bool dt_ok(int dtype) { return dtype == EDGL_F32 || dtype == EDGL_BF16; }

template <typename T>
void cat_fwd_t(const void* h, const float* pos, const int64_t* ids, long rows, int Tlen, int C, void* out, hipStream_t st) {
    hipLaunchKernelGGL((cat_pos_mask_fwd_kernel<T>), dim3(grid_for(rows * 2 * C)), dim3(256), 0, st, reinterpret_cast<const T*>(h), pos,
                       ids, rows, Tlen, C, reinterpret_cast<T*>(out));
}
template <typename T>
void cat_bwd_t(const void* dout, const int64_t* ids, int B, int Tlen, int C, void* dh, float* dpos, hipStream_t st) {
    const long rows = (long)B * Tlen;
    hipLaunchKernelGGL((cat_pos_mask_bwd_h_kernel<T>), dim3(grid_for(rows * C)), dim3(256), 0, st, reinterpret_cast<const T*>(dout), ids,
                       rows, C, reinterpret_cast<T*>(dh));
    hipLaunchKernelGGL((cat_pos_mask_bwd_pos_kernel<T>), dim3((Tlen * C + 255) / 256), dim3(256), 0, st,
                       reinterpret_cast<const T*>(dout), ids, B, Tlen, C, dpos);
}
template <typename T>
void feat_fwd_t(const void* g, const void* h, long n, int C, void* out, hipStream_t st) {
    hipLaunchKernelGGL((dict_feat_fwd_kernel<T>), dim3(grid_for(n)), dim3(256), 0, st, reinterpret_cast<const T*>(g),
                       reinterpret_cast<const T*>(h), n, C, reinterpret_cast<T*>(out));
}
template <typename T>
void feat_bwd_t(const void* g, const void* h, const void* df, long n, int C, void* dg, void* dh, hipStream_t st) {
    hipLaunchKernelGGL((dict_feat_bwd_kernel<T>), dim3(grid_for(n)), dim3(256), 0, st, reinterpret_cast<const T*>(g),
                       reinterpret_cast<const T*>(h), reinterpret_cast<const T*>(df), n, C, reinterpret_cast<T*>(dg),
                       reinterpret_cast<T*>(dh));
}
template <typename T>
void sig_t(const void* a, const void* b, void* out, long n, bool bwd, hipStream_t st) {
    if (bwd)
        hipLaunchKernelGGL((sigmoid_bwd_kernel<T>), dim3(grid_for(n)), dim3(256), 0, st, reinterpret_cast<const T*>(a),
                           reinterpret_cast<const T*>(b), reinterpret_cast<T*>(out), n);
    else
        hipLaunchKernelGGL((sigmoid_fwd_kernel<T>), dim3(grid_for(n)), dim3(256), 0, st, reinterpret_cast<const T*>(a),
                           reinterpret_cast<T*>(out), n);
}

}  // namespace

extern "C" int edgl_cat_pos_mask_fwd(const void* h, const float* pos, const int64_t* ids, int B, int T, int C, void* out, int dtype,
                                     void* stream) {
    EDGL_REQUIRE(h && pos && ids && out, EDGL_ERR_NULL, "edgl_cat_pos_mask_fwd: null pointer");
    EDGL_REQUIRE(B > 0 && T > 0 && C > 0, EDGL_ERR_SHAPE, "edgl_cat_pos_mask_fwd: bad shape B=%d T=%d C=%d", B, T, C);
    EDGL_REQUIRE(dt_ok(dtype), EDGL_ERR_DTYPE, "edgl_cat_pos_mask_fwd: bad dtype %d", dtype);
    if (dtype == EDGL_F32) cat_fwd_t<float>(h, pos, ids, (long)B * T, T, C, out, (hipStream_t)stream);
    else cat_fwd_t<bf16>(h, pos, ids, (long)B * T, T, C, out, (hipStream_t)stream);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_cat_pos_mask_bwd(const void* d_out, const int64_t* ids, int B, int T, int C, void* d_h, float* d_pos, int dtype,
                                     void* stream) {
    EDGL_REQUIRE(d_out && ids && d_h && d_pos, EDGL_ERR_NULL, "edgl_cat_pos_mask_bwd: null pointer");
    EDGL_REQUIRE(B > 0 && T > 0 && C > 0 && (long)T * C < 2147483647L, EDGL_ERR_SHAPE, "edgl_cat_pos_mask_bwd: bad shape B=%d T=%d C=%d", B, T, C);
    EDGL_REQUIRE(dt_ok(dtype), EDGL_ERR_DTYPE, "edgl_cat_pos_mask_bwd: bad dtype %d", dtype);
    if (dtype == EDGL_F32) cat_bwd_t<float>(d_out, ids, B, T, C, d_h, d_pos, (hipStream_t)stream);
    else cat_bwd_t<bf16>(d_out, ids, B, T, C, d_h, d_pos, (hipStream_t)stream);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_dict_feat_fwd(const void* g, const void* h, long rows, int C, void* out, int dtype, void* stream) {
    EDGL_REQUIRE(g && h && out, EDGL_ERR_NULL, "edgl_dict_feat_fwd: null pointer");
    EDGL_REQUIRE(rows > 0 && C > 0, EDGL_ERR_SHAPE, "edgl_dict_feat_fwd: bad shape rows=%ld C=%d", rows, C);
    EDGL_REQUIRE(dt_ok(dtype), EDGL_ERR_DTYPE, "edgl_dict_feat_fwd: bad dtype %d", dtype);
    if (dtype == EDGL_F32) feat_fwd_t<float>(g, h, rows * C, C, out, (hipStream_t)stream);
    else feat_fwd_t<bf16>(g, h, rows * C, C, out, (hipStream_t)stream);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_dict_feat_bwd(const void* g, const void* h, const void* d_feat, long rows, int C, void* d_g, void* d_h, int dtype,
                                  void* stream) {
    EDGL_REQUIRE(g && h && d_feat && d_g && d_h, EDGL_ERR_NULL, "edgl_dict_feat_bwd: null pointer");
    EDGL_REQUIRE(rows > 0 && C > 0, EDGL_ERR_SHAPE, "edgl_dict_feat_bwd: bad shape rows=%ld C=%d", rows, C);
    EDGL_REQUIRE(dt_ok(dtype), EDGL_ERR_DTYPE, "edgl_dict_feat_bwd: bad dtype %d", dtype);
    if (dtype == EDGL_F32) feat_bwd_t<float>(g, h, d_feat, rows * C, C, d_g, d_h, (hipStream_t)stream);
    else feat_bwd_t<bf16>(g, h, d_feat, rows * C, C, d_g, d_h, (hipStream_t)stream);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_sigmoid_fwd(const void* x, void* y, long n, int dtype, void* stream) {
    EDGL_REQUIRE(x && y, EDGL_ERR_NULL, "edgl_sigmoid_fwd: null pointer");
    EDGL_REQUIRE(n > 0, EDGL_ERR_SHAPE, "edgl_sigmoid_fwd: bad length %ld", n);
    EDGL_REQUIRE(dt_ok(dtype), EDGL_ERR_DTYPE, "edgl_sigmoid_fwd: bad dtype %d", dtype);
    if (dtype == EDGL_F32) sig_t<float>(x, nullptr, y, n, false, (hipStream_t)stream);
    else sig_t<bf16>(x, nullptr, y, n, false, (hipStream_t)stream);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_sigmoid_bwd(const void* dy, const void* y, void* dx, long n, int dtype, void* stream) {
    EDGL_REQUIRE(dy && y && dx, EDGL_ERR_NULL, "edgl_sigmoid_bwd: null pointer");
    EDGL_REQUIRE(n > 0, EDGL_ERR_SHAPE, "edgl_sigmoid_bwd: bad length %ld", n);
    EDGL_REQUIRE(dt_ok(dtype), EDGL_ERR_DTYPE, "edgl_sigmoid_bwd: bad dtype %d", dtype);
    if (dtype == EDGL_F32) sig_t<float>(dy, y, dx, n, true, (hipStream_t)stream);
    else sig_t<bf16>(dy, y, dx, n, true, (hipStream_t)stream);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_clip_scale(float* grad, long n, const float* sumsq, float clip, void* stream) {
    EDGL_REQUIRE(grad && sumsq, EDGL_ERR_NULL, "edgl_clip_scale: null pointer");
    EDGL_REQUIRE(n > 0 && clip > 0.f, EDGL_ERR_SHAPE, "edgl_clip_scale: bad length %ld / clip %g", n, (double)clip);
    hipLaunchKernelGGL(clip_scale_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, grad, n, sumsq, clip);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
