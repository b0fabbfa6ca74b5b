// Small things around the hot path: error text, the one-shot profile bracket, f32 <-> dtype casts, element-wise add / add_cols,
// dropout, the FeedForward tail and the relu / gelu backward.  (TPP regulariser: k_tpp.hip; optimizer: k_optim.hip; partial-sum
// reductions: k_reduce.hip.)
#include <cstdarg>
#include <cstdio>

#include "edgl_common.h"
#include "lds_limit.h"

namespace {
thread_local char g_err[512] = "";
}  // namespace

extern "C" void edgl_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* edgl_last_error(void) { return g_err; }

int edgl_lds_limit(const void* kern, size_t bytes, const char* who) {
    static LdsLimitMemo memo;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;
    const int e = memo.ensure(kern, dev, bytes, [](const void* k, size_t b) {
        return (int)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);   // hipSuccess is 0
    });
    if (e == 0) return EDGL_OK;
    edgl_set_error("%s: cannot raise the dynamic-LDS limit to %zu B: %s", who, bytes, hipGetErrorString((hipError_t)e));
    return EDGL_ERR_LAUNCH;
}

// ---- one-shot event bracket -----------------------------------------------------------------------------------
namespace {
struct ProfSlot { int id = -1; hipEvent_t e0 = nullptr, e1 = nullptr; };
thread_local ProfSlot g_prof;
}  // namespace
extern "C" int edgl_profile_next(int kernel_id, void* ev_start, void* ev_stop) {
    g_prof.id = kernel_id; g_prof.e0 = (hipEvent_t)ev_start; g_prof.e1 = (hipEvent_t)ev_stop;
    return EDGL_OK;
}
void edgl_prof_begin(int kernel_id, hipStream_t st) {
    if (g_prof.id == kernel_id && g_prof.e0) (void)hipEventRecord(g_prof.e0, st);
}
void edgl_prof_end(int kernel_id, hipStream_t st) {
    if (g_prof.id == kernel_id && g_prof.e1) { (void)hipEventRecord(g_prof.e1, st); g_prof.id = -1; }
}
extern "C" int edgl_version(void) { return 100; }

namespace {

template <typename T>
__global__ void cast_kernel(const float* src, T* dst, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) dst[i] = from_f32<T>(src[i]);
}
template <typename T>
__global__ void cast_back_kernel(const T* src, float* dst, long n, int accumulate) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        dst[i] = accumulate ? dst[i] + to_f32(src[i]) : to_f32(src[i]);
}
template <typename T>
__global__ void add_kernel(const T* a, const T* b, T* out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = from_f32<T>(to_f32(a[i]) + to_f32(b[i]));
}
// dst[r, :ncols] += src[r, :ncols] with independent row strides (residual gradients into the first C channels)
template <typename T>
__global__ void add_cols_kernel(T* dst, int ld_dst, const T* src, const T* src2, int ld_src, long rows, int ncols) {
    const long total = rows * ncols;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / ncols; const int c = (int)(i % ncols);
        float v = to_f32(dst[r * ld_dst + c]) + to_f32(src[r * ld_src + c]);
        if (src2) v += to_f32(src2[r * ld_src + c]);
        dst[r * ld_dst + c] = from_f32<T>(v);
    }
}
// 16-byte vectors along the row (ncols, ld_dst, ld_src multiples of the vector width, 16-byte aligned bases)
template <typename T>
__global__ void add_cols_vec_kernel(T* dst, int ld_dst, const T* src, const T* src2, int ld_src, long rows, int ncols) {
    constexpr int VEC = ElemTraits<T>::VEC;
    const int vpr = ncols / VEC;
    const long total = rows * vpr;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / vpr; const int c = (int)(i % vpr) * VEC;
        Vec16<T> d = ld16<T>(dst + r * ld_dst + c);
        const Vec16<T> a = ld16<T>(src + r * ld_src + c);
        Vec16<T> b = a;
        if (src2) b = ld16<T>(src2 + r * ld_src + c);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            float v = to_f32(d.v[j]) + to_f32(a.v[j]);
            if (src2) v += to_f32(b.v[j]);
            d.v[j] = from_f32<T>(v);
        }
        st16<T>(dst + r * ld_dst + c, d);
    }
}

template <typename T>
__global__ void gelu_bwd_kernel(const T* dy, const T* pre, T* dz, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        dz[i] = from_f32<T>(to_f32(dy[i]) * dgelu_t<T>(to_f32(pre[i])));
}

template <typename T>
__global__ void relu_bwd_kernel(const T* dy, const T* y, T* dz, long n) {   // dz = dy * [y > 0]
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        dz[i] = to_f32(y[i]) > 0.f ? dy[i] : from_f32<T>(0.f);
}

}  // namespace

extern "C" int edgl_cast(const float* src, void* dst, long n, int dtype, void* stream) {
    EDGL_REQUIRE(src && dst, EDGL_ERR_NULL, "edgl_cast: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == EDGL_BF16) hipLaunchKernelGGL((cast_kernel<bf16>), dim3(grid_for(n)), dim3(256), 0, st, src, (bf16*)dst, n);
    else if (dtype == EDGL_F32) hipLaunchKernelGGL((cast_kernel<float>), dim3(grid_for(n)), dim3(256), 0, st, src, (float*)dst, n);
    else { edgl_set_error("edgl_cast: bad dtype %d", dtype); return EDGL_ERR_DTYPE; }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_cast_back(const void* src, float* dst, long n, int accumulate, int dtype, void* stream) {
    EDGL_REQUIRE(src && dst, EDGL_ERR_NULL, "edgl_cast_back: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == EDGL_BF16) hipLaunchKernelGGL((cast_back_kernel<bf16>), dim3(grid_for(n)), dim3(256), 0, st, (const bf16*)src, dst, n, accumulate);
    else if (dtype == EDGL_F32) hipLaunchKernelGGL((cast_back_kernel<float>), dim3(grid_for(n)), dim3(256), 0, st, (const float*)src, dst, n, accumulate);
    else { edgl_set_error("edgl_cast_back: bad dtype %d", dtype); return EDGL_ERR_DTYPE; }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_add(const void* a, const void* b, void* out, long n, int dtype, void* stream) {
    EDGL_REQUIRE(a && b && out, EDGL_ERR_NULL, "edgl_add: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == EDGL_BF16) hipLaunchKernelGGL((add_kernel<bf16>), dim3(grid_for(n)), dim3(256), 0, st, (const bf16*)a, (const bf16*)b, (bf16*)out, n);
    else if (dtype == EDGL_F32) hipLaunchKernelGGL((add_kernel<float>), dim3(grid_for(n)), dim3(256), 0, st, (const float*)a, (const float*)b, (float*)out, n);
    else { edgl_set_error("edgl_add: bad dtype %d", dtype); return EDGL_ERR_DTYPE; }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_add_cols(void* dst, int ld_dst, const void* src, const void* src2, int ld_src, long rows, int ncols,
                             int dtype, void* stream) {
    EDGL_REQUIRE(dst && src, EDGL_ERR_NULL, "edgl_add_cols: null pointer");
    EDGL_REQUIRE(dtype == EDGL_BF16 || dtype == EDGL_F32, EDGL_ERR_DTYPE, "edgl_add_cols: bad dtype %d", dtype);
    hipStream_t st = (hipStream_t)stream;
    const int vec = dtype == EDGL_BF16 ? 8 : 4;
    const bool vok = ncols % vec == 0 && ld_dst % vec == 0 && ld_src % vec == 0 &&
                     (((uintptr_t)dst | (uintptr_t)src | (uintptr_t)src2) & 15) == 0;
    const long n = vok ? rows * (ncols / vec) : rows * ncols;
    if (dtype == EDGL_BF16) {
        if (vok) hipLaunchKernelGGL((add_cols_vec_kernel<bf16>), dim3(grid_for(n)), dim3(256), 0, st, (bf16*)dst, ld_dst, (const bf16*)src, (const bf16*)src2, ld_src, rows, ncols);
        else hipLaunchKernelGGL((add_cols_kernel<bf16>), dim3(grid_for(n)), dim3(256), 0, st, (bf16*)dst, ld_dst, (const bf16*)src, (const bf16*)src2, ld_src, rows, ncols);
    } else {
        if (vok) hipLaunchKernelGGL((add_cols_vec_kernel<float>), dim3(grid_for(n)), dim3(256), 0, st, (float*)dst, ld_dst, (const float*)src, (const float*)src2, ld_src, rows, ncols);
        else hipLaunchKernelGGL((add_cols_kernel<float>), dim3(grid_for(n)), dim3(256), 0, st, (float*)dst, ld_dst, (const float*)src, (const float*)src2, ld_src, rows, ncols);
    }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

template <typename T>
__global__ void dropout_state_kernel(const T* x, T* y, long n, const uint64_t* rng, uint32_t stream_id, float rate) {
    const DropKey dk = make_dropkey(rng, stream_id, rate);
    const long n4 = n >> 2;   // 4 elements per thread; the mask depends on the element index only
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < n4; g += (long)gridDim.x * blockDim.x) {
        const Frag4<T> v = frag_ld<T>(x + g * 4);
        Frag4<T> o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o.v[j] = from_f32<T>(drop_apply(dk, (uint64_t)(g * 4 + j), to_f32(v.v[j])));
        if constexpr (sizeof(T) == 4) *reinterpret_cast<uint4*>(y + g * 4) = *reinterpret_cast<uint4*>(&o);
        else *reinterpret_cast<uint2*>(y + g * 4) = *reinterpret_cast<uint2*>(&o);
    }
    for (long i = n4 * 4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        y[i] = from_f32<T>(drop_apply(dk, (uint64_t)i, to_f32(x[i])));
}

extern "C" int edgl_dropout(const void* x, void* y, long n, float drop_rate, const uint64_t* rng_state, uint32_t stream_id,
                            int dtype, void* stream) {
    EDGL_REQUIRE(x && y && (drop_rate == 0.f || rng_state), EDGL_ERR_NULL, "edgl_dropout: null pointer");
    hipStream_t st = (hipStream_t)stream;
    EDGL_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, EDGL_ERR_SHAPE, "edgl_dropout: buffers must be 16-byte aligned");
    const dim3 grid(grid_for((n + 3) / 4));
    if (dtype == EDGL_BF16) hipLaunchKernelGGL((dropout_state_kernel<bf16>), grid, dim3(256), 0, st, (const bf16*)x, (bf16*)y, n, rng_state, stream_id, drop_rate);
    else if (dtype == EDGL_F32) hipLaunchKernelGGL((dropout_state_kernel<float>), grid, dim3(256), 0, st, (const float*)x, (float*)y, n, rng_state, stream_id, drop_rate);
    else { edgl_set_error("edgl_dropout: bad dtype %d", dtype); return EDGL_ERR_DTYPE; }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

// FeedForward tail (Base.py:83-86 followed by `*= seqs_masks`, TGAT.py:70): out = (dropout(a) + b) * (ids != 0), 4 elements
// per thread; b and ids optional.  With b == NULL it is also the backward of the `a` branch (mask and dropout commute).
template <typename T>
__global__ __launch_bounds__(256) void ff_tail_kernel(const T* a, const T* b, const int64_t* ids, long rows, int C, T* out,
                                                      const uint64_t* rng, uint32_t stream_id, float rate) {
    const DropKey dk = make_dropkey(rng, stream_id, rate);
    const int cpr = C >> 2;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < rows * cpr; g += (long)gridDim.x * blockDim.x) {
        const long row = g / cpr;
        const long e0 = g * 4;
        const Frag4<T> av = frag_ld<T>(a + e0);
        const Frag4<T> bv = b ? frag_ld<T>(b + e0) : frag_zero<T>();
        const float m = (!ids || ids[row] != 0) ? 1.f : 0.f;
        Frag4<T> o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o.v[j] = from_f32<T>((drop_apply(dk, (uint64_t)(e0 + j), to_f32(av.v[j])) + to_f32(bv.v[j])) * m);
        if constexpr (sizeof(T) == 4) *reinterpret_cast<uint4*>(out + e0) = *reinterpret_cast<uint4*>(&o);
        else *reinterpret_cast<uint2*>(out + e0) = *reinterpret_cast<uint2*>(&o);
    }
}

extern "C" int edgl_ff_tail(const void* a, const void* b, const int64_t* ids, long rows, int C, float drop_rate,
                            const uint64_t* rng_state, uint32_t stream_id, void* out, int dtype, void* stream) {
    EDGL_REQUIRE(a && out && (drop_rate == 0.f || rng_state), EDGL_ERR_NULL, "edgl_ff_tail: null pointer");
    EDGL_REQUIRE(rows > 0 && C > 0 && C % 4 == 0, EDGL_ERR_SHAPE, "edgl_ff_tail: bad shape rows=%ld C=%d", rows, C);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(grid_for(rows * (C / 4)));
    if (dtype == EDGL_BF16) hipLaunchKernelGGL((ff_tail_kernel<bf16>), grid, dim3(256), 0, st, (const bf16*)a, (const bf16*)b, ids, rows, C, (bf16*)out, rng_state, stream_id, drop_rate);
    else if (dtype == EDGL_F32) hipLaunchKernelGGL((ff_tail_kernel<float>), grid, dim3(256), 0, st, (const float*)a, (const float*)b, ids, rows, C, (float*)out, rng_state, stream_id, drop_rate);
    else { edgl_set_error("edgl_ff_tail: bad dtype %d", dtype); return EDGL_ERR_DTYPE; }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_relu_bwd(const void* dy, const void* y, void* dz, long n, int dtype, void* stream) {
    EDGL_REQUIRE(dy && y && dz, EDGL_ERR_NULL, "edgl_relu_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == EDGL_BF16) hipLaunchKernelGGL((relu_bwd_kernel<bf16>), dim3(grid_for(n)), dim3(256), 0, st, (const bf16*)dy, (const bf16*)y, (bf16*)dz, n);
    else if (dtype == EDGL_F32) hipLaunchKernelGGL((relu_bwd_kernel<float>), dim3(grid_for(n)), dim3(256), 0, st, (const float*)dy, (const float*)y, (float*)dz, n);
    else { edgl_set_error("edgl_relu_bwd: bad dtype %d", dtype); return EDGL_ERR_DTYPE; }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_gelu_bwd(const void* dy, const void* pre, void* dz, long n, int dtype, void* stream) {
    EDGL_REQUIRE(dy && pre && dz, EDGL_ERR_NULL, "edgl_gelu_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == EDGL_BF16) hipLaunchKernelGGL((gelu_bwd_kernel<bf16>), dim3(grid_for(n)), dim3(256), 0, st, (const bf16*)dy, (const bf16*)pre, (bf16*)dz, n);
    else if (dtype == EDGL_F32) hipLaunchKernelGGL((gelu_bwd_kernel<float>), dim3(grid_for(n)), dim3(256), 0, st, (const float*)dy, (const float*)pre, (float*)dz, n);
    else { edgl_set_error("edgl_gelu_bwd: bad dtype %d", dtype); return EDGL_ERR_DTYPE; }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
