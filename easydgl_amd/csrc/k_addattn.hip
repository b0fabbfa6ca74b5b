// K15: causal additive (Bahdanau) attention over recurrent states — the unit of NARM (Li et al., CIKM'17) behind its GRU encoder.
// Per sample, with h [T,C], a12 [T,2C] = h (A1 | A2), v [C] (f32) and the key ids:
//     e[t,j] = sum_c v[c] sigmoid(a1[t,c] + a2[j,c]);   alpha[t,j] = e[t,j] if j <= t and ids[j] != 0 else 0;   out[t] = sum_j alpha[t,j] h[j]
// No softmax (as in the paper); a query whose own id is 0 is computed like any other; a sample without a real key gives zeros.
// The energy is no dot product: a (pair, channel) costs one v_exp_f32 and one v_rcp_f32, so the kernels are bound by the
// transcendental pipe and the matrix pipe only carries alpha H (forward), dOut H^T and alpha^T dOut (backward).
//
// Work split (all three kernels): a workgroup of 4 waves owns one (sample, 16-row tile) and walks the 16-row tiles of the other
// side up to / from the diagonal; the tiles are staged through LDS once per workgroup.  The four waves see the SAME 16 x 16 pair
// tile and split the CHANNELS: wave w runs the sigmoid loop over channels [w C/4, (w+1) C/4) for the four pairs the 16x16 MFMA
// accumulator layout gives each lane (lane = (g, i): pairs (4g + r, i), r = 0..3), the four partial tiles are summed through LDS
// in a fixed order, and every wave then owns the 16-channel output tiles w, w+4, ... of the matrix product.  The finished alpha
// tile is an accumulator image, so it is the B operand of the product as it stands (frag_from_acc); the other operand is read
// from an image staged in the orientation the product needs (h or dOut turned: [C][16 + pad]).  The a1 / a2 images are f32 and
// pre-multiplied by -log2(e): sigmoid(x) = rcp(1 + exp2(a1' + a2')).  No [T,T] or [T,T,C] array exists in memory and the
// forward saves nothing per pair.
//   forward       lane = (keys 4g + r, query i); a1 tile staged once, per key tile: a2 (f32), h turned; out^T += h^T alpha^T
//   query sweep   same orientation; g^T = h dOut^T (contraction split over the waves by 16-channel slices, dOut in registers),
//                 d_a1[t,c] = v[c] sum_j g s (1 - s) and the workgroup's row of d_v[c] = sum g s
//   key sweep     lane = (queries 4g + r, key i); a2 / h of the key tile once, per query tile: a1 (f32), dOut turned;
//                 d_a2[j,c] = v[c] sum_t g s (1 - s), d_h^T += dOut^T alpha
// The sums over the lane's four pairs are local; the sum over the four lane groups is a 4 x 4 transpose-reduce on the row swaps
// of edgl_common.h (three swaps per four channels), after which lane group g owns channel c + g of the row and adds it to its
// own LDS word — one owner per word, no atomics.  d_v: one partial row per query-sweep workgroup, summed by a finishing launch
// in a fixed order.  Every address of d_a12 / d_h has one writer: two calls give the same bits.  A key tile of padding is skipped
// by the walks (its alpha is exactly 0) and gets exact zeros from the key sweep.
#include "tattn_common.h"   // frag_st

namespace {

constexpr int AA_LDT = 20;                          // row stride of a turned image [C][16 + 4]
constexpr float AA_NLOG2E = -1.4426950408889634f;
constexpr int AA_LDS = 160 * 1024;

struct AaP {
    const void *h, *a12; const float* v; const int64_t* ids;
    int B, T, C, NT;
    void *out, *h_copy; int ld_out;                 // forward
    const void *d_out, *d_res; int ld_dout;         // backward
    void *d_a12, *d_h; float* dv_part;
};

__device__ __forceinline__ float aa_sig(float x) {  // sigmoid of the unscaled argument: x = -log2(e) (a1 + a2)
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x));
}

// ---- staging: 16 rows at row0 of src (row stride ld); rows past the end repeat row Tn - 1 (their pairs are masked) ---------
template <typename T>
__device__ __forceinline__ void aa_stage_scaled(float* img, int LDF, const T* src, long ld, int row0, int Tn, int C) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int cpr = C / VEC;
    for (int i = threadIdx.x; i < 16 * cpr; i += 256) {
        const int row = i / cpr, c = (i - row * cpr) * VEC;
        const Vec16<T> x = ld16<T>(src + (long)min(row0 + row, Tn - 1) * ld + c);
        float* d = img + row * LDF + c;
#pragma unroll
        for (int e = 0; e < VEC; e += 4)
            *reinterpret_cast<f32x4*>(d + e) = f32x4{to_f32(x.v[e]) * AA_NLOG2E, to_f32(x.v[e + 1]) * AA_NLOG2E,
                                                     to_f32(x.v[e + 2]) * AA_NLOG2E, to_f32(x.v[e + 3]) * AA_NLOG2E};
    }
}
template <typename T>
__device__ __forceinline__ void aa_stage_rows(T* img, int LDR, const T* src, long ld, int row0, int Tn, int C) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int cpr = C / VEC;
    for (int i = threadIdx.x; i < 16 * cpr; i += 256) {
        const int row = i / cpr, c = (i - row * cpr) * VEC;
        st16<T>(img + row * LDR + c, ld16<T>(src + (long)min(row0 + row, Tn - 1) * ld + c));
    }
}
// [C][AA_LDT]: rows = channels.  4-element chunks (ld is a multiple of 4 only), the 16 rows of a chunk on neighbouring lanes
template <typename T>
__device__ __forceinline__ void aa_stage_turned(T* img, const T* src, long ld, int row0, int Tn, int C) {
    for (int i = threadIdx.x; i < 4 * C; i += 256) {
        const int row = i & 15, c = (i >> 4) * 4;
        const Frag4<T> x = frag_ld<T>(src + (long)min(row0 + row, Tn - 1) * ld + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) img[(c + e) * AA_LDT + row] = x.v[e];
    }
}
template <typename T> __device__ __forceinline__ Frag4<T> aa_frag_strided(const T* p, int stride) {
    Frag4<T> f;
#pragma unroll
    for (int r = 0; r < 4; ++r) f.v[r] = p[r * stride];
    return f;
}

// Bitmap of the 16-key tiles below `kend` that hold a real key, and v in LDS.  Ends with a barrier.
__device__ __forceinline__ uint64_t aa_live(const int64_t* idr, int kend, uint32_t* s_live) {
    if (threadIdx.x < 2) s_live[threadIdx.x] = 0u;
    __syncthreads();
    for (int k = threadIdx.x; k < kend; k += 256)
        if (idr[k] != 0) atomicOr(&s_live[k >> 9], 1u << ((k >> 4) & 31));
    __syncthreads();
    return (uint64_t)s_live[0] | ((uint64_t)s_live[1] << 32);
}

// sum over the four lane groups of four values at once: lane group g returns the total of p<g> (fixed order)
__device__ __forceinline__ float aa_group_reduce4(float p0, float p1, float p2, float p3) {
    const FPair a = swap16(p0, p1), b = swap16(p2, p3);      // rows {p0: 0+1, p1: 0+1, p0: 2+3, p1: 2+3} after the add
    const FPair q = swap32(a.first + a.second, b.first + b.second);
    return q.first + q.second;
}
__device__ __forceinline__ float aa_row16_sum(float v) {     // sum over the 16 lanes of a lane group
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the four partial tiles of the waves -> the whole tile, in wave order
__device__ __forceinline__ f32x4 aa_red_sum(const float* red, int lane) {
    f32x4 s;
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = ((red[r * 64 + lane] + red[(4 + r) * 64 + lane]) + red[(8 + r) * 64 + lane]) + red[(12 + r) * 64 + lane];
    return s;
}
__device__ __forceinline__ void aa_red_put(float* red, int wave, int lane, const f32x4& x) {
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(wave * 4 + r) * 64 + lane] = x[r];
}

// 16 rows of an f32 accumulator image [16][LDF] times v -> columns [col0, col0 + C) of d_a12 rows row0 .. (zeros: img == nullptr)
template <typename T>
__device__ __forceinline__ void aa_store_da(const float* img, int LDF, const float* vs, T* dst, long ld, int row0, int Tn, int C) {
    for (int i = threadIdx.x; i < 4 * C; i += 256) {
        const int row = i / (C >> 2), c = (i - row * (C >> 2)) * 4;
        if (row0 + row >= Tn) continue;
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (img) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(img + row * LDF + c), w = *reinterpret_cast<const f32x4*>(vs + c);
#pragma unroll
            for (int k = 0; k < 4; ++k) x[k] = a[k] * w[k];
        }
        frag_st<T>(dst + (long)(row0 + row) * ld + c, frag_from_acc<T>(x));
    }
}

// ---- forward -------------------------------------------------------------------------------------------------------------
template <typename T, int NTW>
__global__ __launch_bounds__(256) void aa_fwd_kernel(AaP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char aa_smem[];
    __shared__ uint32_t s_live[2];
    const int C = p.C, LDF = C + 4, CW = C >> 2, NCT = C >> 4;
    float* a1s = reinterpret_cast<float*>(aa_smem);          // [16][LDF] queries
    float* a2s = a1s + 16 * LDF;                             // [16][LDF] keys of the tile
    float* red = a2s + 16 * LDF;                             // [4 waves][4][64]
    float* vs = red + 1024;                                  // [C]
    float* kok = vs + C;                                     // [16] 1: a real key
    T* hT = reinterpret_cast<T*>(kok + 16);                  // [C][AA_LDT]
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15, wave = threadIdx.x >> 6;
    const int b = blockIdx.x / p.NT, qt = p.NT - 1 - blockIdx.x % p.NT, t0 = qt * 16;      // long walks first
    const int64_t* idr = p.ids + (long)b * p.T;
    const T* hb = reinterpret_cast<const T*>(p.h) + (long)b * p.T * C;
    const T* ab = reinterpret_cast<const T*>(p.a12) + (long)b * p.T * 2 * C;
    const uint64_t live = aa_live(idr, min(p.T, t0 + 16), s_live);
    for (int c = threadIdx.x; c < C; c += 256) vs[c] = p.v[c];
    aa_stage_scaled<T>(a1s, LDF, ab, 2L * C, t0, p.T, C);
    if (p.h_copy) {                                          // [h | out]: the concatenation NARM decodes, written here
        T* hc = reinterpret_cast<T*>(p.h_copy) + (long)b * p.T * p.ld_out;
        for (int i = threadIdx.x; i < 4 * C; i += 256) {
            const int row = i / CW, c = (i - row * CW) * 4;
            if (t0 + row < p.T) frag_st<T>(hc + (long)(t0 + row) * p.ld_out + c, frag_ld<T>(hb + (long)(t0 + row) * C + c));
        }
    }
    f32x4 acc[NTW];
#pragma unroll
    for (int i = 0; i < NTW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int t = t0 + l15;
    for (int kt = 0; kt <= qt; ++kt) {
        if (!((live >> kt) & 1ull)) continue;
        const int j0 = kt * 16;
        __syncthreads();
        aa_stage_scaled<T>(a2s, LDF, ab + C, 2L * C, j0, p.T, C);
        aa_stage_turned<T>(hT, hb, C, j0, p.T, C);
        if (threadIdx.x < 16) kok[threadIdx.x] = (j0 + threadIdx.x < p.T && idr[min(j0 + (int)threadIdx.x, p.T - 1)] != 0) ? 1.f : 0.f;
        __syncthreads();
        f32x4 e = {0.f, 0.f, 0.f, 0.f};
        const float* one = a1s + l15 * LDF;
        const float* four = a2s + g4 * LDF;
        for (int c = wave * CW; c < (wave + 1) * CW; c += 4) {
            const f32x4 x1 = *reinterpret_cast<const f32x4*>(one + c), w = *reinterpret_cast<const f32x4*>(vs + c);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f32x4 x2 = *reinterpret_cast<const f32x4*>(four + r * LDF + c);
#pragma unroll
                for (int k = 0; k < 4; ++k) e[r] = fmaf(w[k], aa_sig(x1[k] + x2[k]), e[r]);
            }
        }
        aa_red_put(red, wave, lane, e);
        __syncthreads();
        f32x4 al = aa_red_sum(red, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) al[r] = (j0 + g4 + r <= t && kok[g4 + r] != 0.f) ? al[r] : 0.f;
        const Frag4<T> bf = frag_from_acc<T>(al);
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const int ut = wave + 4 * i;
            if (ut < NCT) acc[i] = mma16(frag_ld<T>(hT + (ut * 16 + l15) * AA_LDT + g4), bf, acc[i]);
        }
    }
    if (t >= p.T) return;
    T* dst = reinterpret_cast<T*>(p.out) + ((long)b * p.T + t) * p.ld_out;
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const int ut = wave + 4 * i;
        if (ut < NCT) frag_st<T>(dst + ut * 16 + g4, frag_from_acc<T>(acc[i]));
    }
}

// ---- backward, query sweep: d_a1 and the workgroup's row of d_v --------------------------------------------------------------
template <typename T, int NTW>
__global__ __launch_bounds__(256) void aa_bwd_q_kernel(AaP p) {
    constexpr int VEC = 16 / (int)sizeof(T);
    extern __shared__ __attribute__((aligned(16))) unsigned char aa_smem[];
    __shared__ uint32_t s_live[2];
    const int C = p.C, LDF = C + 4, CW = C >> 2, NCT = C >> 4, LDR = C + VEC;
    float* a1s = reinterpret_cast<float*>(aa_smem);
    float* a2s = a1s + 16 * LDF;
    float* da1 = a2s + 16 * LDF;                             // [16][LDF] sum_j g s (1 - s)
    float* red = da1 + 16 * LDF;
    float* vs = red + 1024;
    float* dvs = vs + C;                                     // [C] sum g s
    float* kok = dvs + C;
    T* hR = reinterpret_cast<T*>(kok + 16);                  // [16][LDR] key rows
    const int lane = threadIdx.x & 63, g = lane >> 4, g4 = g * 4, l15 = lane & 15, wave = threadIdx.x >> 6;
    const int b = blockIdx.x / p.NT, qt = p.NT - 1 - blockIdx.x % p.NT, t0 = qt * 16;
    const int64_t* idr = p.ids + (long)b * p.T;
    const T* hb = reinterpret_cast<const T*>(p.h) + (long)b * p.T * C;
    const T* ab = reinterpret_cast<const T*>(p.a12) + (long)b * p.T * 2 * C;
    const uint64_t live = aa_live(idr, min(p.T, t0 + 16), s_live);
    for (int c = threadIdx.x; c < C; c += 256) { vs[c] = p.v[c]; dvs[c] = 0.f; }
    for (int i = threadIdx.x; i < 16 * LDF; i += 256) da1[i] = 0.f;
    aa_stage_scaled<T>(a1s, LDF, ab, 2L * C, t0, p.T, C);
    const int t = t0 + l15;
    const T* gr = reinterpret_cast<const T*>(p.d_out) + ((long)b * p.T + min(t, p.T - 1)) * p.ld_dout;
    Frag4<T> gf[NTW];                                        // dOut[t][16-channel slices wave, wave + 4, ...]
#pragma unroll
    for (int i = 0; i < NTW; ++i) gf[i] = (wave + 4 * i < NCT) ? frag_ld<T>(gr + (wave + 4 * i) * 16 + g4) : frag_zero<T>();
    for (int kt = 0; kt <= qt; ++kt) {
        if (!((live >> kt) & 1ull)) continue;
        const int j0 = kt * 16;
        __syncthreads();
        aa_stage_scaled<T>(a2s, LDF, ab + C, 2L * C, j0, p.T, C);
        aa_stage_rows<T>(hR, LDR, hb, C, j0, p.T, C);
        if (threadIdx.x < 16) kok[threadIdx.x] = (j0 + threadIdx.x < p.T && idr[min(j0 + (int)threadIdx.x, p.T - 1)] != 0) ? 1.f : 0.f;
        __syncthreads();
        f32x4 gp = {0.f, 0.f, 0.f, 0.f};                     // (h dOut^T)[key 4g + r][query i] over the wave's slices
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const int s = wave + 4 * i;
            if (s < NCT) gp = mma16(frag_ld<T>(hR + l15 * LDR + s * 16 + g4), gf[i], gp);
        }
        aa_red_put(red, wave, lane, gp);
        __syncthreads();
        f32x4 gg = aa_red_sum(red, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) gg[r] = (j0 + g4 + r <= t && t < p.T && kok[g4 + r] != 0.f) ? gg[r] : 0.f;
        const float* one = a1s + l15 * LDF;
        const float* four = a2s + g4 * LDF;
        for (int c = wave * CW; c < (wave + 1) * CW; c += 4) {
            const f32x4 x1 = *reinterpret_cast<const f32x4*>(one + c);
            float pa[4] = {0.f, 0.f, 0.f, 0.f}, pv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f32x4 x2 = *reinterpret_cast<const f32x4*>(four + r * LDF + c);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float s = aa_sig(x1[k] + x2[k]), gs = gg[r] * s;
                    pv[k] += gs;
                    pa[k] += fmaf(-gs, s, gs);
                }
            }
            const float ta = aa_group_reduce4(pa[0], pa[1], pa[2], pa[3]);
            const float tv = aa_row16_sum(aa_group_reduce4(pv[0], pv[1], pv[2], pv[3]));
            da1[l15 * LDF + c + g] += ta;                    // this lane is the only owner of the word
            if (l15 == 0) dvs[c + g] += tv;
        }
    }
    __syncthreads();
    aa_store_da<T>(da1, LDF, vs, reinterpret_cast<T*>(p.d_a12) + (long)b * p.T * 2 * C, 2L * C, t0, p.T, C);
    for (int c = threadIdx.x; c < C; c += 256) p.dv_part[(long)blockIdx.x * C + c] = dvs[c];
}

// ---- backward, key sweep: d_a2, d_h ------------------------------------------------------------------------------------------
template <typename T, int NTW>
__global__ __launch_bounds__(256) void aa_bwd_k_kernel(AaP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char aa_smem[];
    const int C = p.C, LDF = C + 4, CW = C >> 2, NCT = C >> 4;
    float* a2s = reinterpret_cast<float*>(aa_smem);          // [16][LDF] the tile's keys
    float* a1s = a2s + 16 * LDF;                             // [16][LDF] queries of the walked tile
    float* da2 = a1s + 16 * LDF;                             // [16][LDF] sum_t g s (1 - s)
    float* redg = da2 + 16 * LDF;
    float* rede = redg + 1024;
    float* vs = rede + 1024;
    float* kok = vs + C;
    T* gT = reinterpret_cast<T*>(kok + 16);                  // [C][AA_LDT] dOut turned
    const int lane = threadIdx.x & 63, g = lane >> 4, g4 = g * 4, l15 = lane & 15, wave = threadIdx.x >> 6;
    const int b = blockIdx.x / p.NT, kt = blockIdx.x % p.NT, j0 = kt * 16;                 // long walks first
    const int64_t* idr = p.ids + (long)b * p.T;
    const T* hb = reinterpret_cast<const T*>(p.h) + (long)b * p.T * C;
    const T* ab = reinterpret_cast<const T*>(p.a12) + (long)b * p.T * 2 * C;
    const T* gb = reinterpret_cast<const T*>(p.d_out) + (long)b * p.T * p.ld_dout;
    const T* rb = p.d_res ? reinterpret_cast<const T*>(p.d_res) + (long)b * p.T * p.ld_dout : nullptr;
    T* dab = reinterpret_cast<T*>(p.d_a12) + (long)b * p.T * 2 * C + C;
    T* dhb = reinterpret_cast<T*>(p.d_h) + (long)b * p.T * C;
    if (threadIdx.x < 16) kok[threadIdx.x] = (j0 + threadIdx.x < p.T && idr[min(j0 + (int)threadIdx.x, p.T - 1)] != 0) ? 1.f : 0.f;
    __syncthreads();
    bool any = false;
#pragma unroll
    for (int i = 0; i < 16; ++i) any = any || kok[i] != 0.f;
    if (!any) {                                              // a tile of padding: exact zeros (d_h: what else reaches h)
        aa_store_da<T>(nullptr, LDF, nullptr, dab, 2L * C, j0, p.T, C);
        for (int i = threadIdx.x; i < 4 * C; i += 256) {
            const int row = i / CW, c = (i - row * CW) * 4;
            if (j0 + row < p.T)
                frag_st<T>(dhb + (long)(j0 + row) * C + c, rb ? frag_ld<T>(rb + (long)(j0 + row) * p.ld_dout + c) : frag_zero<T>());
        }
        return;
    }
    for (int c = threadIdx.x; c < C; c += 256) vs[c] = p.v[c];
    for (int i = threadIdx.x; i < 16 * LDF; i += 256) da2[i] = 0.f;
    aa_stage_scaled<T>(a2s, LDF, ab + C, 2L * C, j0, p.T, C);
    const int j = j0 + l15;
    const bool jok = kok[l15] != 0.f;
    const T* hr = hb + (long)min(j, p.T - 1) * C;
    Frag4<T> hf[NTW];                                        // h[j][16-channel slices wave, wave + 4, ...]
    f32x4 acc[NTW];
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        hf[i] = (wave + 4 * i < NCT) ? frag_ld<T>(hr + (wave + 4 * i) * 16 + g4) : frag_zero<T>();
        acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int qt = kt; qt < p.NT; ++qt) {
        const int t0 = qt * 16;
        __syncthreads();
        aa_stage_scaled<T>(a1s, LDF, ab, 2L * C, t0, p.T, C);
        aa_stage_turned<T>(gT, gb, p.ld_dout, t0, p.T, C);
        __syncthreads();
        f32x4 gp = {0.f, 0.f, 0.f, 0.f};                     // (dOut h^T)[query 4g + r][key i] over the wave's slices
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const int s = wave + 4 * i;
            if (s < NCT) gp = mma16(aa_frag_strided<T>(gT + (s * 16 + g4) * AA_LDT + l15, AA_LDT), hf[i], gp);
        }
        aa_red_put(redg, wave, lane, gp);
        __syncthreads();
        f32x4 gg = aa_red_sum(redg, lane);
        bool ok[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ok[r] = jok && j <= t0 + g4 + r && t0 + g4 + r < p.T;
            gg[r] = ok[r] ? gg[r] : 0.f;
        }
        f32x4 e = {0.f, 0.f, 0.f, 0.f};
        const float* one = a2s + l15 * LDF;
        const float* four = a1s + g4 * LDF;
        for (int c = wave * CW; c < (wave + 1) * CW; c += 4) {
            const f32x4 x2 = *reinterpret_cast<const f32x4*>(one + c), w = *reinterpret_cast<const f32x4*>(vs + c);
            float pa[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f32x4 x1 = *reinterpret_cast<const f32x4*>(four + r * LDF + c);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float s = aa_sig(x1[k] + x2[k]), gs = gg[r] * s;
                    e[r] = fmaf(w[k], s, e[r]);
                    pa[k] += fmaf(-gs, s, gs);
                }
            }
            da2[l15 * LDF + c + g] += aa_group_reduce4(pa[0], pa[1], pa[2], pa[3]);      // this lane is the only owner of the word
        }
        aa_red_put(rede, wave, lane, e);
        __syncthreads();
        f32x4 al = aa_red_sum(rede, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) al[r] = ok[r] ? al[r] : 0.f;
        const Frag4<T> bf = frag_from_acc<T>(al);            // alpha[query 4g + r][key i]: the B operand as it stands
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const int ut = wave + 4 * i;
            if (ut < NCT) acc[i] = mma16(frag_ld<T>(gT + (ut * 16 + l15) * AA_LDT + g4), bf, acc[i]);
        }
    }
    __syncthreads();
    aa_store_da<T>(da2, LDF, vs, dab, 2L * C, j0, p.T, C);
    if (j >= p.T) return;
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const int ut = wave + 4 * i;
        if (ut >= NCT) continue;
        f32x4 o = acc[i];
        if (rb) {
            const Frag4<T> x = frag_ld<T>(rb + (long)j * p.ld_dout + ut * 16 + g4);
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] += to_f32(x.v[r]);
        }
        frag_st<T>(dhb + (long)j * C + ut * 16 + g4, frag_from_acc<T>(o));
    }
}

// d_v[c] = sum over the P partial rows, in a fixed order: eight interleaved slices, then the slices in order
__global__ __launch_bounds__(256) void aa_dv_finish_kernel(const float* part, int P, int C, float* d_v) {
    __shared__ float sm[8][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, c = blockIdx.x * 32 + tx;
    float s = 0.f;
    if (c < C)
        for (int r = ty; r < P; r += 8) s += part[(long)r * C + c];
    sm[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && c < C) {
        float tot = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) tot += sm[i][tx];
        d_v[c] = tot;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
int aa_check(const char* who, int B, int T, int C, int dtype) {
    EDGL_REQUIRE(B >= 1 && T >= 1 && T <= 1024, EDGL_ERR_SHAPE, "%s: bad shape B=%d T=%d (B >= 1, 1 <= T <= 1024)", who, B, T);
    EDGL_REQUIRE(C >= 16 && C <= 512 && C % 16 == 0, EDGL_ERR_SHAPE, "%s: C=%d unsupported (a multiple of 16 in [16, 512])", who, C);
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "%s: bad dtype %d", who, dtype);
    EDGL_REQUIRE((double)B * T * T < 4294967296.0, EDGL_ERR_SHAPE, "%s: B*T*T must be < 2^32 (B=%d T=%d)", who, B, T);
    return EDGL_OK;
}
int aa_check_ld(const char* who, const char* what, int ld, int C) {
    EDGL_REQUIRE(ld >= C && ld % 4 == 0, EDGL_ERR_SHAPE, "%s: row stride %s=%d must be a multiple of 4 and >= C=%d", who, what, ld, C);
    return EDGL_OK;
}

// dynamic LDS of kernel `which` (0: forward, 1: query sweep, 2: key sweep)
inline size_t aa_smem_bytes(int which, int C, size_t esz) {
    const size_t LDF = C + 4;
    if (which == 0) return (32 * LDF + 1024 + C + 16) * 4 + (size_t)C * AA_LDT * esz;
    if (which == 1) return (48 * LDF + 1024 + 2 * C + 16) * 4 + 16 * (C + 16 / esz) * esz;
    return (48 * LDF + 2048 + C + 16) * 4 + (size_t)C * AA_LDT * esz;
}

template <typename T, int NTW>
int aa_launch_one(const AaP& p, int which, hipStream_t st) {
    const dim3 grid((unsigned)((long)p.B * p.NT)), block(256);
    const size_t smem = aa_smem_bytes(which, p.C, sizeof(T));
    EDGL_REQUIRE(smem <= (size_t)AA_LDS, EDGL_ERR_SHAPE, "edgl_addattn: C=%d needs %zu bytes of LDS", p.C, smem);
    if (which == 0) {
        EDGL_LDS_LIMIT((aa_fwd_kernel<T, NTW>), smem, "edgl_addattn_fwd");
        hipLaunchKernelGGL((aa_fwd_kernel<T, NTW>), grid, block, smem, st, p);
    } else if (which == 1) {
        EDGL_LDS_LIMIT((aa_bwd_q_kernel<T, NTW>), smem, "edgl_addattn_bwd");
        hipLaunchKernelGGL((aa_bwd_q_kernel<T, NTW>), grid, block, smem, st, p);
    } else {
        EDGL_LDS_LIMIT((aa_bwd_k_kernel<T, NTW>), smem, "edgl_addattn_bwd");
        hipLaunchKernelGGL((aa_bwd_k_kernel<T, NTW>), grid, block, smem, st, p);
    }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
template <typename T>
int aa_launch(const AaP& p, int which, hipStream_t st) {
    const int ntw = (p.C / 16 + 3) / 4;       // 16-channel tiles a wave owns
    if (ntw <= 1) return aa_launch_one<T, 1>(p, which, st);
    if (ntw <= 2) return aa_launch_one<T, 2>(p, which, st);
    if (ntw <= 4) return aa_launch_one<T, 4>(p, which, st);
    return aa_launch_one<T, 8>(p, which, st);
}

}  // namespace

extern "C" long edgl_addattn_bwd_workspace(int B, int T, int C) {
    if (B < 1 || T < 1 || T > 1024 || C < 16 || C > 512 || C % 16 || (double)B * T * T >= 4294967296.0) return -1;
    return (long)B * ((T + 15) / 16) * C;
}

extern "C" int edgl_addattn_fwd(const void* h, const void* a12, const float* v, const int64_t* ids, int B, int T, int C, void* out,
                                int ld_out, void* h_copy, int dtype, void* stream) {
    EDGL_REQUIRE(h && a12 && v && ids && out, EDGL_ERR_NULL, "edgl_addattn_fwd: null pointer");
    if (int rc = aa_check("edgl_addattn_fwd", B, T, C, dtype)) return rc;
    if (int rc = aa_check_ld("edgl_addattn_fwd", "ld_out", ld_out, C)) return rc;
    AaP p{};
    p.h = h; p.a12 = a12; p.v = v; p.ids = ids; p.B = B; p.T = T; p.C = C; p.NT = (T + 15) / 16;
    p.out = out; p.h_copy = h_copy; p.ld_out = ld_out;
    return dtype == EDGL_F32 ? aa_launch<float>(p, 0, (hipStream_t)stream) : aa_launch<bf16>(p, 0, (hipStream_t)stream);
}

extern "C" int edgl_addattn_bwd(const void* h, const void* a12, const float* v, const int64_t* ids, const void* d_out, int ld_dout,
                                const void* d_res, int B, int T, int C, void* d_a12, void* d_h, float* d_v, float* workspace,
                                int dtype, void* stream) {
    EDGL_REQUIRE(h && a12 && v && ids && d_out && d_a12 && d_h && d_v && workspace, EDGL_ERR_NULL, "edgl_addattn_bwd: null pointer");
    if (int rc = aa_check("edgl_addattn_bwd", B, T, C, dtype)) return rc;
    if (int rc = aa_check_ld("edgl_addattn_bwd", "ld_dout", ld_dout, C)) return rc;
    AaP p{};
    p.h = h; p.a12 = a12; p.v = v; p.ids = ids; p.B = B; p.T = T; p.C = C; p.NT = (T + 15) / 16;
    p.d_out = d_out; p.d_res = d_res; p.ld_dout = ld_dout; p.d_a12 = d_a12; p.d_h = d_h; p.dv_part = workspace;
    hipStream_t st = (hipStream_t)stream;
    for (int which = 1; which <= 2; ++which)
        if (int rc = dtype == EDGL_F32 ? aa_launch<float>(p, which, st) : aa_launch<bf16>(p, which, st)) return rc;
    hipLaunchKernelGGL(aa_dv_finish_kernel, dim3((C + 31) / 32), dim3(256), 0, st, workspace, B * p.NT, C, d_v);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
