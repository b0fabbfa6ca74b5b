// Time-aware history encoder of TimelyREC (sequential.py:247-265) and the small op that forms its histories:
//   n = l2_normalize(R)      (x * rsqrt(max(sum x^2, 1e-12)))
//   hist[q] = sum_{k <= q} ((1 + n_q . n_k) / 2) Hs[k]                         edgl_tahe_fwd / edgl_tahe_bwd
//   Hs = (emb + te_weight * tcode) * (ids != 0)                                edgl_tahe_mix_fwd / edgl_tahe_mix_bwd
//
// One workgroup of four waves owns one sample.  G = R R^T is taken on the matrix pipe from the RAW rows, one 16x16 tile of the lower
// triangle per wave and step, contraction over all C in blocks of 16: both operands of a tile are row fragments (4 consecutive
// channels of one row per lane), read from global memory / L2 — no [T][C] image is staged in LDS, so the LDS need does not depend on
// C.  The scaling by the two inverse norms, the affine map (1 + S) / 2 and the causal mask (diagonal kept) are applied on the
// accumulator; the weights land in ONE f32 [Tp][Tp + 1] LDS image (Tp = T rounded up to 16).  The second product, W Hs, gives a wave
// one 16-channel column: it loads the column's Hs fragments of all key tiles once and walks the query tiles, contraction over the key
// tiles k <= q only.  The A fragments are converted from the f32 image on the fly (bf16 mode rounds a weight in [0, 1] to bf16).
//
// Backward: the same weights again, then dS = tril(dO Hs^T) / 2 on the matrix pipe into a second image; with M = dS + dS^T
//   dHs = W^T dO        dn = M n        dR_q = rn_q dn_q - rn_q^2 (n_q . dn_q) R_q,   n_q . dn_q = sum_k M[q][k] S[q][k]
// — the row dot comes from the two T x T images alone, so the channel tiles of dn need no exchange.  A row with sum x^2 < 1e-12 is on
// the other branch of the max: n = 1e6 x is linear there, dR_q = 1e6 dn_q (zero when the whole sample is zero), never NaN.
// LDS: (3 Tp + Tp (Tp + 1)) floats forward, (3 Tp + 2 Tp (Tp + 1)) backward: 133.6 KB at T = 128.  No atomics: one writer per element.
#include "edgl_common.h"

namespace {

constexpr int TAHE_NW = 4;
constexpr int TAHE_THREADS = TAHE_NW * 64;
constexpr int TAHE_MAXT = 128;
constexpr int TAHE_MAXNT = TAHE_MAXT / 16;
constexpr float TAHE_EPS = 1e-12f;

struct TaheP { const void* R; const void* Hs; const void* dO; int B, T, C; void* out; void* dR; void* dHs; };

__host__ __device__ inline int tahe_tp(int T) { return (T + 15) & ~15; }
inline size_t tahe_smem(int T, bool bwd) {
    const int Tp = tahe_tp(T);
    return ((size_t)3 * Tp + (size_t)(bwd ? 2 : 1) * Tp * (Tp + 1)) * sizeof(float);
}

// 4 consecutive channels of row `row` (zeros past the sequence)
template <typename T>
__device__ __forceinline__ Frag4<T> tahe_row_frag(const T* X, int row, int Tn, int C, int c) {
    return row < Tn ? frag_ld<T>(X + (long)row * C + c) : frag_zero<T>();
}
// B fragment of X[k][c] for the key tile kt: lane holds k = kt * 16 + (lane >> 4) * 4 + j, column c
template <typename T>
__device__ __forceinline__ Frag4<T> tahe_col_frag(const T* X, int kt, int Tn, int C, int c, int lane) {
    Frag4<T> f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = kt * 16 + (lane >> 4) * 4 + j;
        f.v[j] = k < Tn ? X[(long)k * C + c] : from_f32<T>(0.f);
    }
    return f;
}
// lower-triangle tile index -> (qi, ki), ki <= qi
__device__ __forceinline__ void tahe_tri(int t, int& qi, int& ki) {
    qi = 0;
    while ((qi + 1) * (qi + 2) / 2 <= t) ++qi;
    ki = t - qi * (qi + 1) / 2;
}

// ss[q] = sum x^2, rn[q] = rsqrt(max(ss, eps)) and the masked weights W[q][k] = (1 + n_q . n_k) / 2 for k <= q < Tn, else 0.
// The images were zero-filled by the caller; ends with a barrier.
template <typename T>
__device__ void tahe_weights(const T* R, int Tn, int Tp, int C, float* ss, float* rn, float* W) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, LD = Tp + 1;
    for (int q = wave; q < Tp; q += TAHE_NW) {
        float s = 0.f;
        if (q < Tn)
            for (int c = lane; c < C; c += 64) { const float x = to_f32(R[(long)q * C + c]); s = fmaf(x, x, s); }
        s = wave_sum(s);
        if (lane == 0) { ss[q] = s; rn[q] = q < Tn ? 1.0f / sqrtf(fmaxf(s, TAHE_EPS)) : 0.f; }
    }
    __syncthreads();
    const int nt = Tp >> 4, ntri = nt * (nt + 1) / 2, koff = (lane >> 4) * 4;
    for (int t = wave; t < ntri; t += TAHE_NW) {
        int qi, ki;
        tahe_tri(t, qi, ki);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int ra = qi * 16 + (lane & 15), rb = ki * 16 + (lane & 15);
        for (int c0 = 0; c0 < C; c0 += 16)
            acc = mma16(tahe_row_frag<T>(R, ra, Tn, C, c0 + koff), tahe_row_frag<T>(R, rb, Tn, C, c0 + koff), acc);
        const int k = ki * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = qi * 16 + koff + r;
            float w = 0.f;
            if (k <= q && q < Tn) {
                // the diagonal is n_q . n_q: exactly 1 on the normalised branch, ss * 1e12 on the clamped one
                const float s = k == q ? (ss[q] >= TAHE_EPS ? 1.0f : ss[q] * rn[q] * rn[q]) : acc[r] * rn[q] * rn[k];
                w = 0.5f * (1.0f + s);
            }
            W[q * LD + k] = w;
        }
    }
    __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(TAHE_THREADS) void tahe_fwd_kernel(TaheP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tahe_smem_raw[];
    const int Tn = p.T, C = p.C, Tp = tahe_tp(Tn), LD = Tp + 1, nt = Tp >> 4;
    float* ss = reinterpret_cast<float*>(tahe_smem_raw);
    float* rn = ss + Tp;
    float* W = rn + 2 * Tp;
    const long base = (long)blockIdx.x * Tn * C;
    const T* R = reinterpret_cast<const T*>(p.R) + base;
    const T* Hs = reinterpret_cast<const T*>(p.Hs) + base;
    T* out = reinterpret_cast<T*>(p.out) + base;
    for (int i = threadIdx.x; i < Tp * LD; i += TAHE_THREADS) W[i] = 0.f;
    __syncthreads();
    tahe_weights<T>(R, Tn, Tp, C, ss, rn, W);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, koff = (lane >> 4) * 4;
    for (int ci = wave; ci < (C >> 4); ci += TAHE_NW) {
        const int c = ci * 16 + (lane & 15);
        Frag4<T> bf[TAHE_MAXNT];
#pragma unroll
        for (int kt = 0; kt < TAHE_MAXNT; ++kt) bf[kt] = kt < nt ? tahe_col_frag<T>(Hs, kt, Tn, C, c, lane) : frag_zero<T>();
        for (int qi = 0; qi < nt; ++qi) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const float* wrow = W + (qi * 16 + (lane & 15)) * LD + koff;
#pragma unroll
            for (int kt = 0; kt < TAHE_MAXNT; ++kt) {
                if (kt <= qi) {
                    Frag4<T> a;
#pragma unroll
                    for (int j = 0; j < 4; ++j) a.v[j] = from_f32<T>(wrow[kt * 16 + j]);
                    acc = mma16(a, bf[kt], acc);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = qi * 16 + koff + r;
                if (q < Tn) out[(long)q * C + c] = from_f32<T>(acc[r]);
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(TAHE_THREADS) void tahe_bwd_kernel(TaheP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tahe_smem_raw[];
    const int Tn = p.T, C = p.C, Tp = tahe_tp(Tn), LD = Tp + 1, nt = Tp >> 4;
    float* ss = reinterpret_cast<float*>(tahe_smem_raw);
    float* rn = ss + Tp;
    float* dot = rn + Tp;
    float* W = dot + Tp;
    float* dS = W + Tp * LD;
    const long base = (long)blockIdx.x * Tn * C;
    const T* R = reinterpret_cast<const T*>(p.R) + base;
    const T* Hs = reinterpret_cast<const T*>(p.Hs) + base;
    const T* dO = reinterpret_cast<const T*>(p.dO) + base;
    T* dR = reinterpret_cast<T*>(p.dR) + base;
    T* dHs = reinterpret_cast<T*>(p.dHs) + base;
    for (int i = threadIdx.x; i < 2 * Tp * LD; i += TAHE_THREADS) W[i] = 0.f;      // (both images: they are adjacent)
    __syncthreads();
    tahe_weights<T>(R, Tn, Tp, C, ss, rn, W);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, koff = (lane >> 4) * 4;
    // dS[q][k] = (dO_q . Hs_k) / 2 on k <= q
    const int ntri = nt * (nt + 1) / 2;
    for (int t = wave; t < ntri; t += TAHE_NW) {
        int qi, ki;
        tahe_tri(t, qi, ki);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int ra = qi * 16 + (lane & 15), rb = ki * 16 + (lane & 15);
        for (int c0 = 0; c0 < C; c0 += 16)
            acc = mma16(tahe_row_frag<T>(dO, ra, Tn, C, c0 + koff), tahe_row_frag<T>(Hs, rb, Tn, C, c0 + koff), acc);
        const int k = ki * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = qi * 16 + koff + r;
            // the diagonal weight of a normalised row is the constant 1: its term 2 dS_qq n_q of dn is projected out exactly, so it
            // is dropped here instead of being left to cancel in rounded arithmetic; on the clamped branch it is a real gradient
            const bool live = k < q || (k == q && ss[q] < TAHE_EPS);
            dS[q * LD + k] = (live && q < Tn) ? 0.5f * acc[r] : 0.f;
        }
    }
    __syncthreads();
    // dot[q] = n_q . dn_q = sum_k M[q][k] S[q][k], S = 2 W - 1 read from the lower triangle
    for (int q = wave; q < Tp; q += TAHE_NW) {
        float s = 0.f;
        if (q < Tn)
            for (int k = lane; k < Tn; k += 64) {
                const float m = dS[q * LD + k] + dS[k * LD + q];
                const float w = k <= q ? W[q * LD + k] : W[k * LD + q];
                s = fmaf(m, 2.0f * w - 1.0f, s);
            }
        s = wave_sum(s);
        if (lane == 0) dot[q] = s;
    }
    __syncthreads();
    for (int ci = wave; ci < (C >> 4); ci += TAHE_NW) {
        const int c = ci * 16 + (lane & 15);
        Frag4<T> bf[TAHE_MAXNT];
        // dHs[k][c] = sum_{q >= k} W[q][k] dO[q][c]
#pragma unroll
        for (int qt = 0; qt < TAHE_MAXNT; ++qt) bf[qt] = qt < nt ? tahe_col_frag<T>(dO, qt, Tn, C, c, lane) : frag_zero<T>();
        for (int ki = 0; ki < nt; ++ki) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const int kcol = ki * 16 + (lane & 15);
#pragma unroll
            for (int qt = 0; qt < TAHE_MAXNT; ++qt) {
                if (qt >= ki && qt < nt) {
                    Frag4<T> a;      // A[row = k][kk = q] = W[q][k]
#pragma unroll
                    for (int j = 0; j < 4; ++j) a.v[j] = from_f32<T>(W[(qt * 16 + koff + j) * LD + kcol]);
                    acc = mma16(a, bf[qt], acc);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = ki * 16 + koff + r;
                if (k < Tn) dHs[(long)k * C + c] = from_f32<T>(acc[r]);
            }
        }
        // dn[q][c] = sum_k M[q][k] rn_k R[k][c];  dR = rn_q dn - rn_q^2 dot_q R_q (the second term on the normalised branch only)
#pragma unroll
        for (int kt = 0; kt < TAHE_MAXNT; ++kt) bf[kt] = kt < nt ? tahe_col_frag<T>(R, kt, Tn, C, c, lane) : frag_zero<T>();
        for (int qi = 0; qi < nt; ++qi) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const int qrow = qi * 16 + (lane & 15);
#pragma unroll
            for (int kt = 0; kt < TAHE_MAXNT; ++kt) {
                if (kt < nt) {
                    Frag4<T> a;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int k = kt * 16 + koff + j;
                        a.v[j] = from_f32<T>((dS[qrow * LD + k] + dS[k * LD + qrow]) * rn[k]);
                    }
                    acc = mma16(a, bf[kt], acc);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = qi * 16 + koff + r;
                if (q < Tn) {
                    float g = rn[q] * acc[r];
                    if (ss[q] >= TAHE_EPS) g -= rn[q] * rn[q] * dot[q] * to_f32(R[(long)q * C + c]);
                    dR[(long)q * C + c] = from_f32<T>(g);
                }
            }
        }
    }
}

// ---- Hs = (emb + te * tcode) * mask --------------------------------------------------------------------------------------
constexpr int MIX_ROWS = 64;       // rows of one workgroup of the backward: the partial sums of d_te are per workgroup

template <typename T>
__global__ __launch_bounds__(256) void tahe_mix_fwd_kernel(const T* emb, const T* tc, const float* te, const int64_t* ids, long rows,
                                                            int C, T* out) {
    const float w = te[0];
    const long n = rows * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long r = i / C;
        out[i] = from_f32<T>(ids[r] != 0 ? to_f32(emb[i]) + w * to_f32(tc[i]) : 0.f);
    }
}

// workgroup g owns rows [g * MIX_ROWS, ...): d_emb = d_out * mask; part[g] = sum of d_out * tcode over its unmasked rows
template <typename T>
__global__ __launch_bounds__(256) void tahe_mix_bwd_kernel(const T* d_out, const T* tc, const int64_t* ids, long rows, int C, T* d_emb,
                                                            float* part) {
    __shared__ float red[4];
    const long r0 = (long)blockIdx.x * MIX_ROWS;
    const long r1 = r0 + MIX_ROWS < rows ? r0 + MIX_ROWS : rows;
    float s = 0.f;
    for (long i = r0 * C + threadIdx.x; i < r1 * C; i += 256) {
        const bool on = ids[i / C] != 0;
        const float g = to_f32(d_out[i]);
        d_emb[i] = from_f32<T>(on ? g : 0.f);
        if (on) s = fmaf(g, to_f32(tc[i]), s);
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(64) void tahe_mix_sum_kernel(const float* part, int n, float* out) {
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) s += part[i];      // (a fixed order per lane, then a fixed tree)
    s = wave_sum(s);
    if (threadIdx.x == 0) out[0] = s;
}

// out [rows, 3C] = [a | b | c] (split = false) or the three blocks of `out` back into a, b, c (split = true)
template <typename T, bool SPLIT>
__global__ __launch_bounds__(256) void tahe_cat3_kernel(T* a, T* b, T* c, long rows, int C, T* out) {
    const long n = rows * 3 * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long r = i / (3 * C);
        const int j = (int)(i - r * 3 * C), blk = j / C;
        T* src = (blk == 0 ? a : blk == 1 ? b : c) + r * C + (j - blk * C);
        if (SPLIT) *src = out[i];
        else out[i] = *src;
    }
}

int tahe_check(const char* who, int B, int T, int C, int dtype) {
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "%s: bad dtype %d", who, dtype);
    EDGL_REQUIRE(B > 0 && T >= 1 && T <= TAHE_MAXT && C >= 32 && C <= 512 && (C & (C - 1)) == 0, EDGL_ERR_SHAPE,
                 "%s: bad shape B=%d T=%d C=%d (1 <= T <= %d, C a power of two in [32, 512])", who, B, T, C, TAHE_MAXT);
    return EDGL_OK;
}

}  // namespace

extern "C" int edgl_tahe_fwd(const void* R, const void* Hs, int B, int T, int C, void* hist, int dtype, void* stream) {
    EDGL_REQUIRE(R && Hs && hist, EDGL_ERR_NULL, "edgl_tahe_fwd: null pointer");
    const int rc = tahe_check("edgl_tahe_fwd", B, T, C, dtype);
    if (rc != EDGL_OK) return rc;
    const TaheP p{R, Hs, nullptr, B, T, C, hist, nullptr, nullptr};
    const size_t smem = tahe_smem(T, false);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == EDGL_F32) {
        EDGL_LDS_LIMIT(tahe_fwd_kernel<float>, smem, "edgl_tahe_fwd");
        hipLaunchKernelGGL((tahe_fwd_kernel<float>), dim3(B), dim3(TAHE_THREADS), smem, st, p);
    } else {
        EDGL_LDS_LIMIT(tahe_fwd_kernel<bf16>, smem, "edgl_tahe_fwd");
        hipLaunchKernelGGL((tahe_fwd_kernel<bf16>), dim3(B), dim3(TAHE_THREADS), smem, st, p);
    }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_tahe_bwd(const void* R, const void* Hs, const void* d_hist, int B, int T, int C, void* d_R, void* d_Hs, int dtype,
                             void* stream) {
    EDGL_REQUIRE(R && Hs && d_hist && d_R && d_Hs, EDGL_ERR_NULL, "edgl_tahe_bwd: null pointer");
    const int rc = tahe_check("edgl_tahe_bwd", B, T, C, dtype);
    if (rc != EDGL_OK) return rc;
    const TaheP p{R, Hs, d_hist, B, T, C, nullptr, d_R, d_Hs};
    const size_t smem = tahe_smem(T, true);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == EDGL_F32) {
        EDGL_LDS_LIMIT(tahe_bwd_kernel<float>, smem, "edgl_tahe_bwd");
        hipLaunchKernelGGL((tahe_bwd_kernel<float>), dim3(B), dim3(TAHE_THREADS), smem, st, p);
    } else {
        EDGL_LDS_LIMIT(tahe_bwd_kernel<bf16>, smem, "edgl_tahe_bwd");
        hipLaunchKernelGGL((tahe_bwd_kernel<bf16>), dim3(B), dim3(TAHE_THREADS), smem, st, p);
    }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_tahe_mix_fwd(const void* emb, const void* tcode, const float* te_weight, const int64_t* ids, long rows, int C,
                                 void* out, int dtype, void* stream) {
    EDGL_REQUIRE(emb && tcode && te_weight && ids && out, EDGL_ERR_NULL, "edgl_tahe_mix_fwd: null pointer");
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_tahe_mix_fwd: bad dtype %d", dtype);
    EDGL_REQUIRE(rows > 0 && C > 0 && rows <= 2147483647L / C, EDGL_ERR_SHAPE, "edgl_tahe_mix_fwd: bad shape rows=%ld C=%d", rows, C);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(grid_for(rows * C));
    if (dtype == EDGL_F32)
        hipLaunchKernelGGL((tahe_mix_fwd_kernel<float>), grid, dim3(256), 0, st, (const float*)emb, (const float*)tcode, te_weight, ids, rows, C, (float*)out);
    else
        hipLaunchKernelGGL((tahe_mix_fwd_kernel<bf16>), grid, dim3(256), 0, st, (const bf16*)emb, (const bf16*)tcode, te_weight, ids, rows, C, (bf16*)out);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_cat3(void* a, void* b, void* c, long rows, int C, void* cat, int split, int dtype, void* stream) {
    EDGL_REQUIRE(a && b && c && cat, EDGL_ERR_NULL, "edgl_cat3: null pointer");
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_cat3: bad dtype %d", dtype);
    EDGL_REQUIRE(rows > 0 && C > 0, EDGL_ERR_SHAPE, "edgl_cat3: bad shape rows=%ld C=%d", rows, C);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(grid_for(rows * 3 * C));
    if (dtype == EDGL_F32) {
        if (split) hipLaunchKernelGGL((tahe_cat3_kernel<float, true>), grid, dim3(256), 0, st, (float*)a, (float*)b, (float*)c, rows, C, (float*)cat);
        else hipLaunchKernelGGL((tahe_cat3_kernel<float, false>), grid, dim3(256), 0, st, (float*)a, (float*)b, (float*)c, rows, C, (float*)cat);
    } else {
        if (split) hipLaunchKernelGGL((tahe_cat3_kernel<bf16, true>), grid, dim3(256), 0, st, (bf16*)a, (bf16*)b, (bf16*)c, rows, C, (bf16*)cat);
        else hipLaunchKernelGGL((tahe_cat3_kernel<bf16, false>), grid, dim3(256), 0, st, (bf16*)a, (bf16*)b, (bf16*)c, rows, C, (bf16*)cat);
    }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" long edgl_tahe_mix_bwd_workspace(long rows) { return rows > 0 ? (rows + MIX_ROWS - 1) / MIX_ROWS : -1; }

extern "C" int edgl_tahe_mix_bwd(const void* d_out, const void* tcode, const int64_t* ids, long rows, int C, void* d_emb, float* d_te,
                                 float* workspace, int dtype, void* stream) {
    EDGL_REQUIRE(d_out && tcode && ids && d_emb && d_te && workspace, EDGL_ERR_NULL, "edgl_tahe_mix_bwd: null pointer");
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_tahe_mix_bwd: bad dtype %d", dtype);
    EDGL_REQUIRE(rows > 0 && C > 0 && rows <= 2147483647L / C, EDGL_ERR_SHAPE, "edgl_tahe_mix_bwd: bad shape rows=%ld C=%d", rows, C);
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)edgl_tahe_mix_bwd_workspace(rows);
    if (dtype == EDGL_F32)
        hipLaunchKernelGGL((tahe_mix_bwd_kernel<float>), dim3(nb), dim3(256), 0, st, (const float*)d_out, (const float*)tcode, ids, rows, C, (float*)d_emb, workspace);
    else
        hipLaunchKernelGGL((tahe_mix_bwd_kernel<bf16>), dim3(nb), dim3(256), 0, st, (const bf16*)d_out, (const bf16*)tcode, ids, rows, C, (bf16*)d_emb, workspace);
    hipLaunchKernelGGL(tahe_mix_sum_kernel, dim3(1), dim3(64), 0, st, workspace, nb, d_te);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
