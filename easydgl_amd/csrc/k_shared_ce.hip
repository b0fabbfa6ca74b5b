// K5d: sampled-softmax training with ONE negative list per step.  The per-row definition of k_cand_ce.hip with
// cand[r, :] = shared[:] for every row r, which turns R (N + 1) gathered dot products into dense products on the matrix pipe.
//
//   slots of row r : the label y = labels[r] (kept apart: label_val), then slot s = shared[s], 0 <= s < S
//   v(r, s)        = rows[r] . table_c[shared[s]] + bias_used[shared[s]];  item 0 is the zero row with bias -1000
//   a slot is DEAD for row r (-inf; no part in loss or gradient) when shared[s] < 0, shared[s] >= I or shared[s] == y
//   lse[r]         = log sum exp over the label and the live slots;  loss and coef[r] come from edgl_ce_loss_fwd(lse, label_val)
//   dv(r, s)       = g coef[r] exp(v - lse);   dv_label(r) = g coef[r] (exp(label_val - lse) - 1)
//   d_rows[r]      = sum_s dv table_c[shared[s]] + dv_label table_c[y]
//   d_table[c]    += sum over the slots / labels that name c of dv rows[r]  (row 0 stays zero);   d_bias[c - 1] += sum dv
// Uniform negatives over [1, hi): the log-Q term of sampled softmax is one constant for every slot and cancels.  A weighted sampler
//  hands logq [I] to edgl_shared_ce_fwd_q: the label and every live slot read v - logq[c], one f32 subtraction on the
// finished value (logq = 0 or NULL: the bits above); the backward forms dv from the saved vals / label_val / lse and is unchanged.
//
//   shared_label_kernel   label_val[r]: one gathered dot product per row, cand_gather.h's rule (the bits of k_cand_ce.hip's slot 0).
//   shared_ce_fwd_kernel  a workgroup owns 128 rows and walks the list in tiles of 128 slots.  Per tile the contraction over C runs
//                         on MFMA (gemm_tile.h's LDS image: [row][k], 16-byte padded rows, one ds_read_b128 per fragment); the
//                         table operand is GATHERED into that image — LDS row n holds table_c[shared[s0 + n]], read as 16-byte
//                         vectors of one contiguous table row; a dead id or item 0 stages zeros — so a listed table row is read
//                         once per row tile and no [R, S, C] gather exists.  Wave w owns rows 32 w .. 32 w + 31 against all 128
//                         slots.  Epilogue: + bias_used, the per-row hit mask, vals [R, S], and an online (max, sum) per row.
//                         Reduction order, a function of (dtype, C, S) alone: the k-blocks of a value in ascending order inside the
//                         MFMA chain; a lane joins its slots in ascending order over all tiles; the four lane groups of a row are
//                         joined by a fixed xor butterfly (both partners form the same sum); the label joins last.  No atomics: a
//                         row's outputs depend on neither R nor the other rows.
//   shared_dv_kernel      dv in the compute dtype as [R, Sp] (Sp = S rounded up to 8, pad columns zero) and dv_label (f32, stride 2).
//   shared_rows_kernel    W_S [Sp, C]: the listed table rows once (zeros for dead ids, item 0 and the pad rows).
//   the two products      d_rows = dv W_S and the slab dW_S [Sp, C] = dv^T rows run through the library's dense MFMA GEMMs
//                         (edgl_gemm, edgl_gemm_dw: fixed row splits reduced in order, no atomics); the bias sums are edgl_colsum(dv).
//   shared_finish_kernel  d_rows[r] += dv_label table_c[y] (one wave per row, no atomics) and, in the atomic mode, the label term of
//                         the table gradient: one wave-instruction adds 64 contiguous floats (256 bytes) of table row y.
//   shared_scatter_kernel slab row s and bias sum s into d_table[shared[s]] / d_bias.  Atomic mode: f32 atomics.  Deterministic mode:
//                         the FIRST slot of an id sums the slab rows of its repeats in slot order and is the only writer of the row.
//   deterministic label term: an ordered sum over a k_segsum.hip plan of the labels (edgl_segsum_cand with two entries per row:
//                         the label with dv_label, and a dropped key 0).
// Rows of weight 0 (label outside [1, I), or at / past nvalid[0] of a compacted batch): vals -inf, label_val = lse = 0, d_rows zero.
//
// Other objectives over the same slots (sampled_dv.h): the forward is unchanged (its lse is not used), the row losses come
// from k_sampled_loss.hip and shared_dv_kernel<T, FORM> forms dv and dv_label by the form's rule; everything behind dv is the code
// above.  FORM = softmax is today's kernel, bit for bit.
#include "cand_gather.h"
#include "gemm_tile.h"
#include "sampled_dv.h"

namespace sce {

using candg::RowRegs; using candg::load_pieces; using candg::unpack; using candg::cand_value; using candg::group_of;

constexpr int MAX_S = 8192;
constexpr int TS = 128;                       // slots of a tile

struct P {
    const void* rows; const void* table; const float* bias; const int32_t* shared; const int64_t* labels; const int32_t* nvalid;
    const float* logq;                                               // forward only: [I] or NULL
    int R, C, I, S, Sp;
    float* vals; float* label_val; float* lse;                       // forward: outputs; backward: inputs
    const float* coef; const float* gscale;
    void* d_rows; void* dvt; void* ws_rows; float* dvl; float* slab; float* bsum; float* d_table; float* d_bias;
    int64_t* keys; int det;
};

__device__ __forceinline__ int nlive_of(const P& p) { return p.nvalid ? min(p.R, max(p.nvalid[0], 0)) : p.R; }

// (m, s) <- (m, s) joined with (m2, s2): running maximum and sum of exp(v - m); (-inf, 0) is the empty set
__device__ __forceinline__ void lse_join(float& m, float& s, float m2, float s2) {
    const float M = fmaxf(m, m2);
    s = M == -INFINITY ? 0.0f : s * __expf(m - M) + s2 * __expf(m2 - M);
    m = M;
}

template <typename T, int G, int PPL>
__global__ __launch_bounds__(256) void shared_label_kernel(P p) {
    const int tid = threadIdx.x, gl = tid % G;
    const int r = blockIdx.x * (256 / G) + tid / G;
    const int rr = min(r, p.R - 1);                                   // (every lane takes part in the butterfly)
    const int64_t y64 = p.labels[rr];
    const bool live = r < nlive_of(p) && y64 >= 1 && y64 < p.I;
    const int y = live ? (int)y64 : 1;                                // (I > 1: row 1 exists)
    RowRegs<T, PPL> xq;
    uint4 w[PPL];
    load_pieces<T, G, PPL>(reinterpret_cast<const T*>(p.rows), rr, p.C, gl, w);
#pragma unroll
    for (int pp = 0; pp < PPL; ++pp) unpack<T>(w[pp], gl + pp * 64 < p.C / (int)(16 / sizeof(T)), xq.x[pp]);
    load_pieces<T, G, PPL>(reinterpret_cast<const T*>(p.table), y, p.C, gl, w);
    float v = cand_value<T, G, PPL>(xq, w, y, p.bias[y - 1], p.C, gl);
    if (p.logq) v -= p.logq[y];                                       // (grid-uniform) the label's log-Q term
    if (r < p.R && gl == 0) p.label_val[r] = live ? v : 0.0f;
}

// Q: the per-slot log-Q term rides with the staged bias (slq) and is subtracted from the finished value; Q = false is the
// kernel without it (the two __global__ wrappers follow the body)
template <typename T, bool Q>
__device__ __forceinline__ void shared_ce_fwd_body(const P& p) {
    constexpr int VEC = ElemTraits<T>::VEC, KB = ElemTraits<T>::KB, BK = 2 * KB, LDK = BK + VEC, KV = BK / VEC;
    __shared__ __attribute__((aligned(16))) T As[128 * LDK];
    __shared__ __attribute__((aligned(16))) T Bs[TS * LDK];
    __shared__ int sid[TS];
    __shared__ float sbias[TS];
    __shared__ float slq[Q ? TS : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lm = lane & 15, lq = lane >> 4;
    const int row0 = blockIdx.x * 128, R = p.R, S = p.S, C = p.C;
    const int nlive = nlive_of(p);
    if (row0 >= nlive) {                                              // (block-uniform) a tile of weight-0 rows
        const int nr = min(128, R - row0);
        float* v0 = p.vals + (long)row0 * S;
        for (long e = tid; e < (long)nr * S; e += 256) v0[e] = -INFINITY;
        if (tid < nr) p.lse[row0 + tid] = 0.0f;
        return;
    }
    const T* rows = reinterpret_cast<const T*>(p.rows);
    const T* table = reinterpret_cast<const T*>(p.table);
    int y[2], grow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        grow[i] = row0 + wave * 32 + i * 16 + lm;
        const int64_t y64 = grow[i] < nlive ? p.labels[grow[i]] : 0;
        y[i] = (y64 >= 1 && y64 < p.I) ? (int)y64 : 0;                // 0: weight 0, every slot dead
    }
    float m[2] = {-INFINITY, -INFINITY}, s[2] = {0.0f, 0.0f};
    const int nk = (C + BK - 1) / BK;
    const bool vec4 = (S & 3) == 0;
    Vec16<T> ra[4], rb[4];
    auto load_tiles = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = tid + i * 256, row = v / KV, gk = k0 + (v % KV) * VEC;      // (C % VEC == 0: a vector is inside the row or past it)
            const int gr = row0 + row, c = sid[row];
            ra[i] = (gr < R && gk < C) ? ld16<T>(rows + (long)gr * C + gk) : zero16<T>();
            rb[i] = (c > 0 && gk < C) ? ld16<T>(table + (long)c * C + gk) : zero16<T>();
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = tid + i * 256, row = v / KV, kv = v % KV;
            st16<T>(As + row * LDK + kv * VEC, ra[i]);
            st16<T>(Bs + row * LDK + kv * VEC, rb[i]);
        }
    };
    for (int s0 = 0; s0 < S; s0 += TS) {                              // (block-uniform)
        __syncthreads();                                              // the previous tile's epilogue has read sid / sbias
        if (tid < TS) {
            const int c = s0 + tid < S ? p.shared[s0 + tid] : -1;
            const bool ok = c >= 0 && c < p.I;
            sid[tid] = ok ? c : -1;
            sbias[tid] = ok ? (c == 0 ? -1000.0f : p.bias[c - 1]) : -INFINITY;
            if constexpr (Q) slq[tid] = ok ? p.logq[c] : 0.0f;
        }
        __syncthreads();
        f32x4 acc[8][2];
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        load_tiles(0);
        store_tiles();
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const bool more = kt + 1 < nk;
            if (more) load_tiles((kt + 1) * BK);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const int koff = kb * KB + lq * VEC;
                Vec16<T> af[2], bf[8];
#pragma unroll
                for (int i = 0; i < 2; ++i) af[i] = ld16<T>(As + (wave * 32 + i * 16 + lm) * LDK + koff);
#pragma unroll
                for (int j = 0; j < 8; ++j) bf[j] = ld16<T>(Bs + (j * 16 + lm) * LDK + koff);
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int i = 0; i < 2; ++i) acc[j][i] = mma_kblock(bf[j], af[i], acc[j][i]);
            }
            __syncthreads();
            if (more) store_tiles();
            __syncthreads();
        }
        // lane holds, for tile (j, i): slots n = j * 16 + lq * 4 + r (rows of D), row grow[i] (column lm of D)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int n = j * 16 + lq * 4;
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = sid[n + r];
                    const bool live = c >= 0 && y[i] > 0 && c != y[i];
                    if constexpr (Q) v[r] = live ? (acc[j][i][r] + sbias[n + r]) - slq[n + r] : -INFINITY;
                    else v[r] = live ? acc[j][i][r] + sbias[n + r] : -INFINITY;
                    if (live) {                                       // this lane's slots in ascending order
                        if (v[r] > m[i]) { s[i] = s[i] * __expf(m[i] - v[r]) + 1.0f; m[i] = v[r]; }
                        else s[i] += __expf(v[r] - m[i]);
                    }
                }
                if (grow[i] < R) {
                    float* dst = p.vals + (long)grow[i] * S + s0 + n;
                    if (vec4 && s0 + n + 3 < S) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                    else {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (s0 + n + r < S) dst[r] = v[r];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) {                           // the four lane groups that share the row
            const float m2 = __shfl_xor(m[i], o, 64), s2 = __shfl_xor(s[i], o, 64);
            lse_join(m[i], s[i], m2, s2);
        }
        if (lq == 0 && grow[i] < R) {
            float L = 0.0f;
            if (y[i] > 0) {
                float M = p.label_val[grow[i]], Z = 1.0f;
                lse_join(M, Z, m[i], s[i]);
                L = M + logf(Z);
            }
            p.lse[grow[i]] = L;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void shared_ce_fwd_kernel(P p) { shared_ce_fwd_body<T, false>(p); }

// With the term, two waves per SIMD are asked for: the bf16 form sits at the 256-register edge of that occupancy and the extra
// LDS operand would otherwise halve it (measured: the forward 0.13 -> 0.23 ms at 50 k rows x 1024 slots).
template <typename T>
__global__ __launch_bounds__(256, 2) void shared_ce_fwd_q_kernel(P p) { shared_ce_fwd_body<T, true>(p); }

template <typename T>
__device__ __forceinline__ void store_quad(T* dst, const float (&x)[4]) {
    Frag4<T> f;
#pragma unroll
    for (int r = 0; r < 4; ++r) f.v[r] = from_f32<T>(x[r]);
    if constexpr (sizeof(T) == 4) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<uint4*>(&f);
    else *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<uint2*>(&f);
}

// dvt [R, Sp] (compute dtype), dvl[2 r] = dv_label, dvl[2 r + 1] = 0, keys[2 r] = the label of a weighted row (else 0), keys[2 r + 1] = 0
// FORM: the objective whose dv is formed (sampled_dv.h); L is lse[r] (softmax) or the row auxiliary of another form.
// The pad columns s >= S and the dead slots are written as zeros whatever the form.
template <typename T, int FORM>
__global__ __launch_bounds__(256) void shared_dv_kernel(P p) {
    const int q4 = p.Sp >> 2, nlive = nlive_of(p);
    const long n = (long)p.R * q4;
    const float g = p.gscale ? p.gscale[0] : 1.0f;
    T* dvt = reinterpret_cast<T*>(p.dvt);
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const int r = (int)(e / q4), s = (int)(e % q4) * 4;
        const int64_t y = p.labels[r];
        const bool w = r < nlive && y >= 1 && y < p.I;
        const float gc = w ? g * p.coef[r] : 0.0f, L = p.lse[r];
        const float v0 = FORM == sdv::BPR ? p.label_val[r] : 0.0f;
        float d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float v = (w && s + k < p.S) ? p.vals[(long)r * p.S + s + k] : -INFINITY;
            d[k] = v > -INFINITY ? sdv::dv_slot<FORM>(gc, v, v0, L) : 0.0f;       // (the forward's test: dead slots read -inf)
        }
        store_quad<T>(dvt + (long)r * p.Sp + s, d);
        if (s == 0) {
            *reinterpret_cast<float2*>(p.dvl + 2L * r) = make_float2(w ? sdv::dv_label<FORM>(gc, p.label_val[r], L) : 0.0f, 0.0f);
            if (p.keys) { p.keys[2L * r] = w ? y : 0; p.keys[2L * r + 1] = 0; }
        }
    }
}

// W_S [Sp, C]: table_c[shared[s]]; zeros for a dead id, item 0 and the pad rows
template <typename T>
__global__ __launch_bounds__(256) void shared_rows_kernel(P p) {
    constexpr int VEC = ElemTraits<T>::VEC;
    const int np = p.C / VEC;
    const long n = (long)p.Sp * np;
    const T* table = reinterpret_cast<const T*>(p.table);
    T* out = reinterpret_cast<T*>(p.ws_rows);
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const int s = (int)(e / np), k = (int)(e % np) * VEC;
        const int c = s < p.S ? p.shared[s] : -1;
        st16<T>(out + (long)s * p.C + k, (c > 0 && c < p.I) ? ld16<T>(table + (long)c * p.C + k) : zero16<T>());
    }
}

// one wave per row: d_rows[r] += dv_label table_c[y]; atomic mode: d_table[y] += dv_label rows[r], d_bias[y - 1] += dv_label
template <typename T>
__global__ __launch_bounds__(256) void shared_finish_kernel(P p) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= p.R) return;                                             // (wave-uniform)
    const int64_t y = p.labels[r];
    T* drow = reinterpret_cast<T*>(p.d_rows) + (long)r * p.C;
    if (!(r < nlive_of(p) && y >= 1 && y < p.I)) {                    // weight 0
        for (int c = lane; c < p.C; c += 64) drow[c] = from_f32<T>(0.0f);
        return;
    }
    const float dl = p.dvl[2L * r];
    const T* trow = reinterpret_cast<const T*>(p.table) + y * p.C;
    const T* xrow = reinterpret_cast<const T*>(p.rows) + (long)r * p.C;
    float* dst = p.d_table + y * p.C;
    for (int c = lane; c < p.C; c += 64) {
        drow[c] = from_f32<T>(fmaf(dl, to_f32(trow[c]), to_f32(drow[c])));
        if (!p.det) atomicAdd(dst + c, dl * to_f32(xrow[c]));
    }
    if (!p.det && lane == 0) atomicAdd(p.d_bias + y - 1, dl);
}

// one workgroup per list slot
__global__ __launch_bounds__(256) void shared_scatter_kernel(P p) {
    const int s = blockIdx.x, tid = threadIdx.x, C = p.C;
    const int c = p.shared[s];
    if (c < 1 || c >= p.I) return;                                    // (block-uniform) dead id, or item 0: no parameter
    float* dst = p.d_table + (long)c * C;
    if (!p.det) {
        for (int k = tid; k < C; k += 256) atomicAdd(dst + k, p.slab[(long)s * C + k]);
        if (tid == 0) atomicAdd(p.d_bias + c - 1, p.bsum[s]);
        return;
    }
    int before = 0, after = 0;
    for (int t = tid; t < p.S; t += 256) {
        const bool hit = p.shared[t] == c;
        before |= hit && t < s;
        after |= hit && t > s;
    }
    if (__syncthreads_or(before)) return;                             // (block-uniform) an earlier slot owns the id
    const int rep = __syncthreads_or(after);
    float a0 = 0.0f, a1 = 0.0f, ab = 0.0f;                            // C <= 512: two columns per thread
    const int k0 = tid, k1 = tid + 256;
    const int last = rep ? p.S : s + 1;
    for (int t = s; t < last; ++t) {                                  // the repeats of the id, in slot order
        if (p.shared[t] != c) continue;
        if (k0 < C) a0 += p.slab[(long)t * C + k0];
        if (k1 < C) a1 += p.slab[(long)t * C + k1];
        ab += p.bsum[t];
    }
    if (k0 < C) dst[k0] += a0;
    if (k1 < C) dst[k1] += a1;
    if (tid == 0) p.d_bias[c - 1] += ab;
}

template <typename T, int G, int PPL>
int launch_label(const P& p, hipStream_t st) {
    hipLaunchKernelGGL((shared_label_kernel<T, G, PPL>), dim3((unsigned)edgl_cdiv(p.R, 256 / G)), dim3(256), 0, st, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

template <typename T>
int forward(const P& p, hipStream_t st) {
    const int pieces = p.C / (int)(16 / sizeof(T));
    int rc;
    if (sizeof(T) == 4 && pieces > 64) rc = launch_label<T, 64, 2>(p, st);
    else switch (group_of(pieces)) {
        case 2: rc = launch_label<T, 2, 1>(p, st); break;
        case 4: rc = launch_label<T, 4, 1>(p, st); break;
        case 8: rc = launch_label<T, 8, 1>(p, st); break;
        case 16: rc = launch_label<T, 16, 1>(p, st); break;
        case 32: rc = launch_label<T, 32, 1>(p, st); break;
        default: rc = launch_label<T, 64, 1>(p, st); break;
    }
    if (rc) return rc;
    if (p.logq) hipLaunchKernelGGL((shared_ce_fwd_q_kernel<T>), dim3((unsigned)edgl_cdiv(p.R, 128)), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((shared_ce_fwd_kernel<T>), dim3((unsigned)edgl_cdiv(p.R, 128)), dim3(256), 0, st, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

inline int pad8(int S) { return (S + 7) / 8 * 8; }
inline long up4(long n) { return (n + 3) / 4 * 4; }                   // (every part of the workspace starts on 16 bytes)

// workspace (floats): dvt | W_S | slab | bsum | dvl | the library's own workspaces
struct Layout { long dvt, rows, slab, bsum, dvl, lib, total; };
inline Layout layout(int R, int C, int S, int dtype) {
    const long Sp = pad8(S), es = dtype == EDGL_BF16 ? 2 : 4;
    Layout L;
    L.dvt = 0;
    L.rows = L.dvt + up4(((long)R * Sp * es + 3) / 4);
    L.slab = L.rows + up4((Sp * C * es + 3) / 4);
    L.bsum = L.slab + up4(Sp * C);
    L.dvl = L.bsum + up4(Sp);
    L.lib = L.dvl + up4(2L * R);
    L.total = L.lib + std::max(edgl_gemm_dw_workspace(R, (int)Sp, C, dtype), 256L * Sp);
    return L;
}

template <typename T>
int backward(P p, float* ws, void* plan, int form, int dtype, hipStream_t st) {
    const Layout L = layout(p.R, p.C, p.S, dtype);
    p.dvt = ws + L.dvt; p.ws_rows = ws + L.rows; p.slab = ws + L.slab; p.bsum = ws + L.bsum; p.dvl = ws + L.dvl;
    float* libws = ws + L.lib;
    const dim3 dvgrid((unsigned)grid_for((long)p.R * (p.Sp / 4)));
    if (form == sdv::BCE) hipLaunchKernelGGL((shared_dv_kernel<T, sdv::BCE>), dvgrid, dim3(256), 0, st, p);
    else if (form == sdv::BPR) hipLaunchKernelGGL((shared_dv_kernel<T, sdv::BPR>), dvgrid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((shared_dv_kernel<T, sdv::SOFTMAX>), dvgrid, dim3(256), 0, st, p);
    hipLaunchKernelGGL((shared_rows_kernel<T>), dim3((unsigned)grid_for((long)p.Sp * p.C / 4)), dim3(256), 0, st, p);
    EDGL_LAUNCH_CHECK();
    // d_rows [R, C] = dv [R, Sp] W_S [Sp, C]
    int rc = edgl_gemm(p.dvt, p.ws_rows, p.d_rows, p.R, p.C, p.Sp, p.Sp, p.C, p.C, 1, 0, nullptr, nullptr, 0, 1, nullptr, dtype, st);
    if (rc) return rc;
    // the slab dW_S [Sp, C] = dv^T rows and the bias sums colsum(dv)
    rc = edgl_gemm_dw(p.dvt, p.rows, p.slab, nullptr, p.R, p.Sp, p.C, p.Sp, p.C, 0, libws, dtype, st);
    if (rc) return rc;
    rc = edgl_colsum(p.dvt, p.R, p.Sp, p.Sp, p.bsum, 0, libws, 0, dtype, st);
    if (rc) return rc;
    hipLaunchKernelGGL((shared_finish_kernel<T>), dim3((unsigned)edgl_cdiv(p.R, 4)), dim3(256), 0, st, p);
    EDGL_LAUNCH_CHECK();
    if (p.det) {
        rc = edgl_segsum_cand(p.rows, p.keys, p.dvl, 2L * p.R, 2, p.C, p.I, p.d_table, p.d_bias, plan, dtype, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(shared_scatter_kernel, dim3((unsigned)p.S), dim3(256), 0, st, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

// the shape rule of the entry points
int check_shape(const char* who, int R, int C, int I, int S, int dtype) {
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "%s: dtype %d (f32 = 0 or bf16 = 1)", who, dtype);
    const int vec = dtype == EDGL_BF16 ? 8 : 4;
    EDGL_REQUIRE(C >= 16 && C <= 512 && C % vec == 0, EDGL_ERR_SHAPE, "%s: C=%d (16 <= C <= 512, a multiple of %d for %s)", who, C, vec,
                 dtype == EDGL_BF16 ? "bf16" : "f32");
    EDGL_REQUIRE(R >= 1 && S >= 1 && S <= MAX_S && I > 1 && (long)R * ((long)S + 8) < (1L << 31), EDGL_ERR_SHAPE,
                 "%s: R=%d S=%d I=%d (R >= 1, 1 <= S <= %d, I > 1, R (S + 8) < 2^31)", who, R, S, I, MAX_S);
    return EDGL_OK;
}

}  // namespace sce

extern "C" long edgl_shared_ce_workspace(int R, int C, int S, int dtype) {
    if (sce::check_shape("edgl_shared_ce_workspace", R, C, 2, S, dtype)) return -1;
    return sce::layout(R, C, S, dtype).total;
}

// logq (f32 [I], or NULL): the label and every live slot read v - logq[c]; NULL launches the kernels without the term
extern "C" int edgl_shared_ce_fwd_q(const void* rows, const void* table, const float* out_bias, const float* logq, const int32_t* shared,
                                    const int64_t* labels, const int32_t* nvalid, int R, int C, int I, int S, float* vals,
                                    float* label_val, float* row_lse, int dtype, void* stream) {
    const int rc = sce::check_shape("edgl_shared_ce_fwd", R, C, I, S, dtype);                  // (first: no pointer is read before it)
    if (rc) return rc;
    EDGL_REQUIRE(rows && table && out_bias && shared && labels && vals && label_val && row_lse, EDGL_ERR_NULL,
                 "edgl_shared_ce_fwd: null pointer");
    EDGL_REQUIRE((((uintptr_t)rows | (uintptr_t)table | (uintptr_t)vals) & 15) == 0, EDGL_ERR_SHAPE,
                 "edgl_shared_ce_fwd: rows, table and vals must be 16-byte aligned");
    sce::P p{};
    p.rows = rows; p.table = table; p.bias = out_bias; p.shared = shared; p.labels = labels; p.nvalid = nvalid;
    p.logq = logq;
    p.R = R; p.C = C; p.I = I; p.S = S; p.Sp = sce::pad8(S);
    p.vals = vals; p.label_val = label_val; p.lse = row_lse;
    hipStream_t st = (hipStream_t)stream;
    return dtype == EDGL_BF16 ? sce::forward<bf16>(p, st) : sce::forward<float>(p, st);
}

extern "C" int edgl_shared_ce_fwd(const void* rows, const void* table, const float* out_bias, const int32_t* shared, const int64_t* labels,
                                  const int32_t* nvalid, int R, int C, int I, int S, float* vals, float* label_val, float* row_lse,
                                  int dtype, void* stream) {
    return edgl_shared_ce_fwd_q(rows, table, out_bias, nullptr, shared, labels, nvalid, R, C, I, S, vals, label_val, row_lse, dtype, stream);
}

// form: EDGL_LOSS_SOFTMAX (row_aux = row_lse; edgl_shared_ce_bwd forwards here), EDGL_LOSS_BCE, EDGL_LOSS_BPR (row_aux of
// edgl_sampled_row_loss)
extern "C" int edgl_shared_ce_bwd_form(const void* rows, const void* table, const int32_t* shared, const int64_t* labels,
                                       const float* vals, const float* label_val, const float* row_aux, const float* coef,
                                       const float* gscale, const int32_t* nvalid, int R, int C, int I, int S, void* d_rows,
                                       float* d_table, float* d_bias, float* workspace, int64_t* keys, void* plan, int form, int dtype,
                                       void* stream) {
    const float* row_lse = row_aux;
    const int rc = sce::check_shape("edgl_shared_ce_bwd", R, C, I, S, dtype);
    if (rc) return rc;
    EDGL_REQUIRE(form >= sdv::SOFTMAX && form <= sdv::BPR, EDGL_ERR_SHAPE,
                 "edgl_shared_ce_bwd: form %d (0 <= form <= %d: softmax, bce, bpr)", form, sdv::BPR);
    EDGL_REQUIRE(rows && table && shared && labels && vals && label_val && row_lse && coef && d_rows && d_table && d_bias, EDGL_ERR_NULL,
                 "edgl_shared_ce_bwd: null pointer");
    EDGL_REQUIRE(workspace, EDGL_ERR_WORKSPACE, "edgl_shared_ce_bwd: needs edgl_shared_ce_workspace(R, C, S, dtype) floats");
    EDGL_REQUIRE(!keys == !plan, EDGL_ERR_NULL, "edgl_shared_ce_bwd: keys and plan go together (both NULL: the atomic mode)");
    EDGL_REQUIRE((((uintptr_t)rows | (uintptr_t)table | (uintptr_t)d_rows | (uintptr_t)d_table | (uintptr_t)workspace) & 15) == 0,
                 EDGL_ERR_SHAPE, "edgl_shared_ce_bwd: rows, table, d_rows, d_table and the workspace must be 16-byte aligned");
    sce::P p{};
    p.rows = rows; p.table = table; p.shared = shared; p.labels = labels; p.nvalid = nvalid;
    p.R = R; p.C = C; p.I = I; p.S = S; p.Sp = sce::pad8(S);
    p.vals = const_cast<float*>(vals); p.label_val = const_cast<float*>(label_val); p.lse = const_cast<float*>(row_lse);
    p.coef = coef; p.gscale = gscale; p.d_rows = d_rows; p.d_table = d_table; p.d_bias = d_bias; p.keys = keys; p.det = plan ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    return dtype == EDGL_BF16 ? sce::backward<bf16>(p, workspace, plan, form, dtype, st)
                              : sce::backward<float>(p, workspace, plan, form, dtype, st);
}

extern "C" int edgl_shared_ce_bwd(const void* rows, const void* table, const int32_t* shared, const int64_t* labels, const float* vals,
                                  const float* label_val, const float* row_lse, const float* coef, const float* gscale,
                                  const int32_t* nvalid, int R, int C, int I, int S, void* d_rows, float* d_table, float* d_bias,
                                  float* workspace, int64_t* keys, void* plan, int dtype, void* stream) {
    return edgl_shared_ce_bwd_form(rows, table, shared, labels, vals, label_val, row_lse, coef, gscale, nvalid, R, C, I, S, d_rows,
                                   d_table, d_bias, workspace, keys, plan, EDGL_LOSS_SOFTMAX, dtype, stream);
}
