// K6q: FP8 item-table retrieval, stage 1 — the short list of a two-stage retrieval.  Rows and item table are OCP
// e4m3 bytes with one f32 scale per row (edgl_rows_to_fp8, below);
//     logit[r, i] = rows_scale[r] * table_scale[i] * sum_c q_r[c] q_i[c] + [-1000, out_bias][i]
// -> -inf at the row's seen ids -> top-K by (value desc, id asc), without a logits tile.  The scheme is k_eval_topk.hip's (group
// maxima -> per-row bound -> candidates above it -> one ranking launch, rows whose list overflows redone exactly), the sweep is
// made for 1-byte operands:
//   * operands stay bytes into the matrix pipe: v_mfma_f32_16x16x128_f8f6f4 at C >= 128 (one instruction contracts 128 channels),
//     v_mfma_f32_16x16x32_fp8_fp8 below.  Lane group g = lane / 16 feeds bytes [g KS/4, (g + 1) KS/4) of a KS-channel step for A
//     (items) and B (queries) alike, so the contraction pairs equal channels whatever the instruction's k order inside a lane.
//   * a wave holds 64 query rows (32 at C = 512) as B fragments in registers for the whole walk — 64 VGPRs at C = 256, where bf16
//     operands need 64 VGPRs for 32 rows — and a workgroup is 4 waves: 256 query rows (128 at C = 512) against one item slice.
//     Every wave walks the WHOLE item tile: an A fragment read from LDS meets 4 query blocks of 16, the tile is read from L2 once
//     per 256 rows.
//   * D[item][query] lands with the query on the lane (lane & 15) and 4 consecutive items on the registers: the f32 epilogue
//     (table scale and bias per item from LDS, row scale from a register) and the selection need no cross-lane traffic.
//   * item tiles of 16 KB stream through a double-buffered LDS image (rows of C + 16 bytes), one register staging set, one barrier
//     per tile; slices are placed by eval_sweep.h's XCD-aware order.
//   * selection: 8 groups per (row, slice) — lane group x parity of the 16-item sub-tile; a hit of pass 2 is rare (a few hundred
//     per row and call), so it goes straight to the row's global list behind a test of the slice's seen bitmap (LDS).
//   * ranking: one workgroup per row selects the K largest (value key, ~id) pairs of the list by an 8-pass radix select over the
//     64-bit pair — exact for any K <= 1024 and any ties — and orders them by counting.  A list longer than its capacity sends
//     the row the exact way: the same FP8 scores by VALU dot products into a scratch row, seen mask, the same select.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "eval_sweep.h"
#include "topk_select.h"

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

namespace ev8 {
using evs::sweep_grid;
using evs::sweep_qblock;
using evs::sweep_slice;

constexpr int GPS = 8;             // groups per (row, slice)
constexpr int CAP = 4096;          // candidates a row's list holds
constexpr int MAX_G = 4096;        // group maxima per row the bound kernel keeps in LDS
constexpr int SLICE_CAP = 1024;    // items of a slice: 32 KB of seen bitmap at 256 rows
constexpr int MAX_K = 1024;        // edgl_topk_merge orders up to 1024 candidates per row

struct P {
    const uint8_t* rows; const float* rscale; const uint8_t* table; const float* tscale; const float* bias; const int64_t* seen;
    int T, R, I, i0, i1, K;
    int nslices, tps, G;
    float* gmax; float* thr; int32_t* count; float* cval; int32_t* cidx;
    float* scratch;               // [R, i1 - i0] f32: score rows of the exact fallback (touched by overflowed rows only)
    float* out_val; int32_t* out_idx;
};

__host__ __device__ constexpr bool width_ok(int C) { return C >= 32 && C <= 512 && (C & (C - 1)) == 0; }

template <int C_>
struct Geo {
    static constexpr int C = C_;
    static constexpr int KS = C >= 128 ? 128 : 32;         // channels one matrix instruction contracts
    static constexpr int NK = C / KS, FB = KS / 4;         // steps per logit; fragment bytes per lane
    static constexpr int QW = C == 512 ? 32 : 64;          // query rows a wave holds
    static constexpr int NQ = QW / 16, QB = 4 * QW, NTHR = 256;
    static constexpr int NZ = C <= 128 ? 128 : 16384 / C;  // item rows of a tile
    static constexpr int LDZ = C + 16, ZB = NZ * LDZ;
    static constexpr int PIECES = NZ * C / 16 / NTHR;
    static constexpr int OFF_Z = 0, OFF_TS = 2 * ZB, OFF_BIAS = OFF_TS + 2 * NZ * 4, OFF_BMP = OFF_BIAS + 2 * NZ * 4;
    static constexpr int BYTES_GMAX = OFF_BMP;
    static constexpr int bytes_emit(int slice_items) { return OFF_BMP + QB * ((slice_items + 31) / 32) * 4; }
    static_assert(PIECES >= 1 && NZ % 32 == 0 && NZ <= NTHR && SLICE_CAP % NZ == 0, "tile geometry");
};

template <int KS> struct Frag { typedef i32x8 type; };
template <> struct Frag<32> { typedef long type; };

__device__ __forceinline__ f32x4 mma8(const i32x8& a, const i32x8& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 0, 0, 0);      // both operands e4m3, no block scales
}
__device__ __forceinline__ f32x4 mma8(const long& a, const long& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0);
}

// a fragment's bytes from 16-byte aligned memory (LDS rows are shifted by 16 bytes: no 32-byte alignment to assume)
__device__ __forceinline__ void ld_frag(const void* src, i32x8& f) {
    const u32x4 a = reinterpret_cast<const u32x4*>(src)[0], b = reinterpret_cast<const u32x4*>(src)[1];
    f = i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
}
__device__ __forceinline__ void ld_frag(const void* src, long& f) { f = *reinterpret_cast<const long*>(src); }

// THE epilogue: every kernel of this file that forms a score does it through this function
__device__ __forceinline__ float fp8_logit(float dot, float tscale, float rscale, float bias) { return fmaf(dot * tscale, rscale, bias); }

// one item tile: global -> registers (rows clamped into the table), registers -> LDS with the items' scale and bias beside them:
// item 0 scores -1000 (scale 0: Base.py:106-113), an item behind the range -inf
template <int C>
__device__ __forceinline__ void tile_load(const P& p, int item0, u32x4 (&r)[Geo<C>::PIECES], float& ts, float& bi) {
    constexpr int CP = C / 16;
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < Geo<C>::PIECES; ++j) {
        const int pc = tid + 256 * j, row = pc / CP, c16 = pc % CP;
        r[j] = *reinterpret_cast<const u32x4*>(p.table + (long)min(item0 + row, p.I - 1) * C + c16 * 16);
    }
    const int it = item0 + tid;
    const bool real = tid < Geo<C>::NZ && it < p.i1 && it > 0;
    ts = real ? p.tscale[it] : 0.f;
    bi = real ? p.bias[it - 1] : (it == 0 ? -1000.0f : -INFINITY);
}
template <int C>
__device__ __forceinline__ void tile_store(char* smem, int buf, const u32x4 (&r)[Geo<C>::PIECES], float ts, float bi) {
    using G_ = Geo<C>;
    constexpr int CP = C / 16;
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < G_::PIECES; ++j) {
        const int pc = tid + 256 * j, row = pc / CP, c16 = pc % CP;
        *reinterpret_cast<u32x4*>(smem + G_::OFF_Z + buf * G_::ZB + row * G_::LDZ + c16 * 16) = r[j];
    }
    if (tid < G_::NZ) {
        reinterpret_cast<float*>(smem + G_::OFF_TS)[buf * G_::NZ + tid] = ts;
        reinterpret_cast<float*>(smem + G_::OFF_BIAS)[buf * G_::NZ + tid] = bi;
    }
}

// EMIT = false: pass 1 (group maxima);  true: pass 2 (candidates)
template <int C, bool EMIT>
__global__ __launch_bounds__(256, 2) void fp8_sweep_kernel(P p) {
    using G_ = Geo<C>;
    typedef typename Frag<G_::KS>::type frag_t;
    constexpr int NK = G_::NK, FB = G_::FB, NQ = G_::NQ, QW = G_::QW, QB = G_::QB, NZ = G_::NZ, NTHR = G_::NTHR, LDZ = G_::LDZ;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, g = lane >> 4;
    const int slice = sweep_slice<QB>(p);
    if (slice >= p.nslices) return;
    const int q0 = sweep_qblock<QB>(p) * QB;
    // the wave's query rows: B fragments and row scales, resident for the whole walk
    frag_t xf[NQ][NK];
    float rs[NQ];
#pragma unroll
    for (int qb = 0; qb < NQ; ++qb) {
        const int q = min(q0 + wave * QW + qb * 16 + l16, p.R - 1);
        rs[qb] = p.rscale[q];
#pragma unroll
        for (int k = 0; k < NK; ++k) ld_frag(p.rows + (long)q * C + k * G_::KS + g * FB, xf[qb][k]);
    }
    const int tile_lo = slice * p.tps, ntile_all = (p.i1 - p.i0 + NZ - 1) / NZ;
    const int tile_hi = min(ntile_all, tile_lo + p.tps);
    const int item_lo = p.i0 + tile_lo * NZ;
    uint32_t* bmp = reinterpret_cast<uint32_t*>(smem + G_::OFF_BMP);
    const int bw = (p.tps * NZ + 31) / 32;        // bitmap words per row
    float thr[NQ];
    if constexpr (EMIT) {
        for (int i = tid; i < QB * bw; i += NTHR) bmp[i] = 0u;
#pragma unroll
        for (int qb = 0; qb < NQ; ++qb) thr[qb] = p.thr[min(q0 + wave * QW + qb * 16 + l16, p.R - 1)];
    }
    u32x4 stg[G_::PIECES];
    float sts, sbi;
    if (tile_lo < tile_hi) {
        tile_load<C>(p, p.i0 + tile_lo * NZ, stg, sts, sbi);
        tile_store<C>(smem, 0, stg, sts, sbi);
    }
    __syncthreads();
    if constexpr (EMIT) {
        // the rows' seen ids that fall into this slice as a bitmap (Base.py:156-163)
        const int item_hi = min(p.i1, p.i0 + tile_hi * NZ);
        const int nid = min(QB, p.R - q0) * p.T;
        const int64_t* sbase = p.seen + (long)q0 * p.T;
        for (int i = tid; i < nid; i += NTHR) {
            const int64_t v = sbase[i];
            if (v >= item_lo && v < item_hi) {
                const int o = (int)(v - item_lo);
                atomicOr(bmp + (i / p.T) * bw + (o >> 5), 1u << (o & 31));
            }
        }
        __syncthreads();
    }
    float gm[NQ][2];
#pragma unroll
    for (int qb = 0; qb < NQ; ++qb) gm[qb][0] = gm[qb][1] = -INFINITY;
    int buf = 0;
    for (int t = tile_lo; t < tile_hi; ++t) {
        if (t + 1 < tile_hi) tile_load<C>(p, p.i0 + (t + 1) * NZ, stg, sts, sbi);
        const char* zb = smem + G_::OFF_Z + buf * G_::ZB;
        const float* tsb = reinterpret_cast<const float*>(smem + G_::OFF_TS) + buf * NZ;
        const float* bb = reinterpret_cast<const float*>(smem + G_::OFF_BIAS) + buf * NZ;
#pragma unroll 1
        for (int sub2 = 0; sub2 < NZ / 16; sub2 += 2)
#pragma unroll
        for (int par = 0; par < 2; ++par) {          // (the parity of the sub-tile is the group: a static register index)
            const int sub = sub2 + par;
            frag_t zf[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) ld_frag(zb + (sub * 16 + l16) * LDZ + k * G_::KS + g * FB, zf[k]);
            const int m = sub * 16 + 4 * g;          // the lane's 4 items of this sub-tile
            const f32x4 ts4 = *reinterpret_cast<const f32x4*>(tsb + m), b4 = *reinterpret_cast<const f32x4*>(bb + m);
#pragma unroll
            for (int qb = 0; qb < NQ; ++qb) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < NK; ++k) acc = mma8(zf[k], xf[qb][k], acc);
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fp8_logit(acc[r], ts4[r], rs[qb], b4[r]);
                if constexpr (!EMIT) {
                    gm[qb][par] = fmaxf(fmaxf(gm[qb][par], fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
                } else {
                    const float vmax = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
                    if (vmax >= thr[qb]) {          // rare: a few hundred hits per row and call
                        const int rl = wave * QW + qb * 16 + l16, row = q0 + rl;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int item = p.i0 + t * NZ + m + r, o = item - item_lo;
                            if (v[r] >= thr[qb] && row < p.R && !((bmp[rl * bw + (o >> 5)] >> (o & 31)) & 1u)) {
                                const int pos = atomicAdd(p.count + row, 1);
                                if (pos < CAP) {
                                    p.cval[(long)row * CAP + pos] = v[r];
                                    p.cidx[(long)row * CAP + pos] = item;
                                }
                            }
                        }
                    }
                }
            }
        }
        if (t + 1 < tile_hi) tile_store<C>(smem, buf ^ 1, stg, sts, sbi);
        __syncthreads();
        buf ^= 1;
    }
    if constexpr (!EMIT) {
#pragma unroll
        for (int qb = 0; qb < NQ; ++qb) {
            const int q = q0 + wave * QW + qb * 16 + l16;
            if (q < p.R) {
                float* o = p.gmax + (long)q * p.G + slice * GPS + g * 2;
                o[0] = gm[qb][0]; o[1] = gm[qb][1];
            }
        }
    }
}

// L[row] = a lower bound of the rank-th largest of the row's G group maxima: its key with the low 16 bits cleared, bit by bit over
// an LDS image of the keys.  Fewer than `rank` finite maxima: every finite score passes (and the row goes the exact way when that
// overflows its list).  Clears the row's candidate count.  One workgroup per row.
__global__ __launch_bounds__(256) void fp8_thr_kernel(const float* gmax, int G, int rank, float* thr, int32_t* count) {
    __shared__ uint32_t keys[MAX_G];
    __shared__ int wsum[2][4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int i = tid; i < G; i += 256) keys[i] = float_key(gmax[(long)row * G + i]);
    __syncthreads();
    uint32_t L = 0u;
    for (int bit = 31; bit >= 16; --bit) {
        const uint32_t cand = L | (1u << bit);
        int c = 0;
        for (int i = tid; i < G; i += 256) c += keys[i] >= cand ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) wsum[bit & 1][w] = c;
        __syncthreads();       // (two sum slots: a round's writes cannot meet the reads of the round before)
        if (wsum[bit & 1][0] + wsum[bit & 1][1] + wsum[bit & 1][2] + wsum[bit & 1][3] >= rank) L = cand;
    }
    if (tid == 0) {
        thr[row] = L <= float_key(-INFINITY) ? -3.0e38f : key_float(L);      // (items behind the range carry -inf and never pass)
        count[row] = 0;
    }
}

// the 4 consecutive e4m3 bytes of a word as floats
__device__ __forceinline__ void fp8x4_to_f32(uint32_t w, float (&o)[4]) {
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    o[0] = lo[0]; o[1] = lo[1]; o[2] = hi[0]; o[3] = hi[1];
}

// One workgroup per row: the K best of the row's candidates (n <= CAP of them in its list), or — the list overflowed — of the
// row's scores over the whole range, formed again into its scratch row.  pair(v, id) = float_key(v) << 32 | ~id is distinct per
// item and orders by (value desc, id asc); an 8-pass radix select finds the Keff-th largest pair, the pairs at or above it are
// exactly Keff, each one's count of larger pairs is its place.  A place whose value is -inf (fewer unseen items than K) reads -1.
template <int C>
__global__ __launch_bounds__(256) void fp8_rank_kernel(P p) {
    __shared__ uint32_t hist[256];
    __shared__ uint64_t sel_prefix;
    __shared__ int sel_remaining, wcount;
    __shared__ uint64_t win[MAX_K];
    __shared__ float xr[C];
    const int row = blockIdx.x, tid = threadIdx.x, K = p.K;
    const int n = p.count[row];
    float* ov = p.out_val + (long)row * K;
    int32_t* oi = p.out_idx + (long)row * K;
    const bool exact = n < 0 || n > CAP;
    const int ni = p.i1 - p.i0;
    const float* xv = p.cval + (long)row * CAP;
    const int32_t* xi = p.cidx + (long)row * CAP;
    int m = n;
    if (exact) {
        float* x = p.scratch + (long)row * ni;
        for (int c = tid * 4; c < C; c += 1024) {
            float f[4];
            fp8x4_to_f32(*reinterpret_cast<const uint32_t*>(p.rows + (long)row * C + c), f);
            xr[c] = f[0]; xr[c + 1] = f[1]; xr[c + 2] = f[2]; xr[c + 3] = f[3];
        }
        __syncthreads();
        const float rsc = p.rscale[row];
        for (int i = tid; i < ni; i += 256) {
            const int item = p.i0 + i;
            float a = 0.f;
            const uint8_t* z = p.table + (long)item * C;
#pragma unroll 2
            for (int k = 0; k < C; k += 16) {
                const u32x4 w4 = *reinterpret_cast<const u32x4*>(z + k);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float f[4];
                    fp8x4_to_f32(w4[e], f);
#pragma unroll
                    for (int b = 0; b < 4; ++b) a = fmaf(f[b], xr[k + 4 * e + b], a);
                }
            }
            x[i] = item == 0 ? -1000.0f : fp8_logit(a, p.tscale[item], rsc, p.bias[item - 1]);
        }
        __syncthreads();
        for (int t = tid; t < p.T; t += 256) {
            const long id = p.seen[(long)row * p.T + t] - p.i0;
            if (id >= 0 && id < ni) x[id] = -INFINITY;
        }
        __syncthreads();
        xv = x; xi = nullptr; m = ni;
    }
    auto pair_at = [&](int i) -> uint64_t {
        const uint32_t id = xi ? (uint32_t)xi[i] : (uint32_t)(p.i0 + i);
        return ((uint64_t)float_key(xv[i]) << 32) | (uint64_t)(0xffffffffu - id);
    };
    const int Keff = min(K, m);
    for (int i = tid; i < K; i += 256) { ov[i] = -INFINITY; oi[i] = -1; }
    if (Keff == 0) return;          // (block-uniform)
    uint64_t prefix = 0ull, mask = 0ull;
    int remaining = Keff;
    for (int pass = 7; pass >= 0; --pass) {
        hist[tid] = 0u;
        __syncthreads();
        for (int i = tid; i < m; i += 256) {
            const uint64_t k = pair_at(i);
            if ((k & mask) == prefix) atomicAdd(&hist[(uint32_t)(k >> (pass * 8)) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            int acc = 0, b = 255;
            for (; b > 0; --b) {
                if (acc + (int)hist[b] >= remaining) break;
                acc += hist[b];
            }
            sel_prefix = prefix | ((uint64_t)b << (pass * 8));
            sel_remaining = remaining - acc;
            wcount = 0;
        }
        __syncthreads();
        prefix = sel_prefix;
        remaining = sel_remaining;
        mask |= 255ull << (pass * 8);
    }
    // prefix = the Keff-th largest pair
    for (int i = tid; i < m; i += 256) {
        const uint64_t k = pair_at(i);
        if (k >= prefix) {
            const int pos = atomicAdd(&wcount, 1);
            if (pos < MAX_K) win[pos] = k;
        }
    }
    __syncthreads();
    for (int me = tid; me < Keff; me += 256) {
        const uint64_t a = win[me];
        int rank = 0;
        for (int j = 0; j < Keff; ++j) rank += win[j] > a ? 1 : 0;
        const float v = key_float((uint32_t)(a >> 32));
        ov[rank] = v;
        oi[rank] = v == -INFINITY ? -1 : (int32_t)(0xffffffffu - (uint32_t)a);
    }
}

struct Plan { int nslices, tps, G; size_t off_thr, off_count, off_cval, off_cidx, off_scratch, bytes; };
inline int qb_of(int C) { return C == 512 ? 128 : 256; }
inline int nz_of(int C) { return C <= 128 ? 128 : 16384 / C; }
inline bool make_plan(int R, int C, int n_items, int T, int K, Plan& pl) {
    if (!width_ok(C) || K < 1 || K > MAX_K || R < 1 || T < 0 || n_items < K || n_items > evs::MAX_ITEMS) return false;
    const int nz = nz_of(C), ntile = (n_items + nz - 1) / nz, nrb = (R + qb_of(C) - 1) / qb_of(C);
    // fill the chip (two workgroups per CU) AND keep the bound selective: three times as many groups as the rank of the bound
    int want = std::max(512 / nrb, (3 * (K + T) + GPS - 1) / GPS);
    want = std::min(want, MAX_G / GPS);
    want = std::max(want, (n_items + SLICE_CAP - 1) / SLICE_CAP);         // a slice's seen bitmap
    want = std::min(want, ntile);
    pl.tps = (ntile + want - 1) / want;
    pl.nslices = (ntile + pl.tps - 1) / pl.tps;
    pl.G = pl.nslices * GPS;
    if (pl.G > MAX_G || pl.tps * nz > SLICE_CAP) return false;
    size_t o = 0;
    auto take = [&](size_t b) { const size_t at = o; o += (b + 255) & ~(size_t)255; return at; };
    take((size_t)R * pl.G * 4);
    pl.off_thr = take((size_t)R * 4); pl.off_count = take((size_t)R * 4);
    pl.off_cval = take((size_t)CAP * R * 4); pl.off_cidx = take((size_t)CAP * R * 4);
    pl.off_scratch = take((size_t)R * n_items * 4);      // (never touched unless a row overflows)
    pl.bytes = o;
    return true;
}

template <int C>
int launch(P p, const Plan& pl, hipStream_t st) {
    using G_ = Geo<C>;
    const dim3 grid(sweep_grid(p.R, G_::QB, pl.nslices));
    auto k1 = fp8_sweep_kernel<C, false>;
    auto k2 = fp8_sweep_kernel<C, true>;
    const int be = G_::bytes_emit(pl.tps * G_::NZ);
    EDGL_REQUIRE(be <= 80 * 1024, EDGL_ERR_SHAPE, "edgl_score_topk_fp8: %d B of LDS", be);
    EDGL_LDS_LIMIT(k1, G_::BYTES_GMAX, "edgl_score_topk_fp8");
    EDGL_LDS_LIMIT(k2, be, "edgl_score_topk_fp8");
    hipLaunchKernelGGL(k1, grid, dim3(256), G_::BYTES_GMAX, st, p);
    hipLaunchKernelGGL(fp8_thr_kernel, dim3(p.R), dim3(256), 0, st, p.gmax, p.G, p.K + p.T, p.thr, p.count);
    hipLaunchKernelGGL(k2, grid, dim3(256), be, st, p);
    hipLaunchKernelGGL(fp8_rank_kernel<C>, dim3(p.R), dim3(256), 0, st, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

// ---- the quantiser: rows [R, C] (f32 or bf16) -> e4m3 bytes and one f32 scale per row ---------------------------------------
// A lane owns 16 consecutive channels (one 16-byte store), C / 16 lanes own a row: the row maximum goes by wave shuffles inside
// that lane group, then scale = max|row| / 448 (1 for a zero row), q = x / scale in f32 -> v_cvt_pk_fp8_f32 (round to nearest
// even).  A row with a non-finite element: bytes 0, scale NaN, one count into `violations`.
template <typename T, int C>
__global__ __launch_bounds__(256) void fp8_quant_kernel(const T* src, int R, uint8_t* q8, float* scale, int* violations) {
    constexpr int LPR = C / 16;
    const long gt = (long)blockIdx.x * 256 + threadIdx.x, row = gt / LPR;
    const int part = (int)(gt % LPR);
    const bool live = row < R;
    const T* s = src + (live ? row : (long)R - 1) * C + part * 16;
    float x[16];
    if constexpr (sizeof(T) == 4) {
        f32x4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const f32x4*>(s + 4 * j);
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = v[j >> 2][j & 3];
    } else {
        bf16x8 v[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) v[j] = *reinterpret_cast<const bf16x8*>(s + 8 * j);
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = (float)v[j >> 3][j & 7];
    }
    float mx = 0.f;
    int bad = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const float a = fabsf(x[j]);
        bad |= a <= 3.4028234e38f ? 0 : 1;       // (false for inf and for NaN)
        mx = fmaxf(mx, a);
    }
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        bad |= __shfl_xor(bad, o, 64);
    }
    const float sc = mx > 0.f ? mx / 448.0f : 1.0f;
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = fminf(fmaxf(x[4 * j + e] / sc, -448.0f), 448.0f);
        int pk = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], 0, false);
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], pk, true);
        w[j] = bad ? 0u : (uint32_t)pk;
    }
    if (live) {
        *reinterpret_cast<uint4*>(q8 + row * C + part * 16) = make_uint4(w[0], w[1], w[2], w[3]);
        if (part == 0) {
            scale[row] = bad ? __builtin_nanf("") : sc;
            if (bad && violations) atomicAdd(violations, 1);
        }
    }
}

template <typename T>
int quant_launch(const void* src, int R, int C, uint8_t* q8, float* scale, int* viol, hipStream_t st) {
    const unsigned grid = (unsigned)(((long)R * (C / 16) + 255) / 256);
    const T* s = (const T*)src;
    switch (C) {
        case 32: hipLaunchKernelGGL((fp8_quant_kernel<T, 32>), dim3(grid), dim3(256), 0, st, s, R, q8, scale, viol); break;
        case 64: hipLaunchKernelGGL((fp8_quant_kernel<T, 64>), dim3(grid), dim3(256), 0, st, s, R, q8, scale, viol); break;
        case 128: hipLaunchKernelGGL((fp8_quant_kernel<T, 128>), dim3(grid), dim3(256), 0, st, s, R, q8, scale, viol); break;
        case 256: hipLaunchKernelGGL((fp8_quant_kernel<T, 256>), dim3(grid), dim3(256), 0, st, s, R, q8, scale, viol); break;
        default: hipLaunchKernelGGL((fp8_quant_kernel<T, 512>), dim3(grid), dim3(256), 0, st, s, R, q8, scale, viol); break;
    }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

}  // namespace ev8

extern "C" int edgl_rows_to_fp8(const void* src, int R, int C, int dtype, void* q8_out, float* scale_out, int* violations, void* stream) {
    EDGL_REQUIRE(src && q8_out && scale_out, EDGL_ERR_NULL, "edgl_rows_to_fp8: null pointer");
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_rows_to_fp8: dtype %d (f32 or bf16)", dtype);
    EDGL_REQUIRE(ev8::width_ok(C), EDGL_ERR_SHAPE, "edgl_rows_to_fp8: C=%d is not a power of two in [32, 512]", C);
    EDGL_REQUIRE(R >= 1 && (long)R * C < (1l << 34), EDGL_ERR_SHAPE, "edgl_rows_to_fp8: R=%d rows (R >= 1, R C < 2^34)", R);
    hipStream_t st = (hipStream_t)stream;
    return dtype == EDGL_F32 ? ev8::quant_launch<float>(src, R, C, (uint8_t*)q8_out, scale_out, violations, st)
                             : ev8::quant_launch<bf16>(src, R, C, (uint8_t*)q8_out, scale_out, violations, st);
}

// 1 when edgl_score_topk_fp8 takes this shape: C a power of two in [32, 512], 1 <= K <= 1024, K <= n_items <= 262144 per call
extern "C" int edgl_score_topk_fp8_supported(int R, int C, int n_items, int T, int K) {
    ev8::Plan pl;
    return ev8::make_plan(R, C, n_items, T, K, pl) ? 1 : 0;
}
extern "C" long edgl_score_topk_fp8_workspace(int R, int C, int n_items, int T, int K) {
    ev8::Plan pl;
    if (!ev8::make_plan(R, C, n_items, T, K, pl)) return -1;
    return (long)pl.bytes;
}
extern "C" int edgl_score_topk_fp8(const void* rows_q8, const float* rows_scale, const void* table_q8, const float* table_scale,
                                   const float* out_bias, const int64_t* seen, int T, int R, int C, int I, int i0, int i1, int K,
                                   float* out_val, int32_t* out_idx, void* workspace, void* stream) {
    EDGL_REQUIRE(rows_q8 && rows_scale && table_q8 && table_scale && out_bias && out_val && out_idx && workspace, EDGL_ERR_NULL,
                 "edgl_score_topk_fp8: null pointer");
    EDGL_REQUIRE(seen || T == 0, EDGL_ERR_NULL, "edgl_score_topk_fp8: T > 0 without seen ids");
    EDGL_REQUIRE(ev8::width_ok(C), EDGL_ERR_SHAPE, "edgl_score_topk_fp8: C=%d is not a power of two in [32, 512]", C);
    EDGL_REQUIRE(K >= 1 && K <= ev8::MAX_K, EDGL_ERR_SHAPE, "edgl_score_topk_fp8: K=%d outside [1, %d]", K, ev8::MAX_K);
    EDGL_REQUIRE(R >= 1 && T >= 0, EDGL_ERR_SHAPE, "edgl_score_topk_fp8: R=%d T=%d (R >= 1, T >= 0)", R, T);
    EDGL_REQUIRE(I > 1 && i0 >= 0 && i1 <= I && i0 < i1 && i0 % 8 == 0, EDGL_ERR_SHAPE,
                 "edgl_score_topk_fp8: bad item range [%d, %d) of %d (i0 %% 8 == 0)", i0, i1, I);
    EDGL_REQUIRE(i1 - i0 >= K, EDGL_ERR_SHAPE, "edgl_score_topk_fp8: %d items in the range, fewer than K=%d", i1 - i0, K);
    EDGL_REQUIRE(i1 - i0 <= evs::MAX_ITEMS, EDGL_ERR_SHAPE, "edgl_score_topk_fp8: %d items per call (at most %d: chunks + edgl_topk_merge)",
                 i1 - i0, evs::MAX_ITEMS);
    ev8::Plan pl;
    EDGL_REQUIRE(ev8::make_plan(R, C, i1 - i0, T, K, pl), EDGL_ERR_SHAPE, "edgl_score_topk_fp8: no plan (R=%d C=%d items=%d T=%d K=%d)", R, C,
                 i1 - i0, T, K);
    char* ws = (char*)workspace;
    ev8::P p{};
    p.rows = (const uint8_t*)rows_q8; p.rscale = rows_scale; p.table = (const uint8_t*)table_q8; p.tscale = table_scale; p.bias = out_bias;
    p.seen = seen; p.T = T; p.R = R; p.I = I; p.i0 = i0; p.i1 = i1; p.K = K; p.nslices = pl.nslices; p.tps = pl.tps; p.G = pl.G;
    p.gmax = reinterpret_cast<float*>(ws); p.thr = reinterpret_cast<float*>(ws + pl.off_thr);
    p.count = reinterpret_cast<int32_t*>(ws + pl.off_count); p.cval = reinterpret_cast<float*>(ws + pl.off_cval);
    p.cidx = reinterpret_cast<int32_t*>(ws + pl.off_cidx); p.scratch = reinterpret_cast<float*>(ws + pl.off_scratch);
    p.out_val = out_val; p.out_idx = out_idx;
    hipStream_t st = (hipStream_t)stream;
    switch (C) {
        case 32: return ev8::launch<32>(p, pl, st);
        case 64: return ev8::launch<64>(p, pl, st);
        case 128: return ev8::launch<128>(p, pl, st);
        case 256: return ev8::launch<256>(p, pl, st);
        default: return ev8::launch<512>(p, pl, st);
    }
}
