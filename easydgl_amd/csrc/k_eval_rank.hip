// K6r: evaluation by label rank — Sequential.eval (Base.py:150-201) needs ONE number per evaluated row: the place of the true next
// item y in the (logit desc, item id asc) order of the unseen catalogue.  That place is a count,
//     rank[r] = #{ j != y : v_j > v_y  or  (v_j == v_y and j < y) },      v_j = -inf for the row's seen ids (Base.py:156-163),
// so no top-K list, candidate list or merge is needed: HR@k = [rank < k], NDCG@k = [rank < k] / log2(rank + 2), MRR = 1 / (rank + 1)
// for ANY k, and counts over disjoint item ranges (chunks, table shards) simply add.
//
//   fused form (bf16, C in {64, 128, 256}) — two launches per item range, no logits in HBM:
//     label_value_kernel   v_y of every row by the sweep's own MFMA chain — evs::score_step (eval_sweep.h), k ascending, the accumulator
//                          started from the item's bias — on a tile of GATHERED label rows: 32 query rows against their 32 label
//                          items, the diagonal kept.  An MFMA result element depends on its own operand row and column only, so
//                          these are the bits the sweep forms for the pair (r, y) — the tie rule on duplicated items rests on
//                          that.  -inf where the label is one of the row's seen ids.  Once per batch, whatever the number of ranges.
//     rank_sweep_kernel    eval_sweep.h's sweep (workgroup = query block x item slice, tile ring, seen bitmap, bias-started chain).
//                          This file adds what is done with an MFMA tile: a lane's 16 values belong to ONE row and are compared
//                          with that row's v_y in place, a seen item counting as -inf; the per-row counts in LDS behind the bias
//                          rows; and the epilogue: one integer atomic per (row, workgroup) adds into count[r] — exact and
//                          order-independent (DESIGN rule 13).
//   tile form (any dtype / width) over an [R, n] f32 logits tile that is read and not modified:
//     label_value_tile_kernel   v_y from the tile for the rows whose label lies in it (+ the seen test), other rows untouched
//     rank_count_tile_kernel    one workgroup per (row, segment of 8192 items): seen bitmap of the segment, compare, count
//   rank_metrics_from_rank_kernel   sums[2 nk + 1] += (H@k.., N@k.., MRR) of a batch of ranks, fixed summation order.
#include <algorithm>

#include "eval_sweep.h"

namespace evr {
using namespace evs;

struct P {
    const bf16* rows; const bf16* table; const float* bias; const int64_t* seen; const int64_t* labels; const float* label_val;
    int T, R, I, i0, i1;
    int nslices, tps;             // item slices, tiles per slice
    int32_t* count;
};

template <int C, int NZ, int NWS>
struct Geo : SweepGeo<C, NZ, NWS> {
    using S = SweepGeo<C, NZ, NWS>;
    static constexpr int OFF_CNT = S::OFF_OWN;                 // per-row counts [QB]
    static constexpr int OFF_BMP = OFF_CNT + S::QB * 4;        // seen bitmap [QB][words]
    static constexpr int bytes(int slice_items) { return OFF_BMP + S::QB * ((slice_items + 31) / 32) * 4; }
    static_assert(NZ * C / 8 % S::NTHR == 0 && NZ % (32 * NWS) == 0 && S::PIECES >= 1 && S::NTHR >= NZ, "tile geometry");
};

template <int C, int NZ, int NWS>
__global__ __launch_bounds__(64 * (qb_of(C) / 32) * NWS) void rank_sweep_kernel(P p) {
    using G_ = Geo<C, NZ, NWS>;
    constexpr int CK = C / 16, NTW = NZ / (32 * NWS), NTHR = G_::NTHR, QB = G_::QB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = wave / NWS, sw = wave % NWS, l32 = lane & 31, hi = lane >> 5;
    const int slice = sweep_slice<QB>(p);
    if (slice >= p.nslices) return;
    const int q0 = sweep_qblock<QB>(p) * QB;
    bf16x8 xf[CK];
#pragma unroll
    for (int k = 0; k < CK; ++k) xf[k] = query_frag<C>(p, q0 + 32 * h + l32, hi, k);
    int* rowcnt = reinterpret_cast<int*>(smem + G_::OFF_CNT);
    uint32_t* bmp = reinterpret_cast<uint32_t*>(smem + G_::OFF_BMP);
    const int bw = (p.tps * NZ + 31) / 32;        // bitmap words per row
    for (int i = tid; i < QB; i += NTHR) rowcnt[i] = 0;
    for (int i = tid; i < QB * bw; i += NTHR) bmp[i] = 0u;
    const int tile_lo = slice * p.tps, ntile_all = (p.i1 - p.i0 + NZ - 1) / NZ;
    const int tile_hi = min(ntile_all, tile_lo + p.tps);
    uint4 stg[G_::PIECES], stg2[G_::PIECES];
    float stb, stb2;
    if (tile_lo < tile_hi) {
        tile_load<C, NZ, NWS>(p, p.i0 + tile_lo * NZ, stg, stb);
        tile_store<C, NZ, NWS>(p, p.i0 + tile_lo * NZ, stg, stb, smem + G_::OFF_Z, reinterpret_cast<float*>(smem + G_::OFF_BIAS));
        tile_load<C, NZ, NWS>(p, p.i0 + min(tile_lo + 1, tile_hi - 1) * NZ, stg, stb);      // tile 1 (set A)
    }
    __syncthreads();
    {
        // the rows' seen ids that fall into this slice as a bitmap (Base.py:156-163; the loads in batches: eval_sweep.h)
        const int item_lo = p.i0 + tile_lo * NZ, item_hi = min(p.i1, p.i0 + tile_hi * NZ);
        const int nid = min(QB, p.R - q0) * p.T, npair = nid / 2;
        const int64_t* sbase = p.seen + (long)q0 * p.T;
        auto mark = [&](int i, int64_t v) {
            if (v >= item_lo && v < item_hi) {
                const int o = (int)(v - item_lo);
                atomicOr(bmp + (i / p.T) * bw + (o >> 5), 1u << (o & 31));
            }
        };
        for (int i0_ = tid; i0_ < npair; i0_ += 16 * NTHR) {
            ulonglong2 v[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = *reinterpret_cast<const ulonglong2*>(sbase + 2 * min(i0_ + j * NTHR, npair - 1));
#pragma unroll
            for (int j = 0; j < 16; ++j) asm volatile("" : "+v"(v[j].x), "+v"(v[j].y));
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int i = i0_ + j * NTHR;
                if (i < npair) { mark(2 * i, (int64_t)v[j].x); mark(2 * i + 1, (int64_t)v[j].y); }
            }
        }
        if ((nid & 1) && tid == 0) mark(nid - 1, sbase[nid - 1]);
        __syncthreads();
    }
    const int q = q0 + 32 * h + l32;             // this lane's query row
    const float vy = p.label_val[min(q, p.R - 1)];
    const int y = (int)p.labels[min(q, p.R - 1)];
    const uint32_t* brow = bmp + (32 * h + l32) * bw;
    int tot = 0;
    int buf = 0;
    // the tile ring (eval_sweep.h): tile t from LDS buffer `buf` with set A holding tile t + 1 and set B taking tile t + 2
    auto one_tile = [&](int t, uint4 (&sa)[G_::PIECES], float& ba, uint4 (&sb)[G_::PIECES], float& bbn) {
        const int tn = t + 1, tnn = t + 2;
        if (tnn < tile_hi) tile_load<C, NZ, NWS>(p, p.i0 + tnn * NZ, sb, bbn);
        asm volatile("" ::: "memory");
#pragma unroll
        for (int u = 0; u < NTW; ++u) {
            const int m0 = (sw * NTW + u) * 32;               // the MFMA tile's first item row inside the LDS tile
            const f32x16 acc = score_tile<C, NZ, NWS>(smem, buf, m0, l32, hi, xf);
            // The MFMA tile's 32 items are ONE word of the row's bitmap; register 4 j + i of this lane is the item at offset 8 j + i
            // from `base`.  Items strictly below the label count on >=, items above it on >: both counts are kept and the lane takes
            // the one its 16 items call for; the one tile that holds the label or the end of the range is counted item by item.
            const int base = p.i0 + t * NZ + m0 + 4 * hi;
            const uint32_t w = brow[((t - tile_lo) * NZ + m0) >> 5] >> (4 * hi);
            auto val = [&](int e) { return ((w >> (8 * (e >> 2) + (e & 3))) & 1u) ? -INFINITY : acc[e]; };
            const int dy = y - base, dv = p.i1 - base;
            if ((dy >= 0 && dy < 28) || dv < 28) {
                int c = 0;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int off = 8 * (e >> 2) + (e & 3);
                    const float v = val(e);
                    c += (off < dv && off != dy && (v > vy || (v == vy && off < dy))) ? 1 : 0;
                }
                tot += c;
            } else {
                int lgt = 0, lge = 0;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float v = val(e);
                    lgt += v > vy ? 1 : 0;
                    lge += v >= vy ? 1 : 0;
                }
                tot += dy >= 28 ? lge : lgt;
            }
        }
        if (tn < tile_hi)
            tile_store<C, NZ, NWS>(p, p.i0 + tn * NZ, sa, ba, smem + G_::OFF_Z + (buf ^ 1) * G_::ZB,
                                   reinterpret_cast<float*>(smem + G_::OFF_BIAS) + (buf ^ 1) * NZ);
        __syncthreads();
        buf ^= 1;
    };
    for (int t = tile_lo; t < tile_hi; t += 2) {
        one_tile(t, stg, stb, stg2, stb2);
        if (t + 1 < tile_hi) one_tile(t + 1, stg2, stb2, stg, stb);      // (block-uniform)
    }
    // ---- the lane halves and the NWS waves of a row add up in LDS; ONE global integer atomic per (row, workgroup) ---------------------
    tot += __shfl_xor(tot, 32, 64);
    if (hi == 0 && q < p.R && tot) atomicAdd(rowcnt + 32 * h + l32, tot);
    __syncthreads();
    if (tid < QB && q0 + tid < p.R && rowcnt[tid]) atomicAdd(p.count + q0 + tid, rowcnt[tid]);
}

// v_y of 32 rows per wave: D[m][n] = bias(y_m) + table[y_m] . rows[n] by the sweep's chain, the diagonal m == n kept (see the head
// of the file); -inf where y is one of the row's seen ids.
template <int C>
__global__ __launch_bounds__(64) void label_value_kernel(const bf16* rows, const bf16* table, const float* bias, const int64_t* seen, int T,
                                                         const int64_t* labels, int R, int I, float* label_val) {
    constexpr int CK = C / 16;
    const int lane = threadIdx.x, l32 = lane & 31, hi = lane >> 5;
    const int q = blockIdx.x * 32 + l32, qc = min(q, R - 1);
    const int64_t y64 = labels[qc];
    const int y = (int)min(max(y64, (int64_t)0), (int64_t)(I - 1));       // (addresses stay inside the table whatever the label)
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) {          // register e of this lane is item row m = 8 (e / 4) + 4 hi + e % 4: the label of query row m
        const int ym = __shfl(y, 8 * (e >> 2) + 4 * hi + (e & 3), 64);
        acc[e] = ym == 0 ? -1000.0f : bias[max(ym, 1) - 1];
    }
    const bf16* zrow = table + (long)y * C + hi * 8;
    const bf16* xrow = rows + (long)qc * C + hi * 8;
#pragma unroll
    for (int k = 0; k < CK; ++k) {
        bf16x8 zf = *reinterpret_cast<const bf16x8*>(zrow + k * 16);
        if (y == 0) {                       // the used table's row 0 is the zero constant (coding.py:56-57)
#pragma unroll
            for (int i = 0; i < 8; ++i) zf[i] = (bf16)0.0f;
        }
        const bf16x8 xf = *reinterpret_cast<const bf16x8*>(xrow + k * 16);
        acc = score_step(zf, xf, acc);
    }
    const int esel = 4 * (l32 >> 3) + (l32 & 3);     // the register of row m == l32 (held by the lane half (l32 >> 2) & 1)
    float d = acc[0];
#pragma unroll
    for (int e = 1; e < 16; ++e) d = e == esel ? acc[e] : d;
    int found = 0;
    for (int t = hi; t < T; t += 2) found |= seen[(long)qc * T + t] == y64 ? 1 : 0;
    found |= __shfl_xor(found, 32, 64);
    if (hi == ((l32 >> 2) & 1) && q < R) label_val[q] = found ? -INFINITY : d;
}

// ---- tile form --------------------------------------------------------------------------------------------------------------------
// one wave per row: the lanes share the row's seen ids
__global__ __launch_bounds__(256) void label_value_tile_kernel(const float* logits, int R, int n, int i0, const int64_t* seen, int T,
                                                               const int64_t* labels, float* label_val) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= R) return;                                        // (wave-uniform)
    const int64_t y = labels[r];
    if (y < i0 || y >= (int64_t)i0 + n) return;
    bool found = false;
    for (int t = lane; t < T; t += 64) found |= seen[(long)r * T + t] == y;
    found = __any(found);
    if (lane == 0) label_val[r] = found ? -INFINITY : logits[(long)r * n + (y - i0)];
}

constexpr int SEG = 8192;      // items per workgroup of the tile count: 1 KB of seen bitmap
__global__ __launch_bounds__(256) void rank_count_tile_kernel(const float* logits, int R, int n, int i0, const int64_t* seen, int T,
                                                              const int64_t* labels, const float* label_val, int32_t* count, int nseg) {
    __shared__ uint32_t bmp[SEG / 32];
    __shared__ int wsum[4];
    const int tid = threadIdx.x, row = blockIdx.x / nseg, seg0 = (blockIdx.x % nseg) * SEG, segn = min(SEG, n - seg0);
    for (int i = tid; i < SEG / 32; i += 256) bmp[i] = 0u;
    __syncthreads();
    for (int t = tid; t < T; t += 256) {
        const int64_t o = seen[(long)row * T + t] - i0 - seg0;
        if (o >= 0 && o < segn) atomicOr(bmp + (o >> 5), 1u << (o & 31));
    }
    __syncthreads();
    const float vy = label_val[row];
    const int64_t dy64 = labels[row] - i0 - seg0;
    const int dy = (int)min(max(dy64, (int64_t)-1), (int64_t)SEG);       // (-1: every item is above the label; SEG: every item is below)
    const float* x = logits + (long)row * n + seg0;
    int c = 0;
    for (int j0 = tid; j0 < segn; j0 += 1024) {               // four loads in flight per thread (clamped, unconditional)
        float x4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x4[u] = x[min(j0 + 256 * u, segn - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + 256 * u;
            const float v = ((bmp[(j >> 5) & (SEG / 32 - 1)] >> (j & 31)) & 1u) ? -INFINITY : x4[u];
            c += (j < segn && j != dy && (v > vy || (v == vy && j < dy))) ? 1 : 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        const int s = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (s) atomicAdd(count + row, s);
    }
}

// sums[0 .. nk) += H@k, sums[nk .. 2 nk) += N@k, sums[2 nk] += MRR of the batch (Base.py:181-201 for any k, plus the reciprocal rank):
// a thread's rows in ascending order, then the block's fixed tree, then ONE writer.
__global__ __launch_bounds__(512) void rank_metrics_from_rank_kernel(const int32_t* rank, int R, const int32_t* ks, int nk, float* sums) {
    __shared__ float red[8];
    float hit[8], ndcg[8], mrr = 0.f;
    int kk[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { hit[i] = 0.f; ndcg[i] = 0.f; kk[i] = i < nk ? ks[i] : 0; }
    for (int r = threadIdx.x; r < R; r += blockDim.x) {
        const int rk = rank[r];
        const float gain = 1.0f / log2f((float)rk + 2.0f);
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (rk < kk[i]) { hit[i] += 1.f; ndcg[i] += gain; }
        mrr += 1.0f / ((float)rk + 1.0f);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (i < nk) {      // (block-uniform)
            const float th = block_sum(hit[i], red), tn = block_sum(ndcg[i], red);
            if (threadIdx.x == 0) { sums[i] += th; sums[nk + i] += tn; }
        }
    }
    const float tm = block_sum(mrr, red);
    if (threadIdx.x == 0) sums[2 * nk] += tm;
}

struct Plan { int nz, nslices, tps; };
// Enough slices to fill the chip, and no slice longer than its seen bitmap allows.  None of the top-K plan's constraints (groups against
// K + T, candidate cap, 4096-item minimum) exist here.
inline bool make_plan(int R, int C, int n_items, int T, Plan& pl) {
    if (!(C == 64 || C == 128 || C == 256) || R < 1 || T < 0 || n_items < 1 || n_items > MAX_ITEMS) return false;
    pl.nz = nz_of(C);
    const int ntile = (n_items + pl.nz - 1) / pl.nz;
    const int nrb = (R + qb_of(C) - 1) / qb_of(C);
    int want = std::max(std::max(256 / nrb, 1), (n_items + slice_cap(C) - 1) / slice_cap(C));
    want = std::min(want, ntile);
    pl.tps = (ntile + want - 1) / want;
    pl.nslices = (ntile + pl.tps - 1) / pl.tps;
    return true;
}

template <int C, int NZ, int NWS>
int launch(P p, const Plan& pl, hipStream_t st) {
    using G_ = Geo<C, NZ, NWS>;
    const dim3 grid(sweep_grid(p.R, G_::QB, pl.nslices));
    auto k = rank_sweep_kernel<C, NZ, NWS>;
    const int lds = G_::bytes(pl.tps * NZ);
    EDGL_REQUIRE(lds <= 160 * 1024, EDGL_ERR_SHAPE, "edgl_score_rank_fused: %d B of LDS", lds);
    EDGL_LDS_LIMIT(k, lds, "edgl_score_rank_fused");
    hipLaunchKernelGGL(k, grid, dim3(G_::NTHR), lds, st, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

}  // namespace evr

// 1 when the fused rank form takes this shape (bf16; C in {64, 128, 256}; 1 <= n_items <= 262144 per call), else 0: the caller runs
// the tile form (Base.py:150-201).  There is no silent fallback inside the library.
extern "C" int edgl_score_rank_supported(int R, int C, int n_items, int T, int dtype) {
    evr::Plan pl;
    return dtype == EDGL_BF16 && evr::make_plan(R, C, n_items, T, pl) ? 1 : 0;
}
// (the counts are added by integer atomics: the plan needs no scratch memory — 0 bytes for every shape it takes)
extern "C" long edgl_score_rank_workspace(int R, int C, int n_items, int T) {
    evr::Plan pl;
    return evr::make_plan(R, C, n_items, T, pl) ? 0 : -1;
}
extern "C" int edgl_score_rank_slices(int R, int C, int n_items, int T) {
    evr::Plan pl;
    return evr::make_plan(R, C, n_items, T, pl) ? pl.nslices : -1;
}

extern "C" int edgl_score_label_value(const void* rows, const void* table, const float* out_bias, const int64_t* seen, int T,
                                      const int64_t* labels, int R, int C, int I, float* label_val, int dtype, void* stream) {
    EDGL_REQUIRE(rows && table && out_bias && labels && label_val, EDGL_ERR_NULL, "edgl_score_label_value: null pointer");
    EDGL_REQUIRE(seen || T == 0, EDGL_ERR_NULL, "edgl_score_label_value: T > 0 without seen ids");
    EDGL_REQUIRE(dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_score_label_value: bf16 only (dtype %d)", dtype);
    EDGL_REQUIRE((C == 64 || C == 128 || C == 256) && R >= 1 && T >= 0 && I > 1, EDGL_ERR_SHAPE,
                 "edgl_score_label_value: shape not taken (R=%d C=%d I=%d T=%d; C in {64, 128, 256})", R, C, I, T);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((R + 31) / 32), block(64);
    const bf16 *x = (const bf16*)rows, *z = (const bf16*)table;
    if (C == 64) hipLaunchKernelGGL(evr::label_value_kernel<64>, grid, block, 0, st, x, z, out_bias, seen, T, labels, R, I, label_val);
    else if (C == 128) hipLaunchKernelGGL(evr::label_value_kernel<128>, grid, block, 0, st, x, z, out_bias, seen, T, labels, R, I, label_val);
    else hipLaunchKernelGGL(evr::label_value_kernel<256>, grid, block, 0, st, x, z, out_bias, seen, T, labels, R, I, label_val);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_score_rank_fused(const void* rows, const void* table, const float* out_bias, const int64_t* seen, int T,
                                     const int64_t* labels, const float* label_val, int R, int C, int I, int i0, int i1, int32_t* count,
                                     void* workspace, int dtype, void* stream) {
    (void)workspace;      // (edgl_score_rank_workspace is 0 bytes: may be NULL)
    EDGL_REQUIRE(rows && table && out_bias && labels && label_val && count, EDGL_ERR_NULL, "edgl_score_rank_fused: null pointer");
    EDGL_REQUIRE(seen || T == 0, EDGL_ERR_NULL, "edgl_score_rank_fused: T > 0 without seen ids");
    EDGL_REQUIRE(((uintptr_t)seen & 15) == 0, EDGL_ERR_SHAPE, "edgl_score_rank_fused: seen ids must be 16-byte aligned");
    EDGL_REQUIRE(dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_score_rank_fused: bf16 only (dtype %d)", dtype);
    EDGL_REQUIRE(I > 1 && i0 >= 0 && i1 <= I && i0 < i1 && i0 % 8 == 0, EDGL_ERR_SHAPE, "edgl_score_rank_fused: bad item range [%d, %d) of %d", i0, i1, I);
    evr::Plan pl;
    EDGL_REQUIRE(evr::make_plan(R, C, i1 - i0, T, pl), EDGL_ERR_SHAPE,
                 "edgl_score_rank_fused: shape not taken (R=%d C=%d items=%d T=%d; C in {64, 128, 256}, 1 <= items <= %d per call)", R, C,
                 i1 - i0, T, evs::MAX_ITEMS);
    evr::P p{};
    p.rows = (const bf16*)rows; p.table = (const bf16*)table; p.bias = out_bias; p.seen = seen; p.labels = labels; p.label_val = label_val;
    p.T = T; p.R = R; p.I = I; p.i0 = i0; p.i1 = i1; p.nslices = pl.nslices; p.tps = pl.tps; p.count = count;
    hipStream_t st = (hipStream_t)stream;
    return evs::sweep_dispatch(C, [&](auto g) { return evr::launch<g.C, g.NZ, g.NWS>(p, pl, st); });
}

extern "C" int edgl_label_value_tile(const float* logits, int R, int n, int i0, const int64_t* seen, int T, const int64_t* labels,
                                     float* label_val, void* stream) {
    EDGL_REQUIRE(logits && labels && label_val, EDGL_ERR_NULL, "edgl_label_value_tile: null pointer");
    EDGL_REQUIRE(seen || T == 0, EDGL_ERR_NULL, "edgl_label_value_tile: T > 0 without seen ids");
    EDGL_REQUIRE(R > 0 && n > 0 && T >= 0 && i0 >= 0 && i0 % 8 == 0, EDGL_ERR_SHAPE, "edgl_label_value_tile: bad shape R=%d n=%d i0=%d (i0 %% 8 == 0)", R, n, i0);
    hipLaunchKernelGGL(evr::label_value_tile_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, R, n, i0, seen, T,
                       labels, label_val);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_rank_count_tile(const float* logits, int R, int n, int i0, const int64_t* seen, int T, const int64_t* labels,
                                    const float* label_val, int32_t* count, void* stream) {
    EDGL_REQUIRE(logits && labels && label_val && count, EDGL_ERR_NULL, "edgl_rank_count_tile: null pointer");
    EDGL_REQUIRE(seen || T == 0, EDGL_ERR_NULL, "edgl_rank_count_tile: T > 0 without seen ids");
    EDGL_REQUIRE(R > 0 && n > 0 && T >= 0 && i0 >= 0 && i0 % 8 == 0, EDGL_ERR_SHAPE, "edgl_rank_count_tile: bad shape R=%d n=%d i0=%d (i0 %% 8 == 0)", R, n, i0);
    const int nseg = (n + evr::SEG - 1) / evr::SEG;
    EDGL_REQUIRE((long)R * nseg < (1L << 31), EDGL_ERR_SHAPE, "edgl_rank_count_tile: %ld workgroups", (long)R * nseg);
    hipLaunchKernelGGL(evr::rank_count_tile_kernel, dim3((unsigned)(R * nseg)), dim3(256), 0, (hipStream_t)stream, logits, R, n, i0, seen, T,
                       labels, label_val, count, nseg);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_rank_metrics_from_rank(const int32_t* rank, int R, const int32_t* ks, int nk, float* sums, void* stream) {
    EDGL_REQUIRE(rank && ks && sums, EDGL_ERR_NULL, "edgl_rank_metrics_from_rank: null pointer");
    EDGL_REQUIRE(R > 0 && nk >= 1 && nk <= 8, EDGL_ERR_SHAPE, "edgl_rank_metrics_from_rank: bad shape R=%d nk=%d (1 <= nk <= 8)", R, nk);
    hipLaunchKernelGGL(evr::rank_metrics_from_rank_kernel, dim3(1), dim3(512), 0, (hipStream_t)stream, rank, R, ks, nk, sums);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
