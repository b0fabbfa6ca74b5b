// The evaluation sweep shared by k_eval_topk.hip (K6f: group maxima, candidate runs) and k_eval_rank.hip (K6r: label rank counts):
// logits = rows . table^T + bias over an item range, formed tile by tile and never stored.
//   A workgroup = QB query rows (64; 128 at C = 256) x one item slice.  Item tiles of NZ rows stream through a double-buffered LDS
//   image (rows of C + 8 bf16: the 16-byte shift makes the 16-byte fragment reads conflict-free) with their bias row beside them; the
//   query rows stay in registers as MFMA B fragments; D[item][query] = Z . X^T with v_mfma_f32_32x32x16_bf16, the accumulator started
//   from the items' bias.  The items lie on the accumulator registers and the query on the lane: a lane's 16 values of an MFMA tile
//   belong to ONE row (register 4 j + i is the item at offset 8 j + 4 hi + i), so whatever a sweep does with them needs no
//   cross-lane traffic.  The workgroup is QB / 32 x NWS waves: 32 query rows x NZ / NWS items of a tile each.  bf16, C in {64, 128, 256}.
//   The tile ring: two register staging sets — the loads of tile t + 2 leave while tile t is multiplied and tile t + 1 waits in the
//   other set for its LDS buffer (with one set a workgroup had ONE 32 KB tile in flight per 2 us memory round trip: the sweep ran
//   at 9 % of the matrix pipe on a 1 M-item table).  One trip of the driver = two tiles, the second with the sets swapped (static
//   names: register arrays cannot be indexed by the trip's parity).  Out-of-range tiles are loaded clamped and never stored.
//   The rows' seen ids that fall into the slice are an LDS bitmap [QB][words], built under the second tile's loads: the ids of a
//   query block are one contiguous run of int64 (16-byte aligned), read as pairs, up to 16 loads in flight per thread — one memory
//   round trip at T = 101, two at T = 201 — and all loads of a batch out before the first LDS atomic (a load -> atomic loop is one
//   memory round trip per id: 25 per thread).
// Here: the constants, the tile's way global -> registers -> LDS, the workgroup placement, the query fragments and the chain.  The ring
// driver and the bitmap build are written out in eval_sweep_kernel AND rank_sweep_kernel (a fix goes into both): every shared form
// of them moved instructions, as did helpers that took a derived pointer or wrote through a reference — hence values in and out BY
// VALUE, the LDS image as smem + buffer index (profiles/eval_shared_header.txt).  The helpers are templates over the kernel's
// parameter struct: the structs stay apart, a kernel-argument layout belongs to its entry point.
#pragma once
#include "edgl_common.h"

typedef __attribute__((ext_vector_type(16))) float f32x16;

namespace evs {

// query rows per workgroup: 64; 128 at C = 256, where the table no longer fits an L2 at the catalogues this width is used with and
// every query block reads every slice again (1 M items x 512 B: the sweeps ran on the L2 -> LDS traffic of 8 query blocks)
__host__ __device__ constexpr int qb_of(int C) { return C == 256 ? 128 : 64; }
__host__ __device__ constexpr int nz_of(int C) { return C == 256 ? 64 : 128; }          // item rows of a tile
__host__ __device__ constexpr int slice_cap(int C) { return C == 256 ? 2048 : 4096; }   // items of a slice: 32 KB of seen bitmap per workgroup
constexpr int MAX_ITEMS = 262144;     // per call: 64 item slices of <= 4096 items

// NWS: waves across the items of a tile.  Four at C <= 128 — two waves per SIMD: the sweep's MFMA chains and what is done with their
// results are one dependent stream per wave, and a lone wave per SIMD has nothing to put into the other's shadow.  A kernel's Geo
// derives from this and lays its own LDS regions out from OFF_OWN.
template <int C_, int NZ_, int NWS_>
struct SweepGeo {
    static constexpr int C = C_, NZ = NZ_, NWS = NWS_;
    static constexpr int QB = qb_of(C);
    static constexpr int NTHR = 64 * (QB / 32) * NWS;
    static constexpr int LDZ = C + 8;                          // bf16 elements per LDS row
    static constexpr int ZB = NZ * LDZ * 2;
    static constexpr int OFF_Z = 0, OFF_BIAS = 2 * ZB, OFF_OWN = OFF_BIAS + 2 * NZ * 4;
    static constexpr int PIECES = NZ * C / 8 / NTHR;           // 16-byte pieces of an item tile per thread
};

// one item tile: global -> registers, unconditional loads with the rows clamped into the table (item 0 is the zero-padded row:
// coding.py:56-57); then registers -> LDS with the bias row (threads < NZ; EasyDGL.py:149-151): -1000 for item 0 (Base.py:106-113),
// -inf behind the range
template <int C, int NZ, int NWS, class PT>
__device__ __forceinline__ void tile_load(const PT& p, int item0, uint4 (&r)[SweepGeo<C, NZ, NWS>::PIECES], float& b) {
    constexpr int CP = C / 8, NTHR = SweepGeo<C, NZ, NWS>::NTHR;
#pragma unroll
    for (int j = 0; j < SweepGeo<C, NZ, NWS>::PIECES; ++j) {
        const int pc = threadIdx.x + NTHR * j, row = pc / CP, c8 = pc % CP;
        const int item = min(item0 + row, p.I - 1);
        r[j] = *reinterpret_cast<const uint4*>(p.table + (long)item * C + c8 * 8);
    }
    const int it = item0 + (int)threadIdx.x;
    b = (threadIdx.x < NZ && it < p.i1 && it > 0) ? p.bias[min(it, p.I - 1) - 1] : 0.f;
}
template <int C, int NZ, int NWS, class PT>
__device__ __forceinline__ void tile_store(const PT& p, int item0, uint4 (&r)[SweepGeo<C, NZ, NWS>::PIECES], float b, char* zbuf, float* bbuf) {
    constexpr int CP = C / 8, NTHR = SweepGeo<C, NZ, NWS>::NTHR;
#pragma unroll
    for (int j = 0; j < SweepGeo<C, NZ, NWS>::PIECES; ++j) {
        const int pc = threadIdx.x + NTHR * j, row = pc / CP, c8 = pc % CP;
        if (item0 + row == 0) r[j] = make_uint4(0u, 0u, 0u, 0u);
        *reinterpret_cast<uint4*>(zbuf + row * (SweepGeo<C, NZ, NWS>::LDZ * 2) + c8 * 16) = r[j];
    }
    if (threadIdx.x < NZ) {
        const int it = item0 + (int)threadIdx.x;
        bbuf[threadIdx.x] = it >= p.i1 ? -INFINITY : (it == 0 ? -1000.0f : b);
    }
}

// The workgroup's item slice and query block (first row = QB x the block); a slice >= nslices has no work (sweep_grid rounds up).
// XCD-aware order (speed only; observed placement: workgroup id b runs on XCD b % 8): the query blocks of ONE item slice are
// consecutive workgroups of ONE XCD, so that they run side by side and the slice's table rows come out of that XCD's L2 for all
// but the first of them — in (query block, slice) grid order the 8 query blocks of a slice sat on 8 XCDs and every one of them
// pulled the slice from HBM (1 M items: 8 x 512 MB per sweep)
template <int QB, class PT>
__device__ __forceinline__ int sweep_slice(const PT& p) {
    const int nqb = (p.R + QB - 1) / QB;
    const int xcd = (int)blockIdx.x & 7, jx = (int)blockIdx.x >> 3;
    return (jx / nqb) * 8 + xcd;
}
template <int QB, class PT>
__device__ __forceinline__ int sweep_qblock(const PT& p) {
    const int nqb = (p.R + QB - 1) / QB;
    const int jx = (int)blockIdx.x >> 3;
    return jx % nqb;
}
inline unsigned sweep_grid(int R, int QB, int nslices) { return 8u * ((R + QB - 1) / QB) * ((nslices + 7) / 8); }

// B fragment k of query row q (clamped into the batch) for lane half hi, from global memory (once per workgroup: no LDS image)
template <int C, class PT>
__device__ __forceinline__ bf16x8 query_frag(const PT& p, int q, int hi, int k) {
    const bf16* xrow = p.rows + (long)min(q, p.R - 1) * C + hi * 8;
    return *reinterpret_cast<const bf16x8*>(xrow + k * 16);
}

// THE chain (the arithmetic rule): a logit is its item's bias plus C / 16 of these, k ascending.  Every evaluation kernel
// that forms a logit on the matrix pipe does it through this function, so two of them give the same bits for the same (row, item).
__device__ __forceinline__ f32x16 score_step(const bf16x8& zf, const bf16x8& xf, const f32x16& acc) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(zf, xf, acc, 0, 0, 0);
}
// the 32 items from row m0 of LDS tile buffer `buf` against the wave's 32 query rows
template <int C, int NZ, int NWS>
__device__ __forceinline__ f32x16 score_tile(const char* smem, int buf, int m0, int l32, int hi, const bf16x8 (&xf)[C / 16]) {
    using G_ = SweepGeo<C, NZ, NWS>;
    const char* zb = smem + G_::OFF_Z + buf * G_::ZB;
    const float* bb = reinterpret_cast<const float*>(smem + G_::OFF_BIAS) + buf * NZ;
    f32x16 acc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {                     // D[m][n] starts from the item's bias: m = 8 j + 4 hi + i
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(bb + m0 + 8 * j + 4 * hi);
        acc[4 * j] = b4[0]; acc[4 * j + 1] = b4[1]; acc[4 * j + 2] = b4[2]; acc[4 * j + 3] = b4[3];
    }
#pragma unroll
    for (int k = 0; k < C / 16; ++k) {
        const bf16x8 zf = *reinterpret_cast<const bf16x8*>(zb + (m0 + l32) * (G_::LDZ * 2) + k * 32 + hi * 16);
        acc = score_step(zf, xf[k], acc);
    }
    return acc;
}

// the one list of instantiations: f(SweepGeo<C, NZ, NWS>{}) for the width C (64, 128 or 256: checked by the plans)
template <class F>
int sweep_dispatch(int C, F&& f) {
    if (C == 64) return f(SweepGeo<64, 128, 4>{});
    if (C == 128) return f(SweepGeo<128, 128, 4>{});
    return f(SweepGeo<256, 64, 2>{});
}

}  // namespace evs
