// =========================================================================================================================
// Two workgroups per CU ("t2", C = 128, T <= 101): the same chain on HALF the CU.
// tail_fwd_kernel and tail_bwd_kernel own a CU — 122 KB of LDS, 256 registers per wave — so the 512 samples of the benchmark run as two lock-stepped
// rounds of 256 workgroups, every phase of a sample a dependent round trip (L2 / HBM / LDS hand-over / barrier) with nothing on
// the CU to run in the gaps: 50-53 % of the wave cycles parked, the matrix pipe 6 % busy (DESIGN.md rule 53).  At C = 64 two of the
// 4-wave workgroups already fit a CU, and there the second one costs 32 % more time, not 100 % (tools/tail_probe.py: 22.9 us for
// 256 samples, 30.2 us for 512).  This form gives the C = 128 kernel the same second, independent chain:
//   * three LDS images [101][128] bf16, UNPADDED (256-byte rows) with an XOR swizzle — 16-byte chunk c of row r at c ^ (r & 15) — in
//     place of four padded ones + an f32 image: 3 x 25 856 + 256 + 4 096 = 81 920 bytes = half the CU's LDS.  The swizzle is
//     conflict-free for all three access shapes: MFMA operand reads (16 lanes = 16 rows of one chunk column), the 8-byte quads of
//     the accumulator layout (32 lanes = 16 rows x 2 halves of one chunk), whole rows (any permutation);
//   * the f32 pre-activations of a GELU pass go through TWO of the images ([101][128] f32, same swizzle on its 16-byte chunks);
//     the pass loads its values, and — where the f image lands in the staging area itself — waits for everybody's loads before
//     storing (one more barrier per half of the hidden layer);
//   * <= 128 registers (4 waves per SIMD): no operand is prefetched a whole segment ahead — the other workgroup of the CU is
//     what runs while a load is in flight —, the LayerNorm inputs of the backward come straight from global memory in the
//     accumulator layout (8 bytes per lane and row tile) instead of through LDS images held in registers one phase ahead.
// Same arithmetic, in the same order, as those kernels: the outputs are bit-identical (tests/test_gpu_tail2.py,
// tests/test_gpu_tail_bwd2.py).
// =========================================================================================================================
#pragma once
#include "tail_common.h"

namespace {
namespace t2 {
constexpr int C = 128, NTHR = 512, NKB = 4, TMAX = 101;
constexpr int IMG = TMAX * 256;                                      // one bf16 image
constexpr int OFF_RED = 3 * IMG, OFF_PAR = OFF_RED + 256;
constexpr int PAR_BOUT = 0, PAR_G2 = 1, PAR_B2 = 2, PAR_G3 = 3, PAR_B3 = 4, PAR_BI = 5, PAR_BT = 7, NPAR = 8;      // (bi: two vectors)
constexpr int SMEM_FWD = OFF_PAR + NPAR * C * 4;
static_assert(SMEM_FWD == 81920, "two workgroups per CU");
constexpr int OFF_ROWMAP = OFF_RED + 256, OFF_NEXTJ = OFF_ROWMAP + MAXRT * 16 * 4, OFF_MPOS = OFF_NEXTJ + 256 * 4;
constexpr int SMEM_BWD = OFF_MPOS + 256 * 4;
static_assert(SMEM_BWD <= 81920, "two workgroups per CU");
constexpr int OFF_GAM = SMEM_BWD, SMEM_BWD_ALL = 81920;      // g1 | g2 | g3 behind the chain tables; the launch asks for half a CU:
static_assert(OFF_GAM + 3 * C * 4 <= SMEM_BWD_ALL, "gamma table");
// a product reads whole row tiles: over image R the rows >= T of the last tile lie in the tables behind it (read only; every consumer
// of those rows is guarded) — they must stay inside the allocation
static_assert(2 * IMG + MAXRT * 4096 <= SMEM_BWD_ALL && 2 * IMG + MAXRT * 4096 <= SMEM_FWD, "operand reads of rows >= T leave the workgroup's LDS");

struct Lane {
    int lane, wave, q, l15, nl;
    int frag[NKB];      // byte offset of this lane's MFMA operand chunk of k-block kb in row l15 of an image (+ rt * 4096)
    int quad;           // byte offset of this lane's 4 channels in row l15 of an image (+ rt * 4096)
    int squad;          // the same in the f32 staging image (+ rt * 8192)
};
__device__ __forceinline__ Lane make_lane(int tid) {
    Lane L;
    L.lane = tid & 63; L.wave = tid >> 6; L.q = L.lane >> 4; L.l15 = L.lane & 15; L.nl = L.wave * 16 + L.q * 4;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) L.frag[kb] = L.l15 * 256 + (((kb * 4 + L.q) ^ L.l15) << 4);
    L.quad = L.l15 * 256 + (((L.wave * 2 + (L.q >> 1)) ^ L.l15) << 4) + ((L.q & 1) << 3);
    L.squad = L.l15 * 512 + (((L.wave * 4 + L.q) ^ L.l15) << 4);
    return L;
}
__device__ __forceinline__ Lane make_lane() { return make_lane(threadIdx.x); }
// The same, rebuilt from an opaque copy of the thread index: the backward keeps no operand offset alive from one segment to the next
// (held for the whole kernel they went to scratch, and a reload from scratch waits on vmcnt like any load — behind the stores)
__device__ __forceinline__ int fresh_tid() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}
__device__ __forceinline__ Lane fresh_lane() { return make_lane(fresh_tid()); }
__device__ __forceinline__ int vec_off(int row, int cv) { return row * 256 + ((cv ^ (row & 15)) << 4); }

// acc[rt] += W^T[16 output channels][128 k] . X[rows of tile rt][k] over a swizzled image.  Rows >= T of the last tile(s) read
// whatever lies there (inside the workgroup's LDS): an MFMA output row depends on its own input row only, and every consumer
// of rows >= T is guarded.
template <int NRT>
__device__ __forceinline__ void gemm(const WFrags<NKB>& wf, const char* img, const Lane& L, f32x4 (&acc)[MAXRT]) {
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) {
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
            acc[rt] = mma_kblock(wf.w[kb], *reinterpret_cast<const Vec16<bf16>*>(img + L.frag[kb] + rt * 4096), acc[rt]);
        __builtin_amdgcn_sched_barrier(0);      // one row tile's operand reads in flight (16 registers)
    }
}
template <int NRT>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[MAXRT]) {
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
}
// global [T, 128] (row stride ld) -> image; every load of BOTH images in flight before the first store (clamped tail vectors
// repeat the last one: same data to the same address)
__device__ __forceinline__ void copy_in2(char* d0, const bf16* s0, long ld0, char* d1, const bf16* s1, long ld1, int T) {
    uint4 a[4], b[4];
    const int nv = T * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = min((int)threadIdx.x + i * NTHR, nv - 1), row = v >> 4, cv = v & 15;
        a[i] = *reinterpret_cast<const uint4*>(s0 + (long)row * ld0 + cv * 8);
        b[i] = *reinterpret_cast<const uint4*>(s1 + (long)row * ld1 + cv * 8);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = min((int)threadIdx.x + i * NTHR, nv - 1), row = v >> 4, cv = v & 15;
        *reinterpret_cast<uint4*>(d0 + vec_off(row, cv)) = a[i];
        *reinterpret_cast<uint4*>(d1 + vec_off(row, cv)) = b[i];
    }
}
// image -> global [T, 128] (row stride ld): uniform base + 32-bit lane offset, the thread's offsets rebuilt by every call
__device__ __forceinline__ void copy_out(bf16* dst, int ld, const char* img, int T) {
    const int nv = T * 16, tid = fresh_tid();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = tid + i * NTHR, row = v >> 4, cv = v & 15;
        if (v < nv) *reinterpret_cast<uint4*>(reinterpret_cast<char*>(dst) + (uint32_t)((row * ld + cv * 8) * 2)) = *reinterpret_cast<const uint4*>(img + vec_off(row, cv));
    }
}

}  // namespace t2
}  // namespace
