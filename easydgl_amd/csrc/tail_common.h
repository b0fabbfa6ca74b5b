// What at least two of the four block-tail kernels share (k_tail_fwd.hip: tail_fwd_kernel, t2::tail2_fwd_kernel; k_tail_bwd.hip:
// tail_bwd_kernel, t2::tail2_bwd_kernel): the parameter blocks, the LDS geometry of the one-per-CU form, the row-image copies, the
// MFMA tile product, the quad helpers and the joint (T, C) moments; and, for the host, the checks and the choice of instantiation.
#pragma once
#include <type_traits>

#include "edgl_common.h"

namespace {

#ifdef EDGL_PHASE_TIMING      // one set of slots per unit (forward, backward); see edgl_common.h (PH_MARK)
__device__ unsigned long long g_phase_cycles[16];
inline int tail_phase_cycles(unsigned long long* out16, int reset) {      // behind edgl_debug_phase_cycles_tail / _tail_bwd
    const unsigned long long z[16] = {0};
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_phase_cycles), sizeof(z)) != hipSuccess) return -1;
    return reset && hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles), z, sizeof(z)) != hipSuccess ? -1 : 0;
}
#endif

constexpr int MAXRT = 7;  // 16-row tiles per sample (T <= 112)
// GELU runs as its own pass over an f32 LDS image (gelu_pass), eight elements per thread in a loop that is not unrolled,
// with the one-rcp-one-exp erf of edgl_common.h, and the same pass writes gelu'(pre) — the only thing the backward needs the
// pre-activations for — in place of the pre-activations themselves, so the backward multiplies by a loaded tensor.  Inside
// the epilogues (on the accumulator registers) libm's erff cost ~400 issue cycles per element — 28 % of the forward, 40 %
// of the backward — and the inlined fast form spilled there: the scheduler interleaves all 28 chains of a phase (~80 more
// registers), and with a scheduling fence per row tile the z / acc state still went to scratch (forward 84 -> 88 us,
// backward 120 -> 138 us).  Computing gelu' in the backward's input copy (fast form, 32 per thread and image) still cost
// 7 k of the 60 k cycles of a block, three to five times per step.

struct TailP {
    const bf16* att; const bf16* xin; int ld_x;
    const bf16 *WoT, *WiT, *WoutT, *WtT;            // packed [N][K] images (k contiguous)
    const float *bo, *bi, *bout, *bt, *g1, *b1, *g2, *b2, *g3, *b3;
    int B, T, C;
    float rate; const uint64_t* rng; uint32_t sid1, sid2;
    const int64_t* mpos; int M; int head; const int32_t* hmap;   // hmap: optional destination row of head row b*M + j (< 0: dropped)
    bf16 *ao, *a1, *pre_f, *f, *o, *y, *pre_t, *so, *hrows;   // pre_f / pre_t receive gelu'(pre-activation)
    float *st1, *st2, *st3;
    int dhp, dht;   // channel-padded model (head dim dht stored as dhp, the padded channels all zero): the LayerNorms' moments are
                    // those of the real channels (edgl_tail_fwd_ct); 0, 0: none
};
struct TailBwdP {
    // saved by the forward
    const bf16 *xin; int ld_x;
    const bf16 *ao, *a1, *pre_f, *o, *pre_t, *so;   // pre_f / pre_t: gelu'(pre-activation), as edgl_tail_fwd wrote them
    const float *st1, *st2, *st3;
    const bf16 *Wo, *Wi, *Wout, *Wt;          // [in, out] compute copies
    const float *g1, *g2, *g3;
    int B, T, C;
    float rate; const uint64_t* rng; uint32_t sid1, sid2;
    int head;
    const bf16* d_rows; const int64_t* mpos; int M; const int32_t* rowmap;   // head: compact row gradients, positions, inv map
    const bf16* d_y_in;                                                       // head == 0: gradient w.r.t. y [B,T,C]
    // outputs
    bf16 *d_pre_t, *d_o, *d_pre_f, *d_ao, *d_res1, *d_att;
    float *part1, *part2, *part3;             // [B][2C] (dbeta | dgamma) of LN1 / LN2 / LN3
    int dhp, dht;                             // channel-padded model: see TailP
};

template <int CT>
struct TailGeom {
    static constexpr int C = 16 * CT, NW = CT, NTHR = 64 * CT, LD = C + 8, CV = C / 8;
    static constexpr int LDF = C + 4;                                  // f32 staging image [112][LDF] over buffers A + S
    static constexpr size_t BUF = (size_t)MAXRT * 16 * LD * sizeof(bf16);
    static_assert((size_t)MAXRT * 16 * LDF * sizeof(float) <= 2 * BUF, "f32 staging image exceeds two buffers");
    static constexpr size_t SMEM = 4 * BUF + 64 * sizeof(float);
    static constexpr size_t SMEM_BWD = SMEM + (size_t)(MAXRT * 16 + 512) * sizeof(int);   // + rowmap [112] + nextj, positions [<= 256 each]
    // forward: + the parameter vectors bo | bout | g1 | b1 | g2 | b2 | g3 | b3 | bt | bi (2C)   (see "waits" in tail_fwd_kernel)
    static constexpr int PAR_BO = 0, PAR_BOUT = 1, PAR_G1 = 2, PAR_B1 = 3, PAR_G2 = 4, PAR_B2 = 5, PAR_G3 = 6, PAR_B3 = 7, PAR_BT = 8, PAR_BI = 9;
    static constexpr size_t SMEM_FWD = SMEM + (size_t)11 * C * sizeof(float);
};

// rows [0, T) of a [T, C] global tensor (row stride ld) -> LDS image [112][LD]; rows >= T are zero.  load() issues every
// 16-byte vector of the image, store() writes them to the LDS: all loads of a phase — of BOTH its images — go out before the
// first store (a load / store loop pays one HBM round trip per 8 KB of a 512-thread workgroup, two copies one after the
// other pay two).  Straight-line code: rows are clamped, and the threads that have no vector of their own in the last round
// repeat one of the same round (same data to the same address) — a guard there puts the load and its wait inside a branch.
template <int CT>
struct RowImage {
    using G = TailGeom<CT>;
    static constexpr int NV = MAXRT * 16 * G::CV, NI = (NV + G::NTHR - 1) / G::NTHR;
    static_assert(NI * G::NTHR - NV < G::NTHR && NV >= G::NTHR, "last round: at most one repeat per thread");
    uint4 d[NI];
    static __device__ __forceinline__ int vec(int i) {
        const int v = threadIdx.x + i * G::NTHR;
        return v < NV ? v : v - (NI * G::NTHR - NV);
    }
    __device__ __forceinline__ void load(const bf16* src, long ld, int T) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int v = vec(i), row = v / G::CV, cv = v % G::CV;
            d[i] = *reinterpret_cast<const uint4*>(src + (long)min(row, T - 1) * ld + cv * 8);
        }
    }
    __device__ __forceinline__ void store(bf16* dst, int T) const {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int v = vec(i), row = v / G::CV, cv = v % G::CV;
            *reinterpret_cast<uint4*>(dst + row * G::LD + cv * 8) = row < T ? d[i] : make_uint4(0, 0, 0, 0);
        }
    }
};
template <int CT>
__device__ __forceinline__ void copy_in(bf16* dst, const bf16* src, long ld, int T) {
    RowImage<CT> a;
    a.load(src, ld, T);
    a.store(dst, T);
}
template <int CT>
__device__ __forceinline__ void copy_in2(bf16* dst0, const bf16* src0, long ld0, bf16* dst1, const bf16* src1, long ld1, int T) {
    RowImage<CT> a, b;
    a.load(src0, ld0, T);
    b.load(src1, ld1, T);
    a.store(dst0, T);
    b.store(dst1, T);
}
template <int CT>
__device__ __forceinline__ void copy_out(bf16* dst, long ld, const bf16* src, int T) {
    using G = TailGeom<CT>;
    for (int v = threadIdx.x; v < T * G::CV; v += G::NTHR) {
        const int row = v / G::CV, cv = v % G::CV;
        *reinterpret_cast<uint4*>(dst + (long)row * ld + cv * 8) = *reinterpret_cast<const uint4*>(src + row * G::LD + cv * 8);
    }
}

// acc[rt] += W^T[n-tile rows][k0 .. k0 + 32*NKB) . X[rows of tile rt][same k]   (WT row stride ldw, X image stride LD)
// The weight fragments of a wave's 16 output channels (global, L2-resident) are fetched ahead of the product that uses
// them — one product early, under the epilogue / LayerNorm / copy-out of the previous step — so that no product of the
// chain opens with an L2 round trip (8 waves per CU: nothing else would hide it).
template <int NKB>
struct WFrags { Vec16<bf16> w[NKB]; };
template <int NKB>
__device__ __forceinline__ WFrags<NKB> load_wfrags(const bf16* WTrows, int ldw, int lane) {
    const int l15 = lane & 15, kg = (lane >> 4) * 8;
    WFrags<NKB> f;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) f.w[kb] = ld16<bf16>(WTrows + (long)l15 * ldw + kb * 32 + kg);
    return f;
}
template <int CT, int NKB>
__device__ __forceinline__ void tile_gemm(const WFrags<NKB>& wf, const bf16* Xs, int nrt, int lane, f32x4 (&acc)[MAXRT]) {
    using G = TailGeom<CT>;
    const int l15 = lane & 15, kg = (lane >> 4) * 8;
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt) {
        if (rt < nrt) {
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
                acc[rt] = mma_kblock(wf.w[kb], ld16<bf16>(Xs + (rt * 16 + l15) * G::LD + kb * 32 + kg), acc[rt]);
        }
        // at most two row tiles' operand reads in flight: unbounded, the scheduler hoists all 7 x NKB LDS reads (112+
        // registers) above the first MFMA
        // (four or all seven tiles per batch: +-0, measured)
        if (rt & 1) __builtin_amdgcn_sched_barrier(0);
    }
}

__device__ __forceinline__ void st_bf4(bf16* dst, const float (&v)[4]) {
    const Frag4<bf16> f = frag_from_acc<bf16>(f32x4{v[0], v[1], v[2], v[3]});
    *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(&f);
}
__device__ __forceinline__ void ld_bf4(const bf16* src, float (&v)[4]) {
    const Frag4<bf16> f = frag_ld<bf16>(src);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = to_f32(f.v[r]);
}
__device__ __forceinline__ float rbf(float x) { return to_f32(from_f32<bf16>(x)); }   // round through the activation dtype

// Workgroup sum through LDS with LDS-scoped barriers only: __syncthreads() also drains vmcnt, i.e. it would wait for the
// copy_out stores still in flight (a full HBM write latency at every step of the chain).
__device__ __forceinline__ float block_sum_lds(float v, float* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    lds_barrier();
    if (lane == 0) red[w] = v;
    lds_barrier();
    float t = 0.f;
    for (int i = 0; i < nw; ++i) t += red[i];
    return t;
}

// joint (T, C) moments of the values z[rt][r] held by the workgroup (rows >= T excluded): two passes, as tf.nn.moments
// Channel-padded models (dhp > 0: head dim dht stored as dhp; edgl_add_layernorm_*_ct in k_layernorm.hip): the moments are those of
// the REAL channels — divisor T * C_true, padded entries (exact zeros) left out of the centred second moment.
struct ChanPad {
    float rm[4];      // 1 for a real channel of this lane's four, 0 for a padded one
    float ctrue;      // real channels of the model width
};
template <int CT>
__device__ __forceinline__ ChanPad chan_pad(int nl, int dhp, int dht) {
    ChanPad cp;
#pragma unroll
    for (int r = 0; r < 4; ++r) cp.rm[r] = (dhp <= 0 || ((nl + r) & (dhp - 1)) < dht) ? 1.f : 0.f;      // (dhp is a power of two)
    cp.ctrue = dhp > 0 ? (float)((16 * CT) / dhp * dht) : (float)(16 * CT);
    return cp;
}
template <int CT>
__device__ __forceinline__ void joint_moments(const float (&z)[MAXRT][4], int nrt, int T, int lane, float* red, float& mean, float& rstd,
                                              const ChanPad& cp) {
    const int l15 = lane & 15;
    const float n = (float)T * cp.ctrue;
    float a = 0.f;
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt)
        if (rt < nrt && rt * 16 + l15 < T) a += (z[rt][0] * cp.rm[0] + z[rt][1] * cp.rm[1]) + (z[rt][2] * cp.rm[2] + z[rt][3] * cp.rm[3]);
    mean = block_sum_lds(a, red) / n;
    a = 0.f;
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt)
        if (rt < nrt && rt * 16 + l15 < T) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float d = (z[rt][r] - mean) * cp.rm[r]; a += d * d; }
        }
    rstd = rsqrtf(block_sum_lds(a, red) / n + 1e-12f);
}

// ---- host side: what edgl_tail_fwd_ct and edgl_tail_bwd_ct check and choose alike ----------------------------------------
// shape rule, dropout state and padded-channel spec of both directions; `who` names the entry point, `forms` ends its shape message
inline int tail_check(const char* who, const char* forms, int B, int T, int C, int ld_x, int dtype, float drop_rate,
                      const uint64_t* rng_state, int dh_pad, int dh_true) {
    EDGL_REQUIRE(B > 0 && edgl_tail_supported(T, C, dtype) && ld_x % 8 == 0, EDGL_ERR_SHAPE,
                 "%s: unsupported shape B=%d T=%d C=%d dtype=%d%s", who, B, T, C, dtype, forms);
    EDGL_REQUIRE(drop_rate == 0.f || rng_state, EDGL_ERR_NULL, "%s: dropout without rng_state", who);
    EDGL_REQUIRE((dh_pad == 0 && dh_true == 0) || (dh_pad > 0 && (dh_pad & (dh_pad - 1)) == 0 && dh_true > 0 && dh_true <= dh_pad && C % dh_pad == 0),
                 EDGL_ERR_SHAPE, "%s: padded-channel spec dh_pad=%d dh_true=%d does not fit C=%d", who, dh_pad, dh_true, C);
    return EDGL_OK;
}
// the instantiation that serves T rows: `inst` maps the row-tile count NRT (integral constant 2, 4 or MAXRT) to its kernel
template <class F>
auto tail_pick_nrt(int T, F inst) {
    const int nrt = (T + 15) / 16;
    return nrt <= 2 ? inst(std::integral_constant<int, 2>()) : nrt <= 4 ? inst(std::integral_constant<int, 4>()) : inst(std::integral_constant<int, MAXRT>());
}

}  // namespace
