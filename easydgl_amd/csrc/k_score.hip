// K5: tied-embedding scoring against the item table.  (The rows around the loss — compaction, CE loss — are k_ce.hip; evaluation
// on a materialised logits tile, K6 / K7, is k_eval_tile.hip.)
//   logits[r, n] = rows[r,:] . table[n,:] + bias[n]   (EasyDGL.py:149-150; table row 0 acts as zeros,
//   bias = concat([-1000], output_bias) — coding.py:56-57, Base.py:106-110)
// Training never materialises the [R, I] logits: the forward keeps an online (max, sum-exp) per row
// (EasyDGL.py:155), the backward recomputes logit tiles and feeds dl = coef*(p - onehot) straight back into
// MFMA as an operand.  All three kernels share one structure:
//   * a workgroup = 8 waves (512 threads) owns 256 "x" vectors (rows, or table rows) whose MFMA fragments
//     stay in REGISTERS for the whole kernel; each wave owns a 32-x strip and the full width of every
//     streamed tile, so no cross-wave reduction is ever needed;
//   * the other operand ("z": item tiles, or row tiles) streams through LDS in 128-z tiles, double buffered,
//     prefetched through registers, one barrier per tile;
//   * logit tile in the swapped orientation  D[z][x]  (register layout L(first=z, second=x)), so that dl is
//     directly the A operand of the second product  out[x][c] += sum_z dl[x][z] Z[z][c]; its B operand (z along
//     the contraction) comes out of the SAME row-major LDS tile through gfx950's transpose read
//     (ds_read_b64_tr_b16, bf16) — one image per tile, no transposed copies of the operands in HBM.  f32 has no
//     32-bit transpose read: there a second LDS image in [c][z] order is filled from a pre-transposed copy
//     (tableT [C][ldt] / rowsT [C][ldr]).
//   score_fwd_kernel : x = rows,  z = items   -> per-chunk (max, sumexp) [+ optional logits]
//   score_bwd<ROLE_Y>: x = rows,  z = items   -> d_rows slabs
//   score_bwd<ROLE_W>: x = items, z = rows    -> d_table slabs, d_bias slabs
#include <cstdlib>
#include <mutex>
#include <unordered_map>

#include "edgl_common.h"
#include "score_plan.h"
#include "score_strip.h"

namespace {

constexpr int SNT = 512;   // threads per workgroup of the forward kernel

// Tile shape per (dtype, C).  C <= 128 (and bf16 C = 256): a wave keeps TWO 16-x tiles in registers and 128-z tiles stream
// through LDS.  Wider rows (bf16 C = 512 — every published recipe, runme.sh:15-115; f32 C = 256 / 512 for parity runs) keep
// ONE x tile per wave (its fragments alone are 64-128 registers) and stream narrower z tiles so that the Z / Z^T images of
// a tile still fit the 160 KB of LDS.
template <typename T, int CT>
struct ScoreCfg {
    static constexpr bool BF = sizeof(T) == 2;
    static constexpr bool STD = CT <= 8 || (BF && CT == 16);
    static constexpr int IX = STD ? 2 : 1;                                   // 16-x tiles per wave
    static constexpr int ZB = STD ? 128 : ((BF || CT == 16) ? 64 : 32);      // z vectors per streamed tile
    static constexpr int NWB = (!BF && CT == 32) ? 4 : 8;                    // waves per workgroup, backward kernels
    // output channel tiles per backward pass: bf16 C = 256 / 512 accumulate half the channels per pass (the logits are
    // recomputed per pass) — all [IX][CT] accumulator tiles next to the x fragments spill ~100-300 registers
    static constexpr int CO = (BF && CT >= 16) ? CT / 2 : CT;
};
struct RtCfg { int ix, zb, nwb; };
inline RtCfg rt_cfg(int C, size_t esize) {   // the same table for the host-side planners
    const int ct = C / 16;
    const bool bf = esize == 2, stdc = ct <= 8 || (bf && ct == 16);
    return RtCfg{stdc ? 2 : 1, stdc ? 128 : ((bf || ct == 16) ? 64 : 32), (!bf && ct == 32) ? 4 : 8};
}

template <typename T, int CT, int NTHR = SNT, int ZBT = ScoreCfg<T, CT>::ZB>
struct SC {
    static constexpr int ZB = ZBT;
    static constexpr int VEC = ElemTraits<T>::VEC;
    static constexpr int KB = ElemTraits<T>::KB;
    static constexpr int C = 16 * CT;
    static constexpr int NKB = C / KB;
    static constexpr int LDC = C + 2 * VEC;   // Z  image: [ZB][LDC]   (row z, k contiguous); +32 B: conflict-free b128 reads
    static constexpr int LDZ = ZB + VEC;      // ZT image: [C][LDZ]    (row c, z contiguous)
    static constexpr int CV = C / VEC;
    static constexpr int PER_Z = ZB * CV / NTHR;          // 16-byte vectors per thread, Z image
    static constexpr int PER_ZT = C * (ZB / VEC) / NTHR;  // same count, ZT image
    static constexpr size_t Z_BYTES = (size_t)ZB * LDC * sizeof(T);
    // second image of the tile in [c][z] order: f32 only — bf16 fetches the z-contracting operand of the second product from
    // the Z image itself with the LDS transpose read (ds_read_b64_tr_b16; row stride LDC * 2 B = 8 banks mod 64: conflict-free)
    static constexpr bool WT = sizeof(T) == 4;
    static constexpr size_t ZT_BYTES = WT ? (size_t)C * LDZ * sizeof(T) : 0;
    static constexpr size_t INFO_BYTES = 3 * ZB * sizeof(float);
    static constexpr int JH = ZB >= 64 ? 4 : ZB / 16;     // 16-z tiles per "half" (the unit whose logits are live at once)
    static constexpr int NH = ZB / 16 / JH;               // halves per streamed tile
    static_assert(PER_Z >= 1 && PER_ZT >= 1 && ZB % 16 == 0, "tile does not divide over the workgroup");
};

typedef __attribute__((ext_vector_type(4))) short sc_s16x4;
// B operand of a 16x16x32 MFMA whose contraction index runs along the ROWS of a row-major bf16 LDS tile (rows k0 .. k0+31,
// columns z0 .. z0+15): slots 0-3 <-> k0 + 4G + j, slots 4-7 <-> k0 + 16 + 4G + j (G = lane >> 4) — the order in which the
// dl fragment is packed from the logit accumulators (see csrc/k_gemm2.hip for the measured lane map of the instruction)
__device__ __forceinline__ bf16x8 sc_tr_frag32(const bf16* tile, int ld, int k0, int z0, int lane) {
    const int G = lane >> 4, sl = lane & 15;
    const bf16* p = tile + (k0 + 4 * G + (sl >> 2)) * ld + z0 + 4 * (sl & 3);
    bf16x8 f;
    sc_s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) sc_s16x4*)p);
    sc_s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) sc_s16x4*)(p + 16 * ld));
    *reinterpret_cast<uint2*>(&f) = *reinterpret_cast<uint2*>(&v0);
    *(reinterpret_cast<uint2*>(&f) + 1) = *reinterpret_cast<uint2*>(&v1);
    return f;
}

struct ScoreP {
    const void* rows; const void* rowsT; int ldr;      // rows [R][C], rowsT [C][ldr]
    const void* table; const void* tableT; int ldt;    // table [I][C], tableT [C][ldt]
    const float* out_bias; const int64_t* labels;
    int R, C, I, i0, i1;
    const int32_t* nvalid;                              // optional device count: only rows < *nvalid carry weight
    float* row_lse; float* part; float* logits;         // fwd
    int zchunk, nchunk;                                 // z vectors per block (multiple of ZB), #chunks
    const float* coef; const float* gscale;             // bwd
    float* slabs; float* bias_slabs;
    float* lab_out;                                     // flash forward: label logits [R]
    float* coef_out;                                    // flash forward, compacted rows, whole table: loss coefficients [R]
    int table_ready;                                    // tableT already written by edgl_score_prepare_table
    const int32_t* wtotal;                              // data parallel: weighted rows of the GLOBAL batch (denominator of the loss)
    bool defer_label;                                   // strip path: the caller applies the one-hot term (edgl_score_flash_label_term)
    bool acc_atomic;                                    // strip path: d_table / d_bias are zero-filled and take the chunks as f32 atomics
    bool keep_slabs;                                    // the row-chunk slabs of d_table / d_bias stay in the workspace: no slab_reduce launch (edgl_adam_apply_ex sums them)
    float* ce_part;                                     // one-launch row finish: per-workgroup sums of -log(p_label + 1e-5) (edgl_score_ce_nparts)
};

// ---- streamed tile: global -> registers -> LDS -------------------------------------------------
template <typename T, int CT, bool WITH_T, int NTHR = SNT>
struct ZStream {
    using S = SC<T, CT, NTHR>;
    Vec16<T> rz[S::PER_Z];
    Vec16<T> rt[WITH_T ? S::PER_ZT : 1];
    int z0_, zend_;      // tile start / chunk end of the rows in flight
    bool zero0_;
    // Z image rows [z0, z0+ZB) of src [*, C]; rows >= zend (or global row 0 when zero_row0) read as zeros.
    // The loads are UNCONDITIONAL (addresses clamped into the valid range) and the zeroing happens in store(): a
    // per-lane branch around a load makes the compiler wait for that load inside the branch, which serialises the
    // whole prefetch (one full memory latency per slot).
    __device__ __forceinline__ void load(const T* src, const T* srcT, int ldT, int z0, int zend, bool zero_row0) {
        load_z(src, z0, zend, zero_row0);
        load_t(srcT, ldT, z0, zend, zero_row0);
    }
    __device__ __forceinline__ void load_z(const T* src, int z0, int zend, bool zero_row0) {
        z0_ = z0; zend_ = zend; zero0_ = zero_row0;
#pragma unroll
        for (int i = 0; i < S::PER_Z; ++i) {
            const int v = threadIdx.x + i * NTHR;
            const int row = v / S::CV, cv = v % S::CV, gz = min(z0 + row, zend - 1);
            rz[i] = ld16<T>(src + (long)gz * S::C + cv * S::VEC);
        }
    }
    __device__ __forceinline__ void load_t(const T* srcT, int ldT, int z0, int zend, bool zero_row0) {
        if constexpr (WITH_T) {
            z0_ = z0; zend_ = zend; zero0_ = zero_row0;
            constexpr int ZV = S::ZB / S::VEC;
#pragma unroll
            for (int i = 0; i < S::PER_ZT; ++i) {
                const int v = threadIdx.x + i * NTHR;
                const int c = v / ZV, zv = v % ZV, gz = min(z0 + zv * S::VEC, ldT - S::VEC);   // ldT is a multiple of VEC
                rt[i] = ld16<T>(srcT + (long)c * ldT + gz);
            }
        }
    }
    __device__ __forceinline__ void store(T* Zs, T* ZTs) {
#pragma unroll
        for (int i = 0; i < S::PER_Z; ++i) {
            const int v = threadIdx.x + i * NTHR;
            const int gz = z0_ + v / S::CV;
            const bool ok = gz < zend_ && !(zero0_ && gz == 0);
            st16<T>(Zs + (v / S::CV) * S::LDC + (v % S::CV) * S::VEC, ok ? rz[i] : zero16<T>());
        }
        if constexpr (WITH_T) {
            constexpr int ZV = S::ZB / S::VEC;
#pragma unroll
            for (int i = 0; i < S::PER_ZT; ++i) {
                const int v = threadIdx.x + i * NTHR;
                const int gz = z0_ + (v % ZV) * S::VEC;
                Vec16<T> t = rt[i];
                if (gz + S::VEC > zend_ || (zero0_ && gz == 0)) {   // only the last tile of a chunk / the tile holding row 0
#pragma unroll
                    for (int j = 0; j < S::VEC; ++j)
                        if (gz + j >= zend_ || (zero0_ && gz + j == 0)) t.v[j] = from_f32<T>(0.f);
                }
                st16<T>(ZTs + (v / ZV) * S::LDZ + (v % ZV) * S::VEC, t);
            }
        }
    }
};

// x fragments of this wave's 32-x strip, kept in registers.  Two halves: issue_xfrags() sends every load (row clamped,
// unconditional), finish_xfrags() — called after the first streamed tile's loads have been issued as well — zeroes the
// fragments of rows past the end.  `ok ? load : zero` compiles to a branch around each load with its own wait: IX * NKB
// dependent round trips at the head of the kernel (8 at C = 128).
template <typename T, int CT, int IX>
__device__ __forceinline__ void issue_xfrags(const T* X, int x0, int xend, int lane, Vec16<T> (&xf)[IX][SC<T, CT>::NKB]) {
    using S = SC<T, CT>;
#pragma unroll
    for (int ix = 0; ix < IX; ++ix) {
        const int gx = max(min(x0 + ix * 16 + (lane & 15), xend - 1), 0);
#pragma unroll
        for (int kb = 0; kb < S::NKB; ++kb) xf[ix][kb] = ld16<T>(X + (long)gx * S::C + kb * S::KB + (lane >> 4) * S::VEC);
    }
}
template <typename T, int CT, int IX>
__device__ __forceinline__ void finish_xfrags(int x0, int xend, bool zero_row0, int lane, Vec16<T> (&xf)[IX][SC<T, CT>::NKB]) {
    using S = SC<T, CT>;
#pragma unroll
    for (int ix = 0; ix < IX; ++ix)
#pragma unroll
        for (int kb = 0; kb < S::NKB; ++kb) {      // the loaded values are "used" here: the loads cannot sink into a branch
            uint4& u = *reinterpret_cast<uint4*>(&xf[ix][kb]);
            asm volatile("" : "+v"(u.x), "+v"(u.y), "+v"(u.z), "+v"(u.w));
        }
#pragma unroll
    for (int ix = 0; ix < IX; ++ix) {
        const int gx = x0 + ix * 16 + (lane & 15);
        const bool ok = gx < xend && !(zero_row0 && gx == 0);
#pragma unroll
        for (int kb = 0; kb < S::NKB; ++kb) xf[ix][kb] = ok ? xf[ix][kb] : zero16<T>();
    }
}

// D[z][x] half tile of the wave (64 z = 4 jz tiles starting at jz0): acc[j][ix], L(first = z, second = x).
// The 128-z tile is processed in two halves so that only 32 accumulator registers are live at a time.
template <typename T, int CT, int IX>
__device__ __forceinline__ void logit_half(const T* Zs, int jz0, const Vec16<T> (&xf)[IX][SC<T, CT>::NKB], int lane,
                                           f32x4 (&acc)[SC<T, CT>::JH][IX]) {
    using S = SC<T, CT>;
#pragma unroll
    for (int j = 0; j < S::JH; ++j)
#pragma unroll
        for (int ix = 0; ix < IX; ++ix) acc[j][ix] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < S::NKB; ++kb) {
#pragma unroll
        for (int j = 0; j < S::JH; ++j) {
            const Vec16<T> zf = ld16<T>(Zs + ((jz0 + j) * 16 + (lane & 15)) * S::LDC + kb * S::KB + (lane >> 4) * S::VEC);
#pragma unroll
            for (int ix = 0; ix < IX; ++ix) acc[j][ix] = mma_kblock(zf, xf[ix][kb], acc[j][ix]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// forward: online log-sum-exp per row over this block's item chunk (+ optional logits)
// ---------------------------------------------------------------------------------------------
template <typename T, int CT>
__global__ __launch_bounds__(SNT) void score_fwd_kernel(ScoreP p) {
    using S = SC<T, CT>;
    constexpr int IX = ScoreCfg<T, CT>::IX, ZB = S::ZB, XB = 16 * IX * (SNT / 64), JH = S::JH;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr size_t BUF = S::Z_BYTES + ZB * sizeof(float);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g4 = (lane >> 4) * 4, l15 = lane & 15;
    const int Reff = p.nvalid ? min(p.R, p.nvalid[0]) : p.R;
    const DevPlan dp = dev_plan(Reff, XB, gridDim.x, p.i1 - p.i0, ZB);
    if ((int)blockIdx.x >= dp.nx * dp.nchunk || Reff <= 0) return;
    const int bx = blockIdx.x % dp.nx, by = blockIdx.x / dp.nx;
    const int m0 = bx * XB + wave * 16 * IX;
    const int c_lo = p.i0 + by * dp.zchunk, c_hi = min(p.i1, c_lo + dp.zchunk);
    const T* rows = reinterpret_cast<const T*>(p.rows);
    const T* table = reinterpret_cast<const T*>(p.table);

    Vec16<T> xf[IX][S::NKB];
    issue_xfrags<T, CT, IX>(rows, m0, Reff, lane, xf);
    ZStream<T, CT, false> zs;
    const int ntile = (c_hi - c_lo + ZB - 1) / ZB;
    zs.load(table, nullptr, 0, c_lo, c_hi, true);
    finish_xfrags<T, CT, IX>(m0, Reff, false, lane, xf);
    {
        T* Zs = reinterpret_cast<T*>(smem);
        float* info = reinterpret_cast<float*>(smem + S::Z_BYTES);
        zs.store(Zs, nullptr);
        if (tid < ZB) {
            const int n = c_lo + tid;
            const float ob = p.out_bias[min(max(n, 1), p.I - 1) - 1];
            info[tid] = (n < c_hi && n > 0) ? ob : 0.f;
        }
    }
    __syncthreads();
    float rmax[IX], rsum[IX];
#pragma unroll
    for (int ix = 0; ix < IX; ++ix) { rmax[ix] = -INFINITY; rsum[ix] = 0.f; }
    for (int it = 0; it < ntile; ++it) {
        const int n0 = c_lo + it * ZB;
        const bool more = it + 1 < ntile;
        const char* cur = smem + (size_t)(it & 1) * BUF;
        char* nxt = smem + (size_t)((it + 1) & 1) * BUF;
        float ob_next = 0.f;      // bias of the next tile's items: loaded with the tile, stored after it (no wait in between)
        if (more) {
            zs.load(table, nullptr, 0, n0 + ZB, c_hi, true);
            if (tid < ZB) ob_next = p.out_bias[min(max(n0 + ZB + tid, 1), p.I - 1) - 1];
        }
        const T* Zs = reinterpret_cast<const T*>(cur);
        const float* info = reinterpret_cast<const float*>(cur + S::Z_BYTES);
        const bool edge = (n0 == 0) || (n0 + ZB > c_hi);
#pragma unroll
        for (int half = 0; half < S::NH; ++half) {
            f32x4 acc[JH][IX];
            logit_half<T, CT, IX>(Zs, half * JH, xf, lane, acc);
#pragma unroll
            for (int ix = 0; ix < IX; ++ix) {
                const int m = m0 + ix * 16 + l15;
                float tmax = -INFINITY;
#pragma unroll
                for (int j = 0; j < JH; ++j) {
                    const int jz = half * JH + j;
                    const float4 bz = *reinterpret_cast<const float4*>(info + jz * 16 + g4);
                    const float bb[4] = {bz.x, bz.y, bz.z, bz.w};
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float x = acc[j][ix][r] + bb[r];
                        if (edge) {   // only the tile holding column 0 or the chunk tail needs per-element tests
                            const int n = n0 + jz * 16 + g4 + r;
                            x = (n == 0) ? -1000.0f : x;       // zero-padded row . y + (-1000)  (Base.py:110)
                            x = (n < c_hi) ? x : -INFINITY;
                        }
                        acc[j][ix][r] = x;
                        tmax = fmaxf(tmax, x);
                    }
                }
                if (p.logits && m < Reff) {
                    float* dst = p.logits + (long)m * (p.i1 - p.i0) + (n0 - p.i0);
#pragma unroll
                    for (int j = 0; j < JH; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int zz = (half * JH + j) * 16 + g4 + r;
                            if (n0 + zz < c_hi) dst[zz] = acc[j][ix][r];
                        }
                }
                const float nm = fmaxf(rmax[ix], tmax);
                if (nm > -INFINITY) {
                    float sacc = rsum[ix] * __expf(rmax[ix] - nm);
#pragma unroll
                    for (int j = 0; j < JH; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) sacc += __expf(acc[j][ix][r] - nm);
                    rsum[ix] = sacc;
                    rmax[ix] = nm;
                }
            }
        }
        if (more) {
            zs.store(reinterpret_cast<T*>(nxt), nullptr);
            if (tid < ZB) {
                const int n = n0 + ZB + tid;
                reinterpret_cast<float*>(nxt + S::Z_BYTES)[tid] = (n < c_hi && n > 0) ? ob_next : 0.f;
            }
        }
        __syncthreads();
    }
    // the 4 lane groups of a wave hold disjoint z subsets of the same x: combine them
#pragma unroll
    for (int ix = 0; ix < IX; ++ix) {
        const float mx = group_max4(rmax[ix]);
        float s = (rmax[ix] > -INFINITY) ? rsum[ix] * __expf(rmax[ix] - mx) : 0.f;
        s = group_sum4(s);
        const int m = m0 + ix * 16 + l15;
        if (lane < 16 && m < Reff) {
            p.part[((long)m * dp.nchunk + by) * 2] = mx;
            p.part[((long)m * dp.nchunk + by) * 2 + 1] = s;
        }
    }
}

__global__ void lse_combine_kernel(const float* part, int R, const int32_t* nvalid, int xb, int zb, int G, int ztotal, float* row_lse) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= R) return;
    const int Reff = nvalid ? min(R, nvalid[0]) : R;
    if (m >= Reff) { row_lse[m] = 0.f; return; }
    const int nchunk = dev_plan(Reff, xb, G, ztotal, zb).nchunk;
    float mx = -INFINITY;
    for (int c = 0; c < nchunk; ++c) mx = fmaxf(mx, part[((long)m * nchunk + c) * 2]);
    float s = 0.f;
    for (int c = 0; c < nchunk; ++c) {
        const float pm = part[((long)m * nchunk + c) * 2];
        if (pm > -INFINITY) s += part[((long)m * nchunk + c) * 2 + 1] * __expf(pm - mx);
    }
    row_lse[m] = mx + __logf(s);
}

// lse_combine_kernel + label_logit_kernel in one launch (flash form): one wave per row
template <typename T>
__global__ __launch_bounds__(256) void lse_label_kernel(const float* part, int R, const int32_t* nvalid, int xb, int zb, int G, int ztotal,
                                                        float* row_lse, const T* rows, const T* table, const float* out_bias,
                                                        const int64_t* labels, int C, int i0, int i1, float* lab_out, float* coef_out,
                                                        const int32_t* wtotal) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= R) return;
    // two round trips: {row count, label}, then everything that hangs on them — chunk partials, row, label row of the table, bias —
    // as unconditional loads (indices clamped); guarded loads made this kernel six dependent round trips
    const int Reff = nvalid ? min(R, nvalid[0]) : R;
    const int64_t lab = labels[r];
    const int nchunk = dev_plan(max(Reff, 1), xb, G, ztotal, zb).nchunk;
    const bool own = lab >= i0 && lab < i1;
    const int64_t labc = own ? lab : (int64_t)i0;
    const long pidx = ((long)min(r, max(Reff - 1, 0)) * nchunk + min(lane, nchunk - 1)) * 2;
    float pm = part[pidx], ps = part[pidx + 1];
    float ob = out_bias[max(labc, (int64_t)1) - 1];
    float a = 0.f;
    if (C <= 128) {
        const int c0 = min(lane, C - 1), c1 = min(lane + 64, C - 1);
        float x0 = to_f32(rows[(long)r * C + c0]), x1 = to_f32(rows[(long)r * C + c1]);
        float t0 = to_f32(table[labc * C + c0]), t1 = to_f32(table[labc * C + c1]);
        asm volatile("" : "+v"(pm), "+v"(ps), "+v"(ob), "+v"(x0), "+v"(x1), "+v"(t0), "+v"(t1));
        a = lane < C ? x0 * t0 : 0.f;                       // the summation order of label_logit_kernel (bit-equal results)
        a = lane + 64 < C ? fmaf(x1, t1, a) : a;
    } else {
        asm volatile("" : "+v"(pm), "+v"(ps), "+v"(ob));
        for (int c = lane; c < C; c += 64) a += to_f32(rows[(long)r * C + c]) * to_f32(table[labc * C + c]);
    }
    a = (lab != 0 && own) ? a : 0.f;
    float lse = 0.f;
    if (r < Reff) {
        float mx = lane < nchunk ? pm : -INFINITY;
        for (int c = lane + 64; c < nchunk; c += 64) mx = fmaxf(mx, part[((long)r * nchunk + c) * 2]);
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        float sm = (lane < nchunk && pm > -INFINITY) ? ps * __expf(pm - mx) : 0.f;
        for (int c = lane + 64; c < nchunk; c += 64) {
            const float qm = part[((long)r * nchunk + c) * 2];
            if (qm > -INFINITY) sm += part[((long)r * nchunk + c) * 2 + 1] * __expf(qm - mx);
        }
        sm = wave_sum(sm);
        lse = mx + __logf(sm);
    }
    a = wave_sum(a);
    if (lane == 0) {
        row_lse[r] = lse;
        const float ll = (lab == 0) ? -1000.0f : a + ob;
        if (own) lab_out[r] = ll;
        if (coef_out) {   // d loss / d logit scale of the row: ce_loss_kernel's coefficient, its row count known as *nvalid
            const float v = __expf(ll - lse), W = (float)(wtotal ? wtotal[0] : Reff) + 1e-5f;   // EasyDGL.py:184 over the global batch
            coef_out[r] = (r < Reff && lab != 0) ? (1.f / W) * (v / (v + 1e-5f)) : 0.f;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void label_logit_kernel(const T* rows, const T* table, const float* out_bias,
                                                          const int64_t* labels, int R, int C, int i0, int i1, float* out) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= R) return;
    const int64_t lab = labels[r];
    if (lab < i0 || lab >= i1) return;
    float a = 0.f;
    if (lab != 0)
        for (int c = lane; c < C; c += 64) a += to_f32(rows[(long)r * C + c]) * to_f32(table[lab * C + c]);
    a = wave_sum(a);
    if (lane == 0) out[r] = (lab == 0) ? -1000.0f : a + out_bias[lab - 1];
}

// ---------------------------------------------------------------------------------------------
// backward: ROLE_Y (x = rows, z = items) -> d_rows ; ROLE_W (x = items, z = rows) -> d_table, d_bias
// ---------------------------------------------------------------------------------------------
// ROLE_YF ("flash" form of ROLE_Y, used by edgl_score_flash_*): the SAME pass also produces the row log-sum-exp, so the separate
// forward LSE kernel disappears — dl is exp(logit - running row max) and the accumulators are rescaled whenever the running
// max of a row moves (rare after the first tiles); the finish kernel divides by the row sum, applies the loss coefficient
// and subtracts the label row.
enum { ROLE_Y = 0, ROLE_W = 1, ROLE_YF = 2 };

// NW = 8: one workgroup per CU, double-buffered LDS, register prefetch across the compute phase.
// NW = 4: two independent 4-wave workgroups per CU, single LDS buffer, next tile fetched at the tile boundary —
//         the two workgroups drift apart, so one's MFMA phase overlaps the other's exp/VALU and load phases.
// CO = output channel tiles accumulated per workgroup: CT (one pass) or CT/2 (C = 256: two passes over the channel halves —
// the logits are recomputed per pass, but [2][16] accumulator tiles + operands do not fit 256 registers and spill ~300)
template <typename T, int CT, int ROLE, int NW, int CO = CT>
__global__ __launch_bounds__(64 * NW) void score_bwd_kernel(ScoreP p) {
    constexpr int IX = ScoreCfg<T, CT>::IX;
    constexpr int NTHR = 64 * NW, XBW = 16 * IX * NW;
    constexpr bool YS = ROLE != ROLE_W, FLASH = ROLE == ROLE_YF;   // YS: x = rows, z = items
    const int ct0 = (CO == CT) ? 0 : (YS ? (int)blockIdx.y : (int)blockIdx.z) * CO;
    using S = SC<T, CT, NTHR>;
    constexpr int ZB = S::ZB, JH = S::JH;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr size_t BUF = S::Z_BYTES + S::ZT_BYTES + S::INFO_BYTES;
    constexpr bool DOUBLE = (NW == 8) && (2 * BUF <= 160 * 1024);
    constexpr bool PREFETCH = (NW == 8) && ScoreCfg<T, CT>::STD;   // the wide shapes have no registers to spare for the next tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g4 = (lane >> 4) * 4, l15 = lane & 15;
    const T* rows = reinterpret_cast<const T*>(p.rows);
    const T* rowsT = reinterpret_cast<const T*>(p.rowsT);
    const T* table = reinterpret_cast<const T*>(p.table);
    const T* tableT = reinterpret_cast<const T*>(p.tableT);
    const int Reff = p.nvalid ? min(p.R, p.nvalid[0]) : p.R;
    // ROLE_Y: 1-D launch, (x-block, item chunk) derived from the valid row count; ROLE_W: x = items (blockIdx.x),
    // the valid rows are split evenly over gridDim.y chunks
    int bx, by, zchunk, nchunk_dev = 1;
    long slab_stride;
    if (YS) {
        const DevPlan dp = dev_plan(Reff, XBW, gridDim.x, p.i1 - p.i0, ZB);
        if ((int)blockIdx.x >= dp.nx * dp.nchunk || Reff <= 0) return;
        bx = blockIdx.x % dp.nx; by = blockIdx.x / dp.nx; zchunk = dp.zchunk; nchunk_dev = dp.nchunk;
        slab_stride = (long)dp.nx * XBW * S::C;
    } else {
        bx = blockIdx.x; by = blockIdx.y;
        const int ntiles = (Reff + ZB - 1) / ZB;
        zchunk = (ntiles + (int)gridDim.y - 1) / (int)gridDim.y * ZB;
        slab_stride = (long)p.I * S::C;
    }
    // x side
    const int xbase = (YS ? 0 : p.i0) + bx * XBW + wave * 16 * IX;
    const int xend = YS ? Reff : p.i1;
    Vec16<T> xf[IX][S::NKB];
    issue_xfrags<T, CT, IX>(YS ? rows : table, xbase, xend, lane, xf);
    float x_lse[IX], x_cf[IX], x_bias[IX];
    int x_lab[IX];
    float m_run[IX], s_run[IX];   // ROLE_YF: running row max (uniform over the 4 lane groups) and this lane's part of the row sum
#pragma unroll
    for (int ix = 0; ix < IX; ++ix) {
        const int gx = xbase + ix * 16 + l15;
        const bool ok = gx < xend;
        m_run[ix] = -INFINITY; s_run[ix] = 0.f;
        if (FLASH) {
            x_lse[ix] = 0.f; x_cf[ix] = 0.f; x_lab[ix] = -1; x_bias[ix] = 0.f;
        } else if (ROLE == ROLE_Y) {
            const int gc = max(min(gx, xend - 1), 0);
            const float cf = p.coef[gc], ls = p.row_lse[gc];
            const int64_t lb = p.labels[gc];
            x_cf[ix] = ok ? cf : 0.f;
            // coef*exp(x - lse) = exp(x - (lse - log coef)); coef == 0 (label 0 / row past the end) -> +inf -> 0
            x_lse[ix] = x_cf[ix] > 0.f ? ls - __logf(x_cf[ix]) : INFINITY;
            x_lab[ix] = ok ? (int)lb : -1;
            x_bias[ix] = 0.f;
        } else {
            const float ob = p.out_bias[min(max(gx, 1), p.I - 1) - 1];     // unconditional load, then the select
            x_bias[ix] = (ok && gx > 0) ? ob : 0.f;
            x_lse[ix] = 0.f; x_cf[ix] = 0.f; x_lab[ix] = ok ? gx : -2;   // x_lab = own item id
        }
    }
    // z side
    const int z_lo = (YS ? p.i0 : 0) + by * zchunk;
    const int z_hi = min(YS ? p.i1 : Reff, z_lo + zchunk);
    const T* zsrc = YS ? table : rows;
    const T* zsrcT = YS ? tableT : rowsT;
    const int ldT = YS ? p.ldt : p.ldr;

    // per-z scalars of a streamed tile (ROLE_Y*: bias[z]; ROLE_W: lse[z] - log coef[z], coef[z], label[z]), threads < ZB: the
    // loads are unconditional (index clamped) and issued with the tile's own loads, the LDS stores follow the tile's —
    // a load inside `ok ? .. : 0` waits for its data on the spot, one exposed round trip per streamed tile
    float zi_a = 0.f, zi_b = 0.f;
    int64_t zi_c = 0;
    auto load_info = [&](int z0) {
        if (tid < ZB) {
            const int gz = z0 + tid;
            if (YS) {
                zi_a = p.out_bias[min(max(gz, 1), p.I - 1) - 1];
            } else {
                const int gc = min(gz, Reff - 1);
                zi_a = p.coef[gc]; zi_b = p.row_lse[gc]; zi_c = p.labels[gc];
            }
        }
    };
    auto store_info = [&](char* buf, int z0) {
        float* info = reinterpret_cast<float*>(buf + S::Z_BYTES + S::ZT_BYTES);
        if (tid < ZB) {
            const int gz = z0 + tid;
            const bool ok = gz < z_hi;
            if (YS) {
                info[tid] = (ok && gz > 0) ? zi_a : 0.f;
            } else {
                const float cf = ok ? zi_a : 0.f;
                info[tid] = cf > 0.f ? zi_b - __logf(cf) : INFINITY;
                info[ZB + tid] = cf;
                reinterpret_cast<int*>(info)[2 * ZB + tid] = ok ? (int)zi_c : -1;
            }
        }
    };

    f32x4 out[IX][CO];
#pragma unroll
    for (int ix = 0; ix < IX; ++ix)
#pragma unroll
        for (int ct = 0; ct < CO; ++ct) out[ix][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbias[IX];
#pragma unroll
    for (int ix = 0; ix < IX; ++ix) dbias[ix] = 0.f;

    ZStream<T, CT, S::WT, NTHR> zs;
    const int ntile = z_hi > z_lo ? (z_hi - z_lo + ZB - 1) / ZB : 0;
    if (ntile > 0) { zs.load(zsrc, zsrcT, ldT, z_lo, z_hi, YS); load_info(z_lo); }
    finish_xfrags<T, CT, IX>(xbase, xend, ROLE == ROLE_W, lane, xf);
    if (ntile > 0) {
        zs.store(reinterpret_cast<T*>(smem), reinterpret_cast<T*>(smem + S::Z_BYTES));
        store_info(smem, z_lo);
    }
    __syncthreads();
    for (int it = 0; it < ntile; ++it) {
        const int z0 = z_lo + it * ZB;
        const bool more = it + 1 < ntile;
        char* cur = smem + (DOUBLE ? (size_t)(it & 1) * BUF : 0);
        char* nxt = smem + (DOUBLE ? (size_t)((it + 1) & 1) * BUF : 0);
        if (PREFETCH && more) { zs.load_z(zsrc, z0 + ZB, z_hi, YS); load_info(z0 + ZB); }
        const T* Zs = reinterpret_cast<const T*>(cur);
        const T* ZTs = reinterpret_cast<const T*>(cur + S::Z_BYTES);
        const float* info = reinterpret_cast<const float*>(cur + S::Z_BYTES + S::ZT_BYTES);
        const bool edge = YS && ((z0 == 0) || (z0 + ZB > z_hi));
#pragma unroll
        for (int half = 0; half < S::NH; ++half) {
            f32x4 acc[JH][IX];
            logit_half<T, CT, IX>(Zs, half * JH, xf, lane, acc);
            // ---- dl[z][x] in place ------------------------------------------------------------------
            if constexpr (FLASH) {
                float tmax[IX];
#pragma unroll
                for (int ix = 0; ix < IX; ++ix) tmax[ix] = -INFINITY;
#pragma unroll
                for (int j = 0; j < JH; ++j) {
                    const int jz = half * JH + j;
                    const float4 t4 = *reinterpret_cast<const float4*>(info + jz * 16 + g4);
                    const float zb[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
                    for (int ix = 0; ix < IX; ++ix)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float x = acc[j][ix][r] + zb[r];
                            if (edge) {
                                const int gz = z0 + jz * 16 + g4 + r;
                                x = (gz == 0) ? -1000.0f : x;          // zero-padded row . y + (-1000)  (Base.py:110)
                                x = (gz < z_hi) ? x : -INFINITY;
                            }
                            acc[j][ix][r] = x;
                            tmax[ix] = fmaxf(tmax[ix], x);
                        }
                }
                bool moved = false;
                float corr[IX];
#pragma unroll
                for (int ix = 0; ix < IX; ++ix) {
                    const float m_new = fmaxf(m_run[ix], group_max4(tmax[ix]));
                    corr[ix] = (m_run[ix] > -INFINITY) ? __expf(m_run[ix] - m_new) : 0.f;
                    moved = moved || (m_new > m_run[ix]);
                    m_run[ix] = m_new;
                }
                if (__any(moved)) {     // rescale what was accumulated against the old maxima (wave-uniform branch)
#pragma unroll
                    for (int ix = 0; ix < IX; ++ix) {
                        s_run[ix] *= corr[ix];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float f = __shfl(corr[ix], g4 + r, 64);   // the factor of row x = ix*16 + g4 + r sits in lane g4 + r
#pragma unroll
                            for (int ct = 0; ct < CO; ++ct) out[ix][ct][r] *= f;
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < JH; ++j)
#pragma unroll
                    for (int ix = 0; ix < IX; ++ix)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float d = __expf(acc[j][ix][r] - m_run[ix]);
                            s_run[ix] += d;
                            acc[j][ix][r] = d;
                        }
            } else
#pragma unroll
            for (int j = 0; j < JH; ++j) {
                const int jz = half * JH + j;
                float zb[4];   // ROLE_Y: bias[z] ; ROLE_W: lse[z] - log coef[z]
                int zlab[4];
                {
                    const float4 t = *reinterpret_cast<const float4*>(info + jz * 16 + g4);
                    zb[0] = t.x; zb[1] = t.y; zb[2] = t.z; zb[3] = t.w;
                }
                if (ROLE == ROLE_W) {
                    const int4 c4 = *reinterpret_cast<const int4*>(reinterpret_cast<const int*>(info) + 2 * ZB + jz * 16 + g4);
                    zlab[0] = c4.x; zlab[1] = c4.y; zlab[2] = c4.z; zlab[3] = c4.w;
                }
#pragma unroll
                for (int ix = 0; ix < IX; ++ix)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int gz = z0 + jz * 16 + g4 + r;
                        float d;
                        if (ROLE == ROLE_Y) {
                            float x = acc[j][ix][r] + zb[r];
                            if (edge) x = (gz == 0) ? -1000.0f : x;
                            d = __expf(x - x_lse[ix]);
                            if (gz == x_lab[ix]) d -= x_cf[ix];
                            if (edge) d = (gz < z_hi) ? d : 0.f;
                        } else {
                            float x = acc[j][ix][r] + x_bias[ix];
                            x = (x_lab[ix] == 0) ? -1000.0f : x;
                            d = __expf(x - zb[r]);
                            if (x_lab[ix] == zlab[r]) d -= info[ZB + jz * 16 + g4 + r];   // rare: ~1 hit per tile
                            d = (x_lab[ix] >= 0) ? d : 0.f;     // x beyond the table shard
                            dbias[ix] += d;
                        }
                        acc[j][ix][r] = d;
                    }
            }
            // ---- out[x][c] += sum_z dl[x][z] Z[z][c] --------------------------------------------------
            if constexpr (sizeof(T) == 2) {
#pragma unroll
                for (int jp = 0; jp < JH / 2; ++jp) {
                    bf16x8 af[IX];
#pragma unroll
                    for (int ix = 0; ix < IX; ++ix)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            af[ix][r] = (bf16)acc[2 * jp][ix][r];
                            af[ix][4 + r] = (bf16)acc[2 * jp + 1][ix][r];
                        }
#pragma unroll
                    for (int ct = 0; ct < CO; ++ct) {
                        const bf16x8 bfr = sc_tr_frag32(Zs, S::LDC, (half * (JH / 2) + jp) * 32, (ct0 + ct) * 16, lane);
#pragma unroll
                        for (int ix = 0; ix < IX; ++ix) out[ix][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ix], bfr, out[ix][ct], 0, 0, 0);
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < JH; ++j) {
                    Frag4<T> a[IX];
#pragma unroll
                    for (int ix = 0; ix < IX; ++ix) a[ix] = frag_from_acc<T>(acc[j][ix]);
#pragma unroll
                    for (int ct = 0; ct < CO; ++ct) {
                        const Frag4<T> bfr = frag_ld<T>(ZTs + ((ct0 + ct) * 16 + l15) * S::LDZ + (half * JH + j) * 16 + g4);
#pragma unroll
                        for (int ix = 0; ix < IX; ++ix) out[ix][ct] = mma16(a[ix], bfr, out[ix][ct]);
                    }
                }
            }
        }
        if (!DOUBLE) __syncthreads();
        if (more) {
            if (!PREFETCH) { zs.load_z(zsrc, z0 + ZB, z_hi, YS); load_info(z0 + ZB); }
            zs.load_t(zsrcT, ldT, z0 + ZB, z_hi, YS);   // short-lived: the other wave of the SIMD covers it
            zs.store(reinterpret_cast<T*>(nxt), reinterpret_cast<T*>(nxt + S::Z_BYTES));
            store_info(nxt, z0 + ZB);
        }
        __syncthreads();
    }
    // ---- write the slab: out regs r <-> x = ix*16 + g4 + r, lane l15 <-> c = ct*16 + l15 ----------------
    float* slab = p.slabs + (long)by * slab_stride;
#pragma unroll
    for (int ix = 0; ix < IX; ++ix)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gx = xbase + ix * 16 + g4 + r;
            if (gx < xend) {
#pragma unroll
                for (int ct = 0; ct < CO; ++ct) slab[(long)gx * S::C + (ct0 + ct) * 16 + l15] = out[ix][ct][r];
            }
        }
    if (FLASH && ct0 == 0) {   // (row max, row sum) of this item chunk: lse_combine_kernel / flash_finish_kernel merge the chunks
#pragma unroll
        for (int ix = 0; ix < IX; ++ix) {
            const float sm = group_sum4(s_run[ix]);
            const int gx = xbase + ix * 16 + l15;
            if (lane < 16 && gx < xend) {
                p.part[((long)gx * nchunk_dev + by) * 2] = m_run[ix];
                p.part[((long)gx * nchunk_dev + by) * 2 + 1] = sm;
            }
        }
    }
    if (ROLE == ROLE_W && ct0 == 0) {
#pragma unroll
        for (int ix = 0; ix < IX; ++ix) {
            const float v = group_sum4(dbias[ix]);
            const int gx = xbase + ix * 16 + l15;
            if (lane < 16 && gx < xend && gx > 0) p.bias_slabs[(long)by * (p.I - 1) + gx - 1] = v;
        }
    }
}

// out[i] = (T) sum_s slabs[s][i]; `zero_first` elements at the front are forced to 0 (table row 0).  A second job (the bias
// gradient next to the table gradient) rides in the same launch: workgroups [nb0, gridDim.x) belong to it.
struct SlabJob { const float* slabs; long n, lo, hi, zero_first; void* out; };
template <typename TO>
__global__ void slab_reduce_kernel(SlabJob j0, SlabJob j1, int nb0, int nslab, const float* gscale) {
    const float gs = gscale ? gscale[0] : 1.0f;   // upstream d(loss) scalar
    const bool first = (int)blockIdx.x < nb0;
    const SlabJob& j = first ? j0 : j1;
    const long bid = first ? blockIdx.x : blockIdx.x - nb0, nblk = first ? nb0 : (long)gridDim.x - nb0;
    TO* out = reinterpret_cast<TO*>(j.out);
    if constexpr (sizeof(TO) == 4) {
        // f32 output with everything a multiple of 4 (the table gradient): 16-byte vectors, the slabs of a group of four fetched
        // together (slab index clamped, the surplus weighted 0) — one element per thread and slab was a round trip per slab
        if (((j.lo | j.hi | j.n | j.zero_first) & 3) == 0 && ((uintptr_t)j.slabs & 15) == 0 && ((uintptr_t)out & 15) == 0) {
            for (long i = j.lo + (bid * blockDim.x + threadIdx.x) * 4; i < j.hi; i += nblk * blockDim.x * 4) {
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int s0 = 0; s0 < nslab; s0 += 4) {
                    float4 x[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) x[k] = *reinterpret_cast<const float4*>(j.slabs + (long)min(s0 + k, nslab - 1) * j.n + i);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float w = s0 + k < nslab ? 1.f : 0.f;
                        a.x = s0 + k < nslab ? a.x + x[k].x : a.x; a.y = s0 + k < nslab ? a.y + x[k].y : a.y;
                        a.z = s0 + k < nslab ? a.z + x[k].z : a.z; a.w = s0 + k < nslab ? a.w + x[k].w : a.w;
                        (void)w;
                    }
                }
                const bool z = i < j.zero_first;
                *reinterpret_cast<float4*>(out + i) = z ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(a.x * gs, a.y * gs, a.z * gs, a.w * gs);
            }
            return;
        }
    }
    for (long i = j.lo + bid * blockDim.x + threadIdx.x; i < j.hi; i += nblk * blockDim.x) {
        float a = 0.f;
        for (int s = 0; s < nslab; ++s) a += j.slabs[(long)s * j.n + i];
        out[i] = from_f32<TO>(i < j.zero_first ? 0.f : a * gs);
    }
}

// d_rows[r] = (T) gs * sum over the item chunks' slabs; the slab geometry follows dev_plan of the producing launch.
template <typename TO>
__global__ void slab_reduce_rows_kernel(const float* slabs, const int32_t* nvalid, int R, int C, int xb, int zb, int G, int ztotal,
                                        const float* gscale, TO* out) {
    const float gs = gscale ? gscale[0] : 1.0f;
    const int Reff = nvalid ? min(R, nvalid[0]) : R;
    const DevPlan dp = dev_plan(Reff, xb, G, ztotal, zb);
    const long stride = (long)dp.nx * xb * C, nval = (long)Reff * C, n = (long)R * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float a = 0.f;
        if (i < nval)
            for (int s = 0; s < dp.nchunk; ++s) a += slabs[(long)s * stride + i];
        out[i] = from_f32<TO>(a * gs);
    }
}

// four consecutive slab entries at element offset `off`: f32 slabs, or the bf16 slabs of the strip row pass (StripP::slab16)
template <bool S16>
__device__ __forceinline__ float4 ld_slab4(const float* slabs, long off) {
    if constexpr (S16) {
        const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const bf16*>(slabs) + off);
        return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
    } else {
        return *reinterpret_cast<const float4*>(slabs + off);
    }
}

// lse_label_kernel + flash_finish_kernel in ONE launch (the training engine: both run back to back between the two product passes,
// each a few microseconds of work behind a kernel boundary).  LPR = C / 4 lanes own a row (4 consecutive channels each): every lane
// forms the row's log-sum-exp from the chunk partials itself (<= 16 exponentials), the label logit is the LPR-lane sum of the
// lanes' 4-channel dot products with the label row of the table — the row this kernel loads anyway for the -table[label] term —
// then coefficient and d_rows as in the two kernels.  Chunk counts above MAXCH take the rolled loops.
template <typename TO, int LPR, bool S16 = false>
__global__ __launch_bounds__(256) void flash_finish_lse_kernel(const float* slabs, const float* part, const TO* rows, const TO* table,
                                                               const float* out_bias, const int64_t* labels, const int32_t* nvalid,
                                                               const int32_t* wtotal, int R, int xb, int zb, int G, int ztotal,
                                                               const float* gscale, float* row_lse, float* lab_out, float* coef_out,
                                                               TO* out, float* ce_part) {
    constexpr int C = 4 * LPR, MAXCH = 16;
    __shared__ float ce_red[8];
    float ce_num = 0.f;       // this thread's rows: -log(p_label + 1e-5) of the weighted ones (EasyDGL.py:181-185), one lane per row
    const float gs = gscale ? gscale[0] : 1.0f;
    const int Reff = nvalid ? min(R, nvalid[0]) : R;
    const float W = (float)(wtotal ? wtotal[0] : Reff) + 1e-5f;       // EasyDGL.py:184 over the global batch
    const DevPlan dp = dev_plan(max(Reff, 1), xb, G, ztotal, zb);
    const long stride = (long)dp.nx * xb * C;
    const int nch = dp.nchunk;
    const int nrow_blk = 256 / LPR;
    for (long r0 = (long)blockIdx.x * nrow_blk; r0 < R; r0 += (long)gridDim.x * nrow_blk) {
        const int r = (int)min(r0 + threadIdx.x / LPR, (long)R - 1), c = (threadIdx.x % LPR) * 4, rc = min(r, max(Reff - 1, 0));
        const bool live = r0 + threadIdx.x / LPR < R;
        if (r0 >= Reff) {      // (uniform) rows behind the weighted ones — label 0 by construction of the compaction: nothing to load
            if (live) {
                if (c == 0) { row_lse[r] = 0.f; lab_out[r] = labels[r] == 0 ? -1000.0f : 0.f; coef_out[r] = 0.f; }
                if constexpr (sizeof(TO) == 2) *reinterpret_cast<uint2*>(out + (long)r * C + c) = make_uint2(0u, 0u);
                else *reinterpret_cast<float4*>(out + (long)r * C + c) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            continue;
        }
        int64_t lab = labels[r];
        asm volatile("" : "+v"(lab));
        const int64_t labc = lab > 0 ? lab : 0;
        float ob = out_bias[max(labc, (int64_t)1) - 1];
        float xr[4], tb[4];
        if constexpr (sizeof(TO) == 2) {
            const Frag4<TO> fx = frag_ld<TO>(rows + (long)r * C + c), ft = frag_ld<TO>(table + labc * C + c);
#pragma unroll
            for (int q = 0; q < 4; ++q) { xr[q] = to_f32(fx.v[q]); tb[q] = to_f32(ft.v[q]); }
        } else {
            const float4 fx = *reinterpret_cast<const float4*>(rows + (long)r * C + c), ft = *reinterpret_cast<const float4*>(table + labc * C + c);
            xr[0] = fx.x; xr[1] = fx.y; xr[2] = fx.z; xr[3] = fx.w; tb[0] = ft.x; tb[1] = ft.y; tb[2] = ft.z; tb[3] = ft.w;
        }
        // ---- chunk partials in batches of MAXCH (all loads of a batch in flight together; index clamped, the surplus weighted 0):
        //      the row maximum first, then  sm = sum_c l_c e_c,  a = sum_c slab_c e_c  with e_c = exp(m_c - max);
        //      lse = max + log sm,  sum_c slab_c exp(m_c - lse) = a / sm
        float mx = -INFINITY;
        float4 sl0[MAXCH];                      // the first batch stays in registers (the benchmark has 11-12 chunks): ONE round trip
        float pm0[MAXCH], ps0[MAXCH];
#pragma unroll
        for (int s = 0; s < MAXCH; ++s) {
            const int sc = min(s, nch - 1);
            sl0[s] = ld_slab4<S16>(slabs, (long)sc * stride + (long)rc * C + c);
            pm0[s] = part[((long)rc * nch + sc) * 2];
            ps0[s] = part[((long)rc * nch + sc) * 2 + 1];
        }
#pragma unroll
        for (int s = 0; s < MAXCH; ++s) mx = s < nch ? fmaxf(mx, pm0[s]) : mx;
        for (int s0 = MAXCH; s0 < nch; s0 += MAXCH) {
            float pm[MAXCH];
#pragma unroll
            for (int s = 0; s < MAXCH; ++s) pm[s] = part[((long)rc * nch + min(s0 + s, nch - 1)) * 2];
#pragma unroll
            for (int s = 0; s < MAXCH; ++s) mx = s0 + s < nch ? fmaxf(mx, pm[s]) : mx;
        }
        float sm = 0.f, acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < MAXCH; ++s) {
            const float e = (s < nch && pm0[s] > -INFINITY) ? __expf(pm0[s] - mx) : 0.f;
            sm = fmaf(ps0[s], e, sm);
            acc[0] = fmaf(sl0[s].x, e, acc[0]); acc[1] = fmaf(sl0[s].y, e, acc[1]);
            acc[2] = fmaf(sl0[s].z, e, acc[2]); acc[3] = fmaf(sl0[s].w, e, acc[3]);
        }
        for (int s0 = MAXCH; s0 < nch; s0 += MAXCH) {
            float4 sl[MAXCH];
            float pm[MAXCH], ps[MAXCH];
#pragma unroll
            for (int s = 0; s < MAXCH; ++s) {
                const int sc = min(s0 + s, nch - 1);
                sl[s] = ld_slab4<S16>(slabs, (long)sc * stride + (long)rc * C + c);
                pm[s] = part[((long)rc * nch + sc) * 2];
                ps[s] = part[((long)rc * nch + sc) * 2 + 1];
            }
#pragma unroll
            for (int s = 0; s < MAXCH; ++s) {
                const float e = (s0 + s < nch && pm[s] > -INFINITY) ? __expf(pm[s] - mx) : 0.f;
                sm = fmaf(ps[s], e, sm);
                acc[0] = fmaf(sl[s].x, e, acc[0]); acc[1] = fmaf(sl[s].y, e, acc[1]);
                acc[2] = fmaf(sl[s].z, e, acc[2]); acc[3] = fmaf(sl[s].w, e, acc[3]);
            }
        }
        asm volatile("" : "+v"(ob));
        const float lse = r < Reff ? mx + __logf(sm) : 0.f;
        const float inv_sm = (r < Reff && sm > 0.f) ? 1.0f / sm : 0.f;
        // ---- label logit: LPR-lane sum (a row's lanes are LPR consecutive lanes of one wave)
        float a = (xr[0] * tb[0] + xr[1] * tb[1]) + (xr[2] * tb[2] + xr[3] * tb[3]);
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        const float ll = lab == 0 ? -1000.0f : a + ob;
        const float v = __expf(ll - lse);
        const float cf = (r < Reff && lab != 0) ? (1.f / W) * (v / (v + 1e-5f)) : 0.f;
        if (live && c == 0) {
            row_lse[r] = lse; lab_out[r] = ll; coef_out[r] = cf;
            ce_num += (r < Reff && lab != 0) ? -__logf(v + 1e-5f) : 0.f;
        }
        // ---- d_rows = gs * coef * ( sum_chunks slab_c * exp(m_c - lse)  -  table[label] )
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] *= inv_sm;
        float o4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) o4[q] = cf != 0.f ? gs * cf * (acc[q] - tb[q]) : 0.f;
        if (live) {
            if constexpr (sizeof(TO) == 2) { const Frag4<TO> f = frag_from_acc<TO>(f32x4{o4[0], o4[1], o4[2], o4[3]}); *reinterpret_cast<uint2*>(out + (long)r * C + c) = *reinterpret_cast<const uint2*>(&f); }
            else *reinterpret_cast<float4*>(out + (long)r * C + c) = make_float4(o4[0], o4[1], o4[2], o4[3]);
        }
    }
    if (ce_part) {      // the loss numerator of this workgroup's rows: the loss kernel then adds <= 4096 numbers instead of sweeping the rows
        ce_num = block_sum(ce_num, ce_red);
        if (threadIdx.x == 0) {
            ce_part[blockIdx.x] = ce_num;
            if (blockIdx.x == 0) ce_part[gridDim.x] = (float)Reff;      // ... and the weighted-row count behind the sums (exact below 2^24)
        }
    }
}

// The same launch at C = 512: eight channels per lane, so that a row's 64 lanes stay within one wave (the label logit is a wave
// reduction).  A kernel of its own: the instances above — the headline's among them — keep their code.
template <typename TO, int LPR, bool S16 = false, int CPL = 8>
__global__ __launch_bounds__(256) void flash_finish_lse_wide_kernel(const float* slabs, const float* part, const TO* rows, const TO* table,
                                                               const float* out_bias, const int64_t* labels, const int32_t* nvalid,
                                                               const int32_t* wtotal, int R, int xb, int zb, int G, int ztotal,
                                                               const float* gscale, float* row_lse, float* lab_out, float* coef_out,
                                                               TO* out, float* ce_part) {
    constexpr int C = CPL * LPR, MAXCH = CPL == 4 ? 16 : 8, NQ = CPL / 4;
    __shared__ float ce_red[8];
    float ce_num = 0.f;       // this thread's rows: -log(p_label + 1e-5) of the weighted ones (EasyDGL.py:181-185), one lane per row
    const float gs = gscale ? gscale[0] : 1.0f;
    const int Reff = nvalid ? min(R, nvalid[0]) : R;
    const float W = (float)(wtotal ? wtotal[0] : Reff) + 1e-5f;       // EasyDGL.py:184 over the global batch
    const DevPlan dp = dev_plan(max(Reff, 1), xb, G, ztotal, zb);
    const long stride = (long)dp.nx * xb * C;
    const int nch = dp.nchunk;
    const int nrow_blk = 256 / LPR;
    for (long r0 = (long)blockIdx.x * nrow_blk; r0 < R; r0 += (long)gridDim.x * nrow_blk) {
        const int r = (int)min(r0 + threadIdx.x / LPR, (long)R - 1), c = (threadIdx.x % LPR) * CPL, rc = min(r, max(Reff - 1, 0));
        const bool live = r0 + threadIdx.x / LPR < R;
        if (r0 >= Reff) {      // (uniform) rows behind the weighted ones — label 0 by construction of the compaction: nothing to load
            if (live) {
                if (c == 0) { row_lse[r] = 0.f; lab_out[r] = labels[r] == 0 ? -1000.0f : 0.f; coef_out[r] = 0.f; }
#pragma unroll
                for (int h = 0; h < NQ; ++h) {
                    if constexpr (sizeof(TO) == 2) *reinterpret_cast<uint2*>(out + (long)r * C + c + 4 * h) = make_uint2(0u, 0u);
                    else *reinterpret_cast<float4*>(out + (long)r * C + c + 4 * h) = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            continue;
        }
        int64_t lab = labels[r];
        asm volatile("" : "+v"(lab));
        const int64_t labc = lab > 0 ? lab : 0;
        float ob = out_bias[max(labc, (int64_t)1) - 1];
        float xr[CPL], tb[CPL];
#pragma unroll
        for (int h = 0; h < NQ; ++h) {
            if constexpr (sizeof(TO) == 2) {
                const Frag4<TO> fx = frag_ld<TO>(rows + (long)r * C + c + 4 * h), ft = frag_ld<TO>(table + labc * C + c + 4 * h);
#pragma unroll
                for (int q = 0; q < 4; ++q) { xr[4 * h + q] = to_f32(fx.v[q]); tb[4 * h + q] = to_f32(ft.v[q]); }
            } else {
                const float4 fx = *reinterpret_cast<const float4*>(rows + (long)r * C + c + 4 * h), ft = *reinterpret_cast<const float4*>(table + labc * C + c + 4 * h);
                xr[4 * h] = fx.x; xr[4 * h + 1] = fx.y; xr[4 * h + 2] = fx.z; xr[4 * h + 3] = fx.w;
                tb[4 * h] = ft.x; tb[4 * h + 1] = ft.y; tb[4 * h + 2] = ft.z; tb[4 * h + 3] = ft.w;
            }
        }
        // ---- chunk partials in batches of MAXCH (all loads of a batch in flight together; index clamped, the surplus weighted 0):
        //      the row maximum first, then  sm = sum_c l_c e_c,  a = sum_c slab_c e_c  with e_c = exp(m_c - max);
        //      lse = max + log sm,  sum_c slab_c exp(m_c - lse) = a / sm
        float mx = -INFINITY;
        float4 sl0[MAXCH][NQ];                  // the first batch stays in registers (the benchmark has 11-12 chunks): ONE round trip
        float pm0[MAXCH], ps0[MAXCH];
#pragma unroll
        for (int s = 0; s < MAXCH; ++s) {
            const int sc = min(s, nch - 1);
#pragma unroll
            for (int h = 0; h < NQ; ++h) sl0[s][h] = ld_slab4<S16>(slabs, (long)sc * stride + (long)rc * C + c + 4 * h);
            pm0[s] = part[((long)rc * nch + sc) * 2];
            ps0[s] = part[((long)rc * nch + sc) * 2 + 1];
        }
#pragma unroll
        for (int s = 0; s < MAXCH; ++s) mx = s < nch ? fmaxf(mx, pm0[s]) : mx;
        for (int s0 = MAXCH; s0 < nch; s0 += MAXCH) {
            float pm[MAXCH];
#pragma unroll
            for (int s = 0; s < MAXCH; ++s) pm[s] = part[((long)rc * nch + min(s0 + s, nch - 1)) * 2];
#pragma unroll
            for (int s = 0; s < MAXCH; ++s) mx = s0 + s < nch ? fmaxf(mx, pm[s]) : mx;
        }
        float sm = 0.f, acc[CPL];
#pragma unroll
        for (int q = 0; q < CPL; ++q) acc[q] = 0.f;
#pragma unroll
        for (int s = 0; s < MAXCH; ++s) {
            const float e = (s < nch && pm0[s] > -INFINITY) ? __expf(pm0[s] - mx) : 0.f;
            sm = fmaf(ps0[s], e, sm);
#pragma unroll
            for (int h = 0; h < NQ; ++h) {
                acc[4 * h] = fmaf(sl0[s][h].x, e, acc[4 * h]); acc[4 * h + 1] = fmaf(sl0[s][h].y, e, acc[4 * h + 1]);
                acc[4 * h + 2] = fmaf(sl0[s][h].z, e, acc[4 * h + 2]); acc[4 * h + 3] = fmaf(sl0[s][h].w, e, acc[4 * h + 3]);
            }
        }
        for (int s0 = MAXCH; s0 < nch; s0 += MAXCH) {
            float4 sl[MAXCH][NQ];
            float pm[MAXCH], ps[MAXCH];
#pragma unroll
            for (int s = 0; s < MAXCH; ++s) {
                const int sc = min(s0 + s, nch - 1);
#pragma unroll
                for (int h = 0; h < NQ; ++h) sl[s][h] = ld_slab4<S16>(slabs, (long)sc * stride + (long)rc * C + c + 4 * h);
                pm[s] = part[((long)rc * nch + sc) * 2];
                ps[s] = part[((long)rc * nch + sc) * 2 + 1];
            }
#pragma unroll
            for (int s = 0; s < MAXCH; ++s) {
                const float e = (s0 + s < nch && pm[s] > -INFINITY) ? __expf(pm[s] - mx) : 0.f;
                sm = fmaf(ps[s], e, sm);
#pragma unroll
                for (int h = 0; h < NQ; ++h) {
                    acc[4 * h] = fmaf(sl[s][h].x, e, acc[4 * h]); acc[4 * h + 1] = fmaf(sl[s][h].y, e, acc[4 * h + 1]);
                    acc[4 * h + 2] = fmaf(sl[s][h].z, e, acc[4 * h + 2]); acc[4 * h + 3] = fmaf(sl[s][h].w, e, acc[4 * h + 3]);
                }
            }
        }
        asm volatile("" : "+v"(ob));
        const float lse = r < Reff ? mx + __logf(sm) : 0.f;
        const float inv_sm = (r < Reff && sm > 0.f) ? 1.0f / sm : 0.f;
        // ---- label logit: LPR-lane sum (a row's lanes are LPR consecutive lanes of one wave)
        float a = (xr[0] * tb[0] + xr[1] * tb[1]) + (xr[2] * tb[2] + xr[3] * tb[3]);
        if constexpr (CPL == 8) a += (xr[4] * tb[4] + xr[5] * tb[5]) + (xr[6] * tb[6] + xr[7] * tb[7]);
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        const float ll = lab == 0 ? -1000.0f : a + ob;
        const float v = __expf(ll - lse);
        const float cf = (r < Reff && lab != 0) ? (1.f / W) * (v / (v + 1e-5f)) : 0.f;
        if (live && c == 0) {
            row_lse[r] = lse; lab_out[r] = ll; coef_out[r] = cf;
            ce_num += (r < Reff && lab != 0) ? -__logf(v + 1e-5f) : 0.f;
        }
        // ---- d_rows = gs * coef * ( sum_chunks slab_c * exp(m_c - lse)  -  table[label] )
#pragma unroll
        for (int q = 0; q < CPL; ++q) acc[q] *= inv_sm;
        float o4[CPL];
#pragma unroll
        for (int q = 0; q < CPL; ++q) o4[q] = cf != 0.f ? gs * cf * (acc[q] - tb[q]) : 0.f;
        if (live) {
#pragma unroll
            for (int h = 0; h < NQ; ++h) {
                if constexpr (sizeof(TO) == 2) { const Frag4<TO> f = frag_from_acc<TO>(f32x4{o4[4 * h], o4[4 * h + 1], o4[4 * h + 2], o4[4 * h + 3]}); *reinterpret_cast<uint2*>(out + (long)r * C + c + 4 * h) = *reinterpret_cast<const uint2*>(&f); }
                else *reinterpret_cast<float4*>(out + (long)r * C + c + 4 * h) = make_float4(o4[4 * h], o4[4 * h + 1], o4[4 * h + 2], o4[4 * h + 3]);
            }
        }
    }
    if (ce_part) {      // the loss numerator of this workgroup's rows: the loss kernel then adds <= 4096 numbers instead of sweeping the rows
        ce_num = block_sum(ce_num, ce_red);
        if (threadIdx.x == 0) {
            ce_part[blockIdx.x] = ce_num;
            if (blockIdx.x == 0) ce_part[gridDim.x] = (float)Reff;      // ... and the weighted-row count behind the sums (exact below 2^24)
        }
    }
}

// ROLE_YF finish: d_rows[r] = gs * coef[r] * ( sum_chunks slab_c[r] * exp(m_c - lse[r])  -  table[label[r]] )
//   = gs * coef * (sum_z p_z T_z - T_label)   (Appendix C: dy_rows = dl . table, dl = coef (p - onehot))
template <typename TO>
__global__ void flash_finish_kernel(const float* slabs, const float* part, const float* row_lse, const float* coef,
                                    const int64_t* labels, const TO* table, const int32_t* nvalid, int R, int C, int xb, int zb,
                                    int G, int ztotal, const float* gscale, TO* out, int i0, int i1) {
    // (i0, i1): the item range the slabs were formed over — the label row leaves only where the label lies in it (an item shard of
    //  the vocab-parallel loss: every rank finishes its share of d_rows with the GLOBAL log-sum-exp, the shares add up)
    const float gs = gscale ? gscale[0] : 1.0f;
    const int Reff = nvalid ? min(R, nvalid[0]) : R;
    const DevPlan dp = dev_plan(max(Reff, 1), xb, G, ztotal, zb);
    const long stride = (long)dp.nx * xb * C;
    const int nch = dp.nchunk, C4 = C >> 2;
    constexpr int MAXCH = 16;
    const bool vec = (((uintptr_t)slabs | (uintptr_t)out | (uintptr_t)table) & 15) == 0 && (stride & 3) == 0;
    // a thread = 4 consecutive channels of a row; rounds of loads: the row's scalars with the slab values and maxima of up to
    // MAXCH chunks at a time (chunk index clamped, the surplus weighted 0), then the label row of the table.  One element per
    // thread with the chunk loop rolled was a dependent round trip per chunk (the 512-unit recipe has > 16 chunks: 60 us).
    for (long i4 = (long)blockIdx.x * blockDim.x + threadIdx.x; i4 < (long)R * C4; i4 += (long)gridDim.x * blockDim.x) {
        const int r = (int)(i4 / C4), c = (int)(i4 % C4) * 4, rc = min(r, max(Reff - 1, 0));
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec) {
            float cf = coef[rc], lse = row_lse[rc];
            int64_t lab = labels[rc];
            asm volatile("" : "+v"(cf), "+v"(lse), "+v"(lab));
            float tb[4];
            {
                const TO* trow = table + (lab > 0 ? lab : 0) * C + c;
                if constexpr (sizeof(TO) == 2) { const Frag4<TO> f = frag_ld<TO>(trow); for (int q = 0; q < 4; ++q) tb[q] = to_f32(f.v[q]); }
                else { const float4 f = *reinterpret_cast<const float4*>(trow); tb[0] = f.x; tb[1] = f.y; tb[2] = f.z; tb[3] = f.w; }
            }
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            for (int s0 = 0; s0 < nch; s0 += MAXCH) {
                float4 sl[MAXCH];
                float pm[MAXCH];
#pragma unroll
                for (int s = 0; s < MAXCH; ++s) {
                    const int sc = min(s0 + s, nch - 1);
                    sl[s] = *reinterpret_cast<const float4*>(slabs + (long)sc * stride + (long)rc * C + c);
                    pm[s] = part[((long)rc * nch + sc) * 2];
                }
#pragma unroll
                for (int s = 0; s < MAXCH; ++s) {
                    const float e = s0 + s < nch ? __expf(pm[s] - lse) : 0.f;
                    const float x[4] = {sl[s].x, sl[s].y, sl[s].z, sl[s].w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) a[q] = s0 + s < nch ? fmaf(x[q], e, a[q]) : a[q];
                }
            }
            const bool on = r < Reff && cf != 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = on ? gs * cf * (a[q] - ((lab > 0 && lab >= i0 && lab < i1) ? tb[q] : 0.f)) : 0.f;
        } else if (r < Reff) {
            const float cf = coef[r];
            if (cf != 0.f) {
                const float lse = row_lse[r];
                const int64_t lab = labels[r];
                for (int q = 0; q < 4; ++q) {
                    float a = 0.f;
                    for (int s = 0; s < nch; ++s) a += slabs[(long)s * stride + (long)r * C + c + q] * __expf(part[((long)r * nch + s) * 2] - lse);
                    v[q] = gs * cf * (a - ((lab > 0 && lab >= i0 && lab < i1) ? to_f32(table[lab * C + c + q]) : 0.f));
                }
            }
        }
        if constexpr (sizeof(TO) == 2) { const Frag4<TO> f = frag_from_acc<TO>(f32x4{v[0], v[1], v[2], v[3]}); *reinterpret_cast<uint2*>(out + (long)r * C + c) = *reinterpret_cast<const uint2*>(&f); }
        else *reinterpret_cast<float4*>(out + (long)r * C + c) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// [rows, C] -> [C, ld] transposed copy (operand images for the second MFMA product).  Two matrices per launch (the compacted
// rows and the item table): blocks [0, nbx0) of the x grid belong to the first.
template <typename T>
__global__ __launch_bounds__(256) void transpose_kernel(const T* src0, long rows0, T* dst0, long ld0, int nbx0, const T* src1, long rows1,
                                                        T* dst1, long ld1, int C) {
    __shared__ T tile[64][65];
    const bool first = (int)blockIdx.x < nbx0;
    const T* src = first ? src0 : src1;
    T* dst = first ? dst0 : dst1;
    const long rows = first ? rows0 : rows1, ld = first ? ld0 : ld1;
    const long r0 = (long)((int)blockIdx.x - (first ? 0 : nbx0)) * 64;
    const int c0 = blockIdx.y * 64;
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int r = i / 64, c = i % 64;
        tile[r][c] = (r0 + r < rows && c0 + c < C) ? src[(r0 + r) * C + c0 + c] : from_f32<T>(0.f);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int c = i / 64, r = i % 64;
        if (c0 + c < C && r0 + r < ld) dst[(long)(c0 + c) * ld + r0 + r] = tile[r][c];
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct Chunking { int nchunk, zchunk; };
// `l2_tiles` (0 = no limit): most z tiles one chunk may span.  Every workgroup of a chunk streams the same z range; the
// workgroups drift apart, and once that range no longer fits the 4 MB L2 of an XCD each of them re-reads it from HBM
// (measured at R = 51200 rows: d_rows kernel 917 us with one chunk of 157 item tiles, 474 us with 5 chunks of 32).
inline Chunking pick_chunks(int xblocks, int ztotal, int target_blocks, int ZB, int l2_tiles = 0) {
    const int ntiles = std::max(1, (ztotal + ZB - 1) / ZB);
    int nchunk = std::min(ntiles, std::max(1, target_blocks / std::max(1, xblocks)));
    if (l2_tiles > 0) nchunk = std::min(ntiles, std::max(nchunk, (ntiles + l2_tiles - 1) / l2_tiles));
    const int per = (ntiles + nchunk - 1) / nchunk;
    nchunk = (ntiles + per - 1) / per;
    return Chunking{nchunk, per * ZB};
}
inline int xblocks_of(int n, int xb) { return (n + xb - 1) / xb; }
// waves per workgroup of the generic product passes where the shape allows both: 8 (two waves per SIMD, bf16 C >= 256: half the
// output channels per pass, the logits recomputed per half) or 4 (one wave per SIMD, all channels in one pass).  Measured in the
// engine step (tools/try_shape.py, round 5): C = 256 — equal at 20 K items, 4 waves - 10 % at 100 K, - 13 % at 300 K / 1 M items
// (config 3: 53.0 -> 45.4 ms); C = 512 — 8 waves - 5..8 % (recipe 1.94 against 2.03 ms).
inline int score_nw(int C, size_t esize) { return (C == 256 && esize == 2) ? 4 : 8; }
// workgroups the chunk planners aim for: the backward product passes / the flash forward (one per CU).  Constants: the workspace
// sizes and slab offsets that edgl_score_*_workspace / edgl_score_flash_slab_info report follow from them, and callers cache those.
constexpr int SCORE_TARGET = 256, SCORE_FTARGET = 256;
inline long up8(long v) { return (v + 7) / 8 * 8; }

// z tiles per chunk that keep a chunk's streamed range within ~2 MB (half an XCD's L2); `images` = 2 when the kernel reads the
// tile and its transposed copy (d_rows), 1 for the forward
inline int l2_tiles_for(int C, size_t esize, int images, int ZB) { return std::max(8, (int)((2u << 20) / ((size_t)ZB * C * esize * images))); }
constexpr int F_L2_TILES_MIN = 32;   // smallest value l2_tiles_for(C, esize, 1, zb) takes over the supported (C, dtype): workspace bound
struct BwdPlan {
    Chunking y, w;
    long off_rowsT, off_tableT, off_slabY, off_slabW, off_slabB, off_part, off_infoY, off_infoW, total;  // float offsets
};
// The flash form (edgl_score_flash_*) at bf16 / C = 128 runs the strip kernels (k_score_strip.hip): 256 x vectors per
// workgroup as well, 64-z tiles handed out in pairs.
// 0: the generic kernels, 1: k_score_strip.hip (C = 128, 256 x vectors per workgroup), 2: k_score_stripw.hip (C = 256, 128 per workgroup)
inline int use_strip(int C, size_t esize) {
    if (esize != 2) return 0;
    if (C == 128 && edgl_strip_enabled()) return 1;
    if (edgl_stripw_supports(C) && edgl_stripw_enabled()) return 2;
    return 0;
}
inline int strip_xb(int strip) { return strip == 2 ? 128 : 256; }
inline BwdPlan bwd_plan(int R, int C, int I, int n_items, size_t esize, int strip = 0) {
    BwdPlan b;
    const RtCfg cf = rt_cfg(C, esize);
    const int nw = strip ? 8 : (cf.nwb == 8 ? score_nw(C, esize) : cf.nwb), zb = strip ? 128 : cf.zb;   // strip: pairs of its 64-z tiles
    const int xb = strip ? strip_xb(strip) : 16 * cf.ix * nw;
    b.y = pick_chunks(xblocks_of(R, xb), n_items, SCORE_TARGET, zb, l2_tiles_for(C, esize, 2, zb));
    {   // every chunk writes an [R, C] f32 slab that a later kernel sums: keep that side traffic bounded (1M-item tables would
        // otherwise ask for hundreds of chunks)
        const long slab_bytes = (long)xblocks_of(R, xb) * xb * C * 4;
        const int cap = (int)std::max<long>(SCORE_TARGET / std::max(1, xblocks_of(R, xb)), (256L << 20) / std::max(1L, slab_bytes));
        if (b.y.nchunk > cap) b.y = pick_chunks(xblocks_of(R, xb), n_items, cap * xblocks_of(R, xb), zb);
    }
    b.w = pick_chunks(xblocks_of(n_items, xb), R, SCORE_TARGET, zb);
    long o = 0;
    auto take = [&](long floats) { const long at = o; o += (floats + 63) / 64 * 64; return at; };
    b.off_rowsT = take(((long)C * up8(R) * (long)esize + 3) / 4);
    b.off_tableT = take(((long)C * up8(I) * (long)esize + 3) / 4);
    // G workgroups x one [xb, C] tile each (strip: the grid is at least SCORE_TARGET workgroups, split on the device)
    const long gy = strip ? std::max<long>((long)b.y.nchunk * xblocks_of(R, xb), SCORE_TARGET) : (long)b.y.nchunk * xblocks_of(R, xb);
    b.off_slabY = take(gy * xb * C);
    b.off_slabW = take((long)b.w.nchunk * I * C);
    b.off_slabB = take((long)b.w.nchunk * (I - 1));
    b.off_part = take(2L * gy * xb);   // (max, sum) per (row, item chunk) of the ROLE_YF pass
    b.off_infoY = b.off_infoW = 0;
    if (strip == 2) {                  // k_score_stripw.hip: the C operands of the z rows of a pass (items / rows), -inf padded
        b.off_infoY = take(edgl_stripw_info_floats(n_items));
        b.off_infoW = take(edgl_stripw_info_floats(R));
    }
    b.total = o;
    return b;
}

template <typename T, int CT>
int run_fwd(ScoreP p, hipStream_t st) {
    using S = SC<T, CT>;
    constexpr int XB = 16 * ScoreCfg<T, CT>::IX * (SNT / 64);
    const size_t smem = 2 * (S::Z_BYTES + S::ZB * sizeof(float));
    static_assert(2 * (S::Z_BYTES + S::ZB * sizeof(float)) <= 160 * 1024, "forward tile images exceed the LDS");
    auto k = score_fwd_kernel<T, CT>;
    EDGL_LDS_LIMIT(k, smem, "edgl_score_lse_fwd");
    hipLaunchKernelGGL(k, dim3(xblocks_of(p.R, XB) * p.nchunk), dim3(SNT), smem, st, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

// MODE 0: edgl_score_ce_bwd (transposes, d_rows with the known lse, d_table / d_bias)
// MODE 1: edgl_score_flash_fwd (transposes, ROLE_YF pass: unnormalised d_rows slabs + per-chunk (max, sum) -> row lse)
// MODE 2: edgl_score_flash_bwd (finish d_rows from the slabs of MODE 1, then d_table / d_bias)
// Format of the d_rows slabs a MODE 1 call left in a flash workspace (host-side record keyed by the workspace address: the
// calls of one step are issued by one host thread in order, and a captured graph replays the checked sequence).  The strip row
// pass writes bf16 slabs when the rows are finished in the same call; flash_finish_kernel (MODE 2 with d_rows) reads f32 slabs —
// pairing the two is refused instead of returning garbage row gradients.
static std::mutex g_slabfmt_mu;
static std::unordered_map<const void*, int> g_slabfmt;
static void slab_format_set(const void* ws, int bf16_slabs) {
    std::lock_guard<std::mutex> lk(g_slabfmt_mu);
    g_slabfmt[ws] = bf16_slabs;
}
static int slab_format_get(const void* ws) {
    std::lock_guard<std::mutex> lk(g_slabfmt_mu);
    auto it = g_slabfmt.find(ws);
    return it == g_slabfmt.end() ? 0 : it->second;
}

template <typename T, int CT, int MODE>
int run_bwd_mode(ScoreP p, const BwdPlan& plan, float* ws, void* d_rows, float* d_table, float* d_bias, hipStream_t st) {
    using S = SC<T, CT>;
    constexpr size_t BUF = S::Z_BYTES + S::ZT_BYTES + S::INFO_BYTES;
    const size_t smem = (2 * BUF <= 160 * 1024) ? 2 * BUF : BUF;
    EDGL_REQUIRE(smem <= 160 * 1024, EDGL_ERR_SHAPE, "edgl_score_ce_bwd: C=%d needs %zu B of LDS", p.C, smem);
    // operand images for the second product: rowsT [C][ldr], tableT [C][ldt]
    T* rowsT = reinterpret_cast<T*>(ws + plan.off_rowsT);
    T* tableT = reinterpret_cast<T*>(ws + plan.off_tableT);
    p.ldr = (int)up8(p.R); p.ldt = (int)up8(p.I);
    if (MODE != 2 && S::WT) {   // bf16 reads the transposed operand out of the row-major LDS tile: no transposed copies
        const int nbx0 = (p.ldr + 63) / 64, nbx1 = p.table_ready ? 0 : (p.ldt + 63) / 64;
        hipLaunchKernelGGL((transpose_kernel<T>), dim3((unsigned)(nbx0 + nbx1), (p.C + 63) / 64), dim3(256), 0, st,
                           reinterpret_cast<const T*>(p.rows), (long)p.R, rowsT, (long)p.ldr, nbx0,
                           reinterpret_cast<const T*>(p.table), (long)p.I, tableT, (long)p.ldt, p.C);
        EDGL_LAUNCH_CHECK();
    }
    p.rowsT = rowsT; p.tableT = tableT;
    using Cfg = ScoreCfg<T, CT>;
    constexpr int CO = Cfg::CO;
    const int strip = MODE != 0 ? use_strip(p.C, sizeof(T)) : 0;     // plan built with the same flag by the callers
    const int ZBK = strip ? 128 : S::ZB;
    const int nw = Cfg::NWB == 8 ? score_nw(p.C, sizeof(T)) : Cfg::NWB;
    const size_t smem_nw = nw == 8 ? smem : BUF;
    const int xb = strip ? strip_xb(strip) : 16 * Cfg::IX * nw;
    const int G = strip ? std::max(xblocks_of(p.R, xb) * plan.y.nchunk, SCORE_TARGET) : xblocks_of(p.R, xb) * plan.y.nchunk;
    float* part = ws + plan.off_part;
    // rows finished in one launch (flash_finish_lse_kernel): the strip row pass then leaves bf16 slabs
    const bool one_launch = MODE == 1 && d_rows && (p.C == 128 || p.C == 64 || p.C == 256 || p.C == 512) && p.i0 == 0 && p.i1 == p.I;
    const bool slab16 = strip == 1 && one_launch;
    if (MODE == 1) slab_format_set(ws, slab16 ? 1 : 0);
    if (MODE == 2 && d_rows)
        EDGL_REQUIRE(slab_format_get(ws) == 0, EDGL_ERR_WORKSPACE,
                     "edgl_score_flash_bwd: d_rows != NULL, but this workspace holds the bf16 slabs of edgl_score_flash_fwd_rows_w "
                     "(which has already written d_rows): call with d_rows = NULL, or run edgl_score_flash_fwd_coef for the two-call form");
    if (MODE != 2) {   // the row-side pass
        constexpr int RY = MODE == 1 ? ROLE_YF : ROLE_Y;
        ScoreP q = p;
        q.zchunk = plan.y.zchunk; q.nchunk = plan.y.nchunk; q.slabs = ws + plan.off_slabY; q.part = part;
        edgl_prof_begin(EDGL_KERNEL_SCORE_BWD_ROWS, st);
        if (strip == 2) {
            const int rc = edgl_stripw_rows(p.rows, p.table, p.out_bias, p.R, p.C, p.I, p.i0, p.i1, p.nvalid, q.slabs, part, G, ws + plan.off_infoY, st);
            if (rc) return rc;
        } else if (strip) {
            const int rc = edgl_strip_rows(p.rows, p.table, p.out_bias, p.R, p.I, p.i0, p.i1, p.nvalid, q.slabs, part, G, slab16 ? 1 : 0, st);
            if (rc) return rc;
        } else if (nw == 8) {
            auto k = score_bwd_kernel<T, CT, RY, 8, CO>;
            EDGL_LDS_LIMIT(k, smem_nw, "edgl_score backward (row pass)");
            hipLaunchKernelGGL(k, dim3(G, CT / CO), dim3(512), smem_nw, st, q);
        } else {
            auto k = score_bwd_kernel<T, CT, RY, 4>;
            EDGL_LDS_LIMIT(k, smem_nw, "edgl_score backward (row pass)");
            hipLaunchKernelGGL(k, dim3(G), dim3(256), smem_nw, st, q);
        }
        edgl_prof_end(EDGL_KERNEL_SCORE_BWD_ROWS, st);
        EDGL_LAUNCH_CHECK();
    }
    const long nrc = (long)p.R * p.C;
    if (MODE == 0) {
        hipLaunchKernelGGL((slab_reduce_rows_kernel<T>), dim3((unsigned)std::min<long>((nrc + 255) / 256, 2048)), dim3(256), 0, st,
                           ws + plan.off_slabY, p.nvalid, p.R, p.C, xb, ZBK, G, p.i1 - p.i0, p.gscale, reinterpret_cast<T*>(d_rows));
        EDGL_LAUNCH_CHECK();
    } else if (MODE == 1) {
        if (one_launch) {
            // rows finished in one launch: log-sum-exp, label logit, coefficient and d_rows (edgl_score_flash_fwd_rows_w)
            const T* rows_t = reinterpret_cast<const T*>(p.rows);
            const T* tab_t = reinterpret_cast<const T*>(p.table);
            const float* slabY = ws + plan.off_slabY;
            T* out_t = reinterpret_cast<T*>(d_rows);
#define EDGL_FFL(LPR, S16)                                                                                                     \
    hipLaunchKernelGGL((flash_finish_lse_kernel<T, LPR, S16>), dim3((unsigned)std::min<long>(((long)p.R * LPR + 255) / 256, 4096)), \
                       dim3(256), 0, st, slabY, part, rows_t, tab_t, p.out_bias, p.labels, p.nvalid, p.wtotal, p.R, xb, ZBK, G, \
                       p.i1 - p.i0, p.gscale, p.row_lse, p.lab_out, p.coef_out, out_t, p.ce_part)
            if (p.C == 128 && slab16) EDGL_FFL(32, true); else if (p.C == 128) EDGL_FFL(32, false); else if (p.C == 64) EDGL_FFL(16, false); else if (p.C == 512) hipLaunchKernelGGL((flash_finish_lse_wide_kernel<T, 64, false, 8>), dim3((unsigned)std::min<long>(((long)p.R * 64 + 255) / 256, 4096)), dim3(256), 0, st, slabY, part, rows_t, tab_t, p.out_bias, p.labels, p.nvalid, p.wtotal, p.R, xb, ZBK, G, p.i1 - p.i0, p.gscale, p.row_lse, p.lab_out, p.coef_out, out_t, p.ce_part); else EDGL_FFL(64, false);
#undef EDGL_FFL
            EDGL_LAUNCH_CHECK();
            return EDGL_OK;
        }
        hipLaunchKernelGGL((lse_label_kernel<T>), dim3((p.R + 3) / 4), dim3(256), 0, st, part, p.R, p.nvalid, xb, ZBK, G, p.i1 - p.i0,
                           p.row_lse, reinterpret_cast<const T*>(p.rows), reinterpret_cast<const T*>(p.table), p.out_bias, p.labels,
                           p.C, p.i0, p.i1, p.lab_out, p.coef_out, p.wtotal);
        EDGL_LAUNCH_CHECK();
        if (d_rows) {   // other widths: the two kernels, one after the other
            hipLaunchKernelGGL((flash_finish_kernel<T>), dim3((unsigned)std::min<long>((nrc / 4 + 255) / 256, 2048)), dim3(256), 0, st,
                               ws + plan.off_slabY, part, p.row_lse, p.coef_out, p.labels, reinterpret_cast<const T*>(p.table), p.nvalid,
                               p.R, p.C, xb, ZBK, G, p.i1 - p.i0, p.gscale, reinterpret_cast<T*>(d_rows), p.i0, p.i1);
            EDGL_LAUNCH_CHECK();
        }
        return EDGL_OK;
    } else if (d_rows) {
        hipLaunchKernelGGL((flash_finish_kernel<T>), dim3((unsigned)std::min<long>((nrc / 4 + 255) / 256, 2048)), dim3(256), 0, st,
                           ws + plan.off_slabY, part, p.row_lse, p.coef, p.labels, reinterpret_cast<const T*>(p.table), p.nvalid,
                           p.R, p.C, xb, ZBK, G, p.i1 - p.i0, p.gscale, reinterpret_cast<T*>(d_rows), p.i0, p.i1);
        EDGL_LAUNCH_CHECK();
    }
    // d_table, d_bias
    {
        ScoreP q = p;
        q.zchunk = plan.w.zchunk; q.nchunk = plan.w.nchunk; q.slabs = ws + plan.off_slabW; q.bias_slabs = ws + plan.off_slabB;
        if (strip == 2) {
            const int rc = edgl_stripw_table(p.rows, p.table, p.out_bias, p.coef, p.row_lse, p.R, p.C, p.I, p.i0, p.i1, p.nvalid, q.slabs,
                                             q.bias_slabs, q.nchunk, ws + plan.off_infoW, st);
            if (rc) return rc;
        } else if (strip) {
            const bool acc = p.acc_atomic && !p.gscale;
            const int rc = edgl_strip_table(p.rows, p.table, p.out_bias, p.coef, p.row_lse, p.R, p.I, p.i0, p.i1, p.nvalid, q.slabs,
                                            q.bias_slabs, q.nchunk, acc ? d_table : nullptr, acc ? d_bias : nullptr, st);
            if (rc) return rc;
            if (acc) {      // no slabs, no slab reduction
                if (!p.defer_label) return edgl_strip_label_scatter(p.rows, p.labels, p.coef, p.nvalid, p.R, p.C, p.i0, p.i1, p.gscale, d_table, d_bias, st);
                return EDGL_OK;
            }
        } else if (nw == 8) {
            auto k = score_bwd_kernel<T, CT, ROLE_W, 8, CO>;
            EDGL_LDS_LIMIT(k, smem_nw, "edgl_score backward (table pass)");
            hipLaunchKernelGGL(k, dim3(xblocks_of(p.i1 - p.i0, xb), q.nchunk, CT / CO), dim3(512), smem_nw, st, q);
        } else {
            auto k = score_bwd_kernel<T, CT, ROLE_W, 4>;
            EDGL_LDS_LIMIT(k, smem_nw, "edgl_score backward (table pass)");
            hipLaunchKernelGGL(k, dim3(xblocks_of(p.i1 - p.i0, xb), q.nchunk), dim3(256), smem_nw, st, q);
        }
        EDGL_LAUNCH_CHECK();
        if (p.keep_slabs && !p.gscale) return EDGL_OK;      // (the caller asked edgl_score_flash_slab_info where they are; the one-hot term is deferred too)
        const long n = (long)p.I * p.C, lo = (long)p.i0 * p.C, hi = (long)p.i1 * p.C;
        const long nb = p.I - 1, blo = std::max(p.i0, 1) - 1, bhi = p.i1 - 1;
        const int nb0 = (int)std::min<long>(((hi - lo) / 4 + 255) / 256 + 1, 2048), nb1 = bhi > blo ? (int)std::min<long>((bhi - blo + 255) / 256, 256) : 0;
        hipLaunchKernelGGL((slab_reduce_kernel<float>), dim3((unsigned)(nb0 + nb1)), dim3(256), 0, st,
                           SlabJob{q.slabs, n, lo, hi, (long)p.C, d_table}, SlabJob{q.bias_slabs, nb, blo, bhi, 0L, d_bias}, nb0,
                           q.nchunk, p.gscale);
        EDGL_LAUNCH_CHECK();
        if (strip && !p.defer_label) {   // the one-hot part of dl, which the strip product pass leaves out
            const int rc = edgl_strip_label_scatter(p.rows, p.labels, p.coef, p.nvalid, p.R, p.C, p.i0, p.i1, p.gscale, d_table, d_bias, st);
            if (rc) return rc;
        }
    }
    return EDGL_OK;
}

// The arguments every scoring entry point takes: checked (errors carry the name `who`), then copied into a fresh ScoreP.
int check_score(ScoreP& p, const void* rows, const void* table, const float* out_bias, const int64_t* labels, int R, int C, int I,
                int i0, int i1, const int32_t* nvalid, int dtype, const char* who) {
    EDGL_REQUIRE(rows && table && out_bias, EDGL_ERR_NULL, "%s: null pointer", who);
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "%s: bad dtype %d", who, dtype);
    EDGL_REQUIRE(R > 0 && I > 1 && i0 >= 0 && i1 <= I && i0 < i1 && (i0 % 8) == 0, EDGL_ERR_SHAPE,
                 "%s: bad shape R=%d I=%d [%d,%d) (i0 must be a multiple of 8)", who, R, I, i0, i1);
    EDGL_REQUIRE(((uintptr_t)rows & 15) == 0 && ((uintptr_t)table & 15) == 0, EDGL_ERR_SHAPE,
                 "%s: operands must be 16-byte aligned", who);
    EDGL_REQUIRE(C >= 32 && C <= 512 && (C & (C - 1)) == 0, EDGL_ERR_SHAPE, "%s: C=%d unsupported (power of two in [32, 512])",
                 who, C);
    p = ScoreP{};
    p.rows = rows; p.table = table; p.out_bias = out_bias; p.labels = labels; p.R = R; p.C = C; p.I = I; p.i0 = i0;
    p.i1 = i1; p.nvalid = nvalid;
    return EDGL_OK;
}

#define SCORE_DISPATCH(T, CALL)                                      \
    switch (C / 16) {                                                \
        case 2: return CALL(T, 2);                                   \
        case 4: return CALL(T, 4);                                   \
        case 8: return CALL(T, 8);                                   \
        case 16: return CALL(T, 16);                                 \
        case 32: return CALL(T, 32);                                 \
    }                                                                \
    edgl_set_error("edgl_score: C=%d unsupported", C);               \
    return EDGL_ERR_SHAPE;

template <typename T>
int fwd_dispatch(ScoreP p, int C, hipStream_t st) {
#define CALL_FWD(T, CT) run_fwd<T, CT>(p, st)
    SCORE_DISPATCH(T, CALL_FWD)
#undef CALL_FWD
}
template <typename T, int MODE>
int bwd_dispatch(ScoreP p, int C, const BwdPlan& plan, float* ws, void* d_rows, float* d_table, float* d_bias, hipStream_t st) {
#define CALL_BWD(T, CT) run_bwd_mode<T, CT, MODE>(p, plan, ws, d_rows, d_table, d_bias, st)
    SCORE_DISPATCH(T, CALL_BWD)
#undef CALL_BWD
}

inline size_t esize_of(int dtype) { return dtype == EDGL_BF16 ? 2 : 4; }
// the plan of a workspace: `flash` — the one the MODE 1 / 2 calls share (strip kernels where they apply), else edgl_score_ce_bwd's
inline BwdPlan plan_of(int R, int C, int I, int n_items, int dtype, bool flash) {
    return bwd_plan(R, C, I, n_items, esize_of(dtype), flash ? use_strip(C, esize_of(dtype)) : 0);
}
// run_bwd_mode<T, C / 16, MODE> over the plan of p's shape.  MODE 1 — every flash forward — passes d_rows or NULL and no table side.
template <int MODE>
int score_run(const ScoreP& p, float* workspace, void* d_rows, float* d_table, float* d_bias, int dtype, void* stream) {
    const BwdPlan plan = plan_of(p.R, p.C, p.I, p.i1 - p.i0, dtype, MODE != 0);
    hipStream_t st = (hipStream_t)stream;
    return dtype == EDGL_F32 ? bwd_dispatch<float, MODE>(p, p.C, plan, workspace, d_rows, d_table, d_bias, st)
                             : bwd_dispatch<bf16, MODE>(p, p.C, plan, workspace, d_rows, d_table, d_bias, st);
}

}  // namespace

// workspace rule of the forward: 2 * R * edgl_score_chunks floats >= 2 * XB * (#workgroups), the most (row, chunk)
// partial pairs any device-side split of the launch can produce
extern "C" int edgl_score_chunks(int R, int n_items) {
    long best = 1;   // C is not an argument: take the largest need over the tile shapes of ScoreCfg
    for (int xb : {256, 128})
        for (int zb : {128, 64, 32}) {
            const long g = (long)xblocks_of(R, xb) * pick_chunks(xblocks_of(R, xb), n_items, SCORE_FTARGET, zb, F_L2_TILES_MIN).nchunk;
            best = std::max(best, (g * xb + R - 1) / R);
        }
    return (int)best;
}

extern "C" int edgl_score_lse_fwd(const void* rows, const void* table, const float* out_bias, const int64_t* labels,
                                  int R, int C, int I, int i0, int i1, const int32_t* nvalid, float* row_lse,
                                  float* label_logit, float* logits, float* workspace, int dtype, void* stream) {
    ScoreP p;
    int rc = check_score(p, rows, table, out_bias, labels, R, C, I, i0, i1, nvalid, dtype, "edgl_score_lse_fwd");
    if (rc) return rc;
    // row_lse == NULL (with logits): the logits tile only — the evaluation path (score_topk) has no use for the normaliser, and the
    // one-thread-per-row merge of the chunk partials is a chain of dependent loads (46 us per tile at 512 rows)
    EDGL_REQUIRE((row_lse || logits) && workspace && (!labels || label_logit), EDGL_ERR_NULL, "edgl_score_lse_fwd: null output");
    p.row_lse = row_lse; p.part = workspace; p.logits = logits;
    const RtCfg cf = rt_cfg(C, esize_of(dtype));
    const int xbf = 16 * cf.ix * (SNT / 64);
    const Chunking ch = pick_chunks(xblocks_of(R, xbf), i1 - i0, SCORE_FTARGET, cf.zb, l2_tiles_for(C, esize_of(dtype), 1, cf.zb));
    p.nchunk = ch.nchunk; p.zchunk = ch.zchunk;
    hipStream_t st = (hipStream_t)stream;
    rc = dtype == EDGL_F32 ? fwd_dispatch<float>(p, C, st) : fwd_dispatch<bf16>(p, C, st);
    if (rc) return rc;
    if (row_lse) {
        hipLaunchKernelGGL(lse_combine_kernel, dim3((R + 255) / 256), dim3(256), 0, st, workspace, R, nvalid, xbf, cf.zb,
                           xblocks_of(R, xbf) * p.nchunk, i1 - i0, row_lse);
        EDGL_LAUNCH_CHECK();
    }
    if (labels) {
        if (dtype == EDGL_F32)
            hipLaunchKernelGGL((label_logit_kernel<float>), dim3((R + 3) / 4), dim3(256), 0, st, (const float*)rows, (const float*)table, out_bias, labels, R, C, i0, i1, label_logit);
        else
            hipLaunchKernelGGL((label_logit_kernel<bf16>), dim3((R + 3) / 4), dim3(256), 0, st, (const bf16*)rows, (const bf16*)table, out_bias, labels, R, C, i0, i1, label_logit);
        EDGL_LAUNCH_CHECK();
    }
    return EDGL_OK;
}

extern "C" long edgl_score_bwd_workspace(int R, int C, int I, int n_items, int dtype) {
    return plan_of(R, C, I, n_items, dtype, false).total;
}

extern "C" int edgl_score_ce_bwd(const void* rows, const void* table, const float* out_bias, const int64_t* labels,
                                 const float* row_lse, const float* coef, const float* gscale, int R, int C, int I,
                                 int i0, int i1, const int32_t* nvalid, void* d_rows, float* d_table, float* d_bias,
                                 float* workspace, int dtype, void* stream) {
    ScoreP p;
    const int rc = check_score(p, rows, table, out_bias, labels, R, C, I, i0, i1, nvalid, dtype, "edgl_score_ce_bwd");
    if (rc) return rc;
    EDGL_REQUIRE(labels && row_lse && coef && d_rows && d_table && d_bias && workspace, EDGL_ERR_NULL,
                 "edgl_score_ce_bwd: null pointer");
    p.row_lse = const_cast<float*>(row_lse); p.coef = coef; p.gscale = gscale;
    return score_run<0>(p, workspace, d_rows, d_table, d_bias, dtype, stream);
}

// ---- "flash" form: the forward scoring pass already accumulates the row gradients -------------------------------------------
// edgl_score_flash_fwd: ONE pass over the item table computes, per weighted row, the log-sum-exp of its logits (as
// edgl_score_lse_fwd) AND sum_z exp(logit_z - max) table[z] — the row gradient up to the loss coefficient — with flash-style
// running maxima; the label logits come from the same small gather kernel.  edgl_score_flash_bwd then finishes d_rows
// (divide by the row sum, apply coef, subtract the label row) and computes d_table / d_bias as edgl_score_ce_bwd does.
// The logits are computed 2x per step (here and in the d_table pass) instead of 3x.  `workspace` (edgl_score_flash_workspace
// floats) carries the slabs from the forward to the backward call and must not be touched in between.
extern "C" long edgl_score_flash_workspace(int R, int C, int I, int n_items, int dtype) {
    return plan_of(R, C, I, n_items, dtype, true).total;
}

// The transposed image of the item table depends on the weights only: edgl_score_prepare_table writes it into the flash
// workspace ahead of time (e.g. on a side stream at the start of the step) and edgl_score_flash_fwd_pre(table_ready = 1) then
// transposes the rows alone.  Same R, C, I, [i0, i1) and workspace as the forward call that follows.
extern "C" int edgl_score_prepare_table(const void* table, int R, int C, int I, int i0, int i1, float* workspace, int dtype,
                                        void* stream) {
    EDGL_REQUIRE(table && workspace, EDGL_ERR_NULL, "edgl_score_prepare_table: null pointer");
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_score_prepare_table: bad dtype %d", dtype);
    const BwdPlan plan = plan_of(R, C, I, i1 - i0, dtype, false);
    const long ldt = (long)up8(I);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((ldt + 63) / 64), (C + 63) / 64);
    if (dtype != EDGL_F32) return EDGL_OK;      // the bf16 kernels need no transposed image
    hipLaunchKernelGGL((transpose_kernel<float>), grid, dim3(256), 0, st, (const float*)table, (long)I, reinterpret_cast<float*>(workspace + plan.off_tableT), ldt,
                       (int)grid.x, (const float*)nullptr, 0L, (float*)nullptr, 0L, C);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
// (row LSE and label logits come out of one small kernel behind the scoring pass)
extern "C" int edgl_score_flash_fwd_pre(const void* rows, const void* table, const float* out_bias, const int64_t* labels, int R,
                                        int C, int I, int i0, int i1, const int32_t* nvalid, float* row_lse, float* label_logit,
                                        float* workspace, int table_ready, int dtype, void* stream) {
    ScoreP p;
    const int rc = check_score(p, rows, table, out_bias, labels, R, C, I, i0, i1, nvalid, dtype, "edgl_score_flash_fwd");
    if (rc) return rc;
    EDGL_REQUIRE(labels && row_lse && label_logit && workspace, EDGL_ERR_NULL, "edgl_score_flash_fwd: null pointer");
    p.row_lse = row_lse; p.lab_out = label_logit; p.table_ready = table_ready;
    return score_run<1>(p, workspace, nullptr, nullptr, nullptr, dtype, stream);
}
extern "C" int edgl_score_flash_fwd(const void* rows, const void* table, const float* out_bias, const int64_t* labels, int R,
                                    int C, int I, int i0, int i1, const int32_t* nvalid, float* row_lse, float* label_logit,
                                    float* workspace, int dtype, void* stream) {
    return edgl_score_flash_fwd_pre(rows, table, out_bias, labels, R, C, I, i0, i1, nvalid, row_lse, label_logit, workspace, 0, dtype, stream);
}
// edgl_score_flash_fwd over the whole table for COMPACTED rows (edgl_compact_*: the *nvalid weighted rows first, labels 0 behind
// them) that also writes the loss coefficients coef[r] = (1 / (n + 1e-5)) * p_y / (p_y + 1e-5), n = *nvalid — what edgl_ce_loss_fwd
// computes after a reduction over the rows; with them the backward does not wait for the loss kernel (EasyDGL.py:177-185).
// Data parallel form: `wtotal` (device, may be NULL) = weighted rows of the GLOBAL batch; the coefficients then are those of the
// global loss (EasyDGL.py:183-185 with the denominator summed over the ranks), and the ranks' gradients ADD UP to its gradient.
extern "C" int edgl_score_flash_fwd_coef_w(const void* rows, const void* table, const float* out_bias, const int64_t* labels, int R,
                                           int C, int I, const int32_t* nvalid, const int32_t* wtotal, float* row_lse,
                                           float* label_logit, float* coef, float* workspace, int dtype, void* stream) {
    ScoreP p;
    const int rc = check_score(p, rows, table, out_bias, labels, R, C, I, 0, I, nvalid, dtype, "edgl_score_flash_fwd_coef");
    if (rc) return rc;
    EDGL_REQUIRE(labels && row_lse && label_logit && workspace && nvalid && coef, EDGL_ERR_NULL,
                 "edgl_score_flash_fwd_coef: null pointer (the row count of the compaction is required)");
    p.row_lse = row_lse; p.lab_out = label_logit; p.coef_out = coef; p.wtotal = wtotal;
    return score_run<1>(p, workspace, nullptr, nullptr, nullptr, dtype, stream);
}
extern "C" int edgl_score_flash_fwd_coef(const void* rows, const void* table, const float* out_bias, const int64_t* labels, int R,
                                         int C, int I, const int32_t* nvalid, float* row_lse, float* label_logit, float* coef,
                                         float* workspace, int dtype, void* stream) {
    return edgl_score_flash_fwd_coef_w(rows, table, out_bias, labels, R, C, I, nvalid, nullptr, row_lse, label_logit, coef, workspace,
                                       dtype, stream);
}

// number of per-workgroup loss sums edgl_score_flash_fwd_rows_wp writes (0: this shape has no one-launch row finish)
extern "C" int edgl_score_ce_nparts(int R, int C) {
    if (!(C == 128 || C == 64 || C == 256 || C == 512) || R <= 0) return 0;
    const long lpr = C == 512 ? 64 : C / 4;      // (C = 512: eight channels per lane)
    return (int)std::min<long>(((long)R * lpr + 255) / 256, 4096);
}
// edgl_score_flash_fwd_coef_w that also finishes the rows: d_rows (= gscale * d loss / d rows, what edgl_score_flash_bwd would write)
// comes out of the same launch as lse / label logits / coefficients; edgl_score_flash_bwd is then called with d_rows = NULL and
// only runs the table side.  It also leaves the loss numerator as edgl_score_ce_nparts(R, C) per-workgroup sums in ce_part (NULL:
// none), for edgl_ce_loss_parts — the loss launch then reads nothing of the batch.
extern "C" int edgl_score_flash_fwd_rows_wp(const void* rows, const void* table, const float* out_bias, const int64_t* labels, int R,
                                            int C, int I, const int32_t* nvalid, const int32_t* wtotal, const float* gscale,
                                            float* row_lse, float* label_logit, float* coef, void* d_rows, float* ce_part,
                                            float* workspace, int dtype, void* stream) {
    ScoreP p;
    const int rc = check_score(p, rows, table, out_bias, labels, R, C, I, 0, I, nvalid, dtype, "edgl_score_flash_fwd_rows");
    if (rc) return rc;
    EDGL_REQUIRE(!ce_part || edgl_score_ce_nparts(R, C) > 0, EDGL_ERR_SHAPE, "edgl_score_flash_fwd_rows_wp: no per-workgroup loss sums at C=%d", C);
    EDGL_REQUIRE(labels && row_lse && label_logit && workspace && nvalid && coef && d_rows, EDGL_ERR_NULL,
                 "edgl_score_flash_fwd_rows: null pointer (the row count of the compaction is required)");
    p.row_lse = row_lse; p.lab_out = label_logit; p.coef_out = coef; p.wtotal = wtotal; p.gscale = gscale; p.ce_part = ce_part;
    return score_run<1>(p, workspace, d_rows, nullptr, nullptr, dtype, stream);
}
extern "C" int edgl_score_flash_fwd_rows_w(const void* rows, const void* table, const float* out_bias, const int64_t* labels, int R,
                                           int C, int I, const int32_t* nvalid, const int32_t* wtotal, const float* gscale,
                                           float* row_lse, float* label_logit, float* coef, void* d_rows, float* workspace,
                                           int dtype, void* stream) {
    return edgl_score_flash_fwd_rows_wp(rows, table, out_bias, labels, R, C, I, nvalid, wtotal, gscale, row_lse, label_logit, coef, d_rows,
                                        nullptr, workspace, dtype, stream);
}

extern "C" int edgl_score_flash_bwd_ex(const void* rows, const void* table, const float* out_bias, const int64_t* labels,
                                       const float* row_lse, const float* coef, const float* gscale, int R, int C, int I, int i0,
                                       int i1, const int32_t* nvalid, void* d_rows, float* d_table, float* d_bias,
                                       float* workspace, int defer_label_term, int dtype, void* stream) {
    ScoreP p;
    const int rc = check_score(p, rows, table, out_bias, labels, R, C, I, i0, i1, nvalid, dtype, "edgl_score_flash_bwd");
    if (rc) return rc;
    // d_rows == NULL: the rows were finished by edgl_score_flash_fwd_rows_w; only d_table / d_bias are computed
    EDGL_REQUIRE(labels && row_lse && coef && d_table && d_bias && workspace, EDGL_ERR_NULL,
                 "edgl_score_flash_bwd: null pointer");
    p.row_lse = const_cast<float*>(row_lse); p.coef = coef; p.gscale = gscale;
    p.defer_label = (defer_label_term & 1) != 0;
    p.acc_atomic = (defer_label_term & 2) != 0;      // (bf16, C = 128 strip path only; elsewhere the slabs)
    p.keep_slabs = (defer_label_term & 4) != 0 && (defer_label_term & 1) != 0 && !gscale && i0 == 0 && i1 == I;
    return score_run<2>(p, workspace, d_rows, d_table, d_bias, dtype, stream);
}
extern "C" int edgl_score_flash_bwd(const void* rows, const void* table, const float* out_bias, const int64_t* labels,
                                    const float* row_lse, const float* coef, const float* gscale, int R, int C, int I, int i0,
                                    int i1, const int32_t* nvalid, void* d_rows, float* d_table, float* d_bias,
                                    float* workspace, int dtype, void* stream) {
    return edgl_score_flash_bwd_ex(rows, table, out_bias, labels, row_lse, coef, gscale, R, C, I, i0, i1, nvalid, d_rows, d_table, d_bias,
                                   workspace, 0, dtype, stream);
}
// The one-hot part of dl = coef (p - onehot(label)) as its own call:  d_table[label[r]] -= gscale coef[r] rows[r],
// d_bias[label[r] - 1] -= gscale coef[r]  over the weighted rows (f32 atomics, commutes with every other accumulation into the two
// arrays).  edgl_score_flash_bwd_ex(defer_label_term = 1) leaves exactly this out WHERE ITS PRODUCT PASS DOES NOT CONTAIN IT (bf16,
// C = 128: the strip kernels) — edgl_score_flash_label_term is then a launch, and a no-op (return 0) for every other configuration,
// whose product kernels subtract the one-hot in place.  The training engine runs it on its side stream under the embedding backward.
extern "C" int edgl_score_flash_label_term(const void* rows, const int64_t* labels, const float* coef, const float* gscale, int R, int C,
                                           int I, int i0, int i1, const int32_t* nvalid, float* d_table, float* d_bias, int dtype,
                                           void* stream) {
    EDGL_REQUIRE(rows && labels && coef && d_table && d_bias, EDGL_ERR_NULL, "edgl_score_flash_label_term: null pointer");
    EDGL_REQUIRE(R > 0 && I > 1 && i0 >= 0 && i1 <= I && i0 < i1, EDGL_ERR_SHAPE, "edgl_score_flash_label_term: bad shape");
    if (!use_strip(C, esize_of(dtype))) return EDGL_OK;
    return edgl_strip_label_scatter(rows, labels, coef, nvalid, R, C, i0, i1, gscale, d_table, d_bias, (hipStream_t)stream);
}
// edgl_score_flash_label_term as an ordered sum over a sorted plan (k_segsum.hip): no f32 atomics, one writer per table row, the
// same no-op where the product pass already contains the one-hot term (EasyDGL.py:177-185).
extern "C" int edgl_score_flash_label_term_det(const void* rows, const int64_t* labels, const float* coef, const float* gscale, int R, int C,
                                               int I, int i0, int i1, const int32_t* nvalid, float* d_table, float* d_bias, void* plan,
                                               int dtype, void* stream) {
    EDGL_REQUIRE(rows && labels && coef && d_table && d_bias && plan, EDGL_ERR_NULL, "edgl_score_flash_label_term_det: null pointer");
    EDGL_REQUIRE(R > 0 && I > 1 && i0 >= 0 && i1 <= I && i0 < i1, EDGL_ERR_SHAPE, "edgl_score_flash_label_term_det: bad shape");
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_score_flash_label_term_det: bad dtype %d", dtype);
    if (!use_strip(C, esize_of(dtype))) return EDGL_OK;
    return edgl_segsum_label(rows, labels, coef, gscale, R, C, I, i0, i1, nvalid, d_table, d_bias, plan, dtype, (hipStream_t)stream);
}

// Where edgl_score_flash_bwd_ex(defer_label_term & 4) leaves the partial table / bias gradients: out[0] / out[1] = float offsets of the
// [nslab][I * C] and [nslab][I - 1] slabs inside the flash workspace, out[2] = nslab.  Depends on the shape only.
extern "C" int edgl_score_flash_slab_info(int R, int C, int I, int n_items, int dtype, long* out) {
    EDGL_REQUIRE(out && (dtype == EDGL_F32 || dtype == EDGL_BF16), EDGL_ERR_NULL, "edgl_score_flash_slab_info: bad arguments");
    const BwdPlan plan = plan_of(R, C, I, n_items, dtype, true);
    out[0] = plan.off_slabW; out[1] = plan.off_slabB; out[2] = plan.w.nchunk;
    return EDGL_OK;
}
