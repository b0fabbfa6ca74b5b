// =========================================================================================================================
// Backward of the chain of k_tail_fwd.hip in one launch per block: LN3' -> GELU' -> dX(Wt) -> LN2' -> dX(Wout) -> GELU' -> dX(Wi) -> LN1' ->
// dX(Wo).  The dX products contract over the layer's OUTPUT index, so their weight operand is the [in, out] kernel itself
// (a lane = one input channel k, 8 consecutive n) — no packed image, and the forward's tile_gemm with that kernel as the A operand:
// acc[rt] += W[k-tile rows][n0 .. n0 + 32*NKB) . G[rows of tile rt][same n].  What the weight-gradient GEMMs need (the gradients
// w.r.t. the four dense outputs) is written once; the LayerNorm parameter gradients leave as per-sample partials.
// Rounding points as in the unfused kernels (every tensor those write in the activation dtype is rounded here too).
// =========================================================================================================================
#include "tail2_common.h"

namespace {

// LayerNorm backward on registers: z = LN input sum, dy = upstream gradient; returns d(sum) in dz and writes the
// per-sample (dbeta | dgamma) partials of this wave's channels
// (STORE = false: the partials of lane l15 == 0 are only returned in dga / dbe — the two-per-CU kernel stores them with
// the store batch that ends its phase, so that no load of the phase waits behind them)
template <int CT, bool STORE>
__device__ __forceinline__ void ln_bwd_part(const float (&z)[MAXRT][4], const float (&dy)[MAXRT][4], float mean, float rstd,
                                            const float (&gv)[4], int nrt, int T, int lane, int nl, float* red, float* part_b,
                                            float (&dz)[MAXRT][4], const ChanPad& cp, float (&dga)[4], float (&dbe)[4]) {
    const int l15 = lane & 15;
    const float n = (float)T * cp.ctrue;      // (gamma is 0 on padded channels: they add nothing to s1 / s2)
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) dga[r] = dbe[r] = 0.f;
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt)
        if (rt < nrt && rt * 16 + l15 < T) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float xh = (z[rt][r] - mean) * rstd, gg = dy[rt][r] * gv[r];
                s1 += gg; s2 += gg * xh; dga[r] += dy[rt][r] * xh; dbe[r] += dy[rt][r];
            }
        }
    const float m1 = block_sum_lds(s1, red) / n;
    const float m2 = block_sum_lds(s2, red) / n;
#pragma unroll
    for (int r = 0; r < 4; ++r) {   // sum over the 16 rows held by the lanes of this lane group
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) { dga[r] += __shfl_xor(dga[r], o, 64); dbe[r] += __shfl_xor(dbe[r], o, 64); }
    }
    if (STORE && l15 == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { part_b[nl + r] = dbe[r]; part_b[16 * CT + nl + r] = dga[r]; }
    }
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float xh = (z[rt][r] - mean) * rstd;
            dz[rt][r] = cp.rm[r] * (rstd * (dy[rt][r] * gv[r] - m1 - xh * m2));      // nothing flows into a padded channel
            if (!STORE && r == 3) __builtin_amdgcn_sched_barrier(0);      // (two-per-CU form: one row tile at a time, 128 registers)
        }
}
// STORE = true for the one-per-CU kernel.  Not folded into its call sites: with dga / dbe declared there the register allocation of all
// six tail_bwd_kernel instantiations changes (same counts, other registers; profiles/tail_split.txt)
template <int CT>
__device__ __forceinline__ void ln_bwd_regs(const float (&z)[MAXRT][4], const float (&dy)[MAXRT][4], float mean, float rstd,
                                            const float (&gv)[4], int nrt, int T, int lane, int nl, float* red, float* part_b,
                                            float (&dz)[MAXRT][4], const ChanPad& cp) {
    float dga[4], dbe[4];
    ln_bwd_part<CT, true>(z, dy, mean, rstd, gv, nrt, T, lane, nl, red, part_b, dz, cp, dga, dbe);
}

template <int CT, int NRT>
__global__ __launch_bounds__(64 * CT) void tail_bwd_kernel(TailBwdP p) {
    using G = TailGeom<CT>;
    constexpr int C = G::C, LD = G::LD, NKB = C / 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* bufA = reinterpret_cast<bf16*>(smem);
    bf16* bufS = reinterpret_cast<bf16*>(smem + G::BUF);
    bf16* bufB = reinterpret_cast<bf16*>(smem + 2 * G::BUF);
    bf16* bufC = reinterpret_cast<bf16*>(smem + 3 * G::BUF);
    float* red = reinterpret_cast<float*>(smem + 4 * G::BUF);
    int* rowmap = reinterpret_cast<int*>(red + 64);          // [T] head of the chain of gathered rows naming position t
    int* nextj = rowmap + MAXRT * 16;                        // [M]
    int* mpos_s = nextj + 256;                               // [M] masked positions of this sample
    const int b = blockIdx.x, T = p.T, nrt = NRT ? NRT : (T + 15) / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g4 = (lane >> 4) * 4, l15 = lane & 15;
    const int n0 = wave * 16, nl = n0 + g4;
    const long row0 = (long)b * T;
    const ChanPad cpad = chan_pad<CT>(nl, p.dhp, p.dht);
    float z[MAXRT][4], dy[MAXRT][4], dz[MAXRT][4];
    // weight fragments of the next product, fetched one product ahead (see load_wfrags)
    WFrags<NKB> wf = p.head ? load_wfrags<NKB>(p.Wt + (long)n0 * C, C, lane) : load_wfrags<NKB>(p.Wout + (long)n0 * C, C, lane);
    PH_DECL
    RowImage<CT> im_o, im_a;      // o, a1: loaded one phase ahead

    if (p.head) {
        // ---- LN3' on the gathered rows, GELU' -> d_pre_t (EasyDGL.py:136-146 backward) ------------------------------------
        // the M gathered row gradients of this sample -> buffer C rows [0, M) (compacted-away rows as zeros): walking the
        // chains below against global memory cost one round trip per link and row tile (50 of the head block's 117 k cycles).
        // Their row indices are fetched first, so that the second hop travels with the two images.
        const bool staged = p.M <= MAXRT * 16;
        constexpr int NG = RowImage<CT>::NI;
        int gsrc[NG];
        if (staged && p.rowmap) {      // (uniform branch; straight-line loads inside)
#pragma unroll
            for (int i = 0; i < NG; ++i) gsrc[i] = p.rowmap[(long)b * p.M + min(RowImage<CT>::vec(i) / G::CV, p.M - 1)];
        } else {
#pragma unroll
            for (int i = 0; i < NG; ++i) gsrc[i] = b * p.M + min(RowImage<CT>::vec(i) / G::CV, p.M - 1);
        }
        const int my_pos = (int)p.mpos[(long)b * p.M + min((int)threadIdx.x, p.M - 1)];      // M <= 256 <= threads
        RowImage<CT> im_so, im_dg;
        im_so.load(p.so + row0 * C, C, T);
        im_dg.load(p.pre_t + row0 * C, C, T);
        if (staged) {
            uint4 g[NG];
#pragma unroll
            for (int i = 0; i < NG; ++i)
                g[i] = *reinterpret_cast<const uint4*>(p.d_rows + (long)max(gsrc[i], 0) * C + (RowImage<CT>::vec(i) % G::CV) * 8);
            im_so.store(bufB, T);
            im_dg.store(bufA, T);
#pragma unroll
            for (int i = 0; i < NG; ++i) {
                const int v = RowImage<CT>::vec(i), j = v / G::CV, cv = v % G::CV;
                if (j < p.M) *reinterpret_cast<uint4*>(bufC + j * LD + cv * 8) = gsrc[i] >= 0 ? g[i] : make_uint4(0, 0, 0, 0);
            }
        } else {
            im_so.store(bufB, T);
            im_dg.store(bufA, T);
        }
        if ((int)threadIdx.x < p.M) mpos_s[threadIdx.x] = my_pos;
        for (int t = threadIdx.x; t < MAXRT * 16; t += G::NTHR) rowmap[t] = -1;
        lds_barrier();
        // chains of the gathered rows naming one position, in ascending j (the order the unfused kernel sums in): row j links to
        // the next larger j' with the same position; the smallest j of a position is its head
        for (int j = threadIdx.x; j < p.M; j += G::NTHR) {
            const int t = mpos_s[j];
            int nxt = -1;
            bool first = true;
#pragma unroll 8
            for (int k = 0; k < p.M; ++k) {          // uniform trip count: the LDS reads of an unrolled group travel together
                const bool same = mpos_s[k] == t;
                nxt = (same && k > j && nxt < 0) ? k : nxt;
                first = first && !(same && k < j);
            }
            nextj[j] = nxt;
            if (first) rowmap[t] = j;
        }
        lds_barrier();
        // first link of every row tile's chain as straight-line code (heads, rows, next links: three rounds of LDS reads for
        // all seven tiles instead of three dependent reads per tile); longer chains — repeated positions — in the loop below
        int jn[MAXRT];
        {
            int jh[MAXRT];
#pragma unroll
            for (int rt = 0; rt < MAXRT; ++rt) {
                const int row = rt * 16 + l15;
                ld_bf4(bufB + row * LD + nl, z[rt]);
                jh[rt] = (rt < nrt && row < T) ? rowmap[row] : -1;
            }
#pragma unroll
            for (int rt = 0; rt < MAXRT; ++rt) {
                jn[rt] = nextj[max(jh[rt], 0)];
                if (staged) {
                    ld_bf4(bufC + max(jh[rt], 0) * LD + nl, dy[rt]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) dy[rt][r] = jh[rt] >= 0 ? dy[rt][r] : 0.f;
                    jn[rt] = jh[rt] >= 0 ? jn[rt] : -1;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) dy[rt][r] = 0.f;
                    jn[rt] = jh[rt];
                }
            }
        }
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt)
            for (int j = jn[rt]; j >= 0; j = nextj[j]) {
                float v[4];
                if (staged) {
                    ld_bf4(bufC + j * LD + nl, v);
                } else {
                    long src = (long)b * p.M + j;
                    if (p.rowmap) src = p.rowmap[src];
                    if (src < 0) continue;
                    ld_bf4(p.d_rows + src * C + nl, v);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) dy[rt][r] += v[r];
            }
        PH_MARK(0);   // head inputs, gathered row gradients
        {
            const float4 gg = *reinterpret_cast<const float4*>(p.g3 + nl);
            const float gv[4] = {gg.x, gg.y, gg.z, gg.w};
            ln_bwd_regs<CT>(z, dy, p.st3[2 * b], p.st3[2 * b + 1], gv, nrt, T, lane, nl, red, p.part3 + (long)b * 2 * C, dz, cpad);
        }
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt)
            if (rt < nrt) {
                const int row = rt * 16 + l15;
                float dg[4];
                ld_bf4(bufA + row * LD + nl, dg);
                const float v[4] = {dz[rt][0] * dg[0], dz[rt][1] * dg[1], dz[rt][2] * dg[2], dz[rt][3] * dg[3]};
                st_bf4(bufC + row * LD + nl, v);
            }
        lds_barrier();
        copy_out<CT>(p.d_pre_t + row0 * C, C, bufC, T);
        // ---- d_y = d_pre_t . Wt^T ----------------------------------------------------------------------------------------------
        // (the next phase's two images are requested here: their round trip runs under this product and its barrier)
        im_o.load(p.o + row0 * C, C, T);
        im_a.load(p.a1 + row0 * C, C, T);
        EDGL_PIN();
        f32x4 acc[MAXRT];
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        tile_gemm<CT, NKB>(wf, bufC, nrt, lane, acc);
        wf = load_wfrags<NKB>(p.Wout + (long)n0 * C, C, lane);
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) dy[rt][r] = rbf(acc[rt][r]);
        lds_barrier();     // bufA / bufB / bufC are rewritten below
        PH_MARK(1);   // LN3', gelu', dX(Wt)
    } else {
        im_o.load(p.o + row0 * C, C, T);
        im_a.load(p.a1 + row0 * C, C, T);
        EDGL_PIN();
        copy_in<CT>(bufA, p.d_y_in + row0 * C, C, T);
        lds_barrier();
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt) ld_bf4(bufA + (rt * 16 + l15) * LD + nl, dy[rt]);
        lds_barrier();
    }
    // ---- LN2': z2 = drop(o) + a1 ; d_o = drop(d_z2) ; d_a1 (residual part) = d_z2 (EasyDGL.py:126-128 backward) -----------------
    // (the dropout keys hang on a load of the generator state: created here, not ahead of the head's loads)
    const DropKey dk1 = make_dropkey(p.rng, p.sid1, p.rate), dk2 = make_dropkey(p.rng, p.sid2, p.rate);
    im_o.store(bufA, T);
    im_a.store(bufB, T);
    lds_barrier();
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt) {
        const int row = rt * 16 + l15;
        float ov[4], av[4];
        ld_bf4(bufA + row * LD + nl, ov);
        ld_bf4(bufB + row * LD + nl, av);
        drop_apply4(dk2, (uint64_t)((row0 + min(row, T - 1)) * C + nl), ov);
#pragma unroll
        for (int r = 0; r < 4; ++r) z[rt][r] = ov[r] + av[r];
    }
    RowImage<CT> im_p;            // gelu'(pre_f) half: requested one phase ahead as well
    im_p.load(p.pre_f + row0 * 2 * C, 2 * C, T);
    EDGL_PIN();
    PH_MARK(2);   // o, a1 -> z2
    {
        const float4 gg = *reinterpret_cast<const float4*>(p.g2 + nl);
        const float gv[4] = {gg.x, gg.y, gg.z, gg.w};
        ln_bwd_regs<CT>(z, dy, p.st2[2 * b], p.st2[2 * b + 1], gv, nrt, T, lane, nl, red, p.part2 + (long)b * 2 * C, dz, cpad);
    }
    float da1[MAXRT][4];   // gradient w.r.t. a1: the residual branch now, + d_pre_f . Wi^T below
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt)
        if (rt < nrt) {
            const int row = rt * 16 + l15;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                da1[rt][r] = rbf(dz[rt][r]);
                v[r] = dz[rt][r];
            }
            drop_apply4(dk2, (uint64_t)((row0 + min(row, T - 1)) * C + nl), v);
            st_bf4(bufC + row * LD + nl, v);
        }
    lds_barrier();
    copy_out<CT>(p.d_o + row0 * C, C, bufC, T);
    PH_MARK(3);   // LN2', d_o
    // ---- d_pre_f = (d_o . Wout^T) * gelu'(pre_f), two halves of the 2C hidden channels; d_a1 += d_pre_f . Wi^T -------------------
    f32x4 acc6[MAXRT];
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt) acc6[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int h = 0; h < 2; ++h) {
        im_p.store(bufA, T);
        {
            f32x4 acc[MAXRT];
#pragma unroll
            for (int rt = 0; rt < MAXRT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
            tile_gemm<CT, NKB>(wf, bufC, nrt, lane, acc);
            wf = load_wfrags<NKB>(p.Wi + (long)n0 * 2 * C + h * C, 2 * C, lane);
            lds_barrier();   // gelu'(pre_f half) in place (and, for h = 1, every wave past its reads of the previous d_pre_f half)
#pragma unroll
            for (int rt = 0; rt < MAXRT; ++rt)
                if (rt < nrt) {
                    const int row = rt * 16 + l15;
                    float dg[4];
                    ld_bf4(bufA + row * LD + nl, dg);
                    const float v[4] = {acc[rt][0] * dg[0], acc[rt][1] * dg[1], acc[rt][2] * dg[2], acc[rt][3] * dg[3]};
                    st_bf4(bufB + row * LD + nl, v);
                }
        }
        lds_barrier();
        if (h == 0) {   // the other half's image / the two images of the LN1' phase travel under the rest of this half
            im_p.load(p.pre_f + row0 * 2 * C + C, 2 * C, T);
        } else {
            im_o.load(p.ao + row0 * C, C, T);
            im_a.load(p.xin + row0 * p.ld_x, p.ld_x, T);
        }
        EDGL_PIN();
        copy_out<CT>(p.d_pre_f + row0 * 2 * C + h * C, 2 * C, bufB, T);
        tile_gemm<CT, NKB>(wf, bufB, nrt, lane, acc6);
        wf = h == 0 ? load_wfrags<NKB>(p.Wout + (long)(C + n0) * C, C, lane) : load_wfrags<NKB>(p.Wo + (long)n0 * C, C, lane);
        lds_barrier();
    }
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) dy[rt][r] = rbf(acc6[rt][r] + da1[rt][r]);
    PH_MARK(4);   // the two halves of the hidden layer
    // ---- LN1': z1 = drop(ao) + x_in ; d_ao = drop(d_z1) ; d_res1 = d_z1 (EasyDGL.py:113-116 backward) ------------------------------
    im_o.store(bufA, T);
    im_a.store(bufB, T);
    lds_barrier();
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt) {
        const int row = rt * 16 + l15;
        float ov[4], xv[4];
        ld_bf4(bufA + row * LD + nl, ov);
        ld_bf4(bufB + row * LD + nl, xv);
        drop_apply4(dk1, (uint64_t)((row0 + min(row, T - 1)) * C + nl), ov);
#pragma unroll
        for (int r = 0; r < 4; ++r) z[rt][r] = ov[r] + xv[r];
    }
    PH_MARK(5);   // ao, x_in -> z1
    {
        const float4 gg = *reinterpret_cast<const float4*>(p.g1 + nl);
        const float gv[4] = {gg.x, gg.y, gg.z, gg.w};
        ln_bwd_regs<CT>(z, dy, p.st1[2 * b], p.st1[2 * b + 1], gv, nrt, T, lane, nl, red, p.part1 + (long)b * 2 * C, dz, cpad);
    }
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt)
        if (rt < nrt) {
            const int row = rt * 16 + l15;
            float v[4], w[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                w[r] = dz[rt][r];
                v[r] = dz[rt][r];
            }
            drop_apply4(dk1, (uint64_t)((row0 + min(row, T - 1)) * C + nl), v);
            st_bf4(bufC + row * LD + nl, v);
            st_bf4(bufS + row * LD + nl, w);
        }
    lds_barrier();
    copy_out<CT>(p.d_ao + row0 * C, C, bufC, T);
    copy_out<CT>(p.d_res1 + row0 * C, C, bufS, T);
    PH_MARK(6);   // LN1', d_ao, d_res1
    // ---- d_att = d_ao . Wo^T ---------------------------------------------------------------------------------------------------------
    {
        f32x4 acc[MAXRT];
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        tile_gemm<CT, NKB>(wf, bufC, nrt, lane, acc);
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt)
            if (rt < nrt) {
                const float v[4] = {acc[rt][0], acc[rt][1], acc[rt][2], acc[rt][3]};
                st_bf4(bufA + (rt * 16 + l15) * LD + nl, v);
            }
    }
    lds_barrier();
    copy_out<CT>(p.d_att + row0 * C, C, bufA, T);
    PH_MARK(7);   // dX(Wo), d_att
    PH_FLUSH(0);
}

// ---- backward on half a CU (the form: tail2_common.h) -------------------------------------------------------------------------------
namespace t2 {
// This lane's quads (4 channels, one row per row tile: the accumulator layout) of a global [T, 128] tensor, 8 bytes per lane and row
// tile; rows past the sequence repeat row T - 1 (nothing consumes them: every sum and every store is guarded by row < T).
struct Quads { uint2 q[MAXRT]; };
template <int NRT>
__device__ __forceinline__ Quads load_quads(const bf16* src, int ld, int T) {
    Quads a;
    // uniform base + 32-bit lane offset (one address register per load, not two), rebuilt by every call: held, the clamped offsets of
    // all row tiles are seven registers per row stride
    const Lane L = fresh_lane();
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
        a.q[rt] = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(src) + (uint32_t)((min(rt * 16 + L.l15, T - 1) * ld + L.nl) * 2));
#pragma unroll
    for (int rt = NRT; rt < MAXRT; ++rt) a.q[rt] = make_uint2(0u, 0u);
    return a;
}
__device__ __forceinline__ void quad_f32(const uint2& q, float (&v)[4]) {
    Frag4<bf16> f;
    *reinterpret_cast<uint2*>(&f) = q;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = to_f32(f.v[r]);
}
// byte offset of this lane's 4 channels in row `row` of an image (any row: the gathered rows of the head)
__device__ __forceinline__ int quad_off(int row, const Lane& L) {
    return row * 256 + (((L.wave * 2 + (L.q >> 1)) ^ (row & 15)) << 4) + ((L.q & 1) << 3);
}
// per-sample (dbeta | dgamma) partials of this wave's channels (ln_bwd_part<8, false>)
__device__ __forceinline__ void store_part(float* part_b, const Lane& L, const float (&dga)[4], const float (&dbe)[4]) {
    if (L.l15 == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { part_b[L.nl + r] = dbe[r]; part_b[C + L.nl + r] = dga[r]; }
    }
}

// The chain of tail_bwd_kernel with three images and <= 128 registers (the register plan of the block comment above).
//   images: head  P = gathered row gradients [M] (rows >= 101 run into Q, which is free then), R = d_pre_t
//           LN2'  P = d_a1 (residual part; bf16 exactly: it was rounded through the activation dtype anyway), Q = d_o
//           hidden layer  R = d_pre_f half (product operand and copy-out source)
//           LN1'  Q = d_ao, R = d_res1, P = d_att
//   LayerNorm inputs (so, o / a1, ao / x_in), gelu' factors (pre_t, pre_f halves) and d_y_in arrive as quads straight from global
//   memory: no image, no barrier, 14 registers per tensor.
//   Load order: every quad set and every weight-fragment set is requested at the END of the segment in front of its use — behind the
//   epilogue that frees the registers and behind the segment's store batch (copy_out) — and waited for where it is used.  Nothing
//   is requested a whole segment ahead: a fragment set held across a LayerNorm (z + dy + the sums: 66 registers) spilled, and a
//   reload from scratch waits on vmcnt like any load.  Requesting the loads IN FRONT of the store batch and pinning their wait
//   there (rule 62, worth 5 us in the forward) was built and measured: 79.2 us against 77.5 us for this order at 512 samples, no
//   difference at 256 (profiles/tail_bwd2_ab.txt) — with a second workgroup on the CU the wait behind the stores is hidden, and
//   the pinned wait only delays the stores.  Not kept.  What stays of that rule costs nothing: the per-sample LayerNorm partials
//   (256 floats per LayerNorm) leave with the store batch, not from inside the LayerNorm, and the saved moments are read in the
//   prologue (behind a store a uniform load is a vector load like any other).
//   The epilogue loops end every row tile with a scheduling fence ("one row tile at a time"): left alone, the scheduler interleaves
//   the seven tiles of a loop for latency's sake — the dropout hashes and conversions of all of them at once, ~80 registers — and
//   at four waves per SIMD the other waves are what hides that latency.
template <int NRT>
__global__ __launch_bounds__(NTHR, 4) void tail2_bwd_kernel(TailBwdP p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const P = smem; char* const Q = smem + IMG; char* const R = smem + 2 * IMG;
    float* red = reinterpret_cast<float*>(smem + OFF_RED);
    int* rowmap = reinterpret_cast<int*>(smem + OFF_ROWMAP);      // [T] head of the chain of gathered rows naming position t
    int* nextj = reinterpret_cast<int*>(smem + OFF_NEXTJ);        // [M]
    int* mpos_s = reinterpret_cast<int*>(smem + OFF_MPOS);        // [M] masked positions of this sample
    float* gam = reinterpret_cast<float*>(smem + OFF_GAM);
    const int b = blockIdx.x, T = p.T;
    const Lane L = make_lane();
    const int n0 = L.wave * 16, nl = L.nl, l15 = L.l15;
    const long row0 = (long)b * T;
    // the padded-channel mask is rebuilt in front of each LayerNorm (opaque copy of nl): held for the whole kernel it went to scratch, and
    // a reload from scratch waits on vmcnt — behind the stores
    auto make_cpad = [&]() { int n = nl; asm volatile("" : "+v"(n)); return chan_pad<8>(n, p.dhp, p.dht); };
    const uint64_t idx0 = (uint64_t)((row0 + l15) * C + nl);       // dropout element index of this lane's quad in row tile 0 (+ rt * 16 * C)
    PH_DECL
    if ((int)threadIdx.x < C) {
        const int c = threadIdx.x;
        const float* g3_or = p.head ? p.g3 : p.g1;
        const float x0 = p.g1[c], x1 = p.g2[c], x2 = g3_or[c];
        gam[c] = x0; gam[C + c] = x1; gam[2 * C + c] = x2;
    }
    DropKey dk1 = make_dropkey(p.rng, p.sid1, p.rate), dk2 = make_dropkey(p.rng, p.sid2, p.rate);     // wave-uniform: scalar registers,
    dk1.scale = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(dk1.scale)));                // the scale (a division) too
    dk2.scale = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(dk2.scale)));
    // the moments the forward saved, read in front of the first store (scalar registers): behind one, a uniform load is a vector load
    // like any other and its wait would stand behind the store batch of the segment before
    auto uni = [](float v) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v))); };
    const float* st3_or = p.head ? p.st3 : p.st1;
    const float mean1 = uni(p.st1[2 * b]), rstd1 = uni(p.st1[2 * b + 1]), mean2 = uni(p.st2[2 * b]), rstd2 = uni(p.st2[2 * b + 1]),
                mean3 = uni(st3_or[2 * b]), rstd3 = uni(st3_or[2 * b + 1]);
    float z[MAXRT][4], dy[MAXRT][4], dz[MAXRT][4], dga[4], dbe[4];
    f32x4 acc[MAXRT];
    WFrags<NKB> wf;
    Quads qa, qb;

    if (p.head) {
        // ---- LN3' on the gathered rows, GELU' -> d_pre_t (EasyDGL.py:136-146 backward) ------------------------------------
        // the M <= 112 gathered row gradients of this sample -> image P rows [0, M) (compacted-away rows as zeros); their row indices
        // are fetched first, so that the second hop travels with the so quads
        int gsrc[4];
        if (p.rowmap) {      // (uniform branch; straight-line loads inside)
#pragma unroll
            for (int i = 0; i < 4; ++i) gsrc[i] = p.rowmap[(long)b * p.M + min((int)(threadIdx.x + i * NTHR) >> 4, p.M - 1)];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) gsrc[i] = b * p.M + min((int)(threadIdx.x + i * NTHR) >> 4, p.M - 1);
        }
        const int my_pos = (int)p.mpos[(long)b * p.M + min((int)threadIdx.x, p.M - 1)];      // M <= 112 <= threads
        qa = load_quads<NRT>(p.so + row0 * C, C, T);
        qb = load_quads<NRT>(p.pre_t + row0 * C, C, T);
        {
            uint4 g[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) g[i] = *reinterpret_cast<const uint4*>(p.d_rows + (long)max(gsrc[i], 0) * C + (threadIdx.x & 15) * 8);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = (int)(threadIdx.x + i * NTHR) >> 4;
                if (j < p.M) *reinterpret_cast<uint4*>(P + vec_off(j, threadIdx.x & 15)) = gsrc[i] >= 0 ? g[i] : make_uint4(0, 0, 0, 0);
            }
        }
        if ((int)threadIdx.x < p.M) mpos_s[threadIdx.x] = my_pos;
        if ((int)threadIdx.x < MAXRT * 16) rowmap[threadIdx.x] = -1;
        lds_barrier();
        // chains of the gathered rows naming one position, in ascending j (the order the unfused kernel sums in): row j links to
        // the next larger j' with the same position; the smallest j of a position is its head
        if ((int)threadIdx.x < p.M) {
            const int j = threadIdx.x, t = mpos_s[j];
            int nxt = -1;
            bool first = true;
#pragma unroll 8
            for (int k = 0; k < p.M; ++k) {
                const bool same = mpos_s[k] == t;
                nxt = (same && k > j && nxt < 0) ? k : nxt;
                first = first && !(same && k < j);
            }
            nextj[j] = nxt;
            if (first) rowmap[t] = j;
        }
        lds_barrier();
        // first link of every row tile's chain as straight-line code; longer chains — repeated positions — in the loop below
        int jn[MAXRT];
        {
            int jh[MAXRT];
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt) {
                const int row = rt * 16 + l15;
                quad_f32(qa.q[rt], z[rt]);
                jh[rt] = row < T ? rowmap[row] : -1;
                __builtin_amdgcn_sched_barrier(0);      // (one row tile at a time)
            }
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt) {
                jn[rt] = nextj[max(jh[rt], 0)];
                ld_bf4(reinterpret_cast<const bf16*>(P + quad_off(max(jh[rt], 0), L)), dy[rt]);
#pragma unroll
                for (int r = 0; r < 4; ++r) dy[rt][r] = jh[rt] >= 0 ? dy[rt][r] : 0.f;
                jn[rt] = jh[rt] >= 0 ? jn[rt] : -1;
                __builtin_amdgcn_sched_barrier(0);      // (one row tile at a time)
            }
        }
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt)
            for (int j = jn[rt]; j >= 0; j = nextj[j]) {
                float v[4];
                ld_bf4(reinterpret_cast<const bf16*>(P + quad_off(j, L)), v);
#pragma unroll
                for (int r = 0; r < 4; ++r) dy[rt][r] += v[r];
            }
        PH_MARK(0);   // head inputs, gathered row gradients
        {
            const float4 gg = *reinterpret_cast<const float4*>(gam + 2 * C + nl);
            const float gv[4] = {gg.x, gg.y, gg.z, gg.w};
            ln_bwd_part<8, false>(z, dy, mean3, rstd3, gv, NRT, T, L.lane, nl, red, nullptr, dz, make_cpad(), dga, dbe);
        }
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) {
            float dg[4];
            quad_f32(qb.q[rt], dg);
            const float v[4] = {dz[rt][0] * dg[0], dz[rt][1] * dg[1], dz[rt][2] * dg[2], dz[rt][3] * dg[3]};
            if (rt * 16 + l15 < T) st_bf4(reinterpret_cast<bf16*>(R + L.quad + rt * 4096), v);
            __builtin_amdgcn_sched_barrier(0);      // (one row tile at a time)
        }
        lds_barrier();
        store_part(p.part3 + (long)b * 2 * C, L, dga, dbe);
        copy_out(p.d_pre_t + row0 * C, C, R, T);
        // the product's fragments and the next phase's inputs (behind the store batch: see the kernel's header comment)
        EDGL_PIN();
        wf = load_wfrags<NKB>(p.Wt + (long)n0 * C, C, L.lane);
        qa = load_quads<NRT>(p.o + row0 * C, C, T);
        qb = load_quads<NRT>(p.a1 + row0 * C, C, T);
        // ---- d_y = d_pre_t . Wt^T ----------------------------------------------------------------------------------------------
        zero_acc<NRT>(acc);
        gemm<NRT>(wf, R, fresh_lane(), acc);
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) dy[rt][r] = rbf(acc[rt][r]);
        PH_MARK(1);   // LN3', gelu', dX(Wt)
    } else {
        qa = load_quads<NRT>(p.d_y_in + row0 * C, C, T);
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) quad_f32(qa.q[rt], dy[rt]);
        qa = load_quads<NRT>(p.o + row0 * C, C, T);
        qb = load_quads<NRT>(p.a1 + row0 * C, C, T);
        lds_barrier();      // (the gamma table)
        touch_regs(qa); touch_regs(qb);      // as on the head's side: no wait of the code below is left to be merged with its stores in flight
    }
    // ---- LN2': z2 = drop(o) + a1 ; d_o = drop(d_z2) ; d_a1 (residual part) = d_z2 (EasyDGL.py:126-128 backward) -----------------
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) {
        float ov[4], av[4];
        quad_f32(qa.q[rt], ov);
        quad_f32(qb.q[rt], av);
        drop_apply4(dk2, idx0 + (uint64_t)(rt * 16 * C), ov);
#pragma unroll
        for (int r = 0; r < 4; ++r) z[rt][r] = ov[r] + av[r];
        __builtin_amdgcn_sched_barrier(0);      // (one row tile at a time)
    }
    PH_MARK(2);   // o, a1 -> z2
    {
        const float4 gg = *reinterpret_cast<const float4*>(gam + C + nl);
        const float gv[4] = {gg.x, gg.y, gg.z, gg.w};
        ln_bwd_part<8, false>(z, dy, mean2, rstd2, gv, NRT, T, L.lane, nl, red, nullptr, dz, make_cpad(), dga, dbe);
    }
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) {
        float v[4], w[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            w[r] = rbf(dz[rt][r]);      // gradient w.r.t. a1: the residual branch now, + d_pre_f . Wi^T below
            v[r] = dz[rt][r];
        }
        drop_apply4(dk2, idx0 + (uint64_t)(rt * 16 * C), v);
        if (rt * 16 + l15 < T) {
            st_bf4(reinterpret_cast<bf16*>(P + L.quad + rt * 4096), w);
            st_bf4(reinterpret_cast<bf16*>(Q + L.quad + rt * 4096), v);
        }
        __builtin_amdgcn_sched_barrier(0);      // (one row tile at a time)
    }
    lds_barrier();
    store_part(p.part2 + (long)b * 2 * C, L, dga, dbe);
    copy_out(p.d_o + row0 * C, C, Q, T);
    EDGL_PIN();
    qa = load_quads<NRT>(p.pre_f + row0 * 2 * C, 2 * C, T);        // gelu'(pre_f), first half
    wf = load_wfrags<NKB>(p.Wout + (long)n0 * C, C, L.lane);
    WFrags<NKB> wi = load_wfrags<NKB>(p.Wi + (long)n0 * 2 * C, 2 * C, L.lane);
    PH_MARK(3);   // LN2', d_o
    // ---- d_pre_f = (d_o . Wout^T) * gelu'(pre_f), two halves of the 2C hidden channels; d_a1 += d_pre_f . Wi^T -------------------
    f32x4 acc6[MAXRT];
    zero_acc<NRT>(acc6);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        // product and epilogue row tile by row tile: all seven accumulator tiles beside acc6 (56 registers) do not fit
        const Lane F = fresh_lane();
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) {
            f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) a = mma_kblock(wf.w[kb], *reinterpret_cast<const Vec16<bf16>*>(Q + F.frag[kb] + rt * 4096), a);
            float dg[4];
            quad_f32(qa.q[rt], dg);
            const float v[4] = {a[0] * dg[0], a[1] * dg[1], a[2] * dg[2], a[3] * dg[3]};
            if (rt * 16 + l15 < T) st_bf4(reinterpret_cast<bf16*>(R + L.quad + rt * 4096), v);
            if (rt & 1) __builtin_amdgcn_sched_barrier(0);      // two row tiles in flight
        }
        if (h == 1) {      // (not earlier: beside the first half's second product there was no room for a third fragment set)
            EDGL_PIN();
            wi = load_wfrags<NKB>(p.Wi + (long)n0 * 2 * C + C, 2 * C, L.lane);
        }
        lds_barrier();
        copy_out(p.d_pre_f + row0 * 2 * C + h * C, 2 * C, R, T);
        // (the accumulator tiles of the product above are dead: room for the operands of what follows this half)
        EDGL_PIN();
        if (h == 0) {
            qa = load_quads<NRT>(p.pre_f + row0 * 2 * C + C, 2 * C, T);
            wf = load_wfrags<NKB>(p.Wout + (long)(C + n0) * C, C, L.lane);
        } else {
            qa = load_quads<NRT>(p.ao + row0 * C, C, T);
            qb = load_quads<NRT>(p.xin + row0 * p.ld_x, p.ld_x, T);
        }
        gemm<NRT>(wi, R, fresh_lane(), acc6);
        lds_barrier();      // every wave is past its reads of this half's d_pre_f image
    }
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) {
        float da[4];
        ld_bf4(reinterpret_cast<const bf16*>(P + L.quad + rt * 4096), da);
#pragma unroll
        for (int r = 0; r < 4; ++r) dy[rt][r] = rbf(acc6[rt][r] + da[r]);
        __builtin_amdgcn_sched_barrier(0);      // (one row tile at a time)
    }
    PH_MARK(4);   // the two halves of the hidden layer
    // ---- LN1': z1 = drop(ao) + x_in ; d_ao = drop(d_z1) ; d_res1 = d_z1 (EasyDGL.py:113-116 backward) ------------------------------
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) {
        float ov[4], xv[4];
        quad_f32(qa.q[rt], ov);
        quad_f32(qb.q[rt], xv);
        drop_apply4(dk1, idx0 + (uint64_t)(rt * 16 * C), ov);
#pragma unroll
        for (int r = 0; r < 4; ++r) z[rt][r] = ov[r] + xv[r];
        __builtin_amdgcn_sched_barrier(0);      // (one row tile at a time)
    }
    PH_MARK(5);   // ao, x_in -> z1
    {
        const float4 gg = *reinterpret_cast<const float4*>(gam + nl);
        const float gv[4] = {gg.x, gg.y, gg.z, gg.w};
        ln_bwd_part<8, false>(z, dy, mean1, rstd1, gv, NRT, T, L.lane, nl, red, nullptr, dz, make_cpad(), dga, dbe);
    }
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) {
        float v[4], w[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            w[r] = dz[rt][r];
            v[r] = dz[rt][r];
        }
        drop_apply4(dk1, idx0 + (uint64_t)(rt * 16 * C), v);
        if (rt * 16 + l15 < T) {
            st_bf4(reinterpret_cast<bf16*>(Q + L.quad + rt * 4096), v);
            st_bf4(reinterpret_cast<bf16*>(R + L.quad + rt * 4096), w);
        }
        __builtin_amdgcn_sched_barrier(0);      // (one row tile at a time)
    }
    lds_barrier();
    store_part(p.part1 + (long)b * 2 * C, L, dga, dbe);
    copy_out(p.d_ao + row0 * C, C, Q, T);
    copy_out(p.d_res1 + row0 * C, C, R, T);
    EDGL_PIN();
    wf = load_wfrags<NKB>(p.Wo + (long)n0 * C, C, L.lane);
    PH_MARK(6);   // LN1', d_ao, d_res1
    // ---- d_att = d_ao . Wo^T -> P (d_a1 is consumed, by the lanes that now overwrite it) --------------------------------------------
    zero_acc<NRT>(acc);
    gemm<NRT>(wf, Q, fresh_lane(), acc);
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) {
        const float v[4] = {acc[rt][0], acc[rt][1], acc[rt][2], acc[rt][3]};
        if (rt * 16 + l15 < T) st_bf4(reinterpret_cast<bf16*>(P + L.quad + rt * 4096), v);
        __builtin_amdgcn_sched_barrier(0);      // (one row tile at a time)
    }
    lds_barrier();
    copy_out(p.d_att + row0 * C, C, P, T);
    PH_MARK(7);   // dX(Wo), d_att
    PH_FLUSH(0);
}

}  // namespace t2

}  // namespace

extern "C" int edgl_tail_bwd_ct(const void* xin, int ld_x, const void* ao, const void* a1, const void* pre_f, const void* o,
                             const void* pre_t, const void* so, const float* st1, const float* st2, const float* st3,
                             const void* Wo, const void* Wi, const void* Wout, const void* Wt, const float* g1, const float* g2,
                             const float* g3, int B, int T, int C, float drop_rate, const uint64_t* rng_state, uint32_t sid1,
                             uint32_t sid2, int head, const void* d_rows, const int64_t* masked_pos, int M,
                             const int32_t* dy_rowmap, const void* d_y_in, void* d_pre_t, void* d_o, void* d_pre_f, void* d_ao,
                             void* d_res1, void* d_att, float* dg1, float* db1, float* dg2, float* db2, float* dg3, float* db3,
                             float* workspace, int dh_pad, int dh_true, int dtype, void* stream) {
    EDGL_REQUIRE(xin && ao && a1 && pre_f && o && st1 && st2 && Wo && Wi && Wout && g1 && g2 && d_o && d_pre_f && d_ao && d_res1 &&
                 d_att && dg1 && db1 && dg2 && db2 && workspace, EDGL_ERR_NULL, "edgl_tail_bwd: null pointer");
    EDGL_REQUIRE(head ? (pre_t && so && st3 && Wt && g3 && d_rows && masked_pos && d_pre_t && dg3 && db3 && M >= 1 && M <= 256) : (d_y_in != nullptr),
                 EDGL_ERR_NULL, "edgl_tail_bwd: head needs its tensors (M <= 256); without it d_y_in is the upstream gradient");
    if (const int rc = tail_check("edgl_tail_bwd", "", B, T, C, ld_x, dtype, drop_rate, rng_state, dh_pad, dh_true)) return rc;
    float* part1 = workspace; float* part2 = workspace + (long)B * 2 * C; float* part3 = workspace + (long)B * 4 * C;
    TailBwdP p{(const bf16*)xin, ld_x, (const bf16*)ao, (const bf16*)a1, (const bf16*)pre_f, (const bf16*)o, (const bf16*)pre_t,
               (const bf16*)so, st1, st2, st3, (const bf16*)Wo, (const bf16*)Wi, (const bf16*)Wout, (const bf16*)Wt, g1, g2, g3, B, T, C,
               drop_rate, rng_state, sid1, sid2, head, (const bf16*)d_rows, masked_pos, M, dy_rowmap, (const bf16*)d_y_in,
               (bf16*)d_pre_t, (bf16*)d_o, (bf16*)d_pre_f, (bf16*)d_ao, (bf16*)d_res1, (bf16*)d_att, part1, part2, part3, dh_pad, dh_true};
    hipStream_t st = (hipStream_t)stream;
    // two workgroups per CU (see namespace t2; the switch lives in k_tail_fwd.hip); the unstaged head path (M > 112) keeps the one-per-CU kernel
    if (edgl_tail_variant(-1) && C == 128 && T <= t2::TMAX && (!head || M <= MAXRT * 16)) {
        auto k2 = tail_pick_nrt(T, [](auto n) { return t2::tail2_bwd_kernel<n>; });
        EDGL_LDS_LIMIT(k2, t2::SMEM_BWD_ALL, "edgl_tail_bwd (two per CU)");
        hipLaunchKernelGGL(k2, dim3(B), dim3(t2::NTHR), t2::SMEM_BWD_ALL, st, p);
    } else {
        auto k = C == 128 ? tail_pick_nrt(T, [](auto n) { return tail_bwd_kernel<8, n>; }) : tail_pick_nrt(T, [](auto n) { return tail_bwd_kernel<4, n>; });
        const size_t smem = C == 128 ? TailGeom<8>::SMEM_BWD : TailGeom<4>::SMEM_BWD;
        EDGL_LDS_LIMIT(k, smem, "edgl_tail_bwd (one per CU)");
        hipLaunchKernelGGL(k, dim3(B), dim3(C == 128 ? 512 : 256), smem, st, p);
    }
    EDGL_LAUNCH_CHECK();
    // (dbeta | dgamma) per sample -> parameter gradients, fixed order (deferred-reduction aware)
    auto red2 = [&](float* part, float* dg, float* db) -> int {
        if (dg == db + C) return edgl_reduce_rows(part, B, 2 * C, 2L * C, db, 0, st);
        int rc = edgl_reduce_rows(part, B, C, 2L * C, db, 0, st);
        if (rc) return rc;
        return edgl_reduce_rows(part + C, B, C, 2L * C, dg, 0, st);
    };
    int rc = red2(part1, dg1, db1);
    if (rc) return rc;
    rc = red2(part2, dg2, db2);
    if (rc) return rc;
    if (head) rc = red2(part3, dg3, db3);
    return rc;
}
extern "C" int edgl_tail_bwd(const void* xin, int ld_x, const void* ao, const void* a1, const void* pre_f, const void* o,
                             const void* pre_t, const void* so, const float* st1, const float* st2, const float* st3,
                             const void* Wo, const void* Wi, const void* Wout, const void* Wt, const float* g1, const float* g2,
                             const float* g3, int B, int T, int C, float drop_rate, const uint64_t* rng_state, uint32_t sid1,
                             uint32_t sid2, int head, const void* d_rows, const int64_t* masked_pos, int M,
                             const int32_t* dy_rowmap, const void* d_y_in, void* d_pre_t, void* d_o, void* d_pre_f, void* d_ao,
                             void* d_res1, void* d_att, float* dg1, float* db1, float* dg2, float* db2, float* dg3, float* db3,
                             float* workspace, int dtype, void* stream) {
    return edgl_tail_bwd_ct(xin, ld_x, ao, a1, pre_f, o, pre_t, so, st1, st2, st3, Wo, Wi, Wout, Wt, g1, g2, g3, B, T, C, drop_rate, rng_state,
                            sid1, sid2, head, d_rows, masked_pos, M, dy_rowmap, d_y_in, d_pre_t, d_o, d_pre_f, d_ao, d_res1, d_att, dg1, db1,
                            dg2, db2, dg3, db3, workspace, 0, 0, dtype, stream);
}

extern "C" long edgl_tail_bwd_workspace(int B, int C) { return 6L * B * C; }

#ifdef EDGL_PHASE_TIMING
extern "C" int edgl_debug_phase_cycles_tail_bwd(unsigned long long* out16, int reset) { return tail_phase_cycles(out16, reset); }
#endif
