// Fused per-sample block tail (EasyDGL.py:110-139): the reference's LayerNorm normalises jointly over (T, C) PER SAMPLE
// (Base.py:12-67), so one workgroup that owns a sample can run
//     ao = att.Wo + bo ; a1 = LN1(drop(ao) + x_in) ; f = gelu(a1.Wi + bi) ; o = f.Wout + bout ; y = LN2(drop(o) + a1)
//     [head]  so = gelu(y.Wt + bt) ; rows = LN3(so)[masked positions]
// with the [T, C] activations held in LDS between the steps (T = 101, C = 128: 28 KB per tensor) and the weights streamed
// from L2 as MFMA operands: no HBM round trip between the four dense layers and three LayerNorms — each intermediate is
// written once (the backward needs it) and never read back by this kernel.  The unfused path is seven launches.
//   MFMA orientation: D[n][row] = sum_k W^T[n][k] X[row][k]; a wave owns one 16-wide tile of output channels for ALL rows
//   (A operand = 16 rows of the packed W^T, read from global/L2; B operand = activation rows from LDS), so a lane ends up
//   with 4 consecutive channels of one row: bias, dropout, residual, GELU and the LayerNorm moments all run on registers;
//   results go to the next LDS buffer and leave for HBM as whole 256-byte rows.
// Arithmetic is that of the unfused kernels step for step (GEMM outputs rounded to the activation dtype before the
// LayerNorm reads them, two-pass moments, the same dropout element indices), so both paths produce the same tensors.
// bf16, C in {64, 128}, T <= 112.
// This unit: the forward in both forms (one and two workgroups per CU), the weight pack and the A/B switch; the backward is
// k_tail_bwd.hip, what they share tail_common.h and tail2_common.h.
#include "tail2_common.h"

namespace {

// f32 image stg [112][LDF] of dense outputs (bias not yet added; `bias` = the C biases of these columns) -> with pre = . + bias:
// dact = gelu'(pre) (bf16, global) and act = gelu(pre) (bf16, global + LDS image act_s).  A thread keeps its 8 columns
// over all its rows.
template <int CT>
__device__ __forceinline__ void gelu_pass(const float* stg, const float* bias, bf16* dact_g, bf16* act_g, long ldg, bf16* act_s, int T) {
    using G = TailGeom<CT>;
    static_assert(G::NTHR % G::CV == 0, "a thread's column group must not change from row to row");
    const int cv = threadIdx.x % G::CV;
    const float4 b0 = *reinterpret_cast<const float4*>(bias + cv * 8), b1 = *reinterpret_cast<const float4*>(bias + cv * 8 + 4);   // (LDS)
#pragma unroll 1
    for (int row = threadIdx.x / G::CV; row < MAXRT * 16; row += G::NTHR / G::CV) {
        const float4 x0 = *reinterpret_cast<const float4*>(stg + row * G::LDF + cv * 8);
        const float4 x1 = *reinterpret_cast<const float4*>(stg + row * G::LDF + cv * 8 + 4);
        const float x[8] = {x0.x + b0.x, x0.y + b0.y, x0.z + b0.z, x0.w + b0.w, x1.x + b1.x, x1.y + b1.y, x1.z + b1.z, x1.w + b1.w};
        Vec16<bf16> dact, act;
#pragma unroll
        for (int j = 0; j < 8; ++j) {    // gelu_t / dgelu_t<bf16> of edgl_common.h with the erf shared
            float e;
            const float cdf = 0.5f * (1.0f + erf_as(x[j] * 0.70710678118654752440f, e));
            act.v[j] = from_f32<bf16>(x[j] * cdf);
            dact.v[j] = from_f32<bf16>(cdf + x[j] * (0.39894228040143267794f * e));
        }
        st16<bf16>(act_s + row * G::LD + cv * 8, act);
        if (row < T) {
            st16<bf16>(dact_g + (long)row * ldg + cv * 8, dact);
            st16<bf16>(act_g + (long)row * ldg + cv * 8, act);
        }
    }
}

// Four LDS images per workgroup: A (att -> y), B (x_in -> a1 -> LN3 rows), C (f halves, so), S (staging of the tensors
// that only pass through: ao, o); A + S together hold the f32 pre-activations of a GELU pass.  Everything leaves for HBM as whole 256-byte rows (copy_out); storing
// the pass-through tensors straight from the accumulator registers (8 bytes per lane) measured slower (88 vs 83 us).
// NRT: the row-tile count as a template constant (2, 4 or 7 tiles: T <= 32, 64, 112; tiles past the sequence are padding like
// the rows past it) — every `rt < nrt` guard folds away and the accumulator tiles stay independent tuples.  With a run-time
// count (NRT = 0, not instantiated) the compiler keeps whole 28-register copies of the tile arrays alive across the guards:
// 47 / 129 spilled registers.
template <int CT, int NRT>
__global__ __launch_bounds__(64 * CT) void tail_fwd_kernel(TailP p) {
    using G = TailGeom<CT>;
    constexpr int C = G::C, LD = G::LD, NKB = C / 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* bufA = reinterpret_cast<bf16*>(smem);
    bf16* bufS = reinterpret_cast<bf16*>(smem + G::BUF);
    bf16* bufB = reinterpret_cast<bf16*>(smem + 2 * G::BUF);
    bf16* bufC = reinterpret_cast<bf16*>(smem + 3 * G::BUF);
    float* stg = reinterpret_cast<float*>(smem);             // f32 image over A + S while neither holds a tensor
    float* red = reinterpret_cast<float*>(smem + 4 * G::BUF);
    const int b = blockIdx.x, T = p.T, nrt = NRT ? NRT : (T + 15) / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g4 = (lane >> 4) * 4, l15 = lane & 15;
    const int n0 = wave * 16, nl = n0 + g4;                 // this lane's 4 output channels: nl .. nl + 3
    const long row0 = (long)b * T;
    const DropKey dk1 = make_dropkey(p.rng, p.sid1, p.rate), dk2 = make_dropkey(p.rng, p.sid2, p.rate);
    const ChanPad cpad = chan_pad<CT>(nl, p.dhp, p.dht);

    PH_DECL
    // ---- waits ------------------------------------------------------------------------------------------------------------
    // Loads and stores share ONE in-order counter (vmcnt) on this part: waiting for a load also waits for every store issued
    // before it, and behind a store loop of run-time length the compiler can only wait for "everything".  As first written —
    // parameter vectors loaded where they are used, weight fragments one product ahead — eight points of a sample waited for
    // the store batch issued just before them (copy_out / the GELU pass: 28-56 KB per workgroup, all 256 workgroups at once).
    // Now nothing is loaded in front of its use: every parameter vector is requested before the first store of the kernel,
    // and a product's weight fragments at the START of the segment (the stretch between two store batches) BEFORE the one
    // that uses them, with their wait pinned (touch_regs) to that segment's end — a whole segment after the last stores.
    // (The parameter vectors wait in LDS, not in registers: 56 of them per lane spilled the 7-tile instance.)
    // Measured: 68.5 -> 67 us.  The launch is not bound by its memory side at all — without the GELU passes' global stores
    // (49 % of the bytes written) it takes 61.5 us — but by the serial chain of a workgroup's phases: three GELU passes
    // (15 VALU + 2 transcendental instructions per element, ~35 % of a sample), six LDS-fed products (~27 %), the joint
    // moments and copies.
    float* par = red + 64;     // parameter vectors [11][C] (G::PAR_*)
    if ((int)threadIdx.x < C) {
        const int c = threadIdx.x;
        const float* bt_or = p.head ? p.bt : p.bo;   // (head parameters: valid pointers to load from when there is no head)
        const float *g3_or = p.head ? p.g3 : p.g1, *b3_or = p.head ? p.b3 : p.b1;
        const float x0 = p.bo[c], x1 = p.bout[c], x2 = p.g1[c], x3 = p.b1[c], x4 = p.g2[c], x5 = p.b2[c], x6 = g3_or[c], x7 = b3_or[c],
                    x8 = bt_or[c], x9 = p.bi[c], x10 = p.bi[C + c];
        par[G::PAR_BO * C + c] = x0; par[G::PAR_BOUT * C + c] = x1; par[G::PAR_G1 * C + c] = x2; par[G::PAR_B1 * C + c] = x3;
        par[G::PAR_G2 * C + c] = x4; par[G::PAR_B2 * C + c] = x5; par[G::PAR_G3 * C + c] = x6; par[G::PAR_B3 * C + c] = x7;
        par[G::PAR_BT * C + c] = x8; par[G::PAR_BI * C + c] = x9; par[(G::PAR_BI + 1) * C + c] = x10;
    }
    // first round of the head's row gather (M * C / 8 vectors over the workgroup; later rounds load theirs in the loop)
    int gat_t = 0; long gat_dst = -1;
    if (p.head) {
        const int v = min((int)threadIdx.x, p.M * G::CV - 1), j = v / G::CV;
        const long src = (long)b * p.M + j;
        gat_t = (int)p.mpos[src];
        gat_dst = p.hmap ? (long)p.hmap[src] : src;
    }
    WFrags<NKB> wA = load_wfrags<NKB>(p.WoT + (long)n0 * C, C, lane);      // att_out dense
    WFrags<NKB> wB = load_wfrags<NKB>(p.WiT + (long)n0 * C, C, lane);      // inner dense, first half
    WFrags<NKB> wC;
    copy_in2<CT>(bufA, p.att + row0 * C, C, bufB, p.xin + row0 * p.ld_x, p.ld_x, T);
    lds_barrier();
    PH_MARK(0);   // inputs in LDS
    float z[MAXRT][4];
    // ---- segment A: ao = att.Wo + bo ; z1 = drop(ao) + x_in (EasyDGL.py:113-115) ------------------------------------------
    {
        f32x4 acc[MAXRT];
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        tile_gemm<CT, NKB>(wA, bufA, nrt, lane, acc);
        const float4 v_bo = *reinterpret_cast<const float4*>(par + G::PAR_BO * C + nl);
        const float bv[4] = {v_bo.x, v_bo.y, v_bo.z, v_bo.w};
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt)
            if (rt < nrt) {
                const int row = rt * 16 + l15;
                float v[4], xr[4];
                ld_bf4(bufB + row * LD + nl, xr);
                float dv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) { v[r] = rbf(acc[rt][r] + bv[r]); dv[r] = v[r]; }
                drop_apply4(dk1, (uint64_t)((row0 + min(row, T - 1)) * C + nl), dv);   // one hash per four channels
#pragma unroll
                for (int r = 0; r < 4; ++r) z[rt][r] = dv[r] + xr[r];
                st_bf4(bufS + row * LD + nl, v);
            }
    }
    PH_MARK(1);   // G1 + epilogue
    lds_barrier();
    touch_regs(wB);     // every load so far has arrived: stores may start
    copy_out<CT>(p.ao + row0 * C, C, bufS, T);
    PH_MARK(2);   // barrier + copy_out(ao)
    // ---- segment B: a1 = LN1(z1) (EasyDGL.py:116) -> B, in place of the residual it consumed -------------------------------
    wA = load_wfrags<NKB>(p.WoutT + (long)n0 * 2 * C, 2 * C, lane);        // out dense, first half of its inputs (segment D)
    {
        float mean, rstd;
        joint_moments<CT>(z, nrt, T, lane, red, mean, rstd, cpad);
        if (threadIdx.x == 0) { p.st1[2 * b] = mean; p.st1[2 * b + 1] = rstd; }
        const float4 v_g = *reinterpret_cast<const float4*>(par + G::PAR_G1 * C + nl), v_b = *reinterpret_cast<const float4*>(par + G::PAR_B1 * C + nl);
        const float gv[4] = {v_g.x, v_g.y, v_g.z, v_g.w}, ev[4] = {v_b.x, v_b.y, v_b.z, v_b.w};
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt)
            if (rt < nrt) {
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = (z[rt][r] - mean) * rstd * gv[r] + ev[r];
                st_bf4(bufB + (rt * 16 + l15) * LD + nl, v);
            }
    }
    PH_MARK(3);   // LN1
    lds_barrier();
    touch_regs(wA);
    copy_out<CT>(p.a1 + row0 * C, C, bufB, T);
    PH_MARK(4);   // barrier + copy_out(a1)
    // ---- f = gelu(a1.Wi + bi) in two halves of C columns; o accumulates f.Wout half by half (EasyDGL.py:120-125) ----------
    f32x4 acc3[MAXRT];
    // segment C: first half of the inner dense
    wC = load_wfrags<NKB>(p.WiT + (long)(C + n0) * C, C, lane);            // inner dense, second half (segment D)
    {
        f32x4 acc[MAXRT];
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        tile_gemm<CT, NKB>(wB, bufB, nrt, lane, acc);
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt)   // all 7 tiles, unconditionally (tiles >= nrt hold zeros)
            *reinterpret_cast<float4*>(stg + (rt * 16 + l15) * G::LDF + nl) = make_float4(acc[rt][0], acc[rt][1], acc[rt][2], acc[rt][3]);
    }
    lds_barrier();
    touch_regs(wC);
    gelu_pass<CT>(stg, par + G::PAR_BI * C, p.pre_f + row0 * 2 * C, p.f + row0 * 2 * C, 2 * C, bufC, T);
    PH_MARK(5);   // G2 half + GELU
    lds_barrier();
    // segment D: first half of the out dense, second half of the inner dense
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt) acc3[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
    tile_gemm<CT, NKB>(wA, bufC, nrt, lane, acc3);
    wA = load_wfrags<NKB>(p.WoutT + (long)n0 * 2 * C + C, 2 * C, lane);    // out dense, second half of its inputs (segment E; a third live set spills)
    EDGL_PIN();
    PH_MARK(6);   // G3 half
    {
        f32x4 acc[MAXRT];
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        tile_gemm<CT, NKB>(wC, bufB, nrt, lane, acc);
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt)
            *reinterpret_cast<float4*>(stg + (rt * 16 + l15) * G::LDF + nl) = make_float4(acc[rt][0], acc[rt][1], acc[rt][2], acc[rt][3]);
    }
    lds_barrier();   // (every wave is also past its reads of the first half's f image)
    touch_regs(wA);
    gelu_pass<CT>(stg, par + (G::PAR_BI + 1) * C, p.pre_f + row0 * 2 * C + C, p.f + row0 * 2 * C + C, 2 * C, bufC, T);
    PH_MARK(5);
    lds_barrier();
    // segment E: second half of the out dense
    wB = load_wfrags<NKB>(p.WtT + (long)n0 * C, C, lane);                  // head transform (fetched even without a head: cheap)
    tile_gemm<CT, NKB>(wA, bufC, nrt, lane, acc3);
    PH_MARK(6);
    // ---- o = . + bout ; z2 = drop(o) + a1 ; y = LN2(z2) (EasyDGL.py:126-128) -> A ---------------------------------------------
    {
        const float4 v_bout = *reinterpret_cast<const float4*>(par + G::PAR_BOUT * C + nl);
        const float bv[4] = {v_bout.x, v_bout.y, v_bout.z, v_bout.w};
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt)
            if (rt < nrt) {
                const int row = rt * 16 + l15;
                float v[4], xr[4];
                ld_bf4(bufB + row * LD + nl, xr);
                float dv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) { v[r] = rbf(acc3[rt][r] + bv[r]); dv[r] = v[r]; }
                drop_apply4(dk2, (uint64_t)((row0 + min(row, T - 1)) * C + nl), dv);   // one hash per four channels
#pragma unroll
                for (int r = 0; r < 4; ++r) z[rt][r] = dv[r] + xr[r];
                st_bf4(bufS + row * LD + nl, v);
            }
    }
    lds_barrier();
    touch_regs(wB);
    copy_out<CT>(p.o + row0 * C, C, bufS, T);
    {
        float mean, rstd;
        joint_moments<CT>(z, nrt, T, lane, red, mean, rstd, cpad);
        if (threadIdx.x == 0) { p.st2[2 * b] = mean; p.st2[2 * b + 1] = rstd; }
        const float4 v_g = *reinterpret_cast<const float4*>(par + G::PAR_G2 * C + nl), v_b = *reinterpret_cast<const float4*>(par + G::PAR_B2 * C + nl);
        const float gv[4] = {v_g.x, v_g.y, v_g.z, v_g.w}, ev[4] = {v_b.x, v_b.y, v_b.z, v_b.w};
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt)
            if (rt < nrt) {
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = (z[rt][r] - mean) * rstd * gv[r] + ev[r];
                st_bf4(bufA + (rt * 16 + l15) * LD + nl, v);
            }
    }
    lds_barrier();
    copy_out<CT>(p.y + row0 * C, C, bufA, T);
    PH_MARK(7);   // o, LN2, y
#ifdef EDGL_PHASE_TIMING
    PH_FLUSH(0); ph_acc[0] = 0; ph_t0 = __builtin_readcyclecounter();
#endif
    if (!p.head) return;
    // ---- head: so = gelu(y.Wt + bt) ; rows = LN3(so)[masked positions] (EasyDGL.py:136-146) --------------------------------
    {
        f32x4 acc[MAXRT];
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        tile_gemm<CT, NKB>(wB, bufA, nrt, lane, acc);
        lds_barrier();   // y (buffer A) is overwritten by the f32 image
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt)
            *reinterpret_cast<float4*>(stg + (rt * 16 + l15) * G::LDF + nl) = make_float4(acc[rt][0], acc[rt][1], acc[rt][2], acc[rt][3]);
    }
    lds_barrier();
    gelu_pass<CT>(stg, par + G::PAR_BT * C, p.pre_t + row0 * C, p.so + row0 * C, C, bufC, T);
    lds_barrier();
#pragma unroll
    for (int rt = 0; rt < MAXRT; ++rt) ld_bf4(bufC + (rt * 16 + l15) * LD + nl, z[rt]);   // so, rounded through the activation dtype
    {
        float mean, rstd;
        joint_moments<CT>(z, nrt, T, lane, red, mean, rstd, cpad);
        if (threadIdx.x == 0) { p.st3[2 * b] = mean; p.st3[2 * b + 1] = rstd; }
        const float4 v_g = *reinterpret_cast<const float4*>(par + G::PAR_G3 * C + nl), v_b = *reinterpret_cast<const float4*>(par + G::PAR_B3 * C + nl);
        const float gv[4] = {v_g.x, v_g.y, v_g.z, v_g.w}, ev[4] = {v_b.x, v_b.y, v_b.z, v_b.w};
#pragma unroll
        for (int rt = 0; rt < MAXRT; ++rt)
            if (rt < nrt) {
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = (z[rt][r] - mean) * rstd * gv[r] + ev[r];
                st_bf4(bufB + (rt * 16 + l15) * LD + nl, v);
            }
    }
    lds_barrier();
    // batch_gather of the masked positions (EasyDGL.py:142-143); dst: row compaction of the scoring (edgl_compact_scan's `inv`)
    if ((int)threadIdx.x < p.M * G::CV && gat_dst >= 0)
        *reinterpret_cast<uint4*>(p.hrows + gat_dst * C + (threadIdx.x % G::CV) * 8) =
            *reinterpret_cast<const uint4*>(bufB + gat_t * LD + (threadIdx.x % G::CV) * 8);
    for (int v = threadIdx.x + G::NTHR; v < p.M * G::CV; v += G::NTHR) {
        const int j = v / G::CV, cv = v % G::CV;
        const long src = (long)b * p.M + j;
        const int t = (int)p.mpos[src];
        const long dst = p.hmap ? (long)p.hmap[src] : src;
        if (dst >= 0) *reinterpret_cast<uint4*>(p.hrows + dst * C + cv * 8) = *reinterpret_cast<const uint4*>(bufB + t * LD + cv * 8);
    }
#ifdef EDGL_PHASE_TIMING
    PH_MARK(0);   // head (slot 8)
    if ((threadIdx.x & 63) == 0) atomicAdd(&g_phase_cycles[8], ph_acc[0]);
#endif
}

// ---- forward on half a CU (the form: tail2_common.h) --------------------------------------------------------------------------------
namespace t2 {
// accumulators (bias not yet added) -> f32 staging image, rows < T only (the image is exactly two bf16 images long)
template <int NRT>
__device__ __forceinline__ void stage_acc(char* stg, const f32x4 (&acc)[MAXRT], const Lane& L, int T) {
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
        if (rt * 16 + L.l15 < T)
            *reinterpret_cast<float4*>(stg + L.squad + rt * 8192) = make_float4(acc[rt][0], acc[rt][1], acc[rt][2], acc[rt][3]);
}
// GELU pass over the staging image: a thread owns 8 columns (cv) of rows rsub + 32 k.  dact = gelu'(pre) and act = gelu(pre) go to
// global memory at once; act also into image `act_img` — behind a barrier when that image is part of the staging area (SYNC).
template <bool SYNC>
__device__ __forceinline__ void gelu_pass(const char* stg, const float* bias_g, bf16* dact_g, bf16* act_g, int ldg, char* act_img, int T) {
    const int tid = fresh_tid(), cv = tid & 15, rsub = tid >> 4;
    const float4 b0 = *reinterpret_cast<const float4*>(bias_g + cv * 8), b1 = *reinterpret_cast<const float4*>(bias_g + cv * 8 + 4);
    const int s0 = rsub * 512 + (((2 * cv) ^ (rsub & 15)) << 4);          // (r & 15 == rsub & 15 for r = rsub + 32 k)
    uint4 keep0 = make_uint4(0, 0, 0, 0), keep1 = keep0, keep2 = keep0, keep3 = keep0;
    // a ROLLED loop: unrolled, the scheduler interleaves the 32 erf chains of a thread (~80 registers; see gelu_pass above)
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const int r = rsub + 32 * k;
        if (r < T) {
            const float4 x0 = *reinterpret_cast<const float4*>(stg + s0 + k * 16384), x1 = *reinterpret_cast<const float4*>(stg + ((s0 + k * 16384) ^ 16));
            const float x[8] = {x0.x + b0.x, x0.y + b0.y, x0.z + b0.z, x0.w + b0.w, x1.x + b1.x, x1.y + b1.y, x1.z + b1.z, x1.w + b1.w};
            Vec16<bf16> dact, act;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float e;
                const float cdf = 0.5f * (1.0f + erf_as(x[j] * 0.70710678118654752440f, e));
                act.v[j] = from_f32<bf16>(x[j] * cdf);
                dact.v[j] = from_f32<bf16>(cdf + x[j] * (0.39894228040143267794f * e));
                // two erf chains in flight, not eight: at four waves per SIMD the other waves hide a chain's latency, and the
                // registers of six more chains are what this kernel does not have
                if (j & 1) __builtin_amdgcn_sched_barrier(0);
            }
            const uint32_t go = (uint32_t)((r * ldg + cv * 8) * 2);      // uniform base + 32-bit lane offset
            *reinterpret_cast<uint4*>(reinterpret_cast<char*>(dact_g) + go) = *reinterpret_cast<const uint4*>(&dact);
            *reinterpret_cast<uint4*>(reinterpret_cast<char*>(act_g) + go) = *reinterpret_cast<const uint4*>(&act);
            const uint4 a = *reinterpret_cast<const uint4*>(&act);
            if (!SYNC) *reinterpret_cast<uint4*>(act_img + vec_off(r, cv)) = a;
            else if (k == 0) keep0 = a;
            else if (k == 1) keep1 = a;
            else if (k == 2) keep2 = a;
            else keep3 = a;
        }
    }
    if (SYNC) {
        lds_barrier();                      // everybody's staging reads are done: the image may overwrite the staging area
        if (rsub < T) *reinterpret_cast<uint4*>(act_img + vec_off(rsub, cv)) = keep0;
        if (rsub + 32 < T) *reinterpret_cast<uint4*>(act_img + vec_off(rsub + 32, cv)) = keep1;
        if (rsub + 64 < T) *reinterpret_cast<uint4*>(act_img + vec_off(rsub + 64, cv)) = keep2;
        if (rsub + 96 < T) *reinterpret_cast<uint4*>(act_img + vec_off(rsub + 96, cv)) = keep3;
    }
}

// "No load behind a store": loads and stores share ONE in-order counter (vmcnt) on this part, so waiting for a load also waits for every
// store issued before it — behind a copy_out or a GELU pass that is a full HBM write acknowledge (2-3 us with 512 workgroups storing
// at once), and a sample has ten such batches.  Hence: the three parameter vectors used before the first store batches go to
// registers in the prologue, the others wait in the LDS table, and a product's weight fragments are requested BEFORE the store
// batch in front of it and their wait pinned (touch_regs) in front of that batch's first store — except the out-dense fragments of
// the second hidden half (one load behind the GELU pass's stores per sample).  The same holds for a SPILLED register: its reload
// from scratch is a load.  The kernel must stay free of scratch (tests/test_tail2_resources.py): every store batch rebuilds its
// offsets, and the lane's operand offsets are rebuilt behind it, so that none of them lives across the kernel.
template <int NRT>
__global__ __launch_bounds__(NTHR, 4) void tail2_fwd_kernel(TailP p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const P = smem; char* const Q = smem + IMG; char* const R = smem + 2 * IMG;
    float* red = reinterpret_cast<float*>(smem + OFF_RED);
    float* par = reinterpret_cast<float*>(smem + OFF_PAR);
    const int b = blockIdx.x, T = p.T;
    // rebuilt (fresh) behind every store batch, as in the backward: held across the kernel they went to scratch
    Lane L = make_lane();
    int n0 = L.wave * 16, nl = L.nl, l15 = L.l15;
    auto fresh = [&]() { L = fresh_lane(); n0 = L.wave * 16; nl = L.nl; l15 = L.l15; };
    const long row0 = (long)b * T;
    const ChanPad cpad = chan_pad<8>(nl, p.dhp, p.dht);
    if ((int)threadIdx.x < C) {
        const int c = threadIdx.x;
        const float *g3_or = p.head ? p.g3 : p.g1, *b3_or = p.head ? p.b3 : p.b1, *bt_or = p.head ? p.bt : p.bo;
        const float x0 = p.bout[c], x1 = p.g2[c], x2 = p.b2[c], x3 = g3_or[c], x4 = b3_or[c], x5 = p.bi[c], x6 = p.bi[C + c], x7 = bt_or[c];
        par[PAR_BOUT * C + c] = x0; par[PAR_G2 * C + c] = x1; par[PAR_B2 * C + c] = x2; par[PAR_G3 * C + c] = x3;
        par[PAR_B3 * C + c] = x4; par[PAR_BI * C + c] = x5; par[(PAR_BI + 1) * C + c] = x6; par[PAR_BT * C + c] = x7;
    }
    const float4 v_bo = *reinterpret_cast<const float4*>(p.bo + nl);
    const float4 v_g1 = *reinterpret_cast<const float4*>(p.g1 + nl), v_b1 = *reinterpret_cast<const float4*>(p.b1 + nl);
    WFrags<NKB> wf = load_wfrags<NKB>(p.WoT + (long)n0 * C, C, L.lane);      // att_out dense
    copy_in2(P, p.att + row0 * C, C, Q, p.xin + row0 * p.ld_x, p.ld_x, T);
    const DropKey dk1 = make_dropkey(p.rng, p.sid1, p.rate), dk2 = make_dropkey(p.rng, p.sid2, p.rate);     // (wave-uniform: scalar registers)
    // first round of the head's row gather: position and destination row of this thread's vector (later rounds load theirs in the loop)
    int gat_t = 0; long gat_dst = -1;
    if (p.head) {
        const int j = min((int)threadIdx.x, p.M * 16 - 1) >> 4;
        const long src = (long)b * p.M + j;
        gat_t = (int)p.mpos[src];
        gat_dst = p.hmap ? (long)p.hmap[src] : src;
    }
    const uint64_t idx0 = (uint64_t)((row0 + l15) * C + nl);       // dropout element index of this lane's quad in row tile 0 (+ rt * 16 * C)
    lds_barrier();
    float z[MAXRT][4];
    f32x4 acc[MAXRT];
    // ---- ao = att.Wo + bo ; z1 = drop(ao) + x_in (EasyDGL.py:113-115): att in P, x_in in Q, ao -> R ---------------------------------
    zero_acc<NRT>(acc);
    gemm<NRT>(wf, P, L, acc);
    wf = load_wfrags<NKB>(p.WiT + (long)n0 * C, C, L.lane);                   // inner dense, first half (used behind two store batches)
    {
        const float bv[4] = {v_bo.x, v_bo.y, v_bo.z, v_bo.w};
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) {
            const int row = rt * 16 + l15;
            float v[4], xr[4], dv[4];
            ld_bf4(reinterpret_cast<const bf16*>(Q + L.quad + rt * 4096), xr);
#pragma unroll
            for (int r = 0; r < 4; ++r) { v[r] = rbf(acc[rt][r] + bv[r]); dv[r] = v[r]; }
            drop_apply4(dk1, idx0 + (uint64_t)(rt * 16 * C), dv);
#pragma unroll
            for (int r = 0; r < 4; ++r) z[rt][r] = dv[r] + xr[r];
            if (row < T) st_bf4(reinterpret_cast<bf16*>(R + L.quad + rt * 4096), v);
        }
    }
    lds_barrier();
    touch_regs(wf);                  // every load so far has arrived: stores may start
    copy_out(p.ao + row0 * C, C, R, T);
    fresh();
    // ---- a1 = LN1(z1) (EasyDGL.py:116) -> P (att is consumed) ---------------------------------------------------------------------------
    {
        float mean, rstd;
        joint_moments<8>(z, NRT, T, L.lane, red, mean, rstd, cpad);
        if (threadIdx.x == 0) { p.st1[2 * b] = mean; p.st1[2 * b + 1] = rstd; }
        const float gv[4] = {v_g1.x, v_g1.y, v_g1.z, v_g1.w}, ev[4] = {v_b1.x, v_b1.y, v_b1.z, v_b1.w};
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (z[rt][r] - mean) * rstd * gv[r] + ev[r];
            if (rt * 16 + l15 < T) st_bf4(reinterpret_cast<bf16*>(P + L.quad + rt * 4096), v);
        }
    }
    lds_barrier();
    copy_out(p.a1 + row0 * C, C, P, T);
    fresh();
    // ---- f = gelu(a1.Wi + bi), two halves of C hidden channels; o accumulates f.Wout half by half (EasyDGL.py:120-125) ----------------
    f32x4 acc3[MAXRT];
    zero_acc<NRT>(acc3);
    {   // first half: a1 . Wi[:, :C] -> staging Q + R (x_in / ao: consumed) -> f half in R -> acc3 = f . Wout[:C, :]
        zero_acc<NRT>(acc);
        gemm<NRT>(wf, P, L, acc);
        stage_acc<NRT>(Q, acc, L, T);
        WFrags<NKB> wo = load_wfrags<NKB>(p.WoutT + (long)n0 * 2 * C, 2 * C, L.lane);     // out dense, inputs of the first half
        wf = load_wfrags<NKB>(p.WiT + (long)(C + n0) * C, C, L.lane);                     // inner dense, second half
        lds_barrier();
        touch_regs(wo); touch_regs(wf);          // (acc3 is not live yet: both sets fit across the pass)
        gelu_pass<true>(Q, par + PAR_BI * C, p.pre_f + row0 * 2 * C, p.f + row0 * 2 * C, 2 * C, R, T);
        fresh();
        lds_barrier();
        gemm<NRT>(wo, R, L, acc3);
    }
    {   // second half
        zero_acc<NRT>(acc);
        gemm<NRT>(wf, P, L, acc);
        lds_barrier();                               // the first half's f image (R) is still the operand of somebody's product
        stage_acc<NRT>(Q, acc, L, T);
        lds_barrier();
        gelu_pass<true>(Q, par + (PAR_BI + 1) * C, p.pre_f + row0 * 2 * C + C, p.f + row0 * 2 * C + C, 2 * C, R, T);
        fresh();
        wf = load_wfrags<NKB>(p.WoutT + (long)n0 * 2 * C + C, 2 * C, L.lane);       // out dense, second half (behind the pass's stores; requested ahead of them it measured nothing: DESIGN rule 80)
        lds_barrier();
        gemm<NRT>(wf, R, L, acc3);
    }
    if (p.head) wf = load_wfrags<NKB>(p.WtT + (long)n0 * C, C, L.lane);       // head transform
    // ---- o = . + bout ; z2 = drop(o) + a1 ; y = LN2(z2) (EasyDGL.py:126-128): o -> Q, y -> R ------------------------------------------------
    {
        const float4 v_bout = *reinterpret_cast<const float4*>(par + PAR_BOUT * C + nl);
        const float bv[4] = {v_bout.x, v_bout.y, v_bout.z, v_bout.w};
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) {
            const int row = rt * 16 + l15;
            float v[4], xr[4], dv[4];
            ld_bf4(reinterpret_cast<const bf16*>(P + L.quad + rt * 4096), xr);
#pragma unroll
            for (int r = 0; r < 4; ++r) { v[r] = rbf(acc3[rt][r] + bv[r]); dv[r] = v[r]; }
            drop_apply4(dk2, idx0 + (uint64_t)(rt * 16 * C), dv);
#pragma unroll
            for (int r = 0; r < 4; ++r) z[rt][r] = dv[r] + xr[r];
            if (row < T) st_bf4(reinterpret_cast<bf16*>(Q + L.quad + rt * 4096), v);
        }
    }
    lds_barrier();
    if (p.head) touch_regs(wf);
    copy_out(p.o + row0 * C, C, Q, T);
    fresh();
    {
        float mean, rstd;
        joint_moments<8>(z, NRT, T, L.lane, red, mean, rstd, cpad);
        if (threadIdx.x == 0) { p.st2[2 * b] = mean; p.st2[2 * b + 1] = rstd; }
        const float4 v_g = *reinterpret_cast<const float4*>(par + PAR_G2 * C + nl), v_b = *reinterpret_cast<const float4*>(par + PAR_B2 * C + nl);
        const float gv[4] = {v_g.x, v_g.y, v_g.z, v_g.w}, ev[4] = {v_b.x, v_b.y, v_b.z, v_b.w};
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (z[rt][r] - mean) * rstd * gv[r] + ev[r];
            if (rt * 16 + l15 < T) st_bf4(reinterpret_cast<bf16*>(R + L.quad + rt * 4096), v);
        }
    }
    lds_barrier();
    copy_out(p.y + row0 * C, C, R, T);
    if (!p.head) return;
    fresh();
    // ---- head: so = gelu(y.Wt + bt) ; rows = LN3(so)[masked positions] (EasyDGL.py:136-146): staging = P + Q, so -> R, rows -> Q ----------
    zero_acc<NRT>(acc);
    gemm<NRT>(wf, R, L, acc);
    stage_acc<NRT>(P, acc, L, T);                    // (a1 and o are consumed: every wave is past the barrier behind LN2)
    lds_barrier();                                   // ... which also says that nobody reads y (R) any more
    gelu_pass<false>(P, par + PAR_BT * C, p.pre_t + row0 * C, p.so + row0 * C, C, R, T);
    fresh();
    lds_barrier();
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) ld_bf4(reinterpret_cast<const bf16*>(R + L.quad + rt * 4096), z[rt]);   // so, rounded through the activation dtype
    {
        float mean, rstd;
        joint_moments<8>(z, NRT, T, L.lane, red, mean, rstd, cpad);
        if (threadIdx.x == 0) { p.st3[2 * b] = mean; p.st3[2 * b + 1] = rstd; }
        const float4 v_g = *reinterpret_cast<const float4*>(par + PAR_G3 * C + nl), v_b = *reinterpret_cast<const float4*>(par + PAR_B3 * C + nl);
        const float gv[4] = {v_g.x, v_g.y, v_g.z, v_g.w}, ev[4] = {v_b.x, v_b.y, v_b.z, v_b.w};
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (z[rt][r] - mean) * rstd * gv[r] + ev[r];
            if (rt * 16 + l15 < T) st_bf4(reinterpret_cast<bf16*>(Q + L.quad + rt * 4096), v);
        }
    }
    lds_barrier();
    // batch_gather of the masked positions (EasyDGL.py:142-143); dst: row compaction of the scoring (edgl_compact_scan's `inv`)
    if ((int)threadIdx.x < p.M * 16 && gat_dst >= 0)
        *reinterpret_cast<uint4*>(p.hrows + gat_dst * C + (threadIdx.x & 15) * 8) = *reinterpret_cast<const uint4*>(Q + vec_off(gat_t, threadIdx.x & 15));
    for (int v = threadIdx.x + NTHR; v < p.M * 16; v += NTHR) {
        const int j = v >> 4, cv = v & 15;
        const long src = (long)b * p.M + j;
        const int t = (int)p.mpos[src];
        const long dst = p.hmap ? (long)p.hmap[src] : src;
        if (dst >= 0) *reinterpret_cast<uint4*>(p.hrows + dst * C + cv * 8) = *reinterpret_cast<const uint4*>(Q + vec_off(t, cv));
    }
}

}  // namespace t2

// dst[n][k] = src[k][n]  (tf.layers.dense kernels are [in, out]; the MFMA A operand wants k contiguous)
__global__ void tail_pack_kernel(const bf16* Wo, const bf16* Wi, const bf16* Wout, const bf16* Wt, int C, bf16* pack) {
    const long cc = (long)C * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < 6 * cc; i += (long)gridDim.x * blockDim.x) {
        const bf16* src; long off; int K, N;
        if (i < cc) { src = Wo; off = 0; K = C; N = C; }
        else if (i < 3 * cc) { src = Wi; off = cc; K = C; N = 2 * C; }
        else if (i < 5 * cc) { src = Wout; off = 3 * cc; K = 2 * C; N = C; }
        else { src = Wt; off = 5 * cc; K = C; N = C; }
        const long j = i - off;
        const int n = (int)(j / K), k = (int)(j % K);
        pack[i] = src[(long)k * N + n];
    }
}

}  // namespace

// EDGL_TAIL2=0 / edgl_tail_variant(0): the one-workgroup-per-CU kernels for every shape (A/B switch)
static int g_tail2 = -1;
static bool tail2_enabled() {
    if (g_tail2 < 0) g_tail2 = edgl_env_on("EDGL_TAIL2") ? 1 : 0;
    return g_tail2 != 0;
}
extern "C" int edgl_tail_variant(int variant) {
    const int prev = tail2_enabled() ? 1 : 0;
    if (variant >= 0) g_tail2 = variant ? 1 : 0;
    return prev;
}

extern "C" long edgl_tail_pack_elems(int C) { return 6L * C * C; }

extern "C" int edgl_tail_supported(int T, int C, int dtype) { return dtype == EDGL_BF16 && (C == 64 || C == 128) && T >= 1 && T <= 16 * MAXRT; }

extern "C" int edgl_tail_pack(const void* Wo, const void* Wi, const void* Wout, const void* Wt, int C, void* pack, void* stream) {
    EDGL_REQUIRE(Wo && Wi && Wout && Wt && pack, EDGL_ERR_NULL, "edgl_tail_pack: null pointer");
    EDGL_REQUIRE(C == 64 || C == 128, EDGL_ERR_SHAPE, "edgl_tail_pack: C=%d unsupported (64 or 128)", C);
    hipLaunchKernelGGL(tail_pack_kernel, dim3(96), dim3(256), 0, (hipStream_t)stream, (const bf16*)Wo, (const bf16*)Wi,
                       (const bf16*)Wout, (const bf16*)Wt, C, (bf16*)pack);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_tail_fwd_ct(const void* att, const void* xin, int ld_x, const void* pack, const float* bo, const float* bi,
                             const float* bout, const float* bt, const float* g1, const float* b1, const float* g2,
                             const float* b2, const float* g3, const float* b3, int B, int T, int C, float drop_rate,
                             const uint64_t* rng_state, uint32_t sid1, uint32_t sid2, const int64_t* masked_pos, int M, int head,
                             void* ao, void* a1, float* st1, void* pre_f, void* f, void* o, void* y, float* st2, void* pre_t,
                             void* so, float* st3, void* hrows, const int32_t* hrow_map, int dh_pad, int dh_true, int dtype,
                                void* stream) {
    EDGL_REQUIRE(att && xin && pack && bo && bi && bout && g1 && b1 && g2 && b2 && ao && a1 && st1 && pre_f && f && o && y && st2,
                 EDGL_ERR_NULL, "edgl_tail_fwd: null pointer");
    EDGL_REQUIRE(!head || (bt && g3 && b3 && masked_pos && pre_t && so && st3 && hrows && M >= 1), EDGL_ERR_NULL,
                 "edgl_tail_fwd: the head needs its weights, positions and outputs");
    if (const int rc = tail_check("edgl_tail_fwd", " (bf16, C in {64,128}, T <= 112)", B, T, C, ld_x, dtype, drop_rate, rng_state, dh_pad, dh_true)) return rc;
    const bf16* pk = (const bf16*)pack;
    const long cc = (long)C * C;
    TailP p{(const bf16*)att, (const bf16*)xin, ld_x, pk, pk + cc, pk + 3 * cc, pk + 5 * cc, bo, bi, bout, bt, g1, b1, g2, b2, g3, b3,
            B, T, C, drop_rate, rng_state, sid1, sid2, masked_pos, M, head, hrow_map, (bf16*)ao, (bf16*)a1, (bf16*)pre_f, (bf16*)f, (bf16*)o,
            (bf16*)y, (bf16*)pre_t, (bf16*)so, (bf16*)hrows, st1, st2, st3, dh_pad, dh_true};
    hipStream_t st = (hipStream_t)stream;
    if (tail2_enabled() && C == 128 && T <= t2::TMAX) {      // two workgroups per CU (see namespace t2)
        auto k2 = tail_pick_nrt(T, [](auto n) { return t2::tail2_fwd_kernel<n>; });
        EDGL_LDS_LIMIT(k2, t2::SMEM_FWD, "edgl_tail_fwd (two per CU)");
        hipLaunchKernelGGL(k2, dim3(B), dim3(t2::NTHR), t2::SMEM_FWD, st, p);
        EDGL_LAUNCH_CHECK();
        return EDGL_OK;
    }
    auto k = C == 128 ? tail_pick_nrt(T, [](auto n) { return tail_fwd_kernel<8, n>; }) : tail_pick_nrt(T, [](auto n) { return tail_fwd_kernel<4, n>; });
    const size_t smem = C == 128 ? TailGeom<8>::SMEM_FWD : TailGeom<4>::SMEM_FWD;
    EDGL_LDS_LIMIT(k, smem, "edgl_tail_fwd (one per CU)");
    hipLaunchKernelGGL(k, dim3(B), dim3(C == 128 ? 512 : 256), smem, st, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_tail_fwd(const void* att, const void* xin, int ld_x, const void* pack, const float* bo, const float* bi,
                             const float* bout, const float* bt, const float* g1, const float* b1, const float* g2,
                             const float* b2, const float* g3, const float* b3, int B, int T, int C, float drop_rate,
                             const uint64_t* rng_state, uint32_t sid1, uint32_t sid2, const int64_t* masked_pos, int M, int head,
                             void* ao, void* a1, float* st1, void* pre_f, void* f, void* o, void* y, float* st2, void* pre_t,
                             void* so, float* st3, void* hrows, const int32_t* hrow_map, int dtype, void* stream) {
    return edgl_tail_fwd_ct(att, xin, ld_x, pack, bo, bi, bout, bt, g1, b1, g2, b2, g3, b3, B, T, C, drop_rate, rng_state, sid1, sid2,
                            masked_pos, M, head, ao, a1, st1, pre_f, f, o, y, st2, pre_t, so, st3, hrows, hrow_map, 0, 0, dtype, stream);
}

#ifdef EDGL_PHASE_TIMING
extern "C" int edgl_debug_phase_cycles_tail(unsigned long long* out16, int reset) { return tail_phase_cycles(out16, reset); }
#endif
