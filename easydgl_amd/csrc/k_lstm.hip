// LSTM sequence recurrence in cuDNN's form: gate order i | f | g | o as column blocks, linear input, zero initial h and
// c, every position a step.  The family rules of k_gru_wide.hip hold — one workgroup of 8 waves owns 16 samples for ALL T steps, a
// wave takes channel tiles ct = wave, wave + 8, ..., no atomics, no workgroup ever waits for another one, and R reaches the matrix
// pipe as a fragment-major pack read as one cyclic stream per wave through a ring of registers that is never drained (unrolled by
// the ring depth, refilled unconditionally, waits counted at compile time: the notes at the head of k_gru_wide.hip apply, MODE
// and FULL included).  What is the LSTM's own:
//   * a tile's k-blocks are padded to whole chunks in the OPERAND tile too: its columns past the true K are zero, so an idle ring
//     entry (a re-read of the tile's last k-block) is multiplied like any other and adds nothing.  The chunk body is then free
//     of branches, the only form the compiler refills in place;
//   * the forward ring entry is the gate QUAD (i, f, g, o) of one k-block, 4 KiB that the pack keeps contiguous: one A fragment
//     from LDS meets four B fragments, so a tile runs four independent accumulator chains;
//   * everything that is element-wise in (sample, channel) stays in the registers of the lane that owns the element, across
//     steps: c_t in the forward, the carried dc AND the carried dh in the backward.  The accumulator layout of the MFMA (row =
//     (lane >> 4) * 4 + r, column = lane & 15) is the layout of the element-wise phase, so dh_carry = dG R^T is produced by the
//     lane that consumes it one step later and never goes to LDS.  A wave has at most 4 tiles, so each of these is 4 slots of 4
//     values; the tile loop stays rolled (unrolled over the tiles, every instantiation spilled), works on slot 0 and rotates the
//     slots by one per tile, LS_MAXT rotations per step in all (rot4), so no register is ever indexed by a run-time value;
//   * h is needed only as the next step's A operand (h = o tanh(c) has no carried f32 term), so the forward's LDS is the double-
//     buffered operand tile alone; the backward's LDS is the dG operand tile [16][4C] alone — 131 328 B in f32 at C = 512, which
//     fits the CU in one piece because the 32 KB f32 dh carry is not there;
//   * the backward contracts over K = 4C, which is a whole number of k-blocks at every legal C (no K padding); its ring holds
//     single fragments, a chunk of LSTM_BWD_DEPTH consecutive k-blocks.
// Each accumulator takes its k-blocks in ascending order.  A wave that owns no tile (C / 16 < 8) issues nothing.
#include "edgl_common.h"
#include "gru_common.h"      // gru_check: the shape rules and messages of the recurrence family

#ifndef LSTM_FWD_DEPTH
#define LSTM_FWD_DEPTH 4      // gate quads in flight per wave: 16 KiB, 64 VGPRs
#endif
#ifndef LSTM_BWD_DEPTH
#define LSTM_BWD_DEPTH 16     // fragments in flight per wave in the backward's dG R^T phase: 16 KiB, 64 VGPRs
#endif

namespace {

constexpr int LS_TB = 16;                     // samples per workgroup
constexpr int LS_NW = 8;                      // waves per workgroup
constexpr int LS_THREADS = LS_NW * 64;
constexpr int LS_MAXT = 4;                    // channel tiles per wave at C = 512

// KBN / KBN2: the k-blocks of the contraction; KBNc / KBN2c: rounded up to whole chunks of the ring.  The operand tiles in LDS have
// KBNc / KBN2c k-blocks of columns, zero past the true K, so an idle ring entry contributes 0 (ldo / ldo2: their row pitch).
struct LstmDims { int KBN, Kp, KBNc, ldo, KBN2, KBN2c, ldo2; };
template <typename T> __host__ __device__ inline LstmDims lstm_dims(int C) {
    constexpr int KB = ElemTraits<T>::KB, VEC = ElemTraits<T>::VEC;
    LstmDims d;
    d.KBN = (C + KB - 1) / KB;  d.Kp = d.KBN * KB;                                   // forward: K = C (the pack zero-padded to the k-block)
    d.KBNc = (d.KBN + LSTM_FWD_DEPTH - 1) / LSTM_FWD_DEPTH * LSTM_FWD_DEPTH;  d.ldo = d.KBNc * KB + VEC;
    d.KBN2 = 4 * C / KB;                                                             // backward: K = 4C, a multiple of 64
    d.KBN2c = (d.KBN2 + LSTM_BWD_DEPTH - 1) / LSTM_BWD_DEPTH * LSTM_BWD_DEPTH;  d.ldo2 = d.KBN2c * KB + VEC;
    return d;
}

// R [C, 4C] -> B-fragments; element j of lane l of a fragment: k = kb * KB + (l >> 4) * VEC + j, column = tile * 16 + (l & 15).
// which = 0 (forward, G = h R): [ct][kb][gate][64][VEC], k = row of R (zeros past C), column = gate * C + ct * 16 + (l & 15);
// which = 1 (backward, dh = dG R^T): [ct][kb][64][VEC], k = column of R, output channel = row of R.
template <typename T>
__global__ __launch_bounds__(256) void lstm_pack_kernel(const T* __restrict__ R, T* __restrict__ out, int C, int which) {
    constexpr int KB = ElemTraits<T>::KB, VEC = ElemTraits<T>::VEC;
    const LstmDims d = lstm_dims<T>(C);
    const long total = which ? (long)C * 4 * C : 4L * C * d.Kp;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i % VEC), l = (int)((i / VEC) % 64);
        long f = i / (VEC * 64);
        T v = from_f32<T>(0.f);
        if (which) {
            const int kb = (int)(f % d.KBN2), ct = (int)(f / d.KBN2);
            v = R[(long)(ct * 16 + (l & 15)) * 4 * C + kb * KB + (l >> 4) * VEC + j];
        } else {
            const int g = (int)(f % 4);
            f /= 4;
            const int kb = (int)(f % d.KBN), ct = (int)(f / d.KBN);
            const int k = kb * KB + (l >> 4) * VEC + j;
            if (k < C) v = R[(long)k * 4 * C + g * C + ct * 16 + (l & 15)];
        }
        out[i] = v;
    }
}

template <typename T> long lstm_pack_bytes_t(int C) { return 4L * C * lstm_dims<T>(C).Kp * (long)sizeof(T); }   // (>= the backward's 4 C^2)

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// slot 0 <- 1 <- 2 <- 3 <- 0 of a lane's per-tile values
__device__ __forceinline__ void rot4(float (&v)[LS_MAXT][4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float v0 = v[0][r];
#pragma unroll
        for (int j = 0; j + 1 < LS_MAXT; ++j) v[j][r] = v[j + 1][r];
        v[LS_MAXT - 1][r] = v0;
    }
}

struct LstmFwdP {
    const void* xp; const void* pack; const float* bR; int B, T, C;
    void* h; float* saved; void* hprev_c;
};

// MODE: bit 0 = `saved` is written, bit 1 = `hprev_c` is written.  FULL: every sample of the workgroup exists.
template <typename T, int D, int MODE, bool FULL>
__device__ __forceinline__ void lstm_fwd_steps(const LstmFwdP& p, T* op) {
    constexpr int KB = ElemTraits<T>::KB, VEC = ElemTraits<T>::VEC;
    constexpr long FRAG = 64 * VEC, QUAD = 4 * FRAG;                    // elements of one B-fragment / of the gate quad of a k-block
    const int C = p.C, tiles = C >> 4;
    const LstmDims d = lstm_dims<T>(C);
    const int KBN = d.KBN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T* xp = reinterpret_cast<const T*>(p.xp);
    T* hout = reinterpret_cast<T*>(p.h);
    T* hprev = reinterpret_cast<T*>(p.hprev_c);
    const int b0 = blockIdx.x * LS_TB, col = lane & 15, rg = (lane >> 4) * 4;
    const long C4 = 4L * C, C5 = 5L * C;
    // the wave's slice of the stream: tile ct = wave + j * 8 for j < nt, KBN quads each
    const int nt = wave < tiles ? (tiles - 1 - wave) / LS_NW + 1 : 0;
    const long tstep = (long)LS_NW * KBN * QUAD;
    const T* wbase = reinterpret_cast<const T*>(p.pack) + ((long)wave * KBN * 4 * 64 + lane) * VEC;
    Vec16<T> q[D][4];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) q[i][g] = zero16<T>();
    if (nt) {                                                           // the first chunk of the first tile
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) q[i][g] = ld16(wbase + (i < KBN ? i : KBN - 1) * QUAD + g * FRAG);
    }
    float cst[LS_MAXT][4];                                              // c of the lane's elements: never leaves these registers
#pragma unroll
    for (int j = 0; j < LS_MAXT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) cst[j][r] = 0.f;
    __syncthreads();     // (the zeroed operand tiles of the caller)
    for (int t = 0; t < p.T; ++t) {
        const T* opr = op + (size_t)(t & 1) * LS_TB * d.ldo;
        T* opw = op + (size_t)((t + 1) & 1) * LS_TB * d.ldo;
        const T* arow = opr + col * d.ldo + (lane >> 4) * VEC;          // A: row = sample (lane & 15), k chunk (lane >> 4)
#pragma unroll 1
        for (int j = 0; j < nt; ++j) {                                  // (the tile's c is slot 0 of cst)
            const int c = (wave + j * LS_NW) * 16 + col;
            const T* tb = wbase + j * tstep;
            const T* nb = j + 1 == nt ? wbase : tb + tstep;             // the wave's next tile; past its last one, the next step's first
            float xg[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int b = b0 + rg + r;
                const bool ok = FULL || b < p.B;                        // (a missing sample reads the last one's row and drops it)
                const T* x = xp + ((long)(ok ? b : p.B - 1) * p.T + t) * C4 + c;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float v = to_f32(x[g * C]);
                    xg[g][r] = ok ? v : 0.f;
                }
            }
            float bg[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) bg[g] = p.bR[g * C + c];
            f32x4 acc[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
            // ONE branch-free chunk body (two forms of it made the compiler refill a second register set and copy it over, with a
            // drained ring in front of the copies): an idle entry (kb >= KBN) meets the operand tile's zero columns, and the source
            // of a refill is selected, not branched on
            for (int kb0 = 0; kb0 < d.KBNc; kb0 += D) {
                const bool last = kb0 + D >= d.KBNc;                    // the tile's last chunk refills from the next tile's first
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    const Vec16<T> a = ld16(arow + (kb0 + i) * KB);
                    const int nk = last ? i : kb0 + i + D;
                    const T* s = (last ? nb : tb) + (long)(nk < KBN ? nk : KBN - 1) * QUAD;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        acc[g] = mma_kblock(a, q[i][g], acc[g]);
                        q[i][g] = ld16(s + g * FRAG);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = rg + r, b = b0 + s;
                const bool ok = FULL || b < p.B;
                const long pos = (long)b * p.T + t;
                const float gi = sigmoidf_(xg[0][r] + acc[0][r] + bg[0]);
                const float gf = sigmoidf_(xg[1][r] + acc[1][r] + bg[1]);
                const float gg = tanhf(xg[2][r] + acc[2][r] + bg[2]);
                const float go = sigmoidf_(xg[3][r] + acc[3][r] + bg[3]);
                const float cn = gf * cst[0][r] + gi * gg;
                const T hn = from_f32<T>(go * tanhf(cn));
                cst[0][r] = cn;
                if (ok) {
                    if (MODE & 1) {
                        float* sv = p.saved + pos * C5 + c;
                        sv[0] = gi; sv[C] = gf; sv[2 * C] = gg; sv[3 * C] = go; sv[4 * C] = cn;
                    }
                    hout[pos * C + c] = hn;
                    if (MODE & 2) hprev[pos * C + c] = opr[s * d.ldo + c];     // the state this step read, as the operand held it
                }
                opw[s * d.ldo + c] = hn;
            }
            rot4(cst);
        }
#pragma unroll 1
        for (int j = nt; j < LS_MAXT; ++j) rot4(cst);                   // (back in place for the next step)
        __syncthreads();     // (the other operand tile is complete; nobody reads this step's tile any more)
    }
}

template <typename T, int D, int MODE>
__global__ __launch_bounds__(LS_THREADS) void lstm_fwd_kernel(LstmFwdP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lstm_smem[];
    const LstmDims d = lstm_dims<T>(p.C);
    T* op = reinterpret_cast<T*>(lstm_smem);                            // [2][16][ldo] the state h as MFMA A operand
    for (int i = threadIdx.x; i < 2 * LS_TB * d.ldo; i += LS_THREADS) op[i] = from_f32<T>(0.f);
    if ((int)(blockIdx.x + 1) * LS_TB <= p.B) lstm_fwd_steps<T, D, MODE, true>(p, op);
    else lstm_fwd_steps<T, D, MODE, false>(p, op);
}

struct LstmBwdP {
    const void* d_h; const void* pack; const float* saved; int B, T, C;
    void* d_xp;
};

template <typename T, int DB, bool FULL>
__device__ __forceinline__ void lstm_bwd_steps(const LstmBwdP& p, T* op) {
    constexpr int KB = ElemTraits<T>::KB, VEC = ElemTraits<T>::VEC;
    constexpr long FRAG = 64 * VEC;
    const int C = p.C, tiles = C >> 4;
    const LstmDims d = lstm_dims<T>(C);
    const int KBN2 = d.KBN2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T* dout = reinterpret_cast<const T*>(p.d_h);
    T* dxp = reinterpret_cast<T*>(p.d_xp);
    const int b0 = blockIdx.x * LS_TB, col = lane & 15, rg = (lane >> 4) * 4;
    const long C4 = 4L * C, C5 = 5L * C;
    const int nt = wave < tiles ? (tiles - 1 - wave) / LS_NW + 1 : 0;
    const long tstep = (long)LS_NW * KBN2 * FRAG;
    const T* wbase = reinterpret_cast<const T*>(p.pack) + ((long)wave * KBN2 * 64 + lane) * VEC;
    Vec16<T> fb[DB];
#pragma unroll
    for (int i = 0; i < DB; ++i) fb[i] = zero16<T>();
    if (nt && p.T > 1) {                                                // lands under the first element-wise phase
#pragma unroll
        for (int i = 0; i < DB; ++i) fb[i] = ld16(wbase + (i < KBN2 ? i : KBN2 - 1) * FRAG);
    }
    float dcc[LS_MAXT][4], dhc[LS_MAXT][4];                             // carried dc and dh of the lane's elements
#pragma unroll
    for (int j = 0; j < LS_MAXT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) dcc[j][r] = dhc[j][r] = 0.f;
    __syncthreads();
    const T* arow = op + col * d.ldo2 + (lane >> 4) * VEC;
    for (int t = p.T - 1; t >= 0; --t) {
        const long back = t > 0 ? C5 : 0;                               // c_{t-1} sits one position back; at t = 0 it is the zero state
#pragma unroll 1
        for (int j = 0; j < nt; ++j) {                                  // (the tile's carries are slot 0 of dcc and dhc)
            const int c = (wave + j * LS_NW) * 16 + col;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = rg + r, b = b0 + s;
                const bool ok = FULL || b < p.B;
                const long pos = (long)b * p.T + t;
                float dh = dhc[0][r], gi = 0.f, gf = 0.f, gg = 0.f, go = 0.f, ct = 0.f, cp = 0.f;
                if (ok) {
                    dh += to_f32(dout[pos * C + c]);
                    const float* sv = p.saved + pos * C5 + c;
                    gi = sv[0]; gf = sv[C]; gg = sv[2 * C]; go = sv[3 * C]; ct = sv[4 * C];
                    const float cb = sv[4 * C - back];
                    cp = t > 0 ? cb : 0.f;
                }
                const float tc = tanhf(ct);
                const float dao = dh * tc * go * (1.0f - go);
                const float dc = dcc[0][r] + dh * go * (1.0f - tc * tc);
                const float dai = dc * gg * gi * (1.0f - gi);
                const float daf = dc * cp * gf * (1.0f - gf);
                const float dag = dc * gi * (1.0f - gg * gg);
                dcc[0][r] = dc * gf;
                const T ti = from_f32<T>(dai), tf = from_f32<T>(daf), tg = from_f32<T>(dag), to = from_f32<T>(dao);
                if (ok) {
                    T* x = dxp + pos * C4 + c;
                    x[0] = ti; x[C] = tf; x[2 * C] = tg; x[3 * C] = to;
                }
                T* o = op + s * d.ldo2 + c;
                o[0] = ti; o[C] = tf; o[2 * C] = tg; o[3 * C] = to;
            }
            rot4(dcc); rot4(dhc);
        }
        if (t == 0) break;                                              // (dh of the zero initial state is nobody's gradient)
#pragma unroll 1
        for (int j = nt; j < LS_MAXT; ++j) { rot4(dcc); rot4(dhc); }
        __syncthreads();
#pragma unroll 1
        for (int j = 0; j < nt; ++j) {
            const T* tb = wbase + j * tstep;
            const T* nb = j + 1 == nt ? wbase : tb + tstep;             // past the wave's last tile: the first one, for step t - 1
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int kb0 = 0; kb0 < d.KBN2c; kb0 += DB) {              // (one branch-free chunk body, as in the forward)
                const bool last = kb0 + DB >= d.KBN2c;
#pragma unroll
                for (int i = 0; i < DB; ++i) {
                    acc = mma_kblock(ld16(arow + (kb0 + i) * KB), fb[i], acc);
                    const int nk = last ? i : kb0 + i + DB;
                    fb[i] = ld16((last ? nb : tb) + (long)(nk < KBN2 ? nk : KBN2 - 1) * FRAG);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) dhc[0][r] = acc[r];             // dh_{t-1}'s carried part, on the lane that adds d_out to it
            rot4(dhc);
        }
#pragma unroll 1
        for (int j = nt; j < LS_MAXT; ++j) rot4(dhc);
        __syncthreads();
    }
}

template <typename T, int DB>
__global__ __launch_bounds__(LS_THREADS) void lstm_bwd_kernel(LstmBwdP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lstm_smem[];
    const LstmDims d = lstm_dims<T>(p.C);
    T* op = reinterpret_cast<T*>(lstm_smem);                            // [16][ldo2] dG of this step as MFMA A operand
    for (int i = threadIdx.x; i < LS_TB * d.ldo2; i += LS_THREADS) op[i] = from_f32<T>(0.f);
    if ((int)(blockIdx.x + 1) * LS_TB <= p.B) lstm_bwd_steps<T, DB, true>(p, op);
    else lstm_bwd_steps<T, DB, false>(p, op);
}

template <typename T, int MODE>
int lstm_fwd_launch(const LstmFwdP& p, size_t smem, hipStream_t st) {
    EDGL_LDS_LIMIT((lstm_fwd_kernel<T, LSTM_FWD_DEPTH, MODE>), smem, "edgl_lstm_seq_fwd");
    hipLaunchKernelGGL((lstm_fwd_kernel<T, LSTM_FWD_DEPTH, MODE>), dim3((unsigned)((p.B + LS_TB - 1) / LS_TB)), dim3(LS_THREADS), smem, st, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

template <typename T>
int lstm_fwd_t(const LstmFwdP& p, const void* R, hipStream_t st) {
    const LstmDims d = lstm_dims<T>(p.C);
    hipLaunchKernelGGL((lstm_pack_kernel<T>), dim3(grid_for(4L * p.C * d.Kp)), dim3(256), 0, st, reinterpret_cast<const T*>(R),
                       reinterpret_cast<T*>(const_cast<void*>(p.pack)), p.C, 0);
    const size_t smem = (size_t)2 * LS_TB * d.ldo * sizeof(T);
    switch ((p.saved ? 1 : 0) | (p.hprev_c ? 2 : 0)) {
        case 0: return lstm_fwd_launch<T, 0>(p, smem, st);
        case 1: return lstm_fwd_launch<T, 1>(p, smem, st);
        case 2: return lstm_fwd_launch<T, 2>(p, smem, st);
        default: return lstm_fwd_launch<T, 3>(p, smem, st);
    }
}

template <typename T>
int lstm_bwd_t(const LstmBwdP& p, const void* R, hipStream_t st) {
    const LstmDims d = lstm_dims<T>(p.C);
    hipLaunchKernelGGL((lstm_pack_kernel<T>), dim3(grid_for(4L * p.C * p.C)), dim3(256), 0, st, reinterpret_cast<const T*>(R),
                       reinterpret_cast<T*>(const_cast<void*>(p.pack)), p.C, 1);
    const size_t smem = (size_t)LS_TB * d.ldo2 * sizeof(T);
    EDGL_LDS_LIMIT((lstm_bwd_kernel<T, LSTM_BWD_DEPTH>), smem, "edgl_lstm_seq_bwd");
    hipLaunchKernelGGL((lstm_bwd_kernel<T, LSTM_BWD_DEPTH>), dim3((unsigned)((p.B + LS_TB - 1) / LS_TB)), dim3(LS_THREADS), smem, st, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

}  // namespace

extern "C" long edgl_lstm_seq_pack_bytes(int C, int dtype) {
    if (C < 16 || C > 512 || C % 16 || (dtype != EDGL_F32 && dtype != EDGL_BF16)) return -1;
    return dtype == EDGL_F32 ? lstm_pack_bytes_t<float>(C) : lstm_pack_bytes_t<bf16>(C);
}

extern "C" int edgl_lstm_seq_fwd(const void* xp, const void* R, const float* b_R, int B, int T, int C, void* h, float* saved,
                                 void* hprev_c, void* pack, int dtype, void* stream) {
    EDGL_REQUIRE(xp && R && b_R && h && pack, EDGL_ERR_NULL, "edgl_lstm_seq_fwd: null pointer");
    const int rc = gru_check("edgl_lstm_seq_fwd", B, T, C, dtype);
    if (rc != EDGL_OK) return rc;
    LstmFwdP p{xp, pack, b_R, B, T, C, h, saved, hprev_c};
    return dtype == EDGL_F32 ? lstm_fwd_t<float>(p, R, (hipStream_t)stream) : lstm_fwd_t<bf16>(p, R, (hipStream_t)stream);
}

extern "C" int edgl_lstm_seq_bwd(const void* d_h, const void* R, const float* saved, int B, int T, int C, void* d_xp, void* pack,
                                 int dtype, void* stream) {
    EDGL_REQUIRE(d_h && R && saved && d_xp && pack, EDGL_ERR_NULL, "edgl_lstm_seq_bwd: null pointer");
    const int rc = gru_check("edgl_lstm_seq_bwd", B, T, C, dtype);
    if (rc != EDGL_OK) return rc;
    LstmBwdP p{d_h, pack, saved, B, T, C, d_xp};
    return dtype == EDGL_F32 ? lstm_bwd_t<float>(p, R, (hipStream_t)stream) : lstm_bwd_t<bf16>(p, R, (hipStream_t)stream);
}
