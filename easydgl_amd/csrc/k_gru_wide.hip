// GRU sequence recurrence for the widths whose R does not stay in LDS: the arithmetic, the gate order, the saved
// layout, the operand dtypes and the ownership model of k_gru.hip — one workgroup of 8 waves owns 16 samples for ALL T steps, a
// wave takes channel tiles ct = wave, wave + 8, ..., state and carried dh are f32 in LDS, no atomics, and no workgroup ever waits
// for another one.  What differs is how R reaches the matrix pipe.
//
// Within a step a wave reads a FIXED list of 1 KiB B-fragments from the fragment-major pack (gru_common.h): (r, z, n) triples of
// its tiles' k-blocks in the forward, single fragments in the backward's dG R^T phase.  The list does not depend on the state, so
// it is treated as one cyclic stream per wave and read through a ring of registers, DEPTH entries deep, that is never drained:
//   * the k-loop is unrolled by the ring depth, so every ring index is a compile-time constant (the ring lives in VGPRs; a
//     fragment is already in MFMA B-operand layout and has one reader, so it needs no LDS round trip);
//   * the entry consumed by k-block kb is refilled at once with k-block kb + DEPTH of the same tile; in a tile's last chunk the
//     entries are refilled with the FIRST chunk of the wave's next tile, and in the last tile of a step with the first chunk of
//     the wave's first tile — the next step's.  Those loads are issued before the gate arithmetic and the step barrier and land
//     under them: only the A operand (the state tile in LDS) waits for the barrier.  Past the last step the wrap reads valid
//     addresses of the wave's own slice and is merely unused;
//   * a tile's k-blocks are padded to a whole number of chunks, so ring entry i always holds k-block = i (mod DEPTH) and a tile
//     always starts at entry 0; an idle entry (past the tile's last k-block) re-reads that last k-block and is not used;
//   * the memory counter (vmcnt) retires in order and the compiler sets every wait from the SHORTEST path that reaches it, so the
//     global accesses of the step are the same on every path: refills are unconditional (hence the re-read above), what the gate
//     phase reads (xp, b_R) is loaded at the START of the tile, in front of the refills, and the branches that would make the
//     count depend on the data are compile-time — MODE (is `saved` / `hprev_c` written) and FULL (a workgroup whose 16 samples
//     all exist stores without a row test; the one partial workgroup of a launch takes the other instantiation).
// Each accumulator takes its k-blocks in ascending order, as in k_gru.hip.  A wave that owns no tile (C / 16 < 8) issues nothing.
#include "edgl_common.h"
#include "gru_common.h"

#ifndef GRU_WIDE_FWD_DEPTH
#define GRU_WIDE_FWD_DEPTH 4      // (r, z, n) fragment triples in flight per wave: 12 KiB, 48 VGPRs
#endif
#ifndef GRU_WIDE_BWD_DEPTH
#define GRU_WIDE_BWD_DEPTH 12     // fragments in flight per wave in the backward's dG R^T phase: 12 KiB, 48 VGPRs
#endif

namespace {

constexpr int GW_TB = 16;                     // samples per workgroup
constexpr int GW_NW = 8;                      // waves per workgroup
constexpr int GW_THREADS = GW_NW * 64;

struct GruWideFwdP {
    const void* xp; const void* pack; const float* bR; int B, T, C;
    void* h; float* saved; void* hprev_c;
};

// MODE: bit 0 = `saved` is written, bit 1 = `hprev_c` is written.  FULL: every sample of the workgroup exists.
template <typename T, int D3, int MODE, bool FULL>
__device__ __forceinline__ void gru_wide_fwd_steps(const GruWideFwdP& p, float* hstate, T* op) {
    constexpr int KB = ElemTraits<T>::KB, VEC = ElemTraits<T>::VEC;
    constexpr long FRAG = 64 * VEC;                                     // elements of one B-fragment
    const int C = p.C, tiles = C >> 4;
    const GruDims d = gru_dims<T>(C);
    const int KBN = d.KBN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T* xp = reinterpret_cast<const T*>(p.xp);
    T* hout = reinterpret_cast<T*>(p.h);
    T* hprev = reinterpret_cast<T*>(p.hprev_c);
    const int b0 = blockIdx.x * GW_TB, col = lane & 15, rg = (lane >> 4) * 4;
    const long C3 = 3L * C, C5 = 5L * C;
    // the wave's slice of the stream: tile ct = wave + j * 8 for j < nt; gate g of a tile sits g * `gate` elements further
    const int nt = wave < tiles ? (tiles - 1 - wave) / GW_NW + 1 : 0;
    const long gate = (long)tiles * KBN * FRAG, tstep = (long)GW_NW * KBN * FRAG;
    const T* wbase = reinterpret_cast<const T*>(p.pack) + ((long)wave * KBN * 64 + lane) * VEC;
    Vec16<T> fr[D3], fz[D3], fn[D3];
#pragma unroll
    for (int i = 0; i < D3; ++i) {
        fr[i] = fz[i] = fn[i] = zero16<T>();
        if (nt) {                                                       // the first chunk of the first tile
            const T* s = wbase + (i < KBN ? i : KBN - 1) * FRAG;
            fr[i] = ld16(s); fz[i] = ld16(s + gate); fn[i] = ld16(s + 2 * gate);
        }
    }
    __syncthreads();     // (the zeroed state and operand tiles of the caller)
    for (int t = 0; t < p.T; ++t) {
        const T* opr = op + (size_t)(t & 1) * GW_TB * d.ldo;
        T* opw = op + (size_t)((t + 1) & 1) * GW_TB * d.ldo;
        const T* arow = opr + col * d.ldo + (lane >> 4) * VEC;          // A: row = sample (lane & 15), k chunk (lane >> 4)
        for (int j = 0; j < nt; ++j) {
            const int c = (wave + j * GW_NW) * 16 + col;
            const T* tb = wbase + j * tstep;
            const T* nb = j + 1 == nt ? wbase : tb + tstep;             // the wave's next tile; past its last one, the next step's first
            float xr[4], xz[4], xn[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int b = b0 + rg + r;
                const bool ok = FULL || b < p.B;                        // (a missing sample reads the last one's row and drops it)
                const T* x = xp + ((long)(ok ? b : p.B - 1) * p.T + t) * C3 + c;
                const float vr = to_f32(x[0]), vz = to_f32(x[C]), vn = to_f32(x[2 * C]);
                xr[r] = ok ? vr : 0.f; xz[r] = ok ? vz : 0.f; xn[r] = ok ? vn : 0.f;
            }
            const float bRr = p.bR[c], bRz = p.bR[C + c], bRn = p.bR[2 * C + c];
            f32x4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, an = ar;
            for (int kb0 = 0; kb0 < KBN; kb0 += D3) {
                if (kb0 + 2 * D3 <= KBN) {                              // an interior chunk: every entry is used and refilled in place
#pragma unroll
                    for (int i = 0; i < D3; ++i) {
                        const Vec16<T> a = ld16(arow + (kb0 + i) * KB);
                        ar = mma_kblock(a, fr[i], ar);
                        az = mma_kblock(a, fz[i], az);
                        an = mma_kblock(a, fn[i], an);
                        const T* s = tb + (long)(kb0 + i + D3) * FRAG;
                        fr[i] = ld16(s); fz[i] = ld16(s + gate); fn[i] = ld16(s + 2 * gate);
                    }
                } else {
                    const bool last = kb0 + D3 >= KBN;                  // the tile's last chunk refills from the next tile's first
#pragma unroll
                    for (int i = 0; i < D3; ++i) {
                        const int kb = kb0 + i;
                        if (kb < KBN) {
                            const Vec16<T> a = ld16(arow + kb * KB);
                            ar = mma_kblock(a, fr[i], ar);
                            az = mma_kblock(a, fz[i], az);
                            an = mma_kblock(a, fn[i], an);
                        }
                        const int nk = last ? i : kb + D3;
                        const T* s = (last ? nb : tb) + (long)(nk < KBN ? nk : KBN - 1) * FRAG;
                        fr[i] = ld16(s); fz[i] = ld16(s + gate); fn[i] = ld16(s + 2 * gate);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = rg + r, b = b0 + s;
                const bool ok = FULL || b < p.B;
                const long pos = (long)b * p.T + t;
                const float hp = hstate[s * C + c];
                const float gr = 1.0f / (1.0f + expf(-(xr[r] + ar[r] + bRr)));
                const float gz = 1.0f / (1.0f + expf(-(xz[r] + az[r] + bRz)));
                const float q = an[r] + bRn;
                const float n = tanhf(xn[r] + gr * q);
                const float hn = (1.0f - gz) * n + gz * hp;
                if (ok) {
                    if (MODE & 1) {
                        float* sv = p.saved + pos * C5 + c;
                        sv[0] = gr; sv[C] = gz; sv[2 * C] = n; sv[3 * C] = q; sv[4 * C] = hp;
                    }
                    hout[pos * C + c] = from_f32<T>(hn);
                    if (MODE & 2) hprev[pos * C + c] = from_f32<T>(hp);
                }
                hstate[s * C + c] = hn;
                opw[s * d.ldo + c] = from_f32<T>(hn);
            }
        }
        __syncthreads();     // (the other operand tile is complete; nobody reads this step's tile any more)
    }
}

template <typename T, int D3, int MODE>
__global__ __launch_bounds__(GW_THREADS) void gru_wide_fwd_kernel(GruWideFwdP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gruw_smem[];
    const GruDims d = gru_dims<T>(p.C);
    float* hstate = reinterpret_cast<float*>(gruw_smem);                // [16][C] f32, owner-accessed
    T* op = reinterpret_cast<T*>(gruw_smem + (size_t)GW_TB * p.C * sizeof(float));   // [2][16][ldo] the state as MFMA A operand
    for (int i = threadIdx.x; i < GW_TB * p.C; i += GW_THREADS) hstate[i] = 0.f;
    for (int i = threadIdx.x; i < 2 * GW_TB * d.ldo; i += GW_THREADS) op[i] = from_f32<T>(0.f);
    if ((int)(blockIdx.x + 1) * GW_TB <= p.B) gru_wide_fwd_steps<T, D3, MODE, true>(p, hstate, op);
    else gru_wide_fwd_steps<T, D3, MODE, false>(p, hstate, op);
}

struct GruWideBwdP {
    const void* d_h; const void* pack; const float* saved; int B, T, C;
    void* d_xp; void* d_gh;
};

template <typename T, int DB, bool FULL>
__device__ __forceinline__ void gru_wide_bwd_steps(const GruWideBwdP& p, float* dhc, T* op) {
    constexpr int KB = ElemTraits<T>::KB, VEC = ElemTraits<T>::VEC;
    constexpr long FRAG = 64 * VEC;
    const int C = p.C, tiles = C >> 4;
    const GruDims d = gru_dims<T>(C);
    const int KBN2 = d.KBN2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T* dout = reinterpret_cast<const T*>(p.d_h);
    T* dxp = reinterpret_cast<T*>(p.d_xp);
    T* dgh = reinterpret_cast<T*>(p.d_gh);
    const int b0 = blockIdx.x * GW_TB, col = lane & 15, rg = (lane >> 4) * 4;
    const long C3 = 3L * C, C5 = 5L * C;
    const int nt = wave < tiles ? (tiles - 1 - wave) / GW_NW + 1 : 0;
    const long tstep = (long)GW_NW * KBN2 * FRAG;
    const T* wbase = reinterpret_cast<const T*>(p.pack) + ((long)wave * KBN2 * 64 + lane) * VEC;
    Vec16<T> fb[DB];
#pragma unroll
    for (int i = 0; i < DB; ++i) {
        fb[i] = zero16<T>();
        if (nt && p.T > 1) fb[i] = ld16(wbase + (i < KBN2 ? i : KBN2 - 1) * FRAG);   // lands under the first element-wise phase
    }
    __syncthreads();
    const T* arow = op + col * d.ldo2 + (lane >> 4) * VEC;
    for (int t = p.T - 1; t >= 0; --t) {
        for (int j = 0; j < nt; ++j) {
            const int c = (wave + j * GW_NW) * 16 + col;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = rg + r, b = b0 + s;
                const bool ok = FULL || b < p.B;
                const long pos = (long)b * p.T + t;
                float dh = dhc[s * C + c], gr = 0.f, gz = 0.f, n = 0.f, q = 0.f, hp = 0.f;
                if (ok) {
                    dh += to_f32(dout[pos * C + c]);
                    const float* sv = p.saved + pos * C5 + c;
                    gr = sv[0]; gz = sv[C]; n = sv[2 * C]; q = sv[3 * C]; hp = sv[4 * C];
                }
                const float dan = dh * (1.0f - gz) * (1.0f - n * n);
                const float daz = dh * (hp - n) * gz * (1.0f - gz);
                const float dar = dan * q * gr * (1.0f - gr);
                const float dq = dan * gr;
                const T tr = from_f32<T>(dar), tz = from_f32<T>(daz), tn = from_f32<T>(dan), tq = from_f32<T>(dq);
                if (ok) {
                    T* x = dxp + pos * C3 + c;
                    x[0] = tr; x[C] = tz; x[2 * C] = tn;
                    T* g = dgh + pos * C3 + c;
                    g[0] = tr; g[C] = tz; g[2 * C] = tq;
                }
                T* o = op + s * d.ldo2 + c;
                o[0] = tr; o[C] = tz; o[2 * C] = tq;
                dhc[s * C + c] = gz * dh;                               // dh_prev = z * dh + dG_h R^T (added below)
            }
        }
        if (t == 0) break;                                              // (dh of the zero initial state is nobody's gradient)
        __syncthreads();
        for (int j = 0; j < nt; ++j) {
            const int c = (wave + j * GW_NW) * 16 + col;
            const T* tb = wbase + j * tstep;
            const T* nb = j + 1 == nt ? wbase : tb + tstep;             // past the wave's last tile: the first one, for step t - 1
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int kb0 = 0; kb0 < KBN2; kb0 += DB) {
                if (kb0 + 2 * DB <= KBN2) {
#pragma unroll
                    for (int i = 0; i < DB; ++i) {
                        acc = mma_kblock(ld16(arow + (kb0 + i) * KB), fb[i], acc);
                        fb[i] = ld16(tb + (long)(kb0 + i + DB) * FRAG);
                    }
                } else {
                    const bool last = kb0 + DB >= KBN2;
#pragma unroll
                    for (int i = 0; i < DB; ++i) {
                        const int kb = kb0 + i;
                        if (kb < KBN2) acc = mma_kblock(ld16(arow + kb * KB), fb[i], acc);
                        const int nk = last ? i : kb + DB;
                        fb[i] = ld16((last ? nb : tb) + (long)(nk < KBN2 ? nk : KBN2 - 1) * FRAG);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) dhc[(rg + r) * C + c] += acc[r];
        }
        __syncthreads();
    }
}

template <typename T, int DB>
__global__ __launch_bounds__(GW_THREADS) void gru_wide_bwd_kernel(GruWideBwdP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gruw_smem[];
    const GruDims d = gru_dims<T>(p.C);
    float* dhc = reinterpret_cast<float*>(gruw_smem);                   // [16][C] f32 carried dh, owner-accessed
    T* op = reinterpret_cast<T*>(gruw_smem + (size_t)GW_TB * p.C * sizeof(float));   // [16][ldo2] dG_h of this step as MFMA A operand
    for (int i = threadIdx.x; i < GW_TB * p.C; i += GW_THREADS) dhc[i] = 0.f;
    for (int i = threadIdx.x; i < GW_TB * d.ldo2; i += GW_THREADS) op[i] = from_f32<T>(0.f);
    if ((int)(blockIdx.x + 1) * GW_TB <= p.B) gru_wide_bwd_steps<T, DB, true>(p, dhc, op);
    else gru_wide_bwd_steps<T, DB, false>(p, dhc, op);
}

template <typename T, int MODE>
int gru_wide_fwd_launch(const GruWideFwdP& p, size_t smem, hipStream_t st) {
    EDGL_LDS_LIMIT((gru_wide_fwd_kernel<T, GRU_WIDE_FWD_DEPTH, MODE>), smem, "edgl_gru_wide_fwd");
    hipLaunchKernelGGL((gru_wide_fwd_kernel<T, GRU_WIDE_FWD_DEPTH, MODE>), dim3((unsigned)((p.B + GW_TB - 1) / GW_TB)), dim3(GW_THREADS),
                       smem, st, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

template <typename T>
int gru_wide_fwd_t(const GruWideFwdP& p, const void* R, hipStream_t st) {
    const GruDims d = gru_dims<T>(p.C);
    hipLaunchKernelGGL((gru_pack_kernel<T>), dim3(grid_for(3L * p.C * d.Kp)), dim3(256), 0, st, reinterpret_cast<const T*>(R),
                       reinterpret_cast<T*>(const_cast<void*>(p.pack)), p.C, 0);
    const size_t smem = (size_t)GW_TB * p.C * sizeof(float) + (size_t)2 * GW_TB * d.ldo * sizeof(T);
    switch ((p.saved ? 1 : 0) | (p.hprev_c ? 2 : 0)) {
        case 0: return gru_wide_fwd_launch<T, 0>(p, smem, st);
        case 1: return gru_wide_fwd_launch<T, 1>(p, smem, st);
        case 2: return gru_wide_fwd_launch<T, 2>(p, smem, st);
        default: return gru_wide_fwd_launch<T, 3>(p, smem, st);
    }
}

template <typename T>
int gru_wide_bwd_t(const GruWideBwdP& p, const void* R, hipStream_t st) {
    const GruDims d = gru_dims<T>(p.C);
    hipLaunchKernelGGL((gru_pack_kernel<T>), dim3(grid_for((long)p.C * d.K2p)), dim3(256), 0, st, reinterpret_cast<const T*>(R),
                       reinterpret_cast<T*>(const_cast<void*>(p.pack)), p.C, 1);
    const size_t smem = (size_t)GW_TB * p.C * sizeof(float) + (size_t)GW_TB * d.ldo2 * sizeof(T);
    const dim3 grid((unsigned)((p.B + GW_TB - 1) / GW_TB));
    EDGL_LDS_LIMIT((gru_wide_bwd_kernel<T, GRU_WIDE_BWD_DEPTH>), smem, "edgl_gru_wide_bwd");
    hipLaunchKernelGGL((gru_wide_bwd_kernel<T, GRU_WIDE_BWD_DEPTH>), grid, dim3(GW_THREADS), smem, st, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

}  // namespace

extern "C" int edgl_gru_wide_fwd(const void* xp, const void* R, const float* b_R, int B, int T, int C, void* h, float* saved,
                                 void* hprev_c, void* pack, int dtype, void* stream) {
    EDGL_REQUIRE(xp && R && b_R && h && pack, EDGL_ERR_NULL, "edgl_gru_wide_fwd: null pointer");
    const int rc = gru_check("edgl_gru_wide_fwd", B, T, C, dtype);
    if (rc != EDGL_OK) return rc;
    GruWideFwdP p{xp, pack, b_R, B, T, C, h, saved, hprev_c};
    return dtype == EDGL_F32 ? gru_wide_fwd_t<float>(p, R, (hipStream_t)stream) : gru_wide_fwd_t<bf16>(p, R, (hipStream_t)stream);
}

extern "C" int edgl_gru_wide_bwd(const void* d_h, const void* R, const float* saved, int B, int T, int C, void* d_xp, void* d_gh,
                                 void* pack, int dtype, void* stream) {
    EDGL_REQUIRE(d_h && R && saved && d_xp && d_gh && pack, EDGL_ERR_NULL, "edgl_gru_wide_bwd: null pointer");
    const int rc = gru_check("edgl_gru_wide_bwd", B, T, C, dtype);
    if (rc != EDGL_OK) return rc;
    GruWideBwdP p{d_h, pack, saved, B, T, C, d_xp, d_gh};
    return dtype == EDGL_F32 ? gru_wide_bwd_t<float>(p, R, (hipStream_t)stream) : gru_wide_bwd_t<bf16>(p, R, (hipStream_t)stream);
}
