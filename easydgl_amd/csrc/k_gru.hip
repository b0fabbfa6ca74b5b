// GRU sequence recurrence (S2PNM's recurrent layer): one unidirectional layer in cuDNN's form
//   r = s(xp_r + h R_r + b_Rr)   z = s(xp_z + h R_z + b_Rz)   n = tanh(xp_n + r * (h R_n + b_Rn))   h' = (1 - z) n + z h
// over xp = x W + b_W (one plain GEMM, not here), zero initial state, every position a step.
//
// One workgroup owns GRU_TB = 16 samples (one MFMA row tile) for ALL T steps: no communication between workgroups, no grid
// barrier, no atomics — the op is bit-reproducible by construction.  The parallelism is ceil(B / 16) workgroups: a latency-bound
// kernel on a fraction of the chip.  Per step a wave takes channel tiles ct = wave, wave + 8, ...: three 16x16 accumulators
// (gates r, z, n of the same 16 channels) over K = C, then the gate arithmetic on the accumulator layout itself — the lane that
// holds G[sample][channel] owns the f32 state of that element (LDS, owner-accessed) and writes its operand copy (dtype T) into the
// OTHER of two operand tiles: one barrier per step.  R is read as MFMA B-fragments from a fragment-major pack ([tile][k-block]
// [lane][16 bytes]: every wave load is one contiguous KiB), resident in LDS for the whole launch where it fits in 96 KiB, else
// streamed from L2 every step.  The state, the gates and everything saved are f32; T is the MFMA operand dtype only.
#include "edgl_common.h"

namespace {

constexpr int GRU_TB = 16;                    // samples per workgroup
constexpr int GRU_NW = 8;                     // waves per workgroup
constexpr int GRU_THREADS = GRU_NW * 64;
constexpr long GRU_RES_BYTES = 96 * 1024;     // a pack of at most this many bytes stays in LDS

struct GruDims { int KBN, Kp, ldo, KBN2, K2p, ldo2; };
template <typename T> __host__ __device__ inline GruDims gru_dims(int C) {
    constexpr int KB = ElemTraits<T>::KB, VEC = ElemTraits<T>::VEC;
    GruDims d;
    d.KBN = (C + KB - 1) / KB;  d.Kp = d.KBN * KB;  d.ldo = d.Kp + VEC;              // forward: K = C (zero-padded to the k-block)
    d.KBN2 = (3 * C + KB - 1) / KB;  d.K2p = d.KBN2 * KB;  d.ldo2 = d.K2p + VEC;     // backward: K = 3C
    return d;
}

// R [C, 3C] -> B-fragments.  which = 0 (forward, G = h R): tile nt of the 3C output columns, k = row of R;
// which = 1 (backward, dh = dG R^T): tile ct of the C output channels, k = column of R.
// element j of lane l of (tile, kb): k = kb * KB + (l >> 4) * VEC + j, column = tile * 16 + (l & 15); zeros past the true K.
template <typename T>
__global__ __launch_bounds__(256) void gru_pack_kernel(const T* __restrict__ R, T* __restrict__ out, int C, int which) {
    constexpr int KB = ElemTraits<T>::KB, VEC = ElemTraits<T>::VEC;
    const GruDims d = gru_dims<T>(C);
    const int kbn = which ? d.KBN2 : d.KBN, ntile = which ? C / 16 : 3 * C / 16, ktrue = which ? 3 * C : C;
    const long total = (long)ntile * kbn * 64 * VEC;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i % VEC), l = (int)((i / VEC) % 64);
        const long tk = i / (VEC * 64);
        const int kb = (int)(tk % kbn), tile = (int)(tk / kbn);
        const int k = kb * KB + (l >> 4) * VEC + j, col = tile * 16 + (l & 15);
        T v = from_f32<T>(0.f);
        if (k < ktrue) v = which ? R[(long)col * 3 * C + k] : R[(long)k * 3 * C + col];
        out[i] = v;
    }
}

struct GruFwdP {
    const void* xp; const void* pack; const float* bR; int B, T, C;
    void* h; float* saved; void* hprev_c;
};

template <typename T, bool RES>
__global__ __launch_bounds__(GRU_THREADS) void gru_seq_fwd_kernel(GruFwdP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gru_smem[];
    constexpr int KB = ElemTraits<T>::KB, VEC = ElemTraits<T>::VEC;
    const int C = p.C, tiles = C >> 4;
    const GruDims d = gru_dims<T>(C);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long pack_elems = (long)3 * C * d.Kp;
    T* spack = reinterpret_cast<T*>(gru_smem);
    size_t off = RES ? (size_t)pack_elems * sizeof(T) : 0;
    float* hstate = reinterpret_cast<float*>(gru_smem + off);           // [16][C] f32, owner-accessed
    off += (size_t)GRU_TB * C * sizeof(float);
    T* op = reinterpret_cast<T*>(gru_smem + off);                       // [2][16][ldo] the state as MFMA A operand
    const T* gpack = reinterpret_cast<const T*>(p.pack);
    if (RES)
        for (long i = (long)threadIdx.x * VEC; i < pack_elems; i += (long)GRU_THREADS * VEC) st16(spack + i, ld16(gpack + i));
    for (int i = threadIdx.x; i < GRU_TB * C; i += GRU_THREADS) hstate[i] = 0.f;
    for (int i = threadIdx.x; i < 2 * GRU_TB * d.ldo; i += GRU_THREADS) op[i] = from_f32<T>(0.f);
    __syncthreads();
    const T* bsrc = RES ? spack : gpack;
    const T* xp = reinterpret_cast<const T*>(p.xp);
    T* hout = reinterpret_cast<T*>(p.h);
    T* hprev = reinterpret_cast<T*>(p.hprev_c);
    const int b0 = blockIdx.x * GRU_TB, col = lane & 15, rg = (lane >> 4) * 4;
    const long C3 = 3L * C, C5 = 5L * C;
    for (int t = 0; t < p.T; ++t) {
        const T* opr = op + (size_t)(t & 1) * GRU_TB * d.ldo;
        T* opw = op + (size_t)((t + 1) & 1) * GRU_TB * d.ldo;
        for (int ct = wave; ct < tiles; ct += GRU_NW) {
            f32x4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, an = ar;
            const T* arow = opr + col * d.ldo + (lane >> 4) * VEC;      // A: row = sample (lane & 15), k chunk (lane >> 4)
            const T* br = bsrc + ((long)ct * d.KBN * 64 + lane) * VEC;
            const T* bz = bsrc + ((long)(tiles + ct) * d.KBN * 64 + lane) * VEC;
            const T* bn = bsrc + ((long)(2 * tiles + ct) * d.KBN * 64 + lane) * VEC;
            for (int kb = 0; kb < d.KBN; ++kb) {
                const Vec16<T> a = ld16(arow + kb * KB);
                const long bo = (long)kb * 64 * VEC;
                ar = mma_kblock(a, ld16(br + bo), ar);
                az = mma_kblock(a, ld16(bz + bo), az);
                an = mma_kblock(a, ld16(bn + bo), an);
            }
            const int c = ct * 16 + col;
            const float bRr = p.bR[c], bRz = p.bR[C + c], bRn = p.bR[2 * C + c];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = rg + r, b = b0 + s;
                const bool ok = b < p.B;
                const long pos = (long)b * p.T + t;
                float xr = 0.f, xz = 0.f, xn = 0.f;
                if (ok) {
                    const T* x = xp + pos * C3 + c;
                    xr = to_f32(x[0]); xz = to_f32(x[C]); xn = to_f32(x[2 * C]);
                }
                const float hp = hstate[s * C + c];
                const float gr = 1.0f / (1.0f + expf(-(xr + ar[r] + bRr)));
                const float gz = 1.0f / (1.0f + expf(-(xz + az[r] + bRz)));
                const float q = an[r] + bRn;
                const float n = tanhf(xn + gr * q);
                const float hn = (1.0f - gz) * n + gz * hp;
                if (ok) {
                    if (p.saved) {
                        float* sv = p.saved + pos * C5 + c;
                        sv[0] = gr; sv[C] = gz; sv[2 * C] = n; sv[3 * C] = q; sv[4 * C] = hp;
                    }
                    hout[pos * C + c] = from_f32<T>(hn);
                    if (hprev) hprev[pos * C + c] = from_f32<T>(hp);
                }
                hstate[s * C + c] = hn;
                opw[s * d.ldo + c] = from_f32<T>(hn);
            }
        }
        __syncthreads();     // (the other operand tile is complete; nobody reads this step's tile any more)
    }
}

struct GruBwdP {
    const void* d_h; const void* pack; const float* saved; int B, T, C;
    void* d_xp; void* d_gh;
};

template <typename T, bool RES>
__global__ __launch_bounds__(GRU_THREADS) void gru_seq_bwd_kernel(GruBwdP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gru_smem[];
    constexpr int KB = ElemTraits<T>::KB, VEC = ElemTraits<T>::VEC;
    const int C = p.C, tiles = C >> 4;
    const GruDims d = gru_dims<T>(C);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long pack_elems = (long)C * d.K2p;
    T* spack = reinterpret_cast<T*>(gru_smem);
    size_t off = RES ? (size_t)pack_elems * sizeof(T) : 0;
    float* dhc = reinterpret_cast<float*>(gru_smem + off);              // [16][C] f32 carried dh, owner-accessed
    off += (size_t)GRU_TB * C * sizeof(float);
    T* op = reinterpret_cast<T*>(gru_smem + off);                       // [16][ldo2] dG_h of this step as MFMA A operand
    const T* gpack = reinterpret_cast<const T*>(p.pack);
    if (RES)
        for (long i = (long)threadIdx.x * VEC; i < pack_elems; i += (long)GRU_THREADS * VEC) st16(spack + i, ld16(gpack + i));
    for (int i = threadIdx.x; i < GRU_TB * C; i += GRU_THREADS) dhc[i] = 0.f;
    for (int i = threadIdx.x; i < GRU_TB * d.ldo2; i += GRU_THREADS) op[i] = from_f32<T>(0.f);
    __syncthreads();
    const T* bsrc = RES ? spack : gpack;
    const T* dout = reinterpret_cast<const T*>(p.d_h);
    T* dxp = reinterpret_cast<T*>(p.d_xp);
    T* dgh = reinterpret_cast<T*>(p.d_gh);
    const int b0 = blockIdx.x * GRU_TB, col = lane & 15, rg = (lane >> 4) * 4;
    const long C3 = 3L * C, C5 = 5L * C;
    for (int t = p.T - 1; t >= 0; --t) {
        for (int ct = wave; ct < tiles; ct += GRU_NW) {
            const int c = ct * 16 + col;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = rg + r, b = b0 + s;
                const bool ok = b < p.B;
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
        for (int ct = wave; ct < tiles; ct += GRU_NW) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const T* arow = op + col * d.ldo2 + (lane >> 4) * VEC;
            const T* bp = bsrc + ((long)ct * d.KBN2 * 64 + lane) * VEC;
            for (int kb = 0; kb < d.KBN2; ++kb) acc = mma_kblock(ld16(arow + kb * KB), ld16(bp + (long)kb * 64 * VEC), acc);
            const int c = ct * 16 + col;
#pragma unroll
            for (int r = 0; r < 4; ++r) dhc[(rg + r) * C + c] += acc[r];
        }
        __syncthreads();
    }
}

template <typename T> long gru_pack_bytes_t(int C) {
    const GruDims d = gru_dims<T>(C);
    const long f = 3L * C * d.Kp, b = (long)C * d.K2p;
    return (f > b ? f : b) * (long)sizeof(T);
}

int gru_check(const char* who, int B, int T, int C, int dtype) {
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "%s: bad dtype %d", who, dtype);
    EDGL_REQUIRE(B > 0 && T > 0 && C >= 16 && C <= 512 && C % 16 == 0, EDGL_ERR_SHAPE,
                 "%s: bad shape B=%d T=%d C=%d (C a multiple of 16 up to 512, B >= 1, T >= 1)", who, B, T, C);
    EDGL_REQUIRE((double)B * T * 5.0 * C < 9.0e15 && (long)B * T < 2147483647L, EDGL_ERR_SHAPE, "%s: B*T too large", who);
    return EDGL_OK;
}

template <typename T>
int gru_fwd_t(const GruFwdP& p, void* pack, const void* R, hipStream_t st) {
    const GruDims d = gru_dims<T>(p.C);
    hipLaunchKernelGGL((gru_pack_kernel<T>), dim3(grid_for(3L * p.C * d.Kp)), dim3(256), 0, st, reinterpret_cast<const T*>(R),
                       reinterpret_cast<T*>(pack), p.C, 0);
    const size_t pack_bytes = (size_t)3 * p.C * d.Kp * sizeof(T);
    const bool res = (long)pack_bytes <= GRU_RES_BYTES;
    const size_t smem = (res ? pack_bytes : 0) + (size_t)GRU_TB * p.C * sizeof(float) + (size_t)2 * GRU_TB * d.ldo * sizeof(T);
    const dim3 grid((unsigned)((p.B + GRU_TB - 1) / GRU_TB));
    if (res) {
        EDGL_LDS_LIMIT((gru_seq_fwd_kernel<T, true>), smem, "edgl_gru_seq_fwd");
        hipLaunchKernelGGL((gru_seq_fwd_kernel<T, true>), grid, dim3(GRU_THREADS), smem, st, p);
    } else {
        EDGL_LDS_LIMIT((gru_seq_fwd_kernel<T, false>), smem, "edgl_gru_seq_fwd");
        hipLaunchKernelGGL((gru_seq_fwd_kernel<T, false>), grid, dim3(GRU_THREADS), smem, st, p);
    }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

template <typename T>
int gru_bwd_t(const GruBwdP& p, void* pack, const void* R, hipStream_t st) {
    const GruDims d = gru_dims<T>(p.C);
    hipLaunchKernelGGL((gru_pack_kernel<T>), dim3(grid_for((long)p.C * d.K2p)), dim3(256), 0, st, reinterpret_cast<const T*>(R),
                       reinterpret_cast<T*>(pack), p.C, 1);
    const size_t pack_bytes = (size_t)p.C * d.K2p * sizeof(T);
    const bool res = (long)pack_bytes <= GRU_RES_BYTES;
    const size_t smem = (res ? pack_bytes : 0) + (size_t)GRU_TB * p.C * sizeof(float) + (size_t)GRU_TB * d.ldo2 * sizeof(T);
    const dim3 grid((unsigned)((p.B + GRU_TB - 1) / GRU_TB));
    if (res) {
        EDGL_LDS_LIMIT((gru_seq_bwd_kernel<T, true>), smem, "edgl_gru_seq_bwd");
        hipLaunchKernelGGL((gru_seq_bwd_kernel<T, true>), grid, dim3(GRU_THREADS), smem, st, p);
    } else {
        EDGL_LDS_LIMIT((gru_seq_bwd_kernel<T, false>), smem, "edgl_gru_seq_bwd");
        hipLaunchKernelGGL((gru_seq_bwd_kernel<T, false>), grid, dim3(GRU_THREADS), smem, st, p);
    }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

}  // namespace

extern "C" long edgl_gru_seq_pack_bytes(int C, int dtype) {
    if (C < 16 || C > 512 || C % 16 || (dtype != EDGL_F32 && dtype != EDGL_BF16)) return -1;
    return dtype == EDGL_F32 ? gru_pack_bytes_t<float>(C) : gru_pack_bytes_t<bf16>(C);
}

extern "C" int edgl_gru_seq_resident(int C, int dtype) {
    if (C < 16 || C > 512 || C % 16 || (dtype != EDGL_F32 && dtype != EDGL_BF16)) return -1;
    return edgl_gru_seq_pack_bytes(C, dtype) <= GRU_RES_BYTES ? 1 : 0;
}

extern "C" int edgl_gru_seq_fwd(const void* xp, const void* R, const float* b_R, int B, int T, int C, void* h, float* saved,
                                void* hprev_c, void* pack, int dtype, void* stream) {
    EDGL_REQUIRE(xp && R && b_R && h && pack, EDGL_ERR_NULL, "edgl_gru_seq_fwd: null pointer");
    const int rc = gru_check("edgl_gru_seq_fwd", B, T, C, dtype);
    if (rc != EDGL_OK) return rc;
    GruFwdP p{xp, pack, b_R, B, T, C, h, saved, hprev_c};
    return dtype == EDGL_F32 ? gru_fwd_t<float>(p, pack, R, (hipStream_t)stream) : gru_fwd_t<bf16>(p, pack, R, (hipStream_t)stream);
}

extern "C" int edgl_gru_seq_bwd(const void* d_h, const void* R, const float* saved, int B, int T, int C, void* d_xp, void* d_gh,
                                void* pack, int dtype, void* stream) {
    EDGL_REQUIRE(d_h && R && saved && d_xp && d_gh && pack, EDGL_ERR_NULL, "edgl_gru_seq_bwd: null pointer");
    const int rc = gru_check("edgl_gru_seq_bwd", B, T, C, dtype);
    if (rc != EDGL_OK) return rc;
    GruBwdP p{d_h, pack, saved, B, T, C, d_xp, d_gh};
    return dtype == EDGL_F32 ? gru_bwd_t<float>(p, pack, R, (hipStream_t)stream) : gru_bwd_t<bf16>(p, pack, R, (hipStream_t)stream);
}
