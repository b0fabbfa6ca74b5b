// K13: dilated 1-D convolution over the sequence with a LayerNorm / ReLU epilogue — Conv1D + layernorm + relu of MaskedCNN
// (sequential.py:140-207; GREC, Yuan et al., WWW'20).  x [B,T,C], W [fw,C,C] (tap, in, out), dilation d:
//     o_j = j d - (fw-1) d (causal: left pad, VALID) | j d - floor((fw-1) d / 2) (SAME);   rows outside [0,T) are zero
//     z[b,t,n] = bias[n] + sum_j sum_c x[b,t+o_j,c] W[j,c,n];   y = relu(gamma (z - mean) rstd + beta) (+ r),  eps = 1e-8
// No im2col buffer and no [B,T,C] intermediate besides z: the operand of a tile is read once, not fw times.
//
// Staging primitive (stage_rows): a workgroup owns one sample and DC_TR = 64 consecutive time rows; it writes the rows
// [t0 + min o_j, t0 + 64 + max o_j) of its operand into LDS once, rows outside [0,T) as zeros, in the row-chunk layout of the
// other kernels ([row][channel], rows padded by 4 elements: conflict-free 8 / 16-byte reads).  Every tap reads its 16-row
// windows from that image at a row offset; the MFMA loop has no bounds check.
// Forward / input gradient (dconv_kernel<LN>): one contraction, z^T tile = W_j^T . x^T — a wave owns 16 rows (on lane & 15) and
// all C columns, C/16 accumulator tiles; the weight fragments come straight from L2 (every workgroup reads the same
// fw C^2 elements; the forward reads a [tap][out][in] copy made by dconv_pack_w, the input gradient reads W as it is stored
// with mirrored offsets -o_j).  The forward's epilogue stays in registers: bias, row mean / variance of the f32 accumulators
// (in-lane sums + two row swaps), scale, shift, ReLU, residual.  The ReLU mask is decided ONCE, from the f32 accumulator, and
// saved packed (one byte per four channels, the lane's nibble); the backward reads those bits and never re-derives them from the
// rounded z (a z within bf16 rounding of the threshold would flip against the forward).
// Row-wise backward (dconv_rows_bwd_kernel): 16 lanes per row; ReLU and LayerNorm backward -> dz, one partial row
// dgamma | dbeta | dbias per workgroup.  Weight gradient (dconv_dw_kernel): a workgroup owns (tap, slab of samples, block of
// 128 output columns); per 32 rows it stages x shifted by o_j and dz, turns the tiles through the identity (rows become the
// contraction index) and accumulates [C/4 per wave] x [128] in registers; f32 partials [slab][fw][C][C], summed in a fixed
// order.  No f32 atomics anywhere: the kernels are bitwise reproducible and have no second "deterministic" form.
// Outputs are plain stores (write-through stores were measured for the other kernels and not kept: DESIGN 7, rule 80).
#include "tattn_common.h"   // frag_st, turn

namespace {

constexpr int DC_TR = 64;        // time rows of a workgroup of the forward / input-gradient kernel (4 waves x 16)
constexpr int DC_TRW = 32;       // rows per step of the weight-gradient kernel
constexpr int DC_PAD = 4;        // elements a row of an LDS image is padded by
constexpr int DC_NBT = 8;        // output-column tiles (of 16) per weight-gradient workgroup
constexpr int DC_ROWS_GRID = 1024;
constexpr size_t DC_LDS = 160 * 1024;
constexpr float DC_EPS = 1e-8f;  // normalize.py

struct DcP {
    const void *x, *w, *r, *z, *dy;
    const float *bias, *gamma, *beta;
    void *y, *zout, *dz;
    uint8_t* mask;             // [B*T][C/4]: bit r of a byte = channel 4 q + r passed the ReLU
    float *mean, *rstd, *part;
    int B, T, NB;              // NB: row blocks per sample
    int fw, o0, step, omin, rows, slabs;   // o_j = o0 + j step; image = rows [t0 + omin, t0 + omin + rows)
};

__device__ __forceinline__ float ln_val(float z, float mean, float rstd, float gamma, float beta) {
    return fmaf((z - mean) * rstd, gamma, beta);
}
__device__ __forceinline__ float sum16(float v) {   // over the 16 lanes that share lane >> 4
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// rows [t_lo, t_lo + rows) of one sample (src [T][C]) into img[rows][C + DC_PAD]; rows outside [0, T) are zeros
template <typename T>
__device__ __forceinline__ void stage_rows(T* img, const T* src, int Tn, int C, int t_lo, int rows) {
    const int per = C >> 2, ld = C + DC_PAD;
    for (int i = threadIdx.x; i < rows * per; i += blockDim.x) {
        const int rr = i / per, q = i - rr * per, t = t_lo + rr;
        const Frag4<T> f = (t >= 0 && t < Tn) ? frag_ld<T>(src + (long)t * C + q * 4) : frag_zero<T>();
        frag_st<T>(img + rr * ld + q * 4, f);
    }
}

// acc[nt][r] += sum_j sum_c wrows[j][n = nt 16 + g4 + r][c] img[lr0 + l15 + o_j - omin][c]
template <typename T, int CT>
__device__ __forceinline__ void contract(const T* img, const T* wrows, const DcP& p, int lr0, f32x4 (&acc)[CT]) {
    constexpr int C = CT * 16, LD = C + DC_PAD;
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15;
    for (int j = 0; j < p.fw; ++j) {
        const T* xr = img + (lr0 + l15 + p.o0 + j * p.step - p.omin) * LD + g4;
        const T* wj = wrows + ((long)j * C + l15) * C + g4;
        for (int kc = 0; kc < CT; ++kc) {
            const Frag4<T> b = frag_ld<T>(xr + kc * 16);
#pragma unroll
            for (int nt = 0; nt < CT; ++nt) acc[nt] = mma16(frag_ld<T>(wj + (long)nt * 16 * C + kc * 16), b, acc[nt]);
        }
    }
}

// LN: the forward (x, packed W -> y, z, mean, rstd); otherwise the input gradient (x := dz, W as stored -> y := dx)
template <typename T, int CT, bool LN>
__global__ __launch_bounds__(256) void dconv_kernel(DcP p) {
    constexpr int C = CT * 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char dc_smem[];
    T* img = reinterpret_cast<T*>(dc_smem);
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15, lr0 = (threadIdx.x >> 6) * 16;
    const int b = blockIdx.x / p.NB, t0 = (blockIdx.x % p.NB) * DC_TR;
    stage_rows<T>(img, reinterpret_cast<const T*>(p.x) + (long)b * p.T * C, p.T, C, t0 + p.omin, p.rows);
    __syncthreads();
    if (t0 + lr0 >= p.T) return;      // (wave-uniform, behind the only barrier)
    f32x4 acc[CT];
#pragma unroll
    for (int nt = 0; nt < CT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    contract<T, CT>(img, reinterpret_cast<const T*>(p.w), p, lr0, acc);
    const int t = t0 + lr0 + l15;
    const bool ok = t < p.T;
    const long row = (long)b * p.T + min(t, p.T - 1);
    T* yr = reinterpret_cast<T*>(p.y) + row * C + g4;
    if constexpr (!LN) {
        if (ok) {
#pragma unroll
            for (int nt = 0; nt < CT; ++nt) frag_st<T>(yr + nt * 16, frag_from_acc<T>(acc[nt]));
        }
    } else {
        float s = 0.f;
#pragma unroll
        for (int nt = 0; nt < CT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                acc[nt][r] += p.bias[nt * 16 + g4 + r];
                s += acc[nt][r];
            }
        const float mean = group_sum4(s) * (1.0f / C);
        float q = 0.f;
#pragma unroll
        for (int nt = 0; nt < CT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float dv = acc[nt][r] - mean; q += dv * dv; }
        const float rstd = 1.0f / sqrtf(group_sum4(q) * (1.0f / C) + DC_EPS);
        if (!ok) return;
        const T* rr = p.r ? reinterpret_cast<const T*>(p.r) + row * C + g4 : nullptr;
        T* zr = p.zout ? reinterpret_cast<T*>(p.zout) + row * C + g4 : nullptr;
        uint8_t* mr = p.zout ? p.mask + row * (C / 4) + (g4 >> 2) : nullptr;
#pragma unroll
        for (int nt = 0; nt < CT; ++nt) {
            f32x4 o;
            uint32_t bits = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = nt * 16 + g4 + r;
                o[r] = ln_val(acc[nt][r], mean, rstd, p.gamma[c], p.beta[c]);
                bits |= o[r] > 0.f ? 1u << r : 0u;
                o[r] = fmaxf(o[r], 0.f);
            }
            if (mr) mr[nt * 4] = (uint8_t)bits;
            if (rr) {
                const Frag4<T> rf = frag_ld<T>(rr + nt * 16);
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] += to_f32(rf.v[r]);
            }
            if (zr) frag_st<T>(zr + nt * 16, frag_from_acc<T>(acc[nt]));
            frag_st<T>(yr + nt * 16, frag_from_acc<T>(o));
        }
        if (p.mean && g4 == 0) { p.mean[row] = mean; p.rstd[row] = rstd; }
    }
}

// wt[j][n][c] = w[j][c][n]: the forward's weight fragments are contiguous along the contraction index
template <typename T>
__global__ __launch_bounds__(256) void dconv_pack_w_kernel(const T* w, T* wt, int fw, int C) {
    const long n_all = (long)fw * C * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_all; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C), n = (int)((i / C) % C), j = (int)(i / ((long)C * C));
        wt[i] = w[((long)j * C + c) * C + n];
    }
}

// per row: g = dy where the forward's mask bit is set; dgamma += g xhat, dbeta += g; dz = rstd (g gamma - mean(g gamma) - xhat mean(g gamma xhat))
template <typename T, int CT>
__global__ __launch_bounds__(256) void dconv_rows_bwd_kernel(DcP p) {
    constexpr int C = CT * 16, NQ = C / 4, IT = (NQ + 15) / 16;
    __shared__ float red[4][3 * C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & 15, grp = lane >> 4;
    const long R = (long)p.B * p.T;
    const T* Z = reinterpret_cast<const T*>(p.z);
    const T* DY = reinterpret_cast<const T*>(p.dy);
    T* DZ = reinterpret_cast<T*>(p.dz);
    float ag[IT][4], ab[IT][4], az[IT][4];
#pragma unroll
    for (int i = 0; i < IT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) { ag[i][r] = 0.f; ab[i][r] = 0.f; az[i][r] = 0.f; }
    for (long row0 = (long)blockIdx.x * 16; row0 < R; row0 += (long)gridDim.x * 16) {
        const long row = row0 + wave * 4 + grp;
        const bool ok = row < R;
        const long rc = ok ? row : R - 1;
        const float mean = p.mean[rc], rstd = p.rstd[rc];
        float xh[IT][4], dh[IT][4], s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int q = sub + 16 * i;
#pragma unroll
            for (int r = 0; r < 4; ++r) { xh[i][r] = 0.f; dh[i][r] = 0.f; }
            if (q < NQ) {
                const Frag4<T> zf = frag_ld<T>(Z + rc * C + q * 4), gf = frag_ld<T>(DY + rc * C + q * 4);
                const uint32_t bits = p.mask[rc * (C / 4) + q];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = q * 4 + r;
                    const float gam = p.gamma[c], xhat = (to_f32(zf.v[r]) - mean) * rstd;
                    const float g = (ok && ((bits >> r) & 1u)) ? to_f32(gf.v[r]) : 0.f;
                    ab[i][r] += g;
                    ag[i][r] += g * xhat;
                    xh[i][r] = xhat;
                    dh[i][r] = g * gam;
                    s1 += dh[i][r];
                    s2 += dh[i][r] * xhat;
                }
            }
        }
        s1 = sum16(s1) * (1.0f / C);
        s2 = sum16(s2) * (1.0f / C);
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int q = sub + 16 * i;
            if (q < NQ) {
                f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    o[r] = rstd * (dh[i][r] - s1 - xh[i][r] * s2);
                    az[i][r] += o[r];
                }
                if (ok) frag_st<T>(DZ + row * C + q * 4, frag_from_acc<T>(o));
            }
        }
    }
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int q = sub + 16 * i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float vg = ag[i][r], vb = ab[i][r], vz = az[i][r];
            vg += __shfl_xor(vg, 16, 64); vg += __shfl_xor(vg, 32, 64);
            vb += __shfl_xor(vb, 16, 64); vb += __shfl_xor(vb, 32, 64);
            vz += __shfl_xor(vz, 16, 64); vz += __shfl_xor(vz, 32, 64);
            if (grp == 0 && q < NQ) {
                red[wave][q * 4 + r] = vg; red[wave][C + q * 4 + r] = vb; red[wave][2 * C + q * 4 + r] = vz;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * C; i += blockDim.x)
        p.part[(long)blockIdx.x * 3 * C + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
}

// dW[j][c][n] partial of (slab, tap j, column block nb): sum over the slab's samples and rows of x[t + o_j][c] dz[t][n]
template <typename T, int CT>
__global__ __launch_bounds__(256) void dconv_dw_kernel(DcP p) {
    constexpr int C = CT * 16, LD = C + DC_PAD, NBT = CT < DC_NBT ? CT : DC_NBT, NBLK = CT / NBT, MT = (CT + 3) / 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char dc_smem[];
    T* ximg = reinterpret_cast<T*>(dc_smem);
    T* gimg = ximg + DC_TRW * LD;
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15, wave = threadIdx.x >> 6;
    const int nb = blockIdx.x % NBLK, j = (blockIdx.x / NBLK) % p.fw, slab = blockIdx.x / (NBLK * p.fw);
    const int b0 = (int)((long)slab * p.B / p.slabs), b1 = (int)((long)(slab + 1) * p.B / p.slabs);
    const int oj = p.o0 + j * p.step;
    const Frag4<T> ident = identity_frag<T>(lane);
    f32x4 acc[MT][NBT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int nt = 0; nt < NBT; ++nt) acc[m][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int b = b0; b < b1; ++b) {
        const T* xs = reinterpret_cast<const T*>(p.x) + (long)b * p.T * C;
        const T* gs = reinterpret_cast<const T*>(p.dz) + (long)b * p.T * C;
        for (int t0 = 0; t0 < p.T; t0 += DC_TRW) {
            if (t0 + oj + DC_TRW <= 0 || t0 + oj >= p.T) continue;     // every shifted row is padding (block-uniform)
            __syncthreads();
            stage_rows<T>(ximg, xs, p.T, C, t0 + oj, DC_TRW);
            stage_rows<T>(gimg, gs, p.T, C, t0, DC_TRW);
            __syncthreads();
#pragma unroll
            for (int s16 = 0; s16 < DC_TRW; s16 += 16) {
                Frag4<T> xa[MT];
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const int ct = min(wave + 4 * m, CT - 1);
                    xa[m] = turn<T>(frag_ld<T>(ximg + (s16 + l15) * LD + ct * 16 + g4), ident);
                }
#pragma unroll
                for (int nt = 0; nt < NBT; ++nt) {
                    const Frag4<T> gb = turn<T>(frag_ld<T>(gimg + (s16 + l15) * LD + (nb * NBT + nt) * 16 + g4), ident);
#pragma unroll
                    for (int m = 0; m < MT; ++m) acc[m][nt] = mma16(xa[m], gb, acc[m][nt]);
                }
            }
        }
    }
    float* out = p.part + ((long)slab * p.fw + j) * C * C;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int ct = wave + 4 * m;
        if (ct >= CT) continue;
#pragma unroll
        for (int nt = 0; nt < NBT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(long)(ct * 16 + g4 + r) * C + (nb * NBT + nt) * 16 + l15] = acc[m][nt][r];
    }
}

// tanh-GELU of GREC's projector (GREC.py:14-26) and its derivative times dy
__device__ __forceinline__ float gelu_tanh_f(float x) {
    return 0.5f * x * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x)));
}
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void gelu_tanh_kernel(const T* x, const T* dy, T* out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float v = to_f32(x[i]);
        if constexpr (!BWD) out[i] = from_f32<T>(gelu_tanh_f(v));
        else {
            const float th = tanhf(0.7978845608028654f * (v + 0.044715f * v * v * v));
            const float du = 0.7978845608028654f * (1.0f + 3.0f * 0.044715f * v * v);
            out[i] = from_f32<T>(to_f32(dy[i]) * (0.5f * (1.0f + th) + 0.5f * v * (1.0f - th * th) * du));
        }
    }
}

// out[b,m,:] = relu(x[b, pos[b,m], :]) — tf.batch_gather + relu in front of GREC's head (GREC.py:88-97)
template <typename T>
__global__ __launch_bounds__(256) void gather_relu_fwd_kernel(const T* x, const int64_t* pos, T* out, int B, int Tn, int M, int C) {
    const long n = (long)B * M * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long bm = i / C;
        const int b = (int)(bm / M);
        const int64_t t = pos[bm];
        const float v = (t >= 0 && t < Tn) ? to_f32(x[((long)b * Tn + t) * C + c]) : 0.f;
        out[i] = from_f32<T>(fmaxf(v, 0.f));
    }
}
// dx[b,t,:] = sum over the m with pos[b,m] == t of dout[b,m,:] where out > 0: every element written once, in the order of m
template <typename T>
__global__ __launch_bounds__(256) void gather_relu_bwd_kernel(const T* out, const T* dout, const int64_t* pos, T* dx, int B, int Tn,
                                                              int M, int C) {
    const long n = (long)B * Tn * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long bt = i / C;
        const int b = (int)(bt / Tn), t = (int)(bt % Tn);
        float s = 0.f;
        for (int m = 0; m < M; ++m) {
            const long o = ((long)b * M + m) * C + c;
            if (pos[(long)b * M + m] == t && to_f32(out[o]) > 0.f) s += to_f32(dout[o]);
        }
        dx[i] = from_f32<T>(s);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
inline size_t dc_es(int dtype) { return dtype == EDGL_F32 ? 4 : 2; }
inline bool dc_width_ok(int C) { return C >= 32 && C <= 512 && (C & (C - 1)) == 0; }
inline int dc_nblk(int C) { const int ct = C / 16; return ct < DC_NBT ? 1 : ct / DC_NBT; }
inline int dc_rows_grid(int B, int T) { const long g = ((long)B * T + 15) / 16; return (int)(g < DC_ROWS_GRID ? g : DC_ROWS_GRID); }
// slabs of samples of the weight gradient: as many as fill the chip once with (tap, column block) workgroups
int dc_slabs(int B, int C, int fw) {
    static int cus = 0;
    if (cus <= 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
        cus = n;
    }
    const int s = cus / (fw * dc_nblk(C));
    return s < 1 ? 1 : (s > B ? B : s);
}

int dc_check(const char* who, int B, int T, int C, int fw, int d, int dtype) {
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "%s: bad dtype %d", who, dtype);
    EDGL_REQUIRE(B > 0 && T > 0 && T <= 1024, EDGL_ERR_SHAPE, "%s: bad shape B=%d T=%d (1 <= T <= 1024)", who, B, T);
    EDGL_REQUIRE(dc_width_ok(C), EDGL_ERR_SHAPE, "%s: C=%d unsupported (a power of two in [32, 512])", who, C);
    EDGL_REQUIRE(fw >= 1 && fw <= 5 && d >= 1, EDGL_ERR_SHAPE, "%s: filter width %d / dilation %d unsupported (1 <= fw <= 5, d >= 1)", who, fw, d);
    const long reach = (long)(fw - 1) * d, most = edgl_dconv_max_reach(C, dtype);
    EDGL_REQUIRE(reach <= most, EDGL_ERR_SHAPE, "%s: (fw - 1) d = %ld rows of halo, the LDS image of a %d-row block holds %ld at C=%d", who,
                 reach, DC_TR, most, C);
    EDGL_REQUIRE((double)B * ((T + DC_TR - 1) / DC_TR) < 2147483647.0, EDGL_ERR_SHAPE, "%s: too many workgroups", who);
    return EDGL_OK;
}

// o_j = o0 + j step of the forward (mirrored: of the input gradient)
void dc_geom(DcP& p, int fw, int d, int causal, bool mirrored) {
    const int reach = (fw - 1) * d, lpad = causal ? reach : reach / 2;
    p.fw = fw;
    p.o0 = mirrored ? lpad : -lpad;
    p.step = mirrored ? -d : d;
    p.omin = mirrored ? lpad - reach : -lpad;
    p.rows = DC_TR + reach;
}

template <typename T, int CT>
int dc_launch_one(const DcP& p, int which, hipStream_t st) {
    constexpr int C = CT * 16;
    if (which == 0 || which == 1) {
        const size_t smem = (size_t)p.rows * (C + DC_PAD) * sizeof(T);
        const unsigned grid = (unsigned)((long)p.B * p.NB);
        if (which == 0) {
            EDGL_LDS_LIMIT((dconv_kernel<T, CT, true>), smem, "edgl_dconv_ln_fwd");
            hipLaunchKernelGGL((dconv_kernel<T, CT, true>), dim3(grid), dim3(256), smem, st, p);
        } else {
            EDGL_LDS_LIMIT((dconv_kernel<T, CT, false>), smem, "edgl_dconv_ln_bwd");
            hipLaunchKernelGGL((dconv_kernel<T, CT, false>), dim3(grid), dim3(256), smem, st, p);
        }
    } else if (which == 2) {
        hipLaunchKernelGGL((dconv_rows_bwd_kernel<T, CT>), dim3(dc_rows_grid(p.B, p.T)), dim3(256), 0, st, p);
    } else {
        const size_t smem = (size_t)2 * DC_TRW * (C + DC_PAD) * sizeof(T);
        EDGL_LDS_LIMIT((dconv_dw_kernel<T, CT>), smem, "edgl_dconv_ln_bwd");
        hipLaunchKernelGGL((dconv_dw_kernel<T, CT>), dim3((unsigned)(p.slabs * p.fw * dc_nblk(C))), dim3(256), smem, st, p);
    }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
// which = 0: forward, 1: input gradient, 2: row-wise backward, 3: weight gradient
template <typename T>
int dc_launch(const DcP& p, int C, int which, hipStream_t st) {
    switch (C) {
        case 32: return dc_launch_one<T, 2>(p, which, st);
        case 64: return dc_launch_one<T, 4>(p, which, st);
        case 128: return dc_launch_one<T, 8>(p, which, st);
        case 256: return dc_launch_one<T, 16>(p, which, st);
        case 512: return dc_launch_one<T, 32>(p, which, st);
    }
    edgl_set_error("edgl_dconv: C=%d not supported", C);
    return EDGL_ERR_SHAPE;
}
inline int dc_go(const DcP& p, int C, int which, int dtype, hipStream_t st) {
    return dtype == EDGL_F32 ? dc_launch<float>(p, C, which, st) : dc_launch<bf16>(p, C, which, st);
}

}  // namespace

extern "C" int edgl_dconv_max_reach(int C, int dtype) {
    if (!dc_width_ok(C) || (dtype != EDGL_F32 && dtype != EDGL_BF16)) return -1;
    const long rows = (long)(DC_LDS / ((size_t)(C + DC_PAD) * dc_es(dtype))) - DC_TR;
    return (int)(rows < 0 ? -1 : rows);
}

extern "C" long edgl_dconv_bwd_workspace(int B, int T, int C, int fw) {
    if (B <= 0 || T <= 0 || !dc_width_ok(C) || fw < 1 || fw > 5) return -1;
    return (long)dc_slabs(B, C, fw) * fw * C * C + (long)dc_rows_grid(B, T) * 3 * C;
}

extern "C" int edgl_dconv_ln_fwd(const void* x, const void* w, const float* bias, const float* gamma, const float* beta, const void* r,
                                 int B, int T, int C, int fw, int d, int causal, void* wt, void* y, void* z, float* stats, void* mask,
                                 int dtype, void* stream) {
    EDGL_REQUIRE(x && w && bias && gamma && beta && wt && y, EDGL_ERR_NULL, "edgl_dconv_ln_fwd: null pointer");
    EDGL_REQUIRE((z == nullptr) == (stats == nullptr) && (z == nullptr) == (mask == nullptr), EDGL_ERR_NULL,
                 "edgl_dconv_ln_fwd: z, stats and mask are saved together");
    if (int rc = dc_check("edgl_dconv_ln_fwd", B, T, C, fw, d, dtype)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int pg = grid_for((long)fw * C * C);
    if (dtype == EDGL_F32) hipLaunchKernelGGL(dconv_pack_w_kernel<float>, dim3(pg), dim3(256), 0, st, (const float*)w, (float*)wt, fw, C);
    else hipLaunchKernelGGL(dconv_pack_w_kernel<bf16>, dim3(pg), dim3(256), 0, st, (const bf16*)w, (bf16*)wt, fw, C);
    EDGL_LAUNCH_CHECK();
    DcP p{};
    p.x = x; p.w = wt; p.r = r; p.bias = bias; p.gamma = gamma; p.beta = beta; p.y = y; p.zout = z;
    p.mean = stats; p.rstd = stats ? stats + (long)B * T : nullptr; p.mask = reinterpret_cast<uint8_t*>(mask);
    p.B = B; p.T = T; p.NB = (T + DC_TR - 1) / DC_TR;
    dc_geom(p, fw, d, causal, false);
    return dc_go(p, C, 0, dtype, st);
}

extern "C" int edgl_dconv_ln_bwd(const void* x, const void* w, const float* gamma, const float* beta, const void* z, const float* stats,
                                 const void* mask, const void* dy, int B, int T, int C, int fw, int d, int causal, void* dz, void* dx, float* dw,
                                 float* dvec, float* workspace, int dtype, void* stream) {
    EDGL_REQUIRE(x && w && gamma && beta && z && stats && mask && dy && dz && dx && dw && dvec && workspace, EDGL_ERR_NULL,
                 "edgl_dconv_ln_bwd: null pointer");
    if (int rc = dc_check("edgl_dconv_ln_bwd", B, T, C, fw, d, dtype)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int slabs = dc_slabs(B, C, fw), rg = dc_rows_grid(B, T);
    float* part_w = workspace;
    float* part_v = workspace + (long)slabs * fw * C * C;
    DcP p{};
    p.B = B; p.T = T; p.NB = (T + DC_TR - 1) / DC_TR; p.slabs = slabs;
    p.gamma = gamma; p.beta = beta; p.z = z; p.dy = dy; p.dz = dz;
    p.mean = const_cast<float*>(stats); p.rstd = p.mean + (long)B * T;
    p.mask = reinterpret_cast<uint8_t*>(const_cast<void*>(mask));
    p.part = part_v;
    dc_geom(p, fw, d, causal, false);
    if (int rc = dc_go(p, C, 2, dtype, st)) return rc;                       // dy -> dz, partial rows dgamma | dbeta | dbias
    if (int rc = edgl_reduce_rows(part_v, rg, 3 * C, 3L * C, dvec, 0, st)) return rc;
    p.x = x; p.part = part_w;
    if (int rc = dc_go(p, C, 3, dtype, st)) return rc;                       // x, dz -> partial dW
    if (int rc = edgl_reduce_rows(part_w, slabs, fw * C * C, (long)fw * C * C, dw, 0, st)) return rc;
    p.x = dz; p.w = w; p.y = dx;
    dc_geom(p, fw, d, causal, true);
    return dc_go(p, C, 1, dtype, st);                                         // dz, W -> dx
}

extern "C" int edgl_gelu_tanh_fwd(const void* x, void* y, long n, int dtype, void* stream) {
    EDGL_REQUIRE(x && y, EDGL_ERR_NULL, "edgl_gelu_tanh_fwd: null pointer");
    EDGL_REQUIRE(n > 0 && (dtype == EDGL_F32 || dtype == EDGL_BF16), EDGL_ERR_SHAPE, "edgl_gelu_tanh_fwd: n=%ld dtype=%d", n, dtype);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == EDGL_F32) hipLaunchKernelGGL((gelu_tanh_kernel<float, false>), dim3(grid_for(n)), dim3(256), 0, st, (const float*)x, (const float*)nullptr, (float*)y, n);
    else hipLaunchKernelGGL((gelu_tanh_kernel<bf16, false>), dim3(grid_for(n)), dim3(256), 0, st, (const bf16*)x, (const bf16*)nullptr, (bf16*)y, n);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_gelu_tanh_bwd(const void* x, const void* dy, void* dx, long n, int dtype, void* stream) {
    EDGL_REQUIRE(x && dy && dx, EDGL_ERR_NULL, "edgl_gelu_tanh_bwd: null pointer");
    EDGL_REQUIRE(n > 0 && (dtype == EDGL_F32 || dtype == EDGL_BF16), EDGL_ERR_SHAPE, "edgl_gelu_tanh_bwd: n=%ld dtype=%d", n, dtype);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == EDGL_F32) hipLaunchKernelGGL((gelu_tanh_kernel<float, true>), dim3(grid_for(n)), dim3(256), 0, st, (const float*)x, (const float*)dy, (float*)dx, n);
    else hipLaunchKernelGGL((gelu_tanh_kernel<bf16, true>), dim3(grid_for(n)), dim3(256), 0, st, (const bf16*)x, (const bf16*)dy, (bf16*)dx, n);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_gather_relu_fwd(const void* x, const int64_t* pos, void* out, int B, int T, int M, int C, int dtype, void* stream) {
    EDGL_REQUIRE(x && pos && out, EDGL_ERR_NULL, "edgl_gather_relu_fwd: null pointer");
    EDGL_REQUIRE(B > 0 && T > 0 && M > 0 && C > 0 && (dtype == EDGL_F32 || dtype == EDGL_BF16), EDGL_ERR_SHAPE,
                 "edgl_gather_relu_fwd: bad shape B=%d T=%d M=%d C=%d dtype=%d", B, T, M, C, dtype);
    hipStream_t st = (hipStream_t)stream;
    const int g = grid_for((long)B * M * C);
    if (dtype == EDGL_F32) hipLaunchKernelGGL(gather_relu_fwd_kernel<float>, dim3(g), dim3(256), 0, st, (const float*)x, pos, (float*)out, B, T, M, C);
    else hipLaunchKernelGGL(gather_relu_fwd_kernel<bf16>, dim3(g), dim3(256), 0, st, (const bf16*)x, pos, (bf16*)out, B, T, M, C);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_gather_relu_bwd(const void* out, const void* dout, const int64_t* pos, void* dx, int B, int T, int M, int C, int dtype,
                                    void* stream) {
    EDGL_REQUIRE(out && dout && pos && dx, EDGL_ERR_NULL, "edgl_gather_relu_bwd: null pointer");
    EDGL_REQUIRE(B > 0 && T > 0 && M > 0 && C > 0 && (dtype == EDGL_F32 || dtype == EDGL_BF16), EDGL_ERR_SHAPE,
                 "edgl_gather_relu_bwd: bad shape B=%d T=%d M=%d C=%d dtype=%d", B, T, M, C, dtype);
    hipStream_t st = (hipStream_t)stream;
    const int g = grid_for((long)B * T * C);
    if (dtype == EDGL_F32) hipLaunchKernelGGL(gather_relu_bwd_kernel<float>, dim3(g), dim3(256), 0, st, (const float*)out, (const float*)dout, pos, (float*)dx, B, T, M, C);
    else hipLaunchKernelGGL(gather_relu_bwd_kernel<bf16>, dim3(g), dim3(256), 0, st, (const bf16*)out, (const bf16*)dout, pos, (bf16*)dx, B, T, M, C);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
