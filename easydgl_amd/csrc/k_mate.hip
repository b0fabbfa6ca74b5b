// Multi-aspect time encoder of TimelyREC (TimelyREC.py:57-77,108-135, sequential.py:220-237): calendar slots, the
// per-granularity slot attention and the gated combination in one op.  Granularities g = month, day, weekday, hour with ranges
// M_g = 12, 31, 7, 24, tables E_g [M_g, C] and windows W_g; f = the position's calendar index (-1: the zero row):
//   cs[s][w] = sum_{s' <= s} E[(f[s'] + w) mod M] + E[(f[s'] - w) mod M]        w = 1..W   (running sum over the SEQUENCE, padding too)
//   slot_0 = e = E[f],  slot_w = (e + cs_w) / (2w + 1);   Q = e * u_g,  K_w = slot_w * u_g
//   p = softmax_w(Q . K_w / sqrt(C)),  period_g = sum_w p_w K_w,  a_g = sigmoid(pq . period_g),  R = sum_g a_g period_g
//
// edgl_mate_fwd: one workgroup per sample, wave g owns granularity g for all T positions.  A lane owns the channels lane + 64 i; the
// running sums live in LDS ([W_g][C] f32 per wave, owner-accessed), the per-position dot products over all C are wave reductions, the
// softmax over w = 0..W_g sits on lanes 0..W_g.  The four gated periods meet in an LDS exchange [4][C] and are summed in the order of
// g: two barriers per position.  Saved: the slot probabilities and the four gates, sum(W_g + 1) + 4 floats per position.
//
// edgl_mate_bwd, launch 1 (same split: everything that needs a dot product over ALL channels): recomputes the slots and periods,
// d a_g = dR . period_g, dz_g, d_pq = sum_g dz_g period_g (through the exchange), dp_w = dperiod . K_w and the softmax backward
// dl_w; leaves dl_w and dz_g as `coef`, the same layout as `saved`.  Launch 2 (everything channel-separable): a workgroup owns 64
// channels and a fixed list of samples b = blockIdx.x, + gridDim.x, ...; wave g, one channel per lane.  Per sample it sweeps forward
// to the last running sum, then walks the positions backwards: it steps the running sum back, carries the reverse running sum
// D_w of d cs_w and adds D_w into the two window rows and d e into row f of the wave's own [M_g][64] LDS accumulator — one owner
// per element, no atomics.  d_u is written here.  The accumulators go out as one slab per workgroup and a last kernel adds the slabs
// in ascending order: the same bits in every call.
#include "edgl_common.h"

namespace {

constexpr int MATE_G = 4;
constexpr int MATE_ROWS = 74;            // 12 + 31 + 7 + 24
constexpr int MATE_MAXW = 17;            // window_ratio <= 0.5: max(int(31 * 0.5 + 0.5), 1) + 1
constexpr int MATE_MAXT = 128;
constexpr int MATE_CPL = 8;              // channels per lane at C = 512
constexpr int MATE_SLABS = 64;           // sample lists of launch 2
constexpr int MATE_CS = 64;              // channels per workgroup of launch 2

__host__ __device__ inline int mate_m(int g) { return g == 0 ? 12 : g == 1 ? 31 : g == 2 ? 7 : 24; }
__host__ __device__ inline int mate_row0(int g) { return g == 0 ? 0 : g == 1 ? 12 : g == 2 ? 43 : 50; }

struct MateP {
    const int64_t* idx;            // [4][B][T] calendar indices (month - 1, day - 1, weekday, hour)
    const void* tab[MATE_G];       // E_g [M_g, C]
    const void* u;                 // [B,T,4C]
    const void* pq;                // [B,T,C]
    const void* dR;                // [B,T,C] (backward)
    int B, T, C;
    int W[MATE_G], woff[MATE_G], soff[MATE_G], WT, NSV;
    void* R;                       // forward: R; launch 1 of the backward: d_pq
    float* saved;                  // p_w and gates
    float* coef;                   // dl_w and dz_g
    void* d_u;
    float* slabs;                  // [gridDim.x][74][C]
};

__device__ __forceinline__ int mate_mod(long f, int M) { const int r = (int)(f % M); return r < 0 ? r + M : r; }

// BWD = false: R and `saved`;  BWD = true: d_pq and `coef` from `saved` and dR
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void mate_pos_kernel(MateP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mate_smem_raw[];
    const int C = p.C, Tn = p.T, b = blockIdx.x;
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int M = mate_m(g), W = p.W[g];
    float* cs = reinterpret_cast<float*>(mate_smem_raw) + (size_t)p.woff[g] * C;
    float* xch = reinterpret_cast<float*>(mate_smem_raw) + (size_t)p.WT * C;
    const T* tab = reinterpret_cast<const T*>(p.tab[g]);
    const T* u = reinterpret_cast<const T*>(p.u);
    const T* pq = reinterpret_cast<const T*>(p.pq);
    T* out = reinterpret_cast<T*>(p.R);
    const float rsC = 1.0f / sqrtf((float)C);
    for (int i = lane; i < W * C; i += 64) cs[i] = 0.f;
    for (int s = 0; s < Tn; ++s) {
        const long pos = (long)b * Tn + s;
        const long f = p.idx[((long)g * p.B + b) * Tn + s];
        const bool valid = f >= 0 && f < M;
        const int fm = mate_mod(f, M);
        float ev[MATE_CPL], uv[MATE_CPL], per[MATE_CPL];
#pragma unroll
        for (int i = 0; i < MATE_CPL; ++i) {
            const int c = lane + 64 * i;
            ev[i] = (valid && c < C) ? to_f32(tab[(long)f * C + c]) : 0.f;
            uv[i] = c < C ? to_f32(u[pos * 4 * C + (long)g * C + c]) : 0.f;
            per[i] = 0.f;
        }
        // the running sums of this position, and (forward) the logits: lane w keeps logit w
        float lg = -INFINITY;
        for (int w = 0; w <= W; ++w) {
            const float inv = 1.0f / (float)(2 * w + 1);
            const T* t1 = tab + (long)mate_mod(fm + w, M) * C;
            const T* t2 = tab + (long)mate_mod(fm - w, M) * C;
            float part = 0.f;
#pragma unroll
            for (int i = 0; i < MATE_CPL; ++i) {
                const int c = lane + 64 * i;
                if (c < C) {
                    float slot = ev[i];
                    if (w > 0) {
                        const float v = cs[(w - 1) * C + c] + (to_f32(t1[c]) + to_f32(t2[c]));
                        cs[(w - 1) * C + c] = v;
                        slot = (ev[i] + v) * inv;
                    }
                    part = fmaf(ev[i] * uv[i], slot * uv[i], part);
                }
            }
            if (!BWD) {
                part = wave_sum(part) * rsC;
                if (lane == w) lg = part;
            }
        }
        float pw;
        if (!BWD) {
            const float mx = wave_max(lg);
            const float ex = lane <= W ? expf(lg - mx) : 0.f;
            pw = ex / wave_sum(ex);
            if (p.saved && lane <= W) p.saved[pos * p.NSV + p.soff[g] + lane] = pw;
        } else {
            pw = lane <= W ? p.saved[pos * p.NSV + p.soff[g] + lane] : 0.f;
        }
        // period = u * sum_w p_w slot_w
        for (int w = 0; w <= W; ++w) {
            const float inv = 1.0f / (float)(2 * w + 1), pv = __shfl(pw, w, 64);
#pragma unroll
            for (int i = 0; i < MATE_CPL; ++i) {
                const int c = lane + 64 * i;
                if (c < C) per[i] = fmaf(pv, w == 0 ? ev[i] : (ev[i] + cs[(w - 1) * C + c]) * inv, per[i]);
            }
        }
        float z = 0.f;
#pragma unroll
        for (int i = 0; i < MATE_CPL; ++i) {
            const int c = lane + 64 * i;
            per[i] *= uv[i];
            if (c < C) z = fmaf(to_f32((BWD ? reinterpret_cast<const T*>(p.dR) : pq)[pos * C + c]), per[i], z);
        }
        z = wave_sum(z);
        if (!BWD) {
            const float a = 1.0f / (1.0f + expf(-z));
            if (p.saved && lane == 0) p.saved[pos * p.NSV + p.NSV - MATE_G + g] = a;
#pragma unroll
            for (int i = 0; i < MATE_CPL; ++i) {
                const int c = lane + 64 * i;
                if (c < C) xch[g * C + c] = a * per[i];
            }
        } else {
            // z = d a_g = dR . period
            const float a = p.saved[pos * p.NSV + p.NSV - MATE_G + g];
            const float dz = z * a * (1.0f - a);
            float dper[MATE_CPL];
#pragma unroll
            for (int i = 0; i < MATE_CPL; ++i) {
                const int c = lane + 64 * i;
                dper[i] = 0.f;
                if (c < C) {
                    xch[g * C + c] = dz * per[i];
                    dper[i] = (a * to_f32(reinterpret_cast<const T*>(p.dR)[pos * C + c]) + dz * to_f32(pq[pos * C + c])) * uv[i];
                }
            }
            // dp_w = dperiod . K_w on lane w, then the softmax backward
            float dp = 0.f;
            for (int w = 0; w <= W; ++w) {
                const float inv = 1.0f / (float)(2 * w + 1);
                float part = 0.f;
#pragma unroll
                for (int i = 0; i < MATE_CPL; ++i) {
                    const int c = lane + 64 * i;
                    if (c < C) part = fmaf(dper[i], w == 0 ? ev[i] : (ev[i] + cs[(w - 1) * C + c]) * inv, part);
                }
                part = wave_sum(part);
                if (lane == w) dp = part;
            }
            const float mean = wave_sum(pw * dp);
            if (lane <= W) p.coef[pos * p.NSV + p.soff[g] + lane] = pw * (dp - mean);
            if (lane == 0) p.coef[pos * p.NSV + p.NSV - MATE_G + g] = dz;
        }
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += 256)
            out[pos * C + c] = from_f32<T>(((xch[c] + xch[C + c]) + xch[2 * C + c]) + xch[3 * C + c]);
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(256) void mate_acc_kernel(MateP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mate_smem_raw[];
    const int C = p.C, Tn = p.T;
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int M = mate_m(g), W = p.W[g], row0 = mate_row0(g);
    const int c = blockIdx.y * MATE_CS + lane;
    const bool on = c < C;
    // per wave: cs [W][64], D [W][64], dE [M][64]
    float* base = reinterpret_cast<float*>(mate_smem_raw) + (size_t)(2 * p.woff[g] + row0) * MATE_CS;
    float* cs = base + lane;
    float* D = base + (size_t)W * MATE_CS + lane;
    float* dE = base + (size_t)2 * W * MATE_CS + lane;
    const T* tab = reinterpret_cast<const T*>(p.tab[g]);
    const T* u = reinterpret_cast<const T*>(p.u);
    const T* pq = reinterpret_cast<const T*>(p.pq);
    const T* dR = reinterpret_cast<const T*>(p.dR);
    T* d_u = reinterpret_cast<T*>(p.d_u);
    const float rsC = 1.0f / sqrtf((float)C);
    for (int m = 0; m < M; ++m) dE[m * MATE_CS] = 0.f;
    for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
        const int64_t* idx = p.idx + ((long)g * p.B + b) * Tn;
        for (int w = 0; w < W; ++w) { cs[w * MATE_CS] = 0.f; D[w * MATE_CS] = 0.f; }
        if (on)
            for (int s = 0; s < Tn; ++s) {
                const int fm = mate_mod(idx[s], M);
                for (int w = 1; w <= W; ++w)
                    cs[(w - 1) * MATE_CS] += to_f32(tab[(long)mate_mod(fm + w, M) * C + c]) + to_f32(tab[(long)mate_mod(fm - w, M) * C + c]);
            }
        for (int s = Tn - 1; s >= 0 && on; --s) {
            const long pos = (long)b * Tn + s;
            const long f = idx[s];
            const bool valid = f >= 0 && f < M;
            const int fm = mate_mod(f, M);
            const float ev = valid ? to_f32(tab[(long)f * C + c]) : 0.f;
            const float uv = to_f32(u[pos * 4 * C + (long)g * C + c]);
            const float* sv = p.saved + pos * p.NSV;
            const float* cf = p.coef + pos * p.NSV;
            const float a = sv[p.NSV - MATE_G + g], dz = cf[p.NSV - MATE_G + g];
            const float dper = a * to_f32(dR[pos * C + c]) + dz * to_f32(pq[pos * C + c]);
            const float qv = ev * uv;
            float dQ = 0.f, du = 0.f, de = 0.f;
            for (int w = 0; w <= W; ++w) {
                const float pw = sv[p.soff[g] + w], dl = cf[p.soff[g] + w] * rsC;
                const float inv = 1.0f / (float)(2 * w + 1);
                const float slot = w == 0 ? ev : (ev + cs[(w - 1) * MATE_CS]) * inv;
                const float dK = fmaf(pw, dper, dl * qv);
                dQ = fmaf(dl, slot * uv, dQ);
                du = fmaf(dK, slot, du);
                const float dslot = dK * uv;
                if (w == 0) {
                    de += dslot;
                } else {
                    const int r1 = mate_mod(fm + w, M), r2 = mate_mod(fm - w, M);
                    const float d = dslot * inv;
                    de += d;
                    const float acc = D[(w - 1) * MATE_CS] + d;       // reverse running sum of d cs_w: this position included
                    D[(w - 1) * MATE_CS] = acc;
                    dE[r1 * MATE_CS] += acc;
                    dE[r2 * MATE_CS] += acc;                           // (r1 == r2 where the offsets alias: the row is summed twice)
                    cs[(w - 1) * MATE_CS] -= to_f32(tab[(long)r1 * C + c]) + to_f32(tab[(long)r2 * C + c]);     // back to position s - 1
                }
            }
            de = fmaf(dQ, uv, de);
            du = fmaf(dQ, ev, du);
            if (valid) dE[(int)f * MATE_CS] += de;
            d_u[pos * 4 * C + (long)g * C + c] = from_f32<T>(du);
        }
    }
    if (on) {
        float* slab = p.slabs + ((long)blockIdx.x * MATE_ROWS + row0) * C + c;
        for (int m = 0; m < M; ++m) slab[(long)m * C] = dE[m * MATE_CS];
    }
}

__global__ __launch_bounds__(256) void mate_slab_sum_kernel(const float* slabs, int P, long N, float* out) {
    const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float s = 0.f;
    for (int q = 0; q < P; ++q) s += slabs[(long)q * N + n];
    out[n] = s;
}

int mate_fill(const char* who, MateP& p, int B, int T, int C, int w0, int w1, int w2, int w3, int dtype) {
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "%s: bad dtype %d", who, dtype);
    EDGL_REQUIRE(B > 0 && T >= 1 && T <= MATE_MAXT && C >= 32 && C <= 512 && (C & (C - 1)) == 0, EDGL_ERR_SHAPE,
                 "%s: bad shape B=%d T=%d C=%d (1 <= T <= %d, C a power of two in [32, 512])", who, B, T, C, MATE_MAXT);
    const int W[MATE_G] = {w0, w1, w2, w3};
    int wo = 0, so = 0;
    for (int g = 0; g < MATE_G; ++g) {
        // window_ratio in (0, 0.5]: 2 <= W <= M / 2 + 2 (the formula's largest value), at most 17
        EDGL_REQUIRE(W[g] >= 2 && W[g] <= MATE_MAXW && W[g] <= mate_m(g) / 2 + 2, EDGL_ERR_SHAPE,
                     "%s: window %d of granularity %d unsupported (window_ratio in (0, 0.5])", who, W[g], g);
        p.W[g] = W[g]; p.woff[g] = wo; p.soff[g] = so;
        wo += W[g]; so += W[g] + 1;
    }
    p.WT = wo; p.NSV = so + MATE_G;
    p.B = B; p.T = T; p.C = C;
    return EDGL_OK;
}

template <typename T, bool BWD>
int mate_launch_pos(const MateP& p, hipStream_t st) {
    const size_t smem = (size_t)(p.WT + MATE_G) * p.C * sizeof(float);
    EDGL_LDS_LIMIT((mate_pos_kernel<T, BWD>), smem, BWD ? "edgl_mate_bwd" : "edgl_mate_fwd");
    hipLaunchKernelGGL((mate_pos_kernel<T, BWD>), dim3(p.B), dim3(256), smem, st, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

inline int mate_slab_count(int B) { return B < MATE_SLABS ? B : MATE_SLABS; }

}  // namespace

extern "C" int edgl_mate_saved_floats(int w_month, int w_day, int w_weekday, int w_hour) {
    MateP p{};
    if (mate_fill("edgl_mate_saved_floats", p, 1, 1, 32, w_month, w_day, w_weekday, w_hour, EDGL_F32) != EDGL_OK) return -1;
    return p.NSV;
}

extern "C" int edgl_mate_fwd(const int64_t* idx, const void* month_tab, const void* day_tab, const void* weekday_tab, const void* hour_tab,
                             const void* u, const void* pq, int B, int T, int C, int w_month, int w_day, int w_weekday, int w_hour,
                             void* R, float* saved, int dtype, void* stream) {
    EDGL_REQUIRE(idx && month_tab && day_tab && weekday_tab && hour_tab && u && pq && R, EDGL_ERR_NULL, "edgl_mate_fwd: null pointer");
    MateP p{};
    const int rc = mate_fill("edgl_mate_fwd", p, B, T, C, w_month, w_day, w_weekday, w_hour, dtype);
    if (rc != EDGL_OK) return rc;
    p.idx = idx; p.tab[0] = month_tab; p.tab[1] = day_tab; p.tab[2] = weekday_tab; p.tab[3] = hour_tab;
    p.u = u; p.pq = pq; p.R = R; p.saved = saved;
    return dtype == EDGL_F32 ? mate_launch_pos<float, false>(p, (hipStream_t)stream) : mate_launch_pos<bf16, false>(p, (hipStream_t)stream);
}

extern "C" long edgl_mate_bwd_workspace(int B, int T, int C, int w_month, int w_day, int w_weekday, int w_hour) {
    MateP p{};
    if (mate_fill("edgl_mate_bwd_workspace", p, B, T, C, w_month, w_day, w_weekday, w_hour, EDGL_F32) != EDGL_OK) return -1;
    return (long)B * T * p.NSV + (long)mate_slab_count(B) * MATE_ROWS * C;
}

extern "C" int edgl_mate_bwd(const int64_t* idx, const void* month_tab, const void* day_tab, const void* weekday_tab, const void* hour_tab,
                             const void* u, const void* pq, const float* saved, const void* d_R, int B, int T, int C, int w_month,
                             int w_day, int w_weekday, int w_hour, void* d_u, void* d_pq, float* d_tables, float* workspace, int dtype,
                             void* stream) {
    EDGL_REQUIRE(idx && month_tab && day_tab && weekday_tab && hour_tab && u && pq && saved && d_R && d_u && d_pq && d_tables && workspace,
                 EDGL_ERR_NULL, "edgl_mate_bwd: null pointer");
    MateP p{};
    const int rc = mate_fill("edgl_mate_bwd", p, B, T, C, w_month, w_day, w_weekday, w_hour, dtype);
    if (rc != EDGL_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    p.idx = idx; p.tab[0] = month_tab; p.tab[1] = day_tab; p.tab[2] = weekday_tab; p.tab[3] = hour_tab;
    p.u = u; p.pq = pq; p.dR = d_R; p.saved = const_cast<float*>(saved);
    p.coef = workspace; p.slabs = workspace + (long)B * T * p.NSV;
    p.R = d_pq; p.d_u = d_u;
    const int r2 = dtype == EDGL_F32 ? mate_launch_pos<float, true>(p, st) : mate_launch_pos<bf16, true>(p, st);
    if (r2 != EDGL_OK) return r2;
    const int P = mate_slab_count(B);
    const dim3 grid(P, (C + MATE_CS - 1) / MATE_CS);
    const size_t smem = (size_t)(2 * p.WT + MATE_ROWS) * MATE_CS * sizeof(float);       // <= 40448 bytes
    if (dtype == EDGL_F32) hipLaunchKernelGGL((mate_acc_kernel<float>), grid, dim3(256), smem, st, p);
    else hipLaunchKernelGGL((mate_acc_kernel<bf16>), grid, dim3(256), smem, st, p);
    const long N = (long)MATE_ROWS * C;
    hipLaunchKernelGGL(mate_slab_sum_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, p.slabs, P, N, d_tables);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
