// K11 (time feature map): TimeFunctionCoding.code (coding.py:104-122) folded into the operands of TGAT's attention
// (k_tattn.hip), and the row mask that goes with it.
//
// The reference scores a (query q, key k) pair with
//     S[q,k] = sum_d Q[q,d] * ( K[k,d] + Pos[k,d] + cos(dt[q,k]*w_d + phi_d) ) / sqrt(dh),   dt[q,k] = max(t[q+1] - t[k], 0)
// and materialises the cosine as a [B,T,T,C] tensor.  For every pair the causal + key masks keep (k <= q, key not padding)
// the clamp is inactive when timestamps do not decrease, and cos(a-b) = cos a cos b + sin a sin b turns the time term
// into two more inner products:
//     q~[q] = [ Q | Q*cos(a_q w + phi) | Q*sin(a_q w + phi) ],  k~[k] = [ K + Pos | cos(b_k w) | sin(b_k w) ],  S = q~ . k~^T
// with a_q = t[q+1] - base, b_k = t[k] - base (base = the sequence's last timestamp, so the arguments stay as small as the
// reference's).  T*C transcendentals per sequence instead of T*T*C, and the T*T*C contraction runs on the matrix cores.
// timefn_fwd counts sequences whose timestamps decrease at an unmasked position (the host checks the counter).
#include <algorithm>

#include "tattn_common.h"   // frag_st

namespace {

// ---- time feature map (coding.py:104-122 through the angle-difference identity) ------------------------------------------
struct TfP {
    const void *q, *k; int ldq, ldk;
    const float *pos, *ts, *omega, *phi;
    const int64_t* ids;
    int B, T, C, H;
    float time_scale;
    void *qx, *kx;
    int* viol;
    const void *d_qx, *d_kx;
    void *d_q, *d_k; int ld_dq, ld_dk;
    float* part;   // [blocks][2C]
};

template <typename T>
__global__ __launch_bounds__(256) void timefn_fwd_kernel(TfP p) {
    const int cpr = p.C >> 2, dh = p.C / p.H;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long row = gid / cpr;
    if (row >= (long)p.B * p.T) return;
    const int c0 = (int)(gid % cpr) * 4, t = (int)(row % p.T);
    const long b = row / p.T;
    const float* tr = p.ts + b * (p.T + 1);
    const float base = tr[p.T] / p.time_scale;                       // TGAT.py:46 (seqs_ts = seqs_t / time_scale)
    const float xt = tr[t] / p.time_scale, xn = tr[t + 1] / p.time_scale;
    const float a = xn - base, bk = xt - base;
    if (c0 == 0 && xn < xt && p.ids[row] != 0) atomicAdd(p.viol, 1);  // max(.,0) of TGAT.py:54 would be active here
    const Frag4<T> qv = frag_ld<T>(reinterpret_cast<const T*>(p.q) + row * p.ldq + c0);
    const Frag4<T> kv = frag_ld<T>(reinterpret_cast<const T*>(p.k) + row * p.ldk + c0);
    const float4 w = *reinterpret_cast<const float4*>(p.omega + c0), ph = *reinterpret_cast<const float4*>(p.phi + c0);
    const float4 pp = *reinterpret_cast<const float4*>(p.pos + (long)t * p.C + c0);
    const float ww[4] = {w.x, w.y, w.z, w.w}, pv[4] = {ph.x, ph.y, ph.z, ph.w}, ps[4] = {pp.x, pp.y, pp.z, pp.w};
    Frag4<T> q0, qc, qs, k0, kc, ks;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float sq, cq, sk, ck;
        sincosf(a * ww[i] + pv[i], &sq, &cq);
        sincosf(bk * ww[i], &sk, &ck);
        const float qf = to_f32(qv.v[i]);
        q0.v[i] = qv.v[i];
        qc.v[i] = from_f32<T>(qf * cq);
        qs.v[i] = from_f32<T>(qf * sq);
        k0.v[i] = from_f32<T>(to_f32(kv.v[i]) + ps[i]);              // temporal.py:143,148: Q . (K + pos)^T
        kc.v[i] = from_f32<T>(ck);
        ks.v[i] = from_f32<T>(sk);
    }
    const int head = c0 / dh, u = c0 % dh;
    T* qo = reinterpret_cast<T*>(p.qx) + (row * p.H + head) * 3 * dh + u;
    T* ko = reinterpret_cast<T*>(p.kx) + (row * p.H + head) * 3 * dh + u;
    frag_st<T>(qo, q0); frag_st<T>(qo + dh, qc); frag_st<T>(qo + 2 * dh, qs);
    frag_st<T>(ko, k0); frag_st<T>(ko + dh, kc); frag_st<T>(ko + 2 * dh, ks);
}

// dQ = dq0 + dqc*cos + dqs*sin; dK = dk0 (also the position-table gradient, summed over the batch by the caller);
// dtheta = Q*(dqs*cos - dqc*sin) -> dphi += dtheta, domega += dtheta * a;  dpsi = dks*cos_k - dkc*sin_k -> domega += dpsi * b
template <typename T>
__global__ __launch_bounds__(256) void timefn_bwd_kernel(TfP p) {
    __shared__ float red[256][8];
    const int cpr = p.C >> 2, dh = p.C / p.H, rpb = 256 / cpr;     // rows per pass of a block
    const int cv = threadIdx.x % cpr, rl = threadIdx.x / cpr, c0 = cv * 4;
    const float4 w = *reinterpret_cast<const float4*>(p.omega + c0), ph = *reinterpret_cast<const float4*>(p.phi + c0);
    const float ww[4] = {w.x, w.y, w.z, w.w}, pv[4] = {ph.x, ph.y, ph.z, ph.w};
    float dw[4] = {0.f, 0.f, 0.f, 0.f}, dph[4] = {0.f, 0.f, 0.f, 0.f};
    const long R = (long)p.B * p.T;
    const int head = c0 / dh, u = c0 % dh;
    for (long row = (long)blockIdx.x * rpb + rl; row < R; row += (long)gridDim.x * rpb) {
        const int t = (int)(row % p.T);
        const long b = row / p.T;
        const float* tr = p.ts + b * (p.T + 1);
        const float base = tr[p.T] / p.time_scale;
        const float a = tr[t + 1] / p.time_scale - base, bk = tr[t] / p.time_scale - base;
        const Frag4<T> qv = frag_ld<T>(reinterpret_cast<const T*>(p.q) + row * p.ldq + c0);
        const T* gq = reinterpret_cast<const T*>(p.d_qx) + (row * p.H + head) * 3 * dh + u;
        const T* gk = reinterpret_cast<const T*>(p.d_kx) + (row * p.H + head) * 3 * dh + u;
        const Frag4<T> g0 = frag_ld<T>(gq), gc = frag_ld<T>(gq + dh), gs = frag_ld<T>(gq + 2 * dh);
        const Frag4<T> h0 = frag_ld<T>(gk), hc = frag_ld<T>(gk + dh), hs = frag_ld<T>(gk + 2 * dh);
        Frag4<T> dq;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float sq, cq, sk, ck;
            sincosf(a * ww[i] + pv[i], &sq, &cq);
            sincosf(bk * ww[i], &sk, &ck);
            const float gcf = to_f32(gc.v[i]), gsf = to_f32(gs.v[i]);
            dq.v[i] = from_f32<T>(to_f32(g0.v[i]) + gcf * cq + gsf * sq);
            const float dth = to_f32(qv.v[i]) * (gsf * cq - gcf * sq);
            const float dps = to_f32(hs.v[i]) * ck - to_f32(hc.v[i]) * sk;
            dph[i] += dth;
            dw[i] += dth * a + dps * bk;
        }
        frag_st<T>(reinterpret_cast<T*>(p.d_q) + row * p.ld_dq + c0, dq);
        frag_st<T>(reinterpret_cast<T*>(p.d_k) + row * p.ld_dk + c0, h0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { red[threadIdx.x][i] = dw[i]; red[threadIdx.x][4 + i] = dph[i]; }
    __syncthreads();
    if (rl == 0) {
        float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int r = 0; r < rpb; ++r)
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] += red[r * cpr + cv][i];
        float* dst = p.part + (long)blockIdx.x * 2 * p.C;
#pragma unroll
        for (int i = 0; i < 4; ++i) { dst[c0 + i] = o[i]; dst[p.C + c0 + i] = o[4 + i]; }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void mask_rows_kernel(const T* x, const int64_t* ids, T* y, long rows, int C) {
    const int cpr = C >> 2;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long row = gid / cpr;
    if (row >= rows) return;
    const int c0 = (int)(gid % cpr) * 4;
    const Frag4<T> v = ids[row] != 0 ? frag_ld<T>(x + row * C + c0) : frag_zero<T>();
    frag_st<T>(y + row * C + c0, v);
}

constexpr int TF_BLOCKS = 256;

}  // namespace

extern "C" int edgl_timefn_fwd(const void* q, int ldq, const void* k, int ldk, const float* pos_tab, const float* ts,
                               const int64_t* ids, const float* omega, const float* phi, int B, int T, int C, int H,
                               float time_scale, void* qx, void* kx, int* violations, int dtype, void* stream) {
    EDGL_REQUIRE(q && k && pos_tab && ts && ids && omega && phi && qx && kx && violations, EDGL_ERR_NULL, "edgl_timefn_fwd: null pointer");
    EDGL_REQUIRE(B > 0 && T > 0 && H > 0 && C % H == 0 && (C / H) % 16 == 0 && ldq % 4 == 0 && ldk % 4 == 0, EDGL_ERR_SHAPE,
                 "edgl_timefn_fwd: bad shape B=%d T=%d C=%d H=%d (head dim must be a multiple of 16)", B, T, C, H);
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_timefn_fwd: bad dtype %d", dtype);
    TfP p{};
    p.q = q; p.k = k; p.ldq = ldq; p.ldk = ldk; p.pos = pos_tab; p.ts = ts; p.ids = ids; p.omega = omega; p.phi = phi;
    p.B = B; p.T = T; p.C = C; p.H = H; p.time_scale = time_scale; p.qx = qx; p.kx = kx; p.viol = violations;
    const long total = (long)B * T * (C / 4);
    dim3 grid((unsigned)((total + 255) / 256));
    if (dtype == EDGL_F32) hipLaunchKernelGGL((timefn_fwd_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((timefn_fwd_kernel<bf16>), grid, dim3(256), 0, (hipStream_t)stream, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" long edgl_timefn_bwd_workspace(int C) { return (long)TF_BLOCKS * 2 * C; }

extern "C" int edgl_timefn_bwd(const void* q, int ldq, const float* ts, const float* omega, const float* phi, const void* d_qx,
                               const void* d_kx, int B, int T, int C, int H, float time_scale, void* d_q, int ld_dq, void* d_k,
                               int ld_dk, float* d_omega, float* d_phi, float* workspace, int dtype, void* stream) {
    EDGL_REQUIRE(q && ts && omega && phi && d_qx && d_kx && d_q && d_k && d_omega && d_phi && workspace, EDGL_ERR_NULL,
                 "edgl_timefn_bwd: null pointer");
    EDGL_REQUIRE(B > 0 && T > 0 && H > 0 && C % H == 0 && (C / H) % 16 == 0 && C / 4 <= 256 && 256 % (C / 4) == 0 &&
                     ldq % 4 == 0 && ld_dq % 4 == 0 && ld_dk % 4 == 0, EDGL_ERR_SHAPE,
                 "edgl_timefn_bwd: bad shape B=%d T=%d C=%d H=%d (C/4 must divide 256)", B, T, C, H);
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_timefn_bwd: bad dtype %d", dtype);
    TfP p{};
    p.q = q; p.ldq = ldq; p.ts = ts; p.omega = omega; p.phi = phi; p.B = B; p.T = T; p.C = C; p.H = H;
    p.time_scale = time_scale; p.d_qx = d_qx; p.d_kx = d_kx; p.d_q = d_q; p.d_k = d_k; p.ld_dq = ld_dq; p.ld_dk = ld_dk;
    p.part = workspace;
    hipStream_t st = (hipStream_t)stream;
    const int rpb = 256 / (C / 4);
    const int blocks = (int)std::min<long>(TF_BLOCKS, ((long)B * T + rpb - 1) / rpb);
    if (dtype == EDGL_F32) hipLaunchKernelGGL((timefn_bwd_kernel<float>), dim3(blocks), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((timefn_bwd_kernel<bf16>), dim3(blocks), dim3(256), 0, st, p);
    EDGL_LAUNCH_CHECK();
    // partial rows are [d_omega | d_phi]: one fixed-order reduction (adjacent outputs) or one each
    if (d_phi == d_omega + C) return edgl_reduce_rows(workspace, blocks, 2 * C, 2L * C, d_omega, 0, st);
    if (int rc = edgl_reduce_rows(workspace, blocks, C, 2L * C, d_omega, 0, st)) return rc;
    return edgl_reduce_rows(workspace + C, blocks, C, 2L * C, d_phi, 0, st);
}

extern "C" int edgl_mask_rows(const void* x, const int64_t* ids, void* y, long rows, int C, int dtype, void* stream) {
    EDGL_REQUIRE(x && ids && y, EDGL_ERR_NULL, "edgl_mask_rows: null pointer");
    EDGL_REQUIRE(rows > 0 && C > 0 && C % 4 == 0, EDGL_ERR_SHAPE, "edgl_mask_rows: bad shape rows=%ld C=%d", rows, C);
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_mask_rows: bad dtype %d", dtype);
    const long total = rows * (C / 4);
    dim3 grid((unsigned)((total + 255) / 256));
    if (dtype == EDGL_F32) hipLaunchKernelGGL((mask_rows_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream,
                                              (const float*)x, ids, (float*)y, rows, C);
    else hipLaunchKernelGGL((mask_rows_kernel<bf16>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)x, ids, (bf16*)y, rows, C);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
