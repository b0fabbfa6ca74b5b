// K12: temporal-graph attention with time-coded keys AND values — TgMultiHeadAttention.__call__ (temporal.py:204-258, TGREC,
// Fan et al., CIKM'21) between its dense layers.  The reference projects [x_k | Phi(dt[q,k])] (2C wide) with Wk and with Wv for
// every (q, k) pair, Phi_c(dt) = cos(dt w_c + phi_c), dt = max(t_q - t_k, 0): three [B,T,T,2C]-derived tensors per block.  Here
//     S_h[q,k]  = scale ( Q_h[q] . Kx_h[k] + sum_c U_h[q,c] Phi_c[q,k] ),      U_h[q,:] = Q_h[q] . Wk_t[:,h]^T   (host GEMM)
//     Ox_h[q]   = sum_k P_h[q,k] Vx_h[k],   G_h[q,c] = sum_k P_h[q,k] Phi_c[q,k]   (O_h = Ox_h + G_h . Wv_t[:,h], host GEMM)
// and for k <= q (timestamps do not decrease along the row) Phi_c[q,k] = cosA[q,c] Ck[k,c] + sinA[q,c] Sk[k,c] with
// A = a_q w + phi, Ck = cos(b_k w), Sk = sin(b_k w), a / b re-based on the row's last timestamp (k_timefn.hip); for k > q the
// clamp gives Phi = cos(phi).  So the time part of the score is (U (.) cosA) . Ck^T + (U (.) sinA) . Sk^T and
//     G_h[q,c] = cosA (P° . Ck)_c + sinA (P° . Sk)_c + r_q cos(phi_c),   P° = P (.) tril,  r_q = sum_{k>q} P[q,k]
// (r_q != 0 only in fully masked rows, which are uniform over all T keys and feed a real label: Base.py:119-140).
//
// Work split (forward, query sweep of the backward): a workgroup owns ONE sample and four (head, 16-query tile) waves, heads
// fastest.  Per 16-key tile all 256 lanes compute Ck / Sk once (f32 sincosf, C/16 each) into an LDS image in the row-chunk layout
// the MFMA operands read ([key][channel], rows padded by 4 elements: conflict-free 8 / 16-byte reads); every wave contracts
// against that image for the score and, turned through the identity, for P° . Ck / P° . Sk.  The image never reaches memory.
// Kx / Vx fragments are per head and come from L2.  Online softmax per wave; (dh + 2C)/16 accumulator tiles per wave.
// Backward: the query sweep (same shape) gives dQ, dU and the query-side parts of d_omega / d_phi and leaves the four scaled
// operands U(.)cosA, U(.)sinA, dG(.)cosA, dG(.)sinA for the key sweep (one wave per (sample, head, key tile), Ck / Sk of its own
// tile in registers), which gives dKx, dVx and — from dCk / dSk — the key-side part of d_omega.  Every parameter partial is one
// row per workgroup, summed by edgl_reduce_rows in a fixed order: no f32 atomics.
#include "tattn_common.h"   // PADV, frag_st, turn, first_unpadded

namespace {

struct TgP {
    const void *q, *u, *kv;
    const float* ts; int ld_t;
    const int64_t* ids;
    const float *omega, *phi;
    int B, T, H, C, NT, NWG;
    float cscale, rate, time_scale;
    const uint64_t* rng; uint32_t stream_id;
    void *ox, *g;
    float *st_m, *st_l, *st_d;
    int* viol;
    const void *d_ox, *d_g;
    void *d_q, *d_u, *d_kv, *w4;
    float *part_q, *part_k;
};

constexpr int TG_WAVES = 4;
constexpr int TG_PAD = 4;    // elements a row of the LDS image is padded by

__device__ __forceinline__ float sum16(float v) {   // over the 16 lanes that share lane >> 4
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// which (sample, head, tile) a wave of the query-shaped kernels owns, and how far the workgroup walks the key tiles
struct QJob { int b, head, tile, my_end, kt_max, fnp; bool valid; long bp; };
__device__ __forceinline__ QJob q_job(const TgP& p, int lane) {
    QJob j;
    j.b = blockIdx.x / p.NWG;
    const int job0 = (blockIdx.x % p.NWG) * TG_WAVES, jobs = p.H * p.NT, job = job0 + (threadIdx.x >> 6);
    j.valid = job < jobs;
    const int jc = min(job, jobs - 1);
    j.head = jc % p.H; j.tile = jc / p.H;
    j.bp = (long)j.head * p.B + j.b;
    j.fnp = first_unpadded(p.ids + (long)j.b * p.T, p.T, lane);
    // rows from first_unpadded on give exact zeros to the key tiles above their diagonal (tattn_common.h): skipped
    const int t0 = job0 / p.H, t1 = min(job0 + TG_WAVES - 1, jobs - 1) / p.H;
    const int e0 = t0 * 16 >= j.fnp ? t0 + 1 : p.NT, e1 = t1 * 16 >= j.fnp ? t1 + 1 : p.NT;
    j.kt_max = max(e0, e1);
    j.my_end = !j.valid ? 0 : (j.tile * 16 >= j.fnp ? j.tile + 1 : p.NT);
    return j;
}

// Ck | Sk of key tile kt into the image: 256 lanes, lane -> key tid & 15, channels (tid >> 4) + 16 i
template <typename T, int CT>
__device__ __forceinline__ void fill_image(T (*img)[16][CT * 16 + TG_PAD], const TgP& p, const float* tsr, float base, int kt,
                                           const float (&wreg)[CT]) {
    const int kk = threadIdx.x & 15, c0 = threadIdx.x >> 4;
    const float bk = tsr[min(kt * 16 + kk, p.T - 1)] / p.time_scale - base;
#pragma unroll
    for (int i = 0; i < CT; ++i) {
        float s, c;
        sincosf(bk * wreg[i], &s, &c);
        img[0][kk][c0 + 16 * i] = from_f32<T>(c);
        img[1][kk][c0 + 16 * i] = from_f32<T>(s);
    }
}

// the lane's row chunk of X[q][c] times cos / sin of A[q][c] = a w_c + phi_c
template <typename T>
__device__ __forceinline__ void scale_by_angle(const Frag4<T>& x, float a, const float* omega, const float* phi, int c0,
                                               Frag4<T>& xc, Frag4<T>& xs) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float s, c;
        sincosf(fmaf(a, omega[c0 + j], phi[c0 + j]), &s, &c);
        const float v = to_f32(x.v[j]);
        xc.v[j] = from_f32<T>(v * c);
        xs.v[j] = from_f32<T>(v * s);
    }
}

// scaled, masked scores of a [key g4+r][query l15] tile and the keep bits of its four keys
struct KeepBits { uint32_t hb[4]; };
__device__ __forceinline__ KeepBits keep_bits(const DropKey& dk, uint32_t idx) {
    uint32_t h0 = 0xffffffffu, h1 = 0xffffffffu;
    if (dk.thresh != 0u) { h0 = drop_hash_pair(dk, idx); h1 = drop_hash_pair(dk, idx + 2); }
    return KeepBits{{h0 & 0xffffu, h0 >> 16, h1 & 0xffffu, h1 >> 16}};
}

// ---- forward -----------------------------------------------------------------------------------------------------------
template <typename T, int DHT, int CT>
__global__ __launch_bounds__(256) void tg_fwd_kernel(TgP p) {
    constexpr int C = CT * 16, DH = DHT * 16;
    __shared__ __attribute__((aligned(16))) T img[2][16][C + TG_PAD];
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15;
    const QJob j = q_job(p, lane);
    const float* tsr = p.ts + (long)j.b * p.ld_t;
    const int64_t* idr = p.ids + (long)j.b * p.T;
    const float base = tsr[p.T - 1] / p.time_scale;
    if (p.viol && blockIdx.x % p.NWG == 0)     // the factorisation needs non-decreasing times at EVERY position of the row
        for (int k = threadIdx.x + 1; k < p.T; k += blockDim.x)
            if (tsr[k] < tsr[k - 1]) atomicAdd(p.viol, 1);
    float wreg[CT];
#pragma unroll
    for (int i = 0; i < CT; ++i) wreg[i] = p.omega[(threadIdx.x >> 4) + 16 * i];
    const int q = j.tile * 16 + l15, qc = min(q, p.T - 1);
    const bool qok = j.valid && q < p.T;
    const float aq = tsr[qc] / p.time_scale - base;
    const long qrow = (long)j.b * p.T + qc;
    const T* Qr = reinterpret_cast<const T*>(p.q) + qrow * C + j.head * DH;
    const T* Ur = reinterpret_cast<const T*>(p.u) + (qrow * p.H + j.head) * C;
    const T* KVb = reinterpret_cast<const T*>(p.kv) + (long)j.b * p.T * 2 * C + j.head * DH;
    const DropKey dk = make_dropkey(p.rng, p.stream_id, p.rate);
    const Frag4<T> ident = identity_frag<T>(lane);
    const uint32_t dbase = (uint32_t)((j.bp * p.T + qc) * p.T);
    Frag4<T> qf[DHT], uc[CT], us[CT];
#pragma unroll
    for (int dt = 0; dt < DHT; ++dt) qf[dt] = frag_ld<T>(Qr + dt * 16 + g4);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
        scale_by_angle<T>(frag_ld<T>(Ur + ct * 16 + g4), aq, p.omega, p.phi, ct * 16 + g4, uc[ct], us[ct]);
    float m_run = -INFINITY, l_run = 0.f, r_run = 0.f;
    f32x4 acc[DHT], gc[CT], gs[CT];
#pragma unroll
    for (int ut = 0; ut < DHT; ++ut) acc[ut] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) { gc[ct] = f32x4{0.f, 0.f, 0.f, 0.f}; gs[ct] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int kt = 0; kt < j.kt_max; ++kt) {
        __syncthreads();
        fill_image<T, CT>(img, p, tsr, base, kt, wreg);
        __syncthreads();
        if (kt >= j.my_end) continue;
        const int kr = min(kt * 16 + l15, p.T - 1);
        const T* Krow = KVb + (long)kr * 2 * C;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        Frag4<T> vraw[DHT];
#pragma unroll
        for (int dt = 0; dt < DHT; ++dt) s = mma16(frag_ld<T>(Krow + dt * 16 + g4), qf[dt], s);
#pragma unroll
        for (int ut = 0; ut < DHT; ++ut) vraw[ut] = frag_ld<T>(Krow + C + ut * 16 + g4);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            s = mma16(frag_ld<T>(&img[0][l15][ct * 16 + g4]), uc[ct], s);
            s = mma16(frag_ld<T>(&img[1][l15][ct * 16 + g4]), us[ct], s);
        }
        float x[4], tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = kt * 16 + g4 + r;
            const float madd = k >= p.T ? -INFINITY : (idr[min(k, p.T - 1)] == 0 ? PADV : 0.f);   // temporal.py:235-236
            float v = fmaf(s[r], p.cscale, madd);
            if (k > q && k < p.T) v = PADV;                                                      // :239-244
            x[r] = v;
            tmax = fmaxf(tmax, v);
        }
        tmax = group_max4(tmax);
        const float m_new = fmaxf(m_run, tmax), corr = __expf(m_run - m_new);
        f32x4 e;
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) { e[r] = __expf(x[r] - m_new); psum += e[r]; }
        l_run = l_run * corr + group_sum4(psum);
        m_run = m_new;
        const KeepBits kb = keep_bits(dk, dbase + kt * 16 + g4);                                 // :250
        f32x4 e0;
        float rsum = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = kt * 16 + g4 + r;
            if (dk.thresh != 0u && kb.hb[r] < dk.t16) e[r] = 0.f;
            e0[r] = k <= q ? e[r] : 0.f;
            rsum += (k > q && k < p.T) ? e[r] : 0.f;
        }
        r_run = r_run * corr + group_sum4(rsum);
        const Frag4<T> pf = frag_from_acc<T>(e), pf0 = frag_from_acc<T>(e0);
#pragma unroll
        for (int ut = 0; ut < DHT; ++ut) {
            const Frag4<T> vt = turn<T>(vraw[ut], ident);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[ut][r] *= corr;
            acc[ut] = mma16(vt, pf, acc[ut]);                                                    // :252-255, the x half of V
        }
        const bool below = kt <= j.tile;     // a tile above the diagonal holds no k <= q
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { gc[ct][r] *= corr; gs[ct][r] *= corr; }
            if (below) {
                gc[ct] = mma16(turn<T>(frag_ld<T>(&img[0][l15][ct * 16 + g4]), ident), pf0, gc[ct]);
                gs[ct] = mma16(turn<T>(frag_ld<T>(&img[1][l15][ct * 16 + g4]), ident), pf0, gs[ct]);
            }
        }
    }
    if (!qok) return;
    const float inv = dk.scale / l_run;
    if (p.st_m && g4 == 0) { p.st_m[j.bp * p.T + q] = m_run; p.st_l[j.bp * p.T + q] = l_run; }
    const long orow = (long)j.b * p.T + q;
#pragma unroll
    for (int ut = 0; ut < DHT; ++ut) {
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = acc[ut][r] * inv;
        frag_st<T>(reinterpret_cast<T*>(p.ox) + orow * C + j.head * DH + ut * 16 + g4, frag_from_acc<T>(o));
    }
    T* Gr = reinterpret_cast<T*>(p.g) + (orow * p.H + j.head) * C;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = ct * 16 + g4 + r;
            float sa, ca;
            sincosf(fmaf(aq, p.omega[c], p.phi[c]), &sa, &ca);
            o[r] = (ca * gc[ct][r] + sa * gs[ct][r] + r_run * cosf(p.phi[c])) * inv;
        }
        frag_st<T>(Gr + ct * 16 + g4, frag_from_acc<T>(o));
    }
}

// ---- backward, query sweep ---------------------------------------------------------------------------------------------
// D = dOx . Ox + dG . G; dS = P (dP - D) scale; dQ^T += Kx^T dS^T; X1 = dS . Ck, X2 = dS . Sk, Y1 = P° . Ck, Y2 = P° . Sk;
// dU = cosA X1 + sinA X2; with Z1 = U X1 + dG Y1, Z2 = U X2 + dG Y2 (= dL/dcosA, dL/dsinA) the angle gradient of the row is
// dA = cosA Z2 - sinA Z1: d_phi += dA - sin(phi) dG r_q, d_omega += a_q dA.
template <typename T, int DHT, int CT>
__global__ __launch_bounds__(256) void tg_bwd_q_kernel(TgP p) {
    constexpr int C = CT * 16, DH = DHT * 16;
    __shared__ __attribute__((aligned(16))) T img[2][16][C + TG_PAD];
    __shared__ float red[TG_WAVES][2 * C];
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15, wave = threadIdx.x >> 6;
    const QJob j = q_job(p, lane);
    const float* tsr = p.ts + (long)j.b * p.ld_t;
    const int64_t* idr = p.ids + (long)j.b * p.T;
    const float base = tsr[p.T - 1] / p.time_scale;
    float wreg[CT];
#pragma unroll
    for (int i = 0; i < CT; ++i) wreg[i] = p.omega[(threadIdx.x >> 4) + 16 * i];
    const int q = j.tile * 16 + l15, qc = min(q, p.T - 1);
    const bool qok = j.valid && q < p.T;
    const float aq = tsr[qc] / p.time_scale - base;
    const long qrow = (long)j.b * p.T + qc, hrow = qrow * p.H + j.head;
    const T* Qr = reinterpret_cast<const T*>(p.q) + qrow * C + j.head * DH;
    const T* Ur = reinterpret_cast<const T*>(p.u) + hrow * C;
    const T* dOr = reinterpret_cast<const T*>(p.d_ox) + qrow * C + j.head * DH;
    const T* dGr = reinterpret_cast<const T*>(p.d_g) + hrow * C;
    const T* KVb = reinterpret_cast<const T*>(p.kv) + (long)j.b * p.T * 2 * C + j.head * DH;
    const DropKey dk = make_dropkey(p.rng, p.stream_id, p.rate);
    const Frag4<T> ident = identity_frag<T>(lane);
    const uint32_t dbase = (uint32_t)((j.bp * p.T + qc) * p.T);
    Frag4<T> qf[DHT], gf[DHT], uc[CT], us[CT], dgc[CT], dgs[CT];
    float dsum = 0.f;
    {
        const T* Oxr = reinterpret_cast<const T*>(p.ox) + qrow * C + j.head * DH;
        const T* Gr = reinterpret_cast<const T*>(p.g) + hrow * C;
#pragma unroll
        for (int dt = 0; dt < DHT; ++dt) {
            qf[dt] = frag_ld<T>(Qr + dt * 16 + g4);
            gf[dt] = frag_ld<T>(dOr + dt * 16 + g4);
            const Frag4<T> o = frag_ld<T>(Oxr + dt * 16 + g4);
#pragma unroll
            for (int i = 0; i < 4; ++i) dsum += to_f32(gf[dt].v[i]) * to_f32(o.v[i]);
        }
        T* W = reinterpret_cast<T*>(p.w4) + hrow * 4 * C;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const Frag4<T> dg = frag_ld<T>(dGr + ct * 16 + g4), o = frag_ld<T>(Gr + ct * 16 + g4);
#pragma unroll
            for (int i = 0; i < 4; ++i) dsum += to_f32(dg.v[i]) * to_f32(o.v[i]);
            scale_by_angle<T>(frag_ld<T>(Ur + ct * 16 + g4), aq, p.omega, p.phi, ct * 16 + g4, uc[ct], us[ct]);
            scale_by_angle<T>(dg, aq, p.omega, p.phi, ct * 16 + g4, dgc[ct], dgs[ct]);
            if (qok) {     // the key sweep's query-side operands
                frag_st<T>(W + ct * 16 + g4, uc[ct]); frag_st<T>(W + C + ct * 16 + g4, us[ct]);
                frag_st<T>(W + 2 * C + ct * 16 + g4, dgc[ct]); frag_st<T>(W + 3 * C + ct * 16 + g4, dgs[ct]);
            }
        }
        dsum = group_sum4(dsum);
        if (qok && g4 == 0) p.st_d[j.bp * p.T + q] = dsum;
    }
    const float m = p.st_m[j.bp * p.T + qc], invl = 1.0f / p.st_l[j.bp * p.T + qc];
    float r_sum = 0.f;
    f32x4 acc[DHT], x1[CT], x2[CT], y1[CT], y2[CT];
#pragma unroll
    for (int dt = 0; dt < DHT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        x1[ct] = f32x4{0.f, 0.f, 0.f, 0.f}; x2[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        y1[ct] = f32x4{0.f, 0.f, 0.f, 0.f}; y2[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int kt = 0; kt < j.kt_max; ++kt) {
        __syncthreads();
        fill_image<T, CT>(img, p, tsr, base, kt, wreg);
        __syncthreads();
        if (kt >= j.my_end) continue;
        const int kr = min(kt * 16 + l15, p.T - 1);
        const T* Krow = KVb + (long)kr * 2 * C;
        f32x4 s = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
        Frag4<T> kf[DHT];
#pragma unroll
        for (int dt = 0; dt < DHT; ++dt) {
            kf[dt] = frag_ld<T>(Krow + dt * 16 + g4);
            s = mma16(kf[dt], qf[dt], s);
            da = mma16(frag_ld<T>(Krow + C + dt * 16 + g4), gf[dt], da);
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const Frag4<T> ck = frag_ld<T>(&img[0][l15][ct * 16 + g4]), sk = frag_ld<T>(&img[1][l15][ct * 16 + g4]);
            s = mma16(ck, uc[ct], s); s = mma16(sk, us[ct], s);
            da = mma16(ck, dgc[ct], da); da = mma16(sk, dgs[ct], da);
        }
        const KeepBits kb = keep_bits(dk, dbase + kt * 16 + g4);
        f32x4 ds, a0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = kt * 16 + g4 + r;
            const bool pad = k >= p.T || idr[min(k, p.T - 1)] == 0, fut = k > q;
            float v = fmaf(s[r], p.cscale, k >= p.T ? -INFINITY : (pad ? PADV : 0.f));
            if (fut && k < p.T) v = PADV;
            const float P = __expf(v - m) * invl;
            const bool keep = dk.thresh == 0u || kb.hb[r] >= dk.t16;
            const float Pd = (keep && qok) ? P * dk.scale : 0.f, dP = keep ? da[r] * dk.scale : 0.f;
            // a replaced score is a constant (tf.where): no gradient, also in a fully masked (uniform) row
            ds[r] = (pad || fut || !qok) ? 0.f : P * (dP - dsum) * p.cscale;
            a0[r] = fut ? 0.f : Pd;
            r_sum += (fut && k < p.T) ? Pd : 0.f;
        }
        const Frag4<T> dsf = frag_from_acc<T>(ds), a0f = frag_from_acc<T>(a0);
#pragma unroll
        for (int dt = 0; dt < DHT; ++dt) acc[dt] = mma16(turn<T>(kf[dt], ident), dsf, acc[dt]);
        if (kt <= j.tile) {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const Frag4<T> ckt = turn<T>(frag_ld<T>(&img[0][l15][ct * 16 + g4]), ident);
                const Frag4<T> skt = turn<T>(frag_ld<T>(&img[1][l15][ct * 16 + g4]), ident);
                x1[ct] = mma16(ckt, dsf, x1[ct]); x2[ct] = mma16(skt, dsf, x2[ct]);
                y1[ct] = mma16(ckt, a0f, y1[ct]); y2[ct] = mma16(skt, a0f, y2[ct]);
            }
        }
    }
    r_sum = group_sum4(r_sum);
    if (qok) {
        T* dst = reinterpret_cast<T*>(p.d_q) + qrow * C + j.head * DH;
#pragma unroll
        for (int dt = 0; dt < DHT; ++dt) frag_st<T>(dst + dt * 16 + g4, frag_from_acc<T>(acc[dt]));
    }
    T* dUr = reinterpret_cast<T*>(p.d_u) + hrow * C;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const Frag4<T> uf = frag_ld<T>(Ur + ct * 16 + g4), dg = frag_ld<T>(dGr + ct * 16 + g4);
        f32x4 du;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = ct * 16 + g4 + r;
            float sa, ca;
            sincosf(fmaf(aq, p.omega[c], p.phi[c]), &sa, &ca);
            du[r] = ca * x1[ct][r] + sa * x2[ct][r];
            const float u = to_f32(uf.v[r]), g = to_f32(dg.v[r]);
            const float z1 = u * x1[ct][r] + g * y1[ct][r], z2 = u * x2[ct][r] + g * y2[ct][r];
            const float dA = qok ? ca * z2 - sa * z1 : 0.f;
            const float dph = qok ? dA - sinf(p.phi[c]) * g * r_sum : 0.f;
            const float sw = sum16(aq * dA), sp = sum16(dph);
            if (l15 == 0) { red[wave][c] = sw; red[wave][C + c] = sp; }
        }
        if (qok) frag_st<T>(dUr + ct * 16 + g4, frag_from_acc<T>(du));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += blockDim.x)
        p.part_q[(long)blockIdx.x * 2 * C + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
}

// ---- backward, key sweep -----------------------------------------------------------------------------------------------
// per key tile over the query tiles: dVx^T += dOx^T A, dKx^T += Q^T dS, dCk^T += (U cosA)^T dS + (dG cosA)^T A°, dSk likewise
// with sinA; then d_omega += b_k (Ck dSk - Sk dCk).
template <typename T, int DHT, int CT>
__global__ __launch_bounds__(256) void tg_bwd_k_kernel(TgP p) {
    constexpr int C = CT * 16, DH = DHT * 16;
    __shared__ float red[TG_WAVES][C];
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15, wave = threadIdx.x >> 6;
    const long jobs = (long)p.B * p.H * p.NT, job = (long)blockIdx.x * TG_WAVES + wave;
    const bool valid = job < jobs;
    const long jc = min(job, jobs - 1);
    const int tile = (int)(jc % p.NT), head = (int)((jc / p.NT) % p.H), b = (int)(jc / ((long)p.NT * p.H));
    const long bp = (long)head * p.B + b;
    const float* tsr = p.ts + (long)b * p.ld_t;
    const float base = tsr[p.T - 1] / p.time_scale;
    const int k = tile * 16 + l15, kc = min(k, p.T - 1);
    const bool kok = valid && k < p.T;
    const float bk = tsr[kc] / p.time_scale - base;
    const T* Qb = reinterpret_cast<const T*>(p.q) + (long)b * p.T * C + head * DH;
    const T* dOb = reinterpret_cast<const T*>(p.d_ox) + (long)b * p.T * C + head * DH;
    const T* Wb = reinterpret_cast<const T*>(p.w4) + ((long)b * p.T * p.H + head) * 4 * C;
    const T* Kr = reinterpret_cast<const T*>(p.kv) + ((long)b * p.T + kc) * 2 * C + head * DH;
    const bool pad = k >= p.T || p.ids[(long)b * p.T + kc] == 0;
    const float madd = k >= p.T ? -INFINITY : (pad ? PADV : 0.f);
    const DropKey dk = make_dropkey(p.rng, p.stream_id, p.rate);
    const Frag4<T> ident = identity_frag<T>(lane);
    Frag4<T> kf[DHT], vf[DHT], ckf[CT], skf[CT];
#pragma unroll
    for (int dt = 0; dt < DHT; ++dt) { kf[dt] = frag_ld<T>(Kr + dt * 16 + g4); vf[dt] = frag_ld<T>(Kr + C + dt * 16 + g4); }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float s, c;
            sincosf(bk * p.omega[ct * 16 + g4 + i], &s, &c);
            ckf[ct].v[i] = from_f32<T>(c);
            skf[ct].v[i] = from_f32<T>(s);
        }
    f32x4 accK[DHT], accV[DHT], dck[CT], dsk[CT];
#pragma unroll
    for (int dt = 0; dt < DHT; ++dt) { accK[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; accV[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) { dck[ct] = f32x4{0.f, 0.f, 0.f, 0.f}; dsk[ct] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    const int fnp = first_unpadded(p.ids + (long)b * p.T, p.T, lane);
    for (int qt = 0; valid && qt < p.NT; ++qt) {
        if (qt < tile && qt * 16 >= fnp) continue;   // all 16 queries see this key tile as future: exact zeros
        const int ql = min(qt * 16 + l15, p.T - 1);
        const T* Qrow = Qb + (long)ql * C;
        const T* dOrow = dOb + (long)ql * C;
        const T* Wrow = Wb + (long)ql * p.H * 4 * C;
        f32x4 s = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};   // [q = g4+r][k = l15]
        Frag4<T> qf[DHT], gf[DHT];
#pragma unroll
        for (int dt = 0; dt < DHT; ++dt) {
            qf[dt] = frag_ld<T>(Qrow + dt * 16 + g4); gf[dt] = frag_ld<T>(dOrow + dt * 16 + g4);
            s = mma16(qf[dt], kf[dt], s);
            da = mma16(gf[dt], vf[dt], da);
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            s = mma16(frag_ld<T>(Wrow + ct * 16 + g4), ckf[ct], s);
            s = mma16(frag_ld<T>(Wrow + C + ct * 16 + g4), skf[ct], s);
            da = mma16(frag_ld<T>(Wrow + 2 * C + ct * 16 + g4), ckf[ct], da);
            da = mma16(frag_ld<T>(Wrow + 3 * C + ct * 16 + g4), skf[ct], da);
        }
        f32x4 a4, a0, ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = qt * 16 + g4 + r, qc = min(q, p.T - 1);
            const long si = bp * p.T + qc;
            const bool fut = k > q;
            float v = fmaf(s[r], p.cscale, madd);
            if (fut && k < p.T) v = PADV;
            const float P = (q < p.T) ? __expf(v - p.st_m[si]) / p.st_l[si] : 0.f;
            bool keep = true;
            if (dk.thresh != 0u) {   // the forward's pairing: one hash per (k even, k + 1) of a row
                const uint32_t h = drop_hash_pair(dk, (uint32_t)(si * p.T) + (uint32_t)(k & ~1));
                keep = ((k & 1) ? (h >> 16) : (h & 0xffffu)) >= dk.t16;
            }
            a4[r] = keep ? P * dk.scale : 0.f;
            a0[r] = fut ? 0.f : a4[r];
            const float dP = keep ? da[r] * dk.scale : 0.f;
            ds[r] = (pad || fut || q >= p.T) ? 0.f : P * (dP - p.st_d[si]) * p.cscale;
        }
        const Frag4<T> af = frag_from_acc<T>(a4), a0f = frag_from_acc<T>(a0), dsf = frag_from_acc<T>(ds);
#pragma unroll
        for (int dt = 0; dt < DHT; ++dt) {
            accV[dt] = mma16(turn<T>(gf[dt], ident), af, accV[dt]);
            accK[dt] = mma16(turn<T>(qf[dt], ident), dsf, accK[dt]);
        }
        if (qt >= tile) {     // below it no query has k <= q
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                dck[ct] = mma16(turn<T>(frag_ld<T>(Wrow + ct * 16 + g4), ident), dsf, dck[ct]);
                dsk[ct] = mma16(turn<T>(frag_ld<T>(Wrow + C + ct * 16 + g4), ident), dsf, dsk[ct]);
                dck[ct] = mma16(turn<T>(frag_ld<T>(Wrow + 2 * C + ct * 16 + g4), ident), a0f, dck[ct]);
                dsk[ct] = mma16(turn<T>(frag_ld<T>(Wrow + 3 * C + ct * 16 + g4), ident), a0f, dsk[ct]);
            }
        }
    }
    if (kok) {
        T* dK = reinterpret_cast<T*>(p.d_kv) + ((long)b * p.T + k) * 2 * C + head * DH;
#pragma unroll
        for (int dt = 0; dt < DHT; ++dt) {
            frag_st<T>(dK + dt * 16 + g4, frag_from_acc<T>(accK[dt]));
            frag_st<T>(dK + C + dt * 16 + g4, frag_from_acc<T>(accV[dt]));
        }
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = ct * 16 + g4 + r;
            float sk, ck;
            sincosf(bk * p.omega[c], &sk, &ck);
            const float sw = sum16(kok ? bk * (ck * dsk[ct][r] - sk * dck[ct][r]) : 0.f);
            if (l15 == 0) red[wave][c] = sw;
        }
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += blockDim.x)
        p.part_k[(long)blockIdx.x * C + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
inline size_t tg_rows(int B, int T, int H) { return ((size_t)B * H * T + 63) & ~(size_t)63; }
inline int tg_nwg(int T, int H) { return (H * ((T + 15) / 16) + TG_WAVES - 1) / TG_WAVES; }
inline long tg_kwgs(int B, int T, int H) { return ((long)B * H * ((T + 15) / 16) + TG_WAVES - 1) / TG_WAVES; }

int tg_check(const char* who, int B, int T, int H, int C, int ld_t, int dtype) {
    const int dh = H > 0 && C % H == 0 ? C / H : 0;
    EDGL_REQUIRE(B > 0 && T > 0 && T <= 1024 && ld_t >= T, EDGL_ERR_SHAPE, "%s: bad shape B=%d T=%d ld_t=%d (1 <= T <= 1024)", who, B, T, ld_t);
    EDGL_REQUIRE((C == 32 || C == 64 || C == 128) && (dh == 16 || dh == 32 || dh == 64 || dh == 128), EDGL_ERR_SHAPE,
                 "%s: C=%d H=%d unsupported (C in {32, 64, 128}, head dim C/H in {16, 32, 64, 128})", who, C, H);
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "%s: bad dtype %d", who, dtype);
    EDGL_REQUIRE((double)B * H * T * T < 4294967296.0, EDGL_ERR_SHAPE, "%s: H*B*T*T must be < 2^32", who);
    EDGL_REQUIRE((double)B * tg_nwg(T, H) < 2147483647.0, EDGL_ERR_SHAPE, "%s: too many workgroups", who);
    return EDGL_OK;
}

void bind_tg_saved(TgP& p, void* saved) {
    if (!saved) return;
    const size_t R = tg_rows(p.B, p.T, p.H);
    p.st_m = reinterpret_cast<float*>(saved); p.st_l = p.st_m + R; p.st_d = p.st_l + R;
}

// which = 0: forward, 1: query sweep, 2: key sweep
template <typename T, int DHT, int CT>
int tg_launch_one(const TgP& p, int which, hipStream_t st) {
    const unsigned qgrid = (unsigned)((long)p.B * p.NWG), kgrid = (unsigned)tg_kwgs(p.B, p.T, p.H);
    if (which == 0) hipLaunchKernelGGL((tg_fwd_kernel<T, DHT, CT>), dim3(qgrid), dim3(64 * TG_WAVES), 0, st, p);
    else if (which == 1) hipLaunchKernelGGL((tg_bwd_q_kernel<T, DHT, CT>), dim3(qgrid), dim3(64 * TG_WAVES), 0, st, p);
    else hipLaunchKernelGGL((tg_bwd_k_kernel<T, DHT, CT>), dim3(kgrid), dim3(64 * TG_WAVES), 0, st, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
template <typename T>
int tg_launch(const TgP& p, int which, hipStream_t st) {
    const int dht = p.C / p.H / 16, ct = p.C / 16;
#define EDGL_TG_CASE(D, Cc) if (dht == D && ct == Cc) return tg_launch_one<T, D, Cc>(p, which, st);
    EDGL_TG_CASE(1, 2) EDGL_TG_CASE(2, 2)
    EDGL_TG_CASE(1, 4) EDGL_TG_CASE(2, 4) EDGL_TG_CASE(4, 4)
    EDGL_TG_CASE(1, 8) EDGL_TG_CASE(2, 8) EDGL_TG_CASE(4, 8) EDGL_TG_CASE(8, 8)
#undef EDGL_TG_CASE
    edgl_set_error("edgl_tgattn: C=%d H=%d not supported", p.C, p.H);
    return EDGL_ERR_SHAPE;
}

TgP tg_params(const void* q, const void* u, const void* kv, const float* ts, int ld_t, const int64_t* ids, const float* omega,
              const float* phi, int B, int T, int H, int C, float scale, float time_scale, float drop_rate,
              const uint64_t* rng_state, uint32_t stream_id, void* ox, void* g, void* saved) {
    TgP p{};
    p.q = q; p.u = u; p.kv = kv; p.ts = ts; p.ld_t = ld_t; p.ids = ids; p.omega = omega; p.phi = phi;
    p.B = B; p.T = T; p.H = H; p.C = C; p.NT = (T + 15) / 16; p.NWG = tg_nwg(T, H);
    p.cscale = scale; p.time_scale = time_scale; p.rate = drop_rate; p.rng = rng_state; p.stream_id = stream_id;
    p.ox = ox; p.g = g;
    bind_tg_saved(p, saved);
    return p;
}

}  // namespace

extern "C" long edgl_tgattn_saved_bytes(int B, int T, int H) {
    if (B <= 0 || T <= 0 || H <= 0) return -1;
    return (long)(3 * tg_rows(B, T, H) * 4);
}

// floats of the backward's workspace: the key sweep's operands [B,T,H,4C] (in `dtype`, counted as floats) + the partial rows
extern "C" long edgl_tgattn_bwd_workspace(int B, int T, int H, int C) {
    if (B <= 0 || T <= 0 || H <= 0 || C <= 0) return -1;
    return (long)B * T * H * 4 * C + (long)B * tg_nwg(T, H) * 2 * C + tg_kwgs(B, T, H) * C;
}

extern "C" int edgl_tgattn_fwd(const void* q, const void* u, const void* kv, const float* ts, int ld_t, const int64_t* ids,
                               const float* omega, const float* phi, int B, int T, int H, int C, float scale, float time_scale,
                               float drop_rate, const uint64_t* rng_state, uint32_t stream_id, void* ox, void* g, void* saved,
                               int* violations, int dtype, void* stream) {
    EDGL_REQUIRE(q && u && kv && ts && ids && omega && phi && ox && g, EDGL_ERR_NULL, "edgl_tgattn_fwd: null pointer");
    if (int rc = tg_check("edgl_tgattn_fwd", B, T, H, C, ld_t, dtype)) return rc;
    EDGL_REQUIRE(time_scale > 0.f, EDGL_ERR_SHAPE, "edgl_tgattn_fwd: time_scale must be positive");
    EDGL_REQUIRE(drop_rate == 0.f || rng_state, EDGL_ERR_NULL, "edgl_tgattn_fwd: dropout without rng_state");
    TgP p = tg_params(q, u, kv, ts, ld_t, ids, omega, phi, B, T, H, C, scale, time_scale, drop_rate, rng_state, stream_id, ox, g, saved);
    p.viol = violations;
    return dtype == EDGL_F32 ? tg_launch<float>(p, 0, (hipStream_t)stream) : tg_launch<bf16>(p, 0, (hipStream_t)stream);
}

extern "C" int edgl_tgattn_bwd(const void* q, const void* u, const void* kv, const float* ts, int ld_t, const int64_t* ids,
                               const float* omega, const float* phi, const void* ox, const void* g, const void* d_ox,
                               const void* d_g, void* saved, int B, int T, int H, int C, float scale, float time_scale,
                               float drop_rate, const uint64_t* rng_state, uint32_t stream_id, void* d_q, void* d_u, void* d_kv,
                               float* d_omega, float* d_phi, float* workspace, int dtype, void* stream) {
    EDGL_REQUIRE(q && u && kv && ts && ids && omega && phi && ox && g && d_ox && d_g && saved && d_q && d_u && d_kv && d_omega &&
                     d_phi && workspace, EDGL_ERR_NULL, "edgl_tgattn_bwd: null pointer");
    if (int rc = tg_check("edgl_tgattn_bwd", B, T, H, C, ld_t, dtype)) return rc;
    EDGL_REQUIRE(time_scale > 0.f, EDGL_ERR_SHAPE, "edgl_tgattn_bwd: time_scale must be positive");
    EDGL_REQUIRE(drop_rate == 0.f || rng_state, EDGL_ERR_NULL, "edgl_tgattn_bwd: dropout without rng_state");
    TgP p = tg_params(q, u, kv, ts, ld_t, ids, omega, phi, B, T, H, C, scale, time_scale, drop_rate, rng_state, stream_id,
                      const_cast<void*>(ox), const_cast<void*>(g), saved);
    p.d_ox = d_ox; p.d_g = d_g; p.d_q = d_q; p.d_u = d_u; p.d_kv = d_kv;
    p.w4 = workspace;
    p.part_q = workspace + (long)B * T * H * 4 * C;
    p.part_k = p.part_q + (long)B * p.NWG * 2 * C;
    hipStream_t st = (hipStream_t)stream;
    const int nq = B * p.NWG, nk = (int)tg_kwgs(B, T, H);
    for (int which = 1; which <= 2; ++which)
        if (int rc = dtype == EDGL_F32 ? tg_launch<float>(p, which, st) : tg_launch<bf16>(p, which, st)) return rc;
    // partial rows of the query sweep are [d_omega | d_phi]; the key sweep adds its d_omega rows behind them
    if (int rc = edgl_reduce_rows(p.part_q, nq, C, 2L * C, d_omega, 0, st)) return rc;
    if (int rc = edgl_reduce_rows(p.part_q + C, nq, C, 2L * C, d_phi, 0, st)) return rc;
    return edgl_reduce_rows(p.part_k, nk, C, C, d_omega, 1, st);
}
