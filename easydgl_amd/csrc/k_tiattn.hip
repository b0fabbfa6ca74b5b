// K11b: attention with interval buckets — TiMultiHeadAttention.__call__ (temporal.py:36-105, TiSASRec).  The score adds
// Q[q].Ktime[dt(q,k)] and the value adds Vtime[dt(q,k)], dt = int(clip(t[q+1] - t[k], 0, timelen)) (TiSASREC.py:58-62).  The score
// term of a pair is a dh-long dot product against the gathered table row (packed bf16 dot instructions; the tables are
// L2-resident); on the value side the probabilities are binned per interval (W[q][d] += A[q,k], LDS atomics) and one MFMA chain
// applies Vtime to the bins — likewise dQ += dG . Ktime backward, and the table gradients are dG^T . Q and W^T . dO over all rows.
// The reference builds two [B,T,T,C] gathers instead.  Tile scheme, masking, softmax and dropout: tattn_common.h.
#include "tattn_common.h"

namespace {

struct TiP {
    const float* ts; float time_scale; int timelen;
    const void *ktime, *vtime; int ldt, tab_rows;     // [tab_rows, H*dh] activation dtype; bucket >= tab_rows reads as zeros
    void *wbuf, *dgbuf; int NBp;                      // [H*B*T][NBp] activation dtype: binned probabilities / score gradients
};

__device__ __forceinline__ int bucket_of(float xq1, float xk, int timelen) {
    return (int)fminf(fmaxf(xq1 - xk, 0.f), (float)timelen);                       // clip then tf.to_int64 (truncation)
}
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// The ordered form of the bin adds (TA_ORDERED): the four lanes that share a query row (same l15, g4 = 0, 4, 8, 12) take turns; in
// its turn a lane adds its four pairs to its own row with plain loads and stores, r ascending; a wave-level LDS sync ends every
// turn.  With the key tiles walked in order, a bin receives its terms by ascending key: one order, whatever the timing.
__device__ __forceinline__ void ordered_bin_add(float* row, int g4, const int (&bk)[4], const f32x4& v) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (g4 == g * 4) {
#pragma unroll
            for (int r = 0; r < 4; ++r) row[bk[r]] += v[r];
        }
        wave_lds_sync();
    }
}
// LDS tile of one wave: bins [16][NBp + 4] f32 (binned probabilities in the forward, binned score gradients backward)
__host__ __device__ constexpr size_t ti_tile_f(int NBp) { return (size_t)16 * (NBp + 4) * sizeof(float); }

// acc + <a, b> of 8 bf16 channels: packed v_dot2c_f32_bf16 (2 MACs per instruction), f32 accumulate
__device__ __forceinline__ float dot8(const uint4& a, const uint4& b, float acc) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf2;
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf2, a.x), __builtin_bit_cast(bf2, b.x), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf2, a.y), __builtin_bit_cast(bf2, b.y), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf2, a.z), __builtin_bit_cast(bf2, b.z), acc, false);
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf2, a.w), __builtin_bit_cast(bf2, b.w), acc, false);
}
// <a, b> over one head slice (16*DT channels), both rows read from global / L1: the interval term of a (query, key) pair,
// Q[q] . Ktime[bucket] or dO[q] . Vtime[bucket].
template <typename T, int DT>
__device__ __forceinline__ float dot_rows(const T* a, const T* b) {
    float acc = 0.f;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int c = 0; c < 2 * DT; ++c)
            acc = dot8(*reinterpret_cast<const uint4*>(a + c * 8), *reinterpret_cast<const uint4*>(b + c * 8), acc);
    } else {
#pragma unroll
        for (int c = 0; c < 4 * DT; ++c) {
            const float4 x = *reinterpret_cast<const float4*>(a + c * 4), y = *reinterpret_cast<const float4*>(b + c * 4);
            acc = fmaf(x.x, y.x, acc); acc = fmaf(x.y, y.y, acc); acc = fmaf(x.z, y.z, acc); acc = fmaf(x.w, y.w, acc);
        }
    }
    return acc;
}
// row of an interval table for `bucket` (clamped address; the caller zeroes the result for bucket >= tab_rows)
template <typename T>
__device__ __forceinline__ const T* tab_row(const T* tab, int ldt, int tab_rows, int bucket) {
    return tab + (long)min(bucket, tab_rows - 1) * ldt;
}
template <typename T> __device__ __forceinline__ Frag4<T> frag_from_f4(const float* p) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    return frag_from_acc<T>(f32x4{v.x, v.y, v.z, v.w});
}
// acc[dt] += sum_d tab[d][dt*16 + .]^T . Ws[row][d]   (the bucket contraction on the matrix cores)
template <typename T, int DT>
__device__ __forceinline__ void bucket_apply(const float* Ws, int LDG, const T* tab, int ldt, int tab_rows, int NBp,
                                             const Frag4<T>& ident, f32x4 (&acc)[DT], int lane) {
    const int g4 = (lane >> 4) * 4, l15 = lane & 15;
#pragma unroll 4
    for (int d0 = 0; d0 < NBp; d0 += 16) {
        const Frag4<T> bf = frag_from_f4<T>(Ws + l15 * LDG + d0 + g4);
        const int dl = d0 + l15;
        const T* trow = tab + (long)min(dl, tab_rows - 1) * ldt;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            Frag4<T> tf = frag_ld<T>(trow + dt * 16 + g4);
            if (dl >= tab_rows) tf = frag_zero<T>();
            acc[dt] = mma16(turn<T>(tf, ident), bf, acc[dt]);
        }
    }
}
template <typename T>
__device__ __forceinline__ void bucket_store(const float* Ws, int LDG, int NBp, T* dst_row, int lane) {
    const int l15 = lane & 15;
#pragma unroll 4
    for (int c = (lane >> 4) * 4; c < NBp; c += 16) frag_st<T>(dst_row + c, frag_from_f4<T>(Ws + l15 * LDG + c));
}
// Interval dot products of a key tile's four pairs for 16-wide head slices (bf16, DT = 1; at DT = 2 the batches cost a wave of occupancy): all table rows are fetched before the
// first use (clamped addresses; the caller masks out-of-table buckets) — per pair, behind `bucket < tab_rows ? .. : 0`, they
// were a branch and a wait each.  xa: this lane's row a (2*DT 16-byte vectors, loaded once); TWO: also <xb, tab2[bucket]>.
template <int DT, bool TWO>
__device__ __forceinline__ void interval_dots4(const uint4 (&xa)[2 * DT], const uint4 (&xb)[2 * DT], const bf16* tab1, const bf16* tab2,
                                               int ldt, int tab_rows, const int (&bk)[4], float (&g1)[4], float (&g2)[4]) {
    uint4 y1[4][2 * DT], y2[TWO ? 4 : 1][2 * DT];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long off = (long)min(bk[r], tab_rows - 1) * ldt;
#pragma unroll
        for (int c = 0; c < 2 * DT; ++c) {
            y1[r][c] = *reinterpret_cast<const uint4*>(tab1 + off + c * 8);
            if constexpr (TWO) y2[r][c] = *reinterpret_cast<const uint4*>(tab2 + off + c * 8);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 2 * DT; ++c) {
            asm volatile("" : "+v"(y1[r][c].x), "+v"(y1[r][c].y), "+v"(y1[r][c].z), "+v"(y1[r][c].w));
            if constexpr (TWO) asm volatile("" : "+v"(y2[r][c].x), "+v"(y2[r][c].y), "+v"(y2[r][c].z), "+v"(y2[r][c].w));
        }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int c = 0; c < 2 * DT; ++c) {
            a1 = dot8(xa[c], y1[r][c], a1);
            if constexpr (TWO) a2 = dot8(xb[c], y2[r][c], a2);
        }
        g1[r] = a1; g2[r] = a2;
    }
}

// ... the same with a different left row per pair (the key-side backward: rows of four queries against their buckets' rows)
template <int DT>
__device__ __forceinline__ void interval_dots4_rows(const bf16* a0, long lda, const int (&arow)[4], const bf16* tab, int ldt,
                                                    int tab_rows, const int (&bk)[4], float (&g)[4]) {
    uint4 x[4][2 * DT], y[4][2 * DT];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long off = (long)min(bk[r], tab_rows - 1) * ldt;
#pragma unroll
        for (int c = 0; c < 2 * DT; ++c) {
            x[r][c] = *reinterpret_cast<const uint4*>(a0 + (long)arow[r] * lda + c * 8);
            y[r][c] = *reinterpret_cast<const uint4*>(tab + off + c * 8);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 2 * DT; ++c) {
            asm volatile("" : "+v"(x[r][c].x), "+v"(x[r][c].y), "+v"(x[r][c].z), "+v"(x[r][c].w));
            asm volatile("" : "+v"(y[r][c].x), "+v"(y[r][c].y), "+v"(y[r][c].z), "+v"(y[r][c].w));
        }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < 2 * DT; ++c) acc = dot8(x[r][c], y[r][c], acc);
        g[r] = acc;
    }
}

template <typename T, int DT, bool ORD = false>
__global__ __launch_bounds__(256) void tiattn_fwd_kernel(TaP p, TiP t) {
    extern __shared__ __attribute__((aligned(16))) char lds_c[];
    Job j;
    if (!get_job(p, j)) return;
    constexpr int dh = 16 * DT;
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15, LDG = t.NBp + 4;
    float* Ws = reinterpret_cast<float*>(lds_c + (size_t)(threadIdx.x >> 6) * ti_tile_f(t.NBp));
    const int q = j.tile * 16 + l15, qc = min(q, p.T - 1);
    const bool qok = q < p.T, causal = (p.flags & TA_CAUSAL) != 0;
    const T* Qr = reinterpret_cast<const T*>(p.qx) + ((long)j.b * p.T + qc) * p.ldq + j.head * dh;
    const T* Kb = reinterpret_cast<const T*>(p.kx) + (long)j.b * p.T * p.ldk + j.head * dh;
    const T* Vb = reinterpret_cast<const T*>(p.v) + (long)j.b * p.T * p.ldv + j.head * dh;
    const T* Kt = reinterpret_cast<const T*>(t.ktime) + j.head * dh;
    const T* Vt = reinterpret_cast<const T*>(t.vtime) + j.head * dh;
    const int64_t* idr = p.ids + (long)j.b * p.T;
    const float* tsr = t.ts + (long)j.b * (p.T + 1);
    const float xq1 = tsr[qc + 1] / t.time_scale;                                         // TiSASREC.py:49
    const DropKey dk = make_dropkey(p.rng, p.stream_id, p.rate);
    const Frag4<T> ident = identity_frag<T>(lane);
    const uint32_t dbase = (uint32_t)((j.bp * p.T + qc) * p.T);
    const int kt_end = (causal && j.tile * 16 >= first_unpadded(idr, p.T, lane)) ? j.tile + 1 : p.NT;
    for (int i = lane * 4; i < 16 * LDG; i += 256) *reinterpret_cast<float4*>(Ws + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    wave_lds_sync();
    Frag4<T> qf[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) qf[dt] = frag_ld<T>(Qr + dt * 16 + g4);
    uint4 qrow[(sizeof(T) == 2 && DT == 1) ? 2 * DT : 1];   // bf16: this lane's query row (one head slice), kept for the interval dot products
    if constexpr (sizeof(T) == 2 && DT == 1) {
#pragma unroll
        for (int c = 0; c < 2 * DT; ++c) qrow[c] = *reinterpret_cast<const uint4*>(Qr + c * 8);
    }
    // The interval term of a pair hangs on two dependent loads (timestamp -> bucket -> table row).  Written per pair — with the
    // table row behind `bucket < tab_rows ? .. : 0` — that is a branch and two waits per pair: 8 dependent round trips per key
    // tile.  Here the four timestamps / ids of a tile travel together, then the four table rows (clamped, unconditional).
    auto scores = [&](int kt, float (&x)[4], int (&bk)[4]) {
        const int kr = min(kt * 16 + l15, p.T - 1);
        if constexpr (!(sizeof(T) == 2 && DT == 1)) {       // wide head slices / f32: per pair (four rows do not fit in registers)
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) s = mma16(frag_ld<T>(Kb + (long)kr * p.ldk + dt * 16 + g4), qf[dt], s);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = kt * 16 + g4 + r, kcl = min(k, p.T - 1);
                bk[r] = bucket_of(xq1, tsr[kcl] / t.time_scale, t.timelen);
                const float madd = k >= p.T ? -INFINITY : (idr[kcl] == 0 ? PADV : 0.f);
                const float g = bk[r] < t.tab_rows ? dot_rows<T, DT>(Qr, tab_row<T>(Kt, t.ldt, t.tab_rows, bk[r])) : 0.f;   // temporal.py:58
                float v = fmaf(s[r] + g, p.cscale, madd);                                     // temporal.py:56-62
                if (causal && k > q && k < p.T) v = PADV;
                x[r] = v;
            }
            return;
        }
        float tsk[4];
        int64_t idk[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kcl = min(kt * 16 + g4 + r, p.T - 1);
            tsk[r] = tsr[kcl]; idk[r] = idr[kcl];
        }
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) s = mma16(frag_ld<T>(Kb + (long)kr * p.ldk + dt * 16 + g4), qf[dt], s);
        const T* rowp[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            bk[r] = bucket_of(xq1, tsk[r] / t.time_scale, t.timelen);
            rowp[r] = tab_row<T>(Kt, t.ldt, t.tab_rows, bk[r]);
        }
        float g[4];
        if constexpr (sizeof(T) == 2 && DT == 1) {     // (wider head slices: the four rows no longer fit in registers)
            uint4 y[4][2 * DT];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 2 * DT; ++c) y[r][c] = *reinterpret_cast<const uint4*>(rowp[r] + c * 8);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 2 * DT; ++c) asm volatile("" : "+v"(y[r][c].x), "+v"(y[r][c].y), "+v"(y[r][c].z), "+v"(y[r][c].w));
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float acc = 0.f;
#pragma unroll
                for (int c = 0; c < 2 * DT; ++c) acc = dot8(qrow[c], y[r][c], acc);
                g[r] = acc;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = kt * 16 + g4 + r;
            const float madd = k >= p.T ? -INFINITY : (idk[r] == 0 ? PADV : 0.f);
            const float gi = bk[r] < t.tab_rows ? g[r] : 0.f;                            // temporal.py:58
            float v = fmaf(s[r] + gi, p.cscale, madd);                                    // temporal.py:56-62
            if (causal && k > q && k < p.T) v = PADV;
            x[r] = v;
        }
    };
    // pass 1: scores of every key tile, kept in registers for pass 2 (LDS, not registers, bounds the occupancy here, and the
    // second pass would otherwise repeat the S MFMA and the dependent timestamp -> bucket -> table-row loads of each pair)
    constexpr int NTM = 16;                   // T <= 256 (host-checked)
    float xs[NTM][4];
    float m = -INFINITY, l = 0.f;
#pragma unroll
    for (int kt = 0; kt < NTM; ++kt) {
        if (kt < kt_end) {
            float x[4]; int bk[4];
            scores(kt, x, bk);
#pragma unroll
            for (int r = 0; r < 4; ++r) xs[kt][r] = x[r];
            const float tmax = group_max4(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
            const float m_new = fmaxf(m, tmax);
            const float ps = __expf(x[0] - m_new) + __expf(x[1] - m_new) + __expf(x[2] - m_new) + __expf(x[3] - m_new);
            l = l * __expf(m - m_new) + group_sum4(ps);
            m = m_new;
        }
    }
    const float invl = 1.0f / l;
    f32x4 acc[DT];
#pragma unroll
    for (int ut = 0; ut < DT; ++ut) acc[ut] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NTM; ++kt) {
        if (kt < kt_end) {
            const int kr = min(kt * 16 + l15, p.T - 1);
            uint32_t h0 = 0xffffffffu, h1 = 0xffffffffu;
            if (dk.thresh != 0u) { h0 = drop_hash_pair(dk, dbase + kt * 16 + g4); h1 = drop_hash_pair(dk, dbase + kt * 16 + g4 + 2); }
            const uint32_t hb[4] = {h0 & 0xffffu, h0 >> 16, h1 & 0xffffu, h1 >> 16};
            f32x4 a4;
            int bko[ORD ? 4 : 1];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kcl = min(kt * 16 + g4 + r, p.T - 1);
                const int bk = bucket_of(xq1, tsr[kcl] / t.time_scale, t.timelen);
                const float P = __expf(xs[kt][r] - m) * invl;
                a4[r] = (dk.thresh == 0u || hb[r] >= dk.t16) ? P * dk.scale : 0.f;            // temporal.py:90
                if constexpr (ORD) bko[r] = bk;
                else atomicAdd(&Ws[l15 * LDG + bk], a4[r]);
            }
            if constexpr (ORD) ordered_bin_add(Ws + l15 * LDG, g4, bko, a4);
            const Frag4<T> pf = frag_from_acc<T>(a4);
#pragma unroll
            for (int ut = 0; ut < DT; ++ut)
                acc[ut] = mma16(turn<T>(frag_ld<T>(Vb + (long)kr * p.ldv + ut * 16 + g4), ident), pf, acc[ut]);   // :93-94
        }
    }
    wave_lds_sync();
    bucket_apply<T, DT>(Ws, LDG, Vt, t.ldt, t.tab_rows, t.NBp, ident, acc, lane);                               // :95
    if (t.wbuf && qok) bucket_store<T>(Ws, LDG, t.NBp, reinterpret_cast<T*>(t.wbuf) + (j.bp * p.T + q) * (long)t.NBp, lane);
    if (p.st_m && qok && g4 == 0) { p.st_m[j.bp * p.T + q] = m; p.st_l[j.bp * p.T + q] = l; }
    if (!qok) return;
    const long orow = (long)j.b * p.T + q;
#pragma unroll
    for (int ut = 0; ut < DT; ++ut) {
        const int col = j.head * dh + ut * 16 + g4;
        f32x4 o = acc[ut];
        if (p.oatt) *reinterpret_cast<float4*>(p.oatt + orow * ((long)p.H * dh) + col) = make_float4(o[0], o[1], o[2], o[3]);
        const Frag4<T> rf = frag_ld<T>(reinterpret_cast<const T*>(p.resid) + orow * p.ldr + col);
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] += to_f32(rf.v[r]);                                                    // :102-104
        frag_st<T>(reinterpret_cast<T*>(p.out) + orow * p.ldo + col, frag_from_acc<T>(o));
    }
}

template <typename T, int DT, bool ORD = false>
__global__ __launch_bounds__(256) void tiattn_bwd_q_kernel(TaP p, TiP t) {
    extern __shared__ __attribute__((aligned(16))) char lds_c[];
    Job j;
    if (!get_job(p, j)) return;
    constexpr int dh = 16 * DT;
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15, LDG = t.NBp + 4;
    float* dGs = reinterpret_cast<float*>(lds_c + (size_t)(threadIdx.x >> 6) * ti_tile_f(t.NBp));
    const int q = j.tile * 16 + l15, qc = min(q, p.T - 1);
    const bool qok = q < p.T, causal = (p.flags & TA_CAUSAL) != 0;
    const T* Qr = reinterpret_cast<const T*>(p.qx) + ((long)j.b * p.T + qc) * p.ldq + j.head * dh;
    const T* Kb = reinterpret_cast<const T*>(p.kx) + (long)j.b * p.T * p.ldk + j.head * dh;
    const T* Vb = reinterpret_cast<const T*>(p.v) + (long)j.b * p.T * p.ldv + j.head * dh;
    const T* dOr = reinterpret_cast<const T*>(p.d_out) + ((long)j.b * p.T + qc) * p.ld_do + j.head * dh;
    const T* Kt = reinterpret_cast<const T*>(t.ktime) + j.head * dh;
    const T* Vt = reinterpret_cast<const T*>(t.vtime) + j.head * dh;
    const int64_t* idr = p.ids + (long)j.b * p.T;
    const float* tsr = t.ts + (long)j.b * (p.T + 1);
    const float xq1 = tsr[qc + 1] / t.time_scale;
    const DropKey dk = make_dropkey(p.rng, p.stream_id, p.rate);
    const Frag4<T> ident = identity_frag<T>(lane);
    const uint32_t dbase = (uint32_t)((j.bp * p.T + qc) * p.T);
    const int kt_end = (causal && j.tile * 16 >= first_unpadded(idr, p.T, lane)) ? j.tile + 1 : p.NT;
    for (int i = lane * 4; i < 16 * LDG; i += 256) *reinterpret_cast<float4*>(dGs + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    float dsum = 0.f;
    Frag4<T> qf[DT], gf[DT];
    {
        const float* oa = p.oatt + ((long)j.b * p.T + qc) * ((long)p.H * dh) + j.head * dh;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            qf[dt] = frag_ld<T>(Qr + dt * 16 + g4);
            gf[dt] = frag_ld<T>(dOr + dt * 16 + g4);
            const float4 o = *reinterpret_cast<const float4*>(oa + dt * 16 + g4);
            dsum += to_f32(gf[dt].v[0]) * o.x + to_f32(gf[dt].v[1]) * o.y + to_f32(gf[dt].v[2]) * o.z + to_f32(gf[dt].v[3]) * o.w;
        }
        dsum = group_sum4(dsum);
        if (qok && g4 == 0) p.st_d[j.bp * p.T + q] = dsum;
    }
    const float m = p.st_m[j.bp * p.T + qc], invl = 1.0f / p.st_l[j.bp * p.T + qc];
    constexpr bool NARROW = sizeof(T) == 2 && DT == 1;      // interval dots with batched table rows (interval_dots4)
    uint4 qrow[NARROW ? 2 * DT : 1], dorow[NARROW ? 2 * DT : 1];
    if constexpr (NARROW) {
#pragma unroll
        for (int c = 0; c < 2 * DT; ++c) { qrow[c] = *reinterpret_cast<const uint4*>(Qr + c * 8); dorow[c] = *reinterpret_cast<const uint4*>(dOr + c * 8); }
    }
    wave_lds_sync();
    f32x4 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int kt = 0; kt < kt_end; ++kt) {
        const int kr = min(kt * 16 + l15, p.T - 1);
        f32x4 s = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            s = mma16(frag_ld<T>(Kb + (long)kr * p.ldk + dt * 16 + g4), qf[dt], s);
            da = mma16(frag_ld<T>(Vb + (long)kr * p.ldv + dt * 16 + g4), gf[dt], da);
        }
        uint32_t h0 = 0xffffffffu, h1 = 0xffffffffu;
        if (dk.thresh != 0u) { h0 = drop_hash_pair(dk, dbase + kt * 16 + g4); h1 = drop_hash_pair(dk, dbase + kt * 16 + g4 + 2); }
        const uint32_t hb[4] = {h0 & 0xffffu, h0 >> 16, h1 & 0xffffu, h1 >> 16};
        f32x4 ds;
        float tsk[4];
        int64_t idk[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kcl = min(kt * 16 + g4 + r, p.T - 1);
            tsk[r] = tsr[kcl]; idk[r] = idr[kcl];
        }
        int bks[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) bks[r] = bucket_of(xq1, tsk[r] / t.time_scale, t.timelen);
        float gq[4], gd[4];
        if constexpr (NARROW) {
            interval_dots4<DT, true>(qrow, dorow, reinterpret_cast<const bf16*>(Kt), reinterpret_cast<const bf16*>(Vt), t.ldt, t.tab_rows,
                                     bks, gq, gd);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool inb = bks[r] < t.tab_rows;
                gq[r] = inb ? dot_rows<T, DT>(Qr, tab_row<T>(Kt, t.ldt, t.tab_rows, bks[r])) : 0.f;
                gd[r] = inb ? dot_rows<T, DT>(dOr, tab_row<T>(Vt, t.ldt, t.tab_rows, bks[r])) : 0.f;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = kt * 16 + g4 + r;
            const int bk = bks[r];
            const bool pad = k >= p.T || idk[r] == 0, fut = causal && k > q;
            const bool inb = bk < t.tab_rows;
            const float g = inb ? gq[r] : 0.f;
            const float dw = inb ? gd[r] : 0.f;                                                          // dA[q,k] gets dO[q].Vtime[dt(q,k)]
            float v = fmaf(s[r] + g, p.cscale, k >= p.T ? -INFINITY : (pad ? PADV : 0.f));
            if (fut && k < p.T) v = PADV;
            const float P = __expf(v - m) * invl;
            const float dP = (dk.thresh == 0u || hb[r] >= dk.t16) ? (da[r] + dw) * dk.scale : 0.f;
            ds[r] = (pad || fut || !qok) ? 0.f : P * (dP - dsum) * p.cscale;
            if constexpr (!ORD) atomicAdd(&dGs[l15 * LDG + bk], ds[r]);
        }
        if constexpr (ORD) ordered_bin_add(dGs + l15 * LDG, g4, bks, ds);
        const Frag4<T> dsf = frag_from_acc<T>(ds);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
            acc[dt] = mma16(turn<T>(frag_ld<T>(Kb + (long)kr * p.ldk + dt * 16 + g4), ident), dsf, acc[dt]);
    }
    wave_lds_sync();
    bucket_apply<T, DT>(dGs, LDG, Kt, t.ldt, t.tab_rows, t.NBp, ident, acc, lane);   // dQ[q] += sum_d dG[q][d] Ktime[d]
    if (qok) bucket_store<T>(dGs, LDG, t.NBp, reinterpret_cast<T*>(t.dgbuf) + (j.bp * p.T + q) * (long)t.NBp, lane);
    if (!qok) return;
    T* dst = reinterpret_cast<T*>(p.d_qx) + ((long)j.b * p.T + q) * p.ld_dq + j.head * dh;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) frag_st<T>(dst + dt * 16 + g4, frag_from_acc<T>(acc[dt]));
}

template <typename T, int DT>
__global__ __launch_bounds__(256) void tiattn_bwd_k_kernel(TaP p, TiP t) {
    Job j;
    if (!get_job(p, j)) return;
    constexpr int dh = 16 * DT;
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15;
    const int k = j.tile * 16 + l15, kc = min(k, p.T - 1);
    const bool kok = k < p.T, causal = (p.flags & TA_CAUSAL) != 0;
    const T* Qb = reinterpret_cast<const T*>(p.qx) + (long)j.b * p.T * p.ldq + j.head * dh;
    const T* Kr = reinterpret_cast<const T*>(p.kx) + ((long)j.b * p.T + kc) * p.ldk + j.head * dh;
    const T* Vr = reinterpret_cast<const T*>(p.v) + ((long)j.b * p.T + kc) * p.ldv + j.head * dh;
    const T* dOb = reinterpret_cast<const T*>(p.d_out) + (long)j.b * p.T * p.ld_do + j.head * dh;
    const T* Kt = reinterpret_cast<const T*>(t.ktime) + j.head * dh;
    const T* Vt = reinterpret_cast<const T*>(t.vtime) + j.head * dh;
    const float* tsr = t.ts + (long)j.b * (p.T + 1);
    const float xk = tsr[kc] / t.time_scale;
    const bool pad = !kok || p.ids[(long)j.b * p.T + kc] == 0;
    const float madd = !kok ? -INFINITY : (pad ? PADV : 0.f);
    const DropKey dk = make_dropkey(p.rng, p.stream_id, p.rate);
    const Frag4<T> ident = identity_frag<T>(lane);
    const int fnp = first_unpadded(p.ids + (long)j.b * p.T, p.T, lane);
    Frag4<T> kf[DT], vf[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) { kf[dt] = frag_ld<T>(Kr + dt * 16 + g4); vf[dt] = frag_ld<T>(Vr + dt * 16 + g4); }
    f32x4 accK[DT], accV[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) { accK[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; accV[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll 2
    for (int qt = 0; qt < p.NT; ++qt) {
        if (causal && qt < j.tile && qt * 16 >= fnp) continue;
        const int ql = min(qt * 16 + l15, p.T - 1);
        const T* Qrow = Qb + (long)ql * p.ldq;
        const T* dOrow = dOb + (long)ql * p.ld_do;
        f32x4 s = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
        Frag4<T> qf[DT], gf[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            qf[dt] = frag_ld<T>(Qrow + dt * 16 + g4);
            gf[dt] = frag_ld<T>(dOrow + dt * 16 + g4);
            s = mma16(qf[dt], kf[dt], s);
            da = mma16(gf[dt], vf[dt], da);
        }
        // interval terms of the 4 (q, k) pairs of this lane
        float gq[4], dwq[4];
        int qcs[4], bks[4];
        float tsq[4], stm[4], stl[4], std_[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {      // per-query scalars of the tile: one batch (unconditional, clamped rows)
            qcs[r] = min(qt * 16 + g4 + r, p.T - 1);
            const long si = j.bp * p.T + qcs[r];
            tsq[r] = tsr[qcs[r] + 1]; stm[r] = p.st_m[si]; stl[r] = p.st_l[si]; std_[r] = p.st_d[si];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) bks[r] = bucket_of(tsq[r] / t.time_scale, xk, t.timelen);
        if constexpr (sizeof(T) == 2 && DT == 1) {
            interval_dots4_rows<DT>(reinterpret_cast<const bf16*>(Qb), p.ldq, qcs, reinterpret_cast<const bf16*>(Kt), t.ldt, t.tab_rows, bks, gq);
            interval_dots4_rows<DT>(reinterpret_cast<const bf16*>(dOb), p.ld_do, qcs, reinterpret_cast<const bf16*>(Vt), t.ldt, t.tab_rows, bks, dwq);
#pragma unroll
            for (int r = 0; r < 4; ++r) { const bool inb = bks[r] < t.tab_rows; gq[r] = inb ? gq[r] : 0.f; dwq[r] = inb ? dwq[r] : 0.f; }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool inb = bks[r] < t.tab_rows;
                gq[r] = inb ? dot_rows<T, DT>(Qb + (long)qcs[r] * p.ldq, tab_row<T>(Kt, t.ldt, t.tab_rows, bks[r])) : 0.f;
                dwq[r] = inb ? dot_rows<T, DT>(dOb + (long)qcs[r] * p.ld_do, tab_row<T>(Vt, t.ldt, t.tab_rows, bks[r])) : 0.f;
            }
        }
        f32x4 a4, ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = qt * 16 + g4 + r;
            const long si = j.bp * p.T + qcs[r];
            const bool fut = causal && k > q;
            float v = fmaf(s[r] + gq[r], p.cscale, madd);
            if (fut && kok) v = PADV;
            const float P = (q < p.T) ? __expf(v - stm[r]) / stl[r] : 0.f;
            bool keep = true;
            if (dk.thresh != 0u) {
                const uint32_t h = drop_hash_pair(dk, (uint32_t)(si * p.T) + (uint32_t)(k & ~1));
                keep = ((k & 1) ? (h >> 16) : (h & 0xffffu)) >= dk.t16;
            }
            a4[r] = keep ? P * dk.scale : 0.f;
            const float dP = keep ? (da[r] + dwq[r]) * dk.scale : 0.f;
            ds[r] = (pad || fut || q >= p.T) ? 0.f : P * (dP - std_[r]) * p.cscale;
        }
        const Frag4<T> af = frag_from_acc<T>(a4), dsf = frag_from_acc<T>(ds);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            accV[dt] = mma16(turn<T>(gf[dt], ident), af, accV[dt]);
            accK[dt] = mma16(turn<T>(qf[dt], ident), dsf, accK[dt]);
        }
    }
    if (!kok) return;
    T* dK = reinterpret_cast<T*>(p.d_kx) + ((long)j.b * p.T + k) * p.ld_dk + j.head * dh;
    T* dV = reinterpret_cast<T*>(p.d_v) + ((long)j.b * p.T + k) * p.ld_dv + j.head * dh;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) { frag_st<T>(dK + dt * 16 + g4, frag_from_acc<T>(accK[dt])); frag_st<T>(dV + dt * 16 + g4, frag_from_acc<T>(accV[dt])); }
}

// d_tab[d][head*dh + u] += sum_r Wb[head*BT + r][d] * X[r][head*dh + u]: the interval-table gradients
//   d(Ktime) = dG^T . Q,  d(Vtime) = W^T . dO   (contraction over all B*T rows; f32 atomics of per-split partial tiles)
// SLAB: d_tab is [splits][tab_rows][ldt] and every split stores its partial tile into its own slab — each element
// has one writer — for bucket_dtable_sum_kernel to add up in split order.
template <typename T, bool SLAB = false>
__global__ __launch_bounds__(256) void bucket_dtable_kernel(const T* Wb, int NBp, const T* X, int ldx, long BT, int H, int dh,
                                                            int tab_rows, float* d_tab, int ldt, int splits) {
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15;
    const int ndt = NBp / 16, nut = dh / 16;
    long job = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (job >= (long)H * ndt * nut * splits) return;
    const int sp = (int)(job % splits); job /= splits;
    const int ut = (int)(job % nut); job /= nut;
    const int dti = (int)(job % ndt);
    const int head = (int)(job / ndt);
    const Frag4<T> ident = identity_frag<T>(lane);
    const long ntile = (BT + 15) / 16, per = (ntile + splits - 1) / splits;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (long rt = sp * per; rt < min(ntile, (sp + 1) * per); ++rt) {
        const long r = rt * 16 + l15, rc = min(r, BT - 1);
        Frag4<T> wf = frag_ld<T>(Wb + ((long)head * BT + rc) * NBp + dti * 16 + g4);
        if (r >= BT) wf = frag_zero<T>();
        const Frag4<T> xf = frag_ld<T>(X + rc * ldx + head * dh + ut * 16 + g4);
        acc = mma16(turn<T>(wf, ident), turn<T>(xf, ident), acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int d = dti * 16 + g4 + r;
        if constexpr (SLAB) {
            if (d < tab_rows) d_tab[((long)sp * tab_rows + d) * ldt + head * dh + ut * 16 + l15] = acc[r];
        } else {
            if (d < tab_rows) atomicAdd(d_tab + (long)d * ldt + head * dh + ut * 16 + l15, acc[r]);
        }
    }
}
// d_ktime | d_vtime [n4 float4 each] = the sum of their `splits` slabs (slabs: [2][splits][n4]) in split order; one writer per element
__global__ __launch_bounds__(256) void bucket_dtable_sum_kernel(const float4* slabs, long n4, int splits, float4* d_ktime, float4* d_vtime) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= 2 * n4) return;
    const int tab = gid >= n4;
    const long e = gid - tab * n4;
    const float4* src = slabs + (long)tab * splits * n4 + e;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s0 = 0; s0 < splits; s0 += 8) {
        float4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = src[(long)min(s0 + k, splits - 1) * n4];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (s0 + k >= splits) break;
            a.x += v[k].x; a.y += v[k].y; a.z += v[k].z; a.w += v[k].w;
        }
    }
    (tab ? d_vtime : d_ktime)[e] = a;
}

template <typename T>
__global__ __launch_bounds__(256) void add_pos2_kernel(const T* kv, const float* posK, const float* posV, T* out, long rows, int T_, int C) {
    const int cpr = (2 * C) >> 2;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long row = gid / cpr;
    if (row >= rows) return;
    const int c0 = (int)(gid % cpr) * 4, tpos = (int)(row % T_);
    const Frag4<T> v = frag_ld<T>(kv + row * 2 * C + c0);
    const float4 pp = *reinterpret_cast<const float4*>((c0 < C ? posK + (long)tpos * C + c0 : posV + (long)tpos * C + c0 - C));
    Frag4<T> o;
    o.v[0] = from_f32<T>(to_f32(v.v[0]) + pp.x); o.v[1] = from_f32<T>(to_f32(v.v[1]) + pp.y);
    o.v[2] = from_f32<T>(to_f32(v.v[2]) + pp.z); o.v[3] = from_f32<T>(to_f32(v.v[3]) + pp.w);
    frag_st<T>(out + row * 2 * C + c0, o);
}

// four waves per block, `wave_bytes` of LDS each
template <typename K>
int launch_ti(K kern, const TaP& p, const TiP& t, size_t wave_bytes, hipStream_t st) {
    const size_t smem = 4 * wave_bytes;
    EDGL_REQUIRE(smem <= 160 * 1024, EDGL_ERR_SHAPE, "edgl_tiattn: timelen %d needs %zu B of LDS", t.timelen, smem);
    EDGL_LDS_LIMIT(kern, smem, "edgl_tiattn");
    return launch_jobs(kern, p, 1, 4, smem, st, t);
}
constexpr int TI_SPLITS = 32;      // row splits of the interval-table gradients
template <typename T, int DT>
int ti_fwd(const TaP& p, const TiP& t, hipStream_t st) {
    if (p.flags & TA_ORDERED) return launch_ti(tiattn_fwd_kernel<T, DT, true>, p, t, ti_tile_f(t.NBp), st);
    return launch_ti(tiattn_fwd_kernel<T, DT>, p, t, ti_tile_f(t.NBp), st);
}
// d(Ktime) = dG^T . Q and d(Vtime) = W^T . dO over all rows, into dst_k / dst_v
template <typename T, int DT, bool SLAB>
int ti_dtables(const TaP& p, const TiP& t, float* dst_k, float* dst_v, hipStream_t st) {
    const long jobs = (long)p.H * (t.NBp / 16) * DT * TI_SPLITS, BT = (long)p.B * p.T;
    const dim3 grid((unsigned)((jobs + 3) / 4));
    hipLaunchKernelGGL((bucket_dtable_kernel<T, SLAB>), grid, dim3(256), 0, st, reinterpret_cast<const T*>(t.dgbuf), t.NBp,
                       reinterpret_cast<const T*>(p.qx), p.ldq, BT, p.H, 16 * DT, t.tab_rows, dst_k, t.ldt, TI_SPLITS);
    EDGL_LAUNCH_CHECK();
    hipLaunchKernelGGL((bucket_dtable_kernel<T, SLAB>), grid, dim3(256), 0, st, reinterpret_cast<const T*>(t.wbuf), t.NBp,
                       reinterpret_cast<const T*>(p.d_out), p.ld_do, BT, p.H, 16 * DT, t.tab_rows, dst_v, t.ldt, TI_SPLITS);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
// Both sweeps, then the table gradients: f32 atomics into the zeroed d_ktime / d_vtime, or — the deterministic form, with the
// slab workspace `ws` — every row split stores its partial tile to a slab of its own and one more launch adds the slabs in order.
template <typename T, int DT>
int ti_bwd(const TaP& p, const TiP& t, float* d_ktime, float* d_vtime, float* ws, hipStream_t st) {
    if (p.flags & TA_ORDERED) {
        if (int rc = launch_ti(tiattn_bwd_q_kernel<T, DT, true>, p, t, ti_tile_f(t.NBp), st)) return rc;
    } else if (int rc = launch_ti(tiattn_bwd_q_kernel<T, DT>, p, t, ti_tile_f(t.NBp), st)) return rc;
    if (int rc = launch_ti(tiattn_bwd_k_kernel<T, DT>, p, t, 0, st)) return rc;
    const long n = (long)t.tab_rows * t.ldt;
    if (ws) {
        if (int rc = ti_dtables<T, DT, true>(p, t, ws, ws + TI_SPLITS * n, st)) return rc;
        hipLaunchKernelGGL(bucket_dtable_sum_kernel, dim3((unsigned)((2 * (n / 4) + 255) / 256)), dim3(256), 0, st,
                           reinterpret_cast<const float4*>(ws), n / 4, TI_SPLITS, reinterpret_cast<float4*>(d_ktime),
                           reinterpret_cast<float4*>(d_vtime));
        EDGL_LAUNCH_CHECK();
        return EDGL_OK;
    }
    if (hipMemsetAsync(d_ktime, 0, n * sizeof(float), st) != hipSuccess || hipMemsetAsync(d_vtime, 0, n * sizeof(float), st) != hipSuccess) {
        edgl_set_error("edgl_tiattn_bwd: memset failed");
        return EDGL_ERR_LAUNCH;
    }
    return ti_dtables<T, DT, false>(p, t, d_ktime, d_vtime, st);
}
int ti_check(const char* who, int B, int T, int H, int dh, int timelen, int tab_rows, int dtype) {
    EDGL_REQUIRE(B > 0 && T > 0 && H > 0 && (dh == 16 || dh == 32 || dh == 64 || dh == 128), EDGL_ERR_SHAPE,
                 "%s: bad shape B=%d T=%d H=%d head dim %d (16, 32, 64 or 128)", who, B, T, H, dh);
    EDGL_REQUIRE(timelen >= 1 && timelen <= 256 && tab_rows >= 1 && tab_rows <= timelen + 1, EDGL_ERR_SHAPE,
                 "%s: timelen %d (1..256) / table rows %d not supported", who, timelen, tab_rows);
    EDGL_REQUIRE(T <= 256, EDGL_ERR_SHAPE, "%s: T=%d not supported (T <= 256: 16 key tiles are kept in registers)", who, T);
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "%s: bad dtype %d", who, dtype);
    EDGL_REQUIRE((double)B * H * T * T < 4294967296.0, EDGL_ERR_SHAPE, "%s: H*B*T*T must be < 2^32", who);
    return EDGL_OK;
}
}  // namespace

extern "C" long edgl_tiattn_bucket_elems(int B, int T, int H, int timelen) {
    if (B <= 0 || T <= 0 || H <= 0 || timelen < 1) return -1;
    return (long)B * T * H * ((timelen + 1 + 15) / 16 * 16);
}

extern "C" int edgl_tiattn_fwd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* resid, int ldr,
                               const int64_t* ids, const float* ts, const void* ktime, const void* vtime, int tab_rows, int B,
                               int T, int H, int dh, float scale, float time_scale, int timelen, float drop_rate,
                               const uint64_t* rng_state, uint32_t stream_id, void* out, int ldo, void* saved, void* wbuf,
                               int flags, int dtype, void* stream) {
    EDGL_REQUIRE(q && k && v && resid && ids && ts && ktime && vtime && out, EDGL_ERR_NULL, "edgl_tiattn_fwd: null pointer");
    if (int rc = ti_check("edgl_tiattn_fwd", B, T, H, dh, timelen, tab_rows, dtype)) return rc;
    EDGL_REQUIRE(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldr % 4 == 0 && ldo % 4 == 0, EDGL_ERR_SHAPE,
                 "edgl_tiattn_fwd: row strides must be multiples of 4");
    EDGL_REQUIRE(drop_rate == 0.f || rng_state, EDGL_ERR_NULL, "edgl_tiattn_fwd: dropout without rng_state");
    EDGL_REQUIRE((saved != nullptr) == (wbuf != nullptr), EDGL_ERR_NULL, "edgl_tiattn_fwd: saved and wbuf go together");
    TaP p = ta_params(q, ldq, k, ldk, v, ldv, ids, B, T, H, dh, dh, scale, drop_rate, rng_state, stream_id, saved, flags);
    p.resid = resid; p.ldr = ldr; p.out = out; p.ldo = ldo;
    TiP t{ts, time_scale, timelen, ktime, vtime, H * dh, tab_rows, wbuf, nullptr, (timelen + 1 + 15) / 16 * 16};
    hipStream_t st = (hipStream_t)stream;
#define EDGL_TI_FWD(TT)                                        \
    switch (dh / 16) {                                         \
        case 1: return ti_fwd<TT, 1>(p, t, st);                \
        case 2: return ti_fwd<TT, 2>(p, t, st);                \
        case 4: return ti_fwd<TT, 4>(p, t, st);                \
        default: return ti_fwd<TT, 8>(p, t, st);               \
    }
    if (dtype == EDGL_F32) { EDGL_TI_FWD(float) }
    EDGL_TI_FWD(bf16)
#undef EDGL_TI_FWD
}

// edgl_tiattn_bwd (det_ws == nullptr) and edgl_tiattn_bwd_det (the slab workspace of the ordered table gradients)
static int tiattn_bwd_any(const char* who, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const int64_t* ids,
                          const float* ts, const void* ktime, const void* vtime, int tab_rows, const void* d_out, int ld_do,
                          void* saved, void* wbuf, int B, int T, int H, int dh, float scale, float time_scale, int timelen,
                          float drop_rate, const uint64_t* rng_state, uint32_t stream_id, void* d_q, int ld_dq, void* d_k,
                          int ld_dk, void* d_v, int ld_dv, void* dgbuf, float* d_ktime, float* d_vtime, float* det_ws, int flags,
                          int dtype, void* stream) {
    EDGL_REQUIRE(q && k && v && ids && ts && ktime && vtime && d_out && saved && wbuf && d_q && d_k && d_v && dgbuf && d_ktime &&
                     d_vtime, EDGL_ERR_NULL, "%s: null pointer", who);
    if (int rc = ti_check(who, B, T, H, dh, timelen, tab_rows, dtype)) return rc;
    EDGL_REQUIRE(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ld_do % 4 == 0 && ld_dq % 4 == 0 && ld_dk % 4 == 0 && ld_dv % 4 == 0,
                 EDGL_ERR_SHAPE, "%s: row strides must be multiples of 4", who);
    EDGL_REQUIRE(drop_rate == 0.f || rng_state, EDGL_ERR_NULL, "%s: dropout without rng_state", who);
    EDGL_REQUIRE(!det_ws || (((uintptr_t)det_ws | (uintptr_t)d_ktime | (uintptr_t)d_vtime) & 15) == 0, EDGL_ERR_SHAPE,
                 "%s: workspace, d_ktime and d_vtime must be 16-byte aligned", who);
    TaP p = ta_params(q, ldq, k, ldk, v, ldv, ids, B, T, H, dh, dh, scale, drop_rate, rng_state, stream_id, saved, flags);
    p.d_out = d_out; p.ld_do = ld_do; p.d_qx = d_q; p.d_kx = d_k; p.d_v = d_v; p.ld_dq = ld_dq; p.ld_dk = ld_dk; p.ld_dv = ld_dv;
    TiP t{ts, time_scale, timelen, ktime, vtime, H * dh, tab_rows, wbuf, dgbuf, (timelen + 1 + 15) / 16 * 16};
    hipStream_t st = (hipStream_t)stream;
#define EDGL_TI_BWD(TT)                                                            \
    switch (dh / 16) {                                                             \
        case 1: return ti_bwd<TT, 1>(p, t, d_ktime, d_vtime, det_ws, st);          \
        case 2: return ti_bwd<TT, 2>(p, t, d_ktime, d_vtime, det_ws, st);          \
        case 4: return ti_bwd<TT, 4>(p, t, d_ktime, d_vtime, det_ws, st);          \
        default: return ti_bwd<TT, 8>(p, t, d_ktime, d_vtime, det_ws, st);         \
    }
    if (dtype == EDGL_F32) { EDGL_TI_BWD(float) }
    EDGL_TI_BWD(bf16)
#undef EDGL_TI_BWD
}

extern "C" int edgl_tiattn_bwd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const int64_t* ids,
                               const float* ts, const void* ktime, const void* vtime, int tab_rows, const void* d_out, int ld_do,
                               void* saved, void* wbuf, int B, int T, int H, int dh, float scale, float time_scale, int timelen,
                               float drop_rate, const uint64_t* rng_state, uint32_t stream_id, void* d_q, int ld_dq, void* d_k,
                               int ld_dk, void* d_v, int ld_dv, void* dgbuf, float* d_ktime, float* d_vtime, int flags, int dtype,
                               void* stream) {
    return tiattn_bwd_any("edgl_tiattn_bwd", q, ldq, k, ldk, v, ldv, ids, ts, ktime, vtime, tab_rows, d_out, ld_do, saved, wbuf, B, T, H,
                          dh, scale, time_scale, timelen, drop_rate, rng_state, stream_id, d_q, ld_dq, d_k, ld_dk, d_v, ld_dv, dgbuf,
                          d_ktime, d_vtime, nullptr, flags, dtype, stream);
}

// floats of the slab workspace of edgl_tiattn_bwd_det: [2 tables][TI_SPLITS][timelen + 1 rows][H * dh]
extern "C" long edgl_tiattn_det_workspace(int H, int dh, int timelen) {
    if (H <= 0 || !(dh == 16 || dh == 32 || dh == 64 || dh == 128) || timelen < 1 || timelen > 256) return -1;
    return 2L * TI_SPLITS * (timelen + 1) * H * dh;
}

// edgl_tiattn_bwd in the deterministic form: the query sweep fills its bins in order (EDGL_TATTN_ORDERED, whatever
// `flags` says) and every row split of the interval-table gradients stores its partial tile to a slab of its own in `workspace`;
// one more launch adds the slabs in split order.  No memset, no atomics: every address has one writer per launch.
extern "C" int edgl_tiattn_bwd_det(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const int64_t* ids,
                                   const float* ts, const void* ktime, const void* vtime, int tab_rows, const void* d_out, int ld_do,
                                   void* saved, void* wbuf, int B, int T, int H, int dh, float scale, float time_scale, int timelen,
                                   float drop_rate, const uint64_t* rng_state, uint32_t stream_id, void* d_q, int ld_dq, void* d_k,
                                   int ld_dk, void* d_v, int ld_dv, void* dgbuf, float* d_ktime, float* d_vtime, float* workspace,
                                   int flags, int dtype, void* stream) {
    EDGL_REQUIRE(workspace, EDGL_ERR_NULL, "edgl_tiattn_bwd_det: null pointer (workspace)");
    return tiattn_bwd_any("edgl_tiattn_bwd_det", q, ldq, k, ldk, v, ldv, ids, ts, ktime, vtime, tab_rows, d_out, ld_do, saved, wbuf, B, T,
                          H, dh, scale, time_scale, timelen, drop_rate, rng_state, stream_id, d_q, ld_dq, d_k, ld_dk, d_v, ld_dv, dgbuf,
                          d_ktime, d_vtime, workspace, flags | TA_ORDERED, dtype, stream);
}

extern "C" int edgl_add_pos2(const void* kv, const float* posK, const float* posV, int B, int T, int C, void* out, int dtype,
                             void* stream) {
    EDGL_REQUIRE(kv && posK && posV && out, EDGL_ERR_NULL, "edgl_add_pos2: null pointer");
    EDGL_REQUIRE(B > 0 && T > 0 && C > 0 && C % 4 == 0, EDGL_ERR_SHAPE, "edgl_add_pos2: bad shape B=%d T=%d C=%d", B, T, C);
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_add_pos2: bad dtype %d", dtype);
    const long rows = (long)B * T, total = rows * (2 * C / 4);
    dim3 grid((unsigned)((total + 255) / 256));
    if (dtype == EDGL_F32) hipLaunchKernelGGL((add_pos2_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, (const float*)kv, posK,
                                              posV, (float*)out, rows, T, C);
    else hipLaunchKernelGGL((add_pos2_kernel<bf16>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)kv, posK, posV, (bf16*)out,
                            rows, T, C);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
