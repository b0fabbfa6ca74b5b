// K3, key-streamed form: the BiMAU attention phases for sequences the in-register kernels cannot hold (T <= 1024).
//
// The kernels of bimau_fwd_impl.h / bimau_bwd_impl.h keep the whole key row of a (sample, head) job in registers and its K / T_ / V
// slices in wave-private LDS: one instance per key-tile count NT, bounded by the register file and the LDS.  The kernels here walk
// the keys in tiles of 16 with a run-time trip count instead (flash style).  They are templated on the element type and the
// head-dim blocks DT only, use no LDS, and read every operand of a key tile as ROW fragments straight from global memory (the
// K / T_ / V slices of one job are T * dh elements: they stay in L2 while the job's tiles run next to each other).  A product that
// contracts over the key (or query) index takes its operand through one MFMA against the identity (bimau_common.h).  Same
// transposed orientation S^T[k][q] and the same helpers as the in-register kernels; the structure is that of k_bimau_big.hip:
//
//   forward   scores (query-major: online softmax over the key tiles, H = P.T_ -> H rows, row statistics)
//             -> intensity_fwd_rows (row-wise: z, lambda; k_bimau_big.hip)
//             -> values (query-major: S recomputed, P from the stored statistics, G, diagonal rule, dropout, O = A.V + residual)
//   backward  sweep 1 (query-major: dlambda -> dz, row term, dscaling partials)
//             -> intensity backward (row-wise, unchanged: k_bimau_bwd.hip / k_bimau_big.hip) + the parameter reductions
//             -> sweep 2, query side (dQ; completes the row term with dH.H)
//             -> sweep 2, key side (key-major, streaming the query tiles: dK, dT_, dV)
//
// One wave owns one tile of 16 query rows (or 16 key rows) of one (sample, head) job; four waves, i.e. four neighbouring tiles, make a
// workgroup.  Every output element has exactly one writer and no kernel uses an atomic: two runs give the same bits.
// The row statistics (the row maximum of the log2-scaled masked scores and 1 / sum of exp2) are two f32 per row in `saved`.
#include "bimau_bwd_impl.h"
#include "bimau_fwd_impl.h"

namespace {
using namespace bimau;

constexpr float PAD_SCORE = -4294967296.0f;   // -2^32: see the key mask of bimau_common.h

// the next key (query) tile's operands are fetched one iteration ahead where two operand sets fit the register file
template <typename T, int DT> constexpr bool stream_pref() { return sizeof(T) * DT <= 16; }

struct TileId { long bp; int b, head, t; };
// wave -> tile t of job b' = head * B + b (temporal.py:413-416); false: past the last tile
__device__ __forceinline__ bool tile_of_wave(int B, int H, int NT, TileId& id) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long tile = (long)blockIdx.x * 4 + wave;
    if (tile >= (long)B * H * NT) return false;
    id.bp = tile / NT;
    id.t = (int)(tile - id.bp * NT);
    id.head = (int)(id.bp / B);
    id.b = (int)(id.bp - (long)id.head * B);
    return true;
}

// additive mask of the lane's keys kg .. kg + 3: 0 real, -2^32 padded (id == 0), -inf for k >= T
__device__ __forceinline__ f32x4 key_madd(const int64_t* ids_row, int T, int kg) {
    f32x4 m;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = kg + r;
        const int64_t id = ids_row[min(k, T - 1)];
        m[r] = k >= T ? -INFINITY : (id == 0 ? PAD_SCORE : 0.f);
    }
    return m;
}
// DT row fragments of row `row` (clamped into the sequence); base already points at the lane's first channel
template <typename T, int DT>
__device__ __forceinline__ void load_rows(Frag4<T> (&f)[DT], const T* base, long ld, int row, int Tlen) {
    const T* p = base + (long)min(row, Tlen - 1) * ld;
#pragma unroll
    for (int ub = 0; ub < DT; ++ub) f[ub] = frag_ld<T>(p + ub * 16);
}
// marks of key k, marks e0 .. e0 + 3 (A operand of G^T = marks . lambda^T); zeros for k >= T and e >= E
template <typename T>
__device__ __forceinline__ Frag4<T> marks_row_frag(const uint8_t* marks_b, int E, int Tlen, int k, int e0) {
    const uint8_t* p = marks_b + (long)min(k, Tlen - 1) * E;
    Frag4<T> f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float x = (float)p[min(e0 + r, E - 1)];
        f.v[r] = from_f32<T>((k < Tlen && e0 + r < E) ? x : 0.f);
    }
    return f;
}
// mark e of keys k0 .. k0 + 3 (A operand of dlambda^T = marks^T . dG^T)
template <typename T>
__device__ __forceinline__ Frag4<T> marks_col_frag(const uint8_t* marks_b, int E, int Tlen, int k0, int e) {
    Frag4<T> f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float x = (float)marks_b[(long)min(k0 + r, Tlen - 1) * E + min(e, E - 1)];
        f.v[r] = from_f32<T>((k0 + r < Tlen && e < E) ? x : 0.f);
    }
    return f;
}
// masked, log2-scaled scores of one tile: v[r] for key kg + r and this lane's query q (temporal.py:422-426, 370-375)
template <typename T, int DT>
__device__ __forceinline__ f32x4 score_tile(const Frag4<T> (&kf)[DT], const Frag4<T> (&qf)[DT], const f32x4& madd, float c2, bool causal,
                                            int kg, int q) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ub = 0; ub < DT; ++ub) a = mma16(kf[ub], qf[ub], a);
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        v[r] = fmaf(a[r], c2, madd[r]);
        if (causal && kg + r > q && madd[r] != -INFINITY) v[r] = PAD_SCORE;
    }
    return v;
}
// row fragment X[row = l15][c = g4 + r] -> A operand that contracts over the rows: lane holds X[row = g4 + r][c = l15]
template <typename T>
__device__ __forceinline__ Frag4<T> rows_to_contraction(const Frag4<T>& f, const Frag4<T>& ident) {
    return frag_from_acc<T>(mma16(f, ident, f32x4{0.f, 0.f, 0.f, 0.f}));
}
template <typename T>
__device__ __forceinline__ void keep4(const DropKey& dk, uint32_t idx0, bool (&keep)[4]) {
    const uint64_t hw = drop_hash_quad(dk, idx0);
    keep[0] = drop_quad_keep<0>(dk, hw); keep[1] = drop_quad_keep<1>(dk, hw);
    keep[2] = drop_quad_keep<2>(dk, hw); keep[3] = drop_quad_keep<3>(dk, hw);
}

// ------------------------------------------------------------------------------------------------------------------
// forward, scores phase: online softmax over the key tiles, H = P.T_, row statistics
// ------------------------------------------------------------------------------------------------------------------
template <typename T, int DT>
__global__ __launch_bounds__(256) void stream_scores_kernel(FwdP p, float* stats) {
    constexpr int dh = 16 * DT;
    const int NT = (p.T + 15) / 16;
    TileId id;
    if (!tile_of_wave(p.B, p.H, NT, id)) return;
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15;
    const long ldq = 4 * (long)p.C;
    const T* qkvt = reinterpret_cast<const T*>(p.qkvt) + (long)id.b * p.T * ldq + id.head * dh + g4;
    const int64_t* ids = p.ids + (long)id.b * p.T;
    const int q = id.t * 16 + l15;
    const float cscale = p.qk_scale > 0.f ? p.qk_scale : rsqrtf((float)dh);
    const float c2 = cscale * 1.4426950408889634f;
    const bool causal = (p.flags & MAU_CAUSAL) != 0;
    const Frag4<T> ident = identity_frag<T>(lane);
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    Frag4<T> qf[DT];
    load_rows<T, DT>(qf, qkvt, ldq, q, p.T);

    struct KOps { Frag4<T> kf[DT], tf[DT]; f32x4 madd; };
    auto load_k = [&](int kt) {
        KOps o;
        load_rows<T, DT>(o.kf, qkvt + p.C, ldq, kt * 16 + l15, p.T);
        load_rows<T, DT>(o.tf, qkvt + 3 * p.C, ldq, kt * 16 + l15, p.T);
        o.madd = key_madd(ids, p.T, kt * 16 + g4);
        return o;
    };
    float m = -INFINITY, l = 0.f;   // running row maximum; this lane's share of the running sum
    f32x4 Hacc[DT];                 // H^T[u][q], L(first = u, second = q), relative to the running maximum
#pragma unroll
    for (int ut = 0; ut < DT; ++ut) Hacc[ut] = zero4;
    KOps cur = load_k(0);
    for (int kt = 0; kt < NT; ++kt) {
        KOps nxt;
        if constexpr (stream_pref<T, DT>()) nxt = load_k(min(kt + 1, NT - 1));
        const f32x4 v = score_tile<T, DT>(cur.kf, qf, cur.madd, c2, causal, kt * 16 + g4, q);
        // every tile holds a key k < T: the new maximum is finite (a padded key keeps its finite -2^32 score)
        const float mn = fmaxf(m, group_max4(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]))));
        const float alpha = __builtin_amdgcn_exp2f(m - mn);   // first tile: exp2(-inf) = 0
        f32x4 e;
#pragma unroll
        for (int r = 0; r < 4; ++r) e[r] = __builtin_amdgcn_exp2f(v[r] - mn);   // (v - max) first: exact 0 at the -2^32 magnitude
        l = fmaf(l, alpha, (e[0] + e[1]) + (e[2] + e[3]));
        const Frag4<T> pf = frag_from_acc<T>(e);
#pragma unroll
        for (int ut = 0; ut < DT; ++ut) {
#pragma unroll
            for (int r = 0; r < 4; ++r) Hacc[ut][r] *= alpha;
            Hacc[ut] = mma16(rows_to_contraction<T>(cur.tf[ut], ident), pf, Hacc[ut]);
        }
        m = mn;
        if constexpr (stream_pref<T, DT>()) cur = nxt;
        else if (kt + 1 < NT) cur = load_k(kt + 1);
    }
    const float inv = fast_rcp(group_sum4(l));
    if (q < p.T) {
        const long row = id.bp * p.T + q;
#pragma unroll
        for (int ut = 0; ut < DT; ++ut) {
            f32x4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) h[r] = Hacc[ut][r] * inv;
            st_frag<T>(reinterpret_cast<T*>(p.hin_out) + row * dh + ut * 16 + g4, h);   // what the intensity MLP consumes
        }
        if (lane < 16) *reinterpret_cast<float2*>(stats + row * 2) = make_float2(m, inv);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// forward, values phase: P from the stored statistics, G = lambda.marks^T, diagonal rule, dropout, O = A.V + residual
// ------------------------------------------------------------------------------------------------------------------
template <typename T, int DT>
__global__ __launch_bounds__(256) void stream_values_kernel(FwdP p, const float* stats) {
    constexpr int dh = 16 * DT;
    const int NT = (p.T + 15) / 16, E = p.E;
    TileId id;
    if (!tile_of_wave(p.B, p.H, NT, id)) return;
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15;
    const long ldq = 4 * (long)p.C;
    const T* qkvt = reinterpret_cast<const T*>(p.qkvt) + (long)id.b * p.T * ldq + id.head * dh + g4;
    const int64_t* ids = p.ids + (long)id.b * p.T;
    const uint8_t* marks = p.marks + (long)id.b * p.T * E;
    const int qt = id.t, q = qt * 16 + l15, qc = min(q, p.T - 1);
    const long row = id.bp * p.T + qc;
    const float cscale = p.qk_scale > 0.f ? p.qk_scale : rsqrtf((float)dh);
    const float c2 = cscale * 1.4426950408889634f;
    const bool causal = (p.flags & MAU_CAUSAL) != 0;
    const DropKey dk = make_dropkey(p.rng, p.stream_id, p.rate);
    const Frag4<T> ident = identity_frag<T>(lane);
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    Frag4<T> qf[DT], rf[DT];
    load_rows<T, DT>(qf, qkvt, ldq, q, p.T);
    load_rows<T, DT>(rf, reinterpret_cast<const T*>(p.resid) + (long)id.b * p.T * p.ld_res + id.head * dh + g4, p.ld_res, q, p.T);
    const float2 st = *reinterpret_cast<const float2*>(stats + row * 2);
    const float mx = st.x, gfac = st.y * dk.scale;   // 1 / sum and the dropout scale ride on lambda (G is linear in it)
    Frag4<T> lf;
#pragma unroll
    for (int i = 0; i < 4; ++i) lf.v[i] = from_f32<T>(g4 + i < E ? p.lam[row * E + g4 + i] * gfac : 0.f);
    const bool set_diag = !(p.flags & MAU_NO_DIAG);
    const float dval = (p.flags & MAU_DIAG_ZERO) ? 0.0f : gfac;
    const uint32_t dbase = (uint32_t)((id.bp * p.T + q) * p.T);   // element index of (b', q, k = 0): as in the in-register kernels

    struct KOps { Frag4<T> kf[DT], vf[DT], mf; f32x4 madd; };
    auto load_k = [&](int kt) {
        KOps o;
        load_rows<T, DT>(o.kf, qkvt + p.C, ldq, kt * 16 + l15, p.T);
        load_rows<T, DT>(o.vf, qkvt + 2 * p.C, ldq, kt * 16 + l15, p.T);
        o.mf = marks_row_frag<T>(marks, E, p.T, kt * 16 + l15, g4);
        o.madd = key_madd(ids, p.T, kt * 16 + g4);
        return o;
    };
    f32x4 Oacc[DT];
#pragma unroll
    for (int vt = 0; vt < DT; ++vt) Oacc[vt] = zero4;
    KOps cur = load_k(0);
    for (int kt = 0; kt < NT; ++kt) {
        KOps nxt;
        if constexpr (stream_pref<T, DT>()) nxt = load_k(min(kt + 1, NT - 1));
        const f32x4 v = score_tile<T, DT>(cur.kf, qf, cur.madd, c2, causal, kt * 16 + g4, q);
        const f32x4 gacc = mma16(cur.mf, lf, zero4);   // G^T[k][q] (temporal.py:432-436)
        const bool dtile = set_diag && kt == qt;        // only this key tile can hold k == q (temporal.py:438-439)
        f32x4 s;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float g = (dtile && g4 + r == l15) ? dval : gacc[r];
            s[r] = g * __builtin_amdgcn_exp2f(v[r] - mx);   // temporal.py:441
        }
        if (dk.thresh != 0u) {                            // temporal.py:442 (the scale is in G already)
            bool keep[4];
            keep4<T>(dk, dbase + kt * 16 + g4, keep);
#pragma unroll
            for (int r = 0; r < 4; ++r) s[r] = keep[r] ? s[r] : 0.f;
        }
        const Frag4<T> pf = frag_from_acc<T>(s);
#pragma unroll
        for (int vt = 0; vt < DT; ++vt) Oacc[vt] = mma16(rows_to_contraction<T>(cur.vf[vt], ident), pf, Oacc[vt]);
        if constexpr (stream_pref<T, DT>()) cur = nxt;
        else if (kt + 1 < NT) cur = load_k(kt + 1);
    }
    if (q < p.T) {
#pragma unroll
        for (int vt = 0; vt < DT; ++vt) {
            f32x4 o4;
#pragma unroll
            for (int r = 0; r < 4; ++r) o4[r] = Oacc[vt][r] + to_f32(rf[vt].v[r]);   // temporal.py:443-447
            st_frag<T>(reinterpret_cast<T*>(p.out) + ((long)id.b * p.T + q) * p.C + id.head * dh + vt * 16 + g4, o4);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// backward, sweep 1 (query-major): dlambda -> dz, the row term sum_k dP1.P, dscaling partials per (job, query tile)
// ------------------------------------------------------------------------------------------------------------------
template <typename T, int DT>
__global__ __launch_bounds__(256) void stream_sweep1_kernel(BwdP p, const float* stats) {
    constexpr int dh = 16 * DT;
    const int NT = (p.T + 15) / 16, E = p.E;
    TileId id;
    if (!tile_of_wave(p.B, p.H, NT, id)) return;
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15;
    const long ldq = 4 * (long)p.C;
    const T* qkvt = reinterpret_cast<const T*>(p.qkvt) + (long)id.b * p.T * ldq + id.head * dh + g4;
    const T* dout = reinterpret_cast<const T*>(p.d_out) + (long)id.b * p.T * p.C + id.head * dh + g4;
    const int64_t* ids = p.ids + (long)id.b * p.T;
    const uint8_t* marks = p.marks + (long)id.b * p.T * E;
    const int qt = id.t, q = qt * 16 + l15, qc = min(q, p.T - 1);
    const bool qok = q < p.T;
    const long row = id.bp * p.T + qc;
    const float cscale = p.qk_scale > 0.f ? p.qk_scale : rsqrtf((float)dh);
    const float c2 = cscale * 1.4426950408889634f;
    const bool causal = (p.flags & MAU_CAUSAL) != 0;
    const DropKey dk = make_dropkey(p.rng, p.stream_id, p.rate);
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const PackDims pd = pack_dims<T>(dh, E);
    const float* iscs_g = reinterpret_cast<const float*>(p.pack + pd.off_f32) + 3 * pd.JE + EP;   // 1 / exp(scaling)

    Frag4<T> qf[DT], dof[DT];
    load_rows<T, DT>(qf, qkvt, ldq, q, p.T);
    load_rows<T, DT>(dof, dout, p.C, q, p.T);
    if (!qok) {
#pragma unroll
        for (int ub = 0; ub < DT; ++ub) dof[ub] = frag_zero<T>();
    }
    const float4 z4v = *reinterpret_cast<const float4*>(p.z + row * EP + g4);
    const float zq4[4] = {z4v.x, z4v.y, z4v.z, z4v.w};
    float lam[4], dlx[4];
    Frag4<T> lf;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool oke = qok && g4 + i < E;
        const long at = row * E + min(g4 + i, E - 1);
        lam[i] = oke ? p.lam[at] : 0.f;
        dlx[i] = (oke && p.d_lam_ext) ? p.d_lam_ext[at] : 0.f;
        lf.v[i] = from_f32<T>(lam[i]);
    }
    const float2 st = *reinterpret_cast<const float2*>(stats + row * 2);
    const float mx = st.x, pfac = st.y * dk.scale;   // every use of P in this sweep carries the dropout scale
    const uint32_t dbase = (uint32_t)((id.bp * p.T + q) * p.T);
    const bool diag_on = !(p.flags & MAU_NO_DIAG);
    const float dval = (p.flags & MAU_DIAG_ZERO) ? 0.0f : 1.0f;

    struct KOps { Frag4<T> kf[DT], vf[DT], mf, mc; f32x4 madd; };
    auto load_k = [&](int kt) {
        KOps o;
        load_rows<T, DT>(o.kf, qkvt + p.C, ldq, kt * 16 + l15, p.T);
        load_rows<T, DT>(o.vf, qkvt + 2 * p.C, ldq, kt * 16 + l15, p.T);
        o.mf = marks_row_frag<T>(marks, E, p.T, kt * 16 + l15, g4);
        o.mc = marks_col_frag<T>(marks, E, p.T, kt * 16 + g4, l15);
        o.madd = key_madd(ids, p.T, kt * 16 + g4);
        return o;
    };
    float rowdot = 0.f;   // this lane's part of sum_k dP1[q][k] P[q][k]
    f32x4 dlamT = zero4;  // L(first = e, second = q)
    KOps cur = load_k(0);
    for (int kt = 0; kt < NT; ++kt) {
        KOps nxt;
        if constexpr (stream_pref<T, DT>()) nxt = load_k(min(kt + 1, NT - 1));
        const f32x4 v = score_tile<T, DT>(cur.kf, qf, cur.madd, c2, causal, kt * 16 + g4, q);
        const f32x4 gacc = mma16(cur.mf, lf, zero4);
        f32x4 da = zero4;   // dA'^T[k][q] = sum_v V[k][v] dO[q][v]
#pragma unroll
        for (int vb = 0; vb < DT; ++vb) da = mma16(cur.vf[vb], dof[vb], da);
        const bool dtile = diag_on && kt == qt;
        bool keep[4];
        keep4<T>(dk, dbase + kt * 16 + g4, keep);
        f32x4 dg;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool dg_el = dtile && g4 + r == l15;
            const float gv = dg_el ? dval : gacc[r];                                  // G' (temporal.py:438-439)
            const float fp = keep[r] ? __builtin_amdgcn_exp2f(v[r] - mx) * pfac : 0.f;   // D.P with the scale
            const float d = da[r] * fp;                                               // dG' = dA' . D . P
            rowdot = fmaf(d, gv, rowdot);                                             // dP1 . P, before the diagonal is blocked
            dg[r] = dg_el ? 0.f : d;                                                  // the diagonal rule passes nothing to lambda
        }
        dlamT = mma16(cur.mc, frag_from_acc<T>(dg), dlamT);
        if constexpr (stream_pref<T, DT>()) cur = nxt;
        else if (kt + 1 < NT) cur = load_k(kt + 1);
    }
    float dz4[4], dsc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float dl = dlamT[i] + dlx[i];
        const float sg = sigmoid_f(zq4[i] * iscs_g[g4 + i]);   // softplus'
        dz4[i] = dl * sg;
        dsc[i] = (qok && g4 + i < E) ? dl * (lam[i] - zq4[i] * sg) : 0.f;
    }
    rowdot = group_sum4(rowdot);
#pragma unroll
    for (int i = 0; i < 4; ++i) {   // dscaling partial of this tile: sum over its 16 query lanes
        float s = dsc[i];
        s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64); s += __shfl_xor(s, 8, 64);
        dsc[i] = s;
    }
    if (qok) {
        *reinterpret_cast<float4*>(p.dz_ws + row * EP + g4) = make_float4(dz4[0], dz4[1], dz4[2], dz4[3]);
        if (lane < 16) p.rowdot_ws[row] = rowdot;
    }
    if (l15 == 0) *reinterpret_cast<float4*>(p.dsc_part + (id.bp * NT + qt) * EP + g4) = make_float4(dsc[0], dsc[1], dsc[2], dsc[3]);
}

// what both halves of sweep 2 need of a query tile
template <typename T, int DT>
struct S2Q {
    Frag4<T> qf[DT], dof[DT];
    f32x4 dHq[DT];      // dH^T[u][q], L(first = u, second = q): the intensity backward's partial slabs summed in a fixed order
    Frag4<T> lf;        // lambda * dropout scale
    float mx, inv, rowdot;
};
// FINAL: rowdot_ws holds the complete row term (key side); otherwise sweep 1's part, completed here with dH[q].H[q]
template <typename T, int DT, bool FINAL>
__device__ __forceinline__ S2Q<T, DT> load_s2q(const BwdP& p, const float* stats, const TileId& id, int qt, int nyp, float scale, int lane) {
    constexpr int dh = 16 * DT;
    const int g4 = (lane >> 4) * 4, l15 = lane & 15, E = p.E;
    const long ldq = 4 * (long)p.C, R = (long)p.B * p.H * p.T;
    const int q = qt * 16 + l15;
    const bool qok = q < p.T;
    const long row = id.bp * p.T + min(q, p.T - 1);
    S2Q<T, DT> o;
    load_rows<T, DT>(o.qf, reinterpret_cast<const T*>(p.qkvt) + (long)id.b * p.T * ldq + id.head * dh + g4, ldq, q, p.T);
    load_rows<T, DT>(o.dof, reinterpret_cast<const T*>(p.d_out) + (long)id.b * p.T * p.C + id.head * dh + g4, p.C, q, p.T);
    float hdot = 0.f;
#pragma unroll
    for (int ub = 0; ub < DT; ++ub) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        for (int y = 0; y < nyp; ++y) {
            const float4 d = *reinterpret_cast<const float4*>(p.dh_ws + ((long)y * R + row) * dh + ub * 16 + g4);
            a[0] += d.x; a[1] += d.y; a[2] += d.z; a[3] += d.w;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) o.dHq[ub][r] = qok ? a[r] : 0.f;
        if (!qok) o.dof[ub] = frag_zero<T>();
        if constexpr (!FINAL) {
            const Frag4<T> hf = frag_ld<T>(reinterpret_cast<const T*>(p.hin) + row * dh + ub * 16 + g4);
#pragma unroll
            for (int r = 0; r < 4; ++r) hdot = fmaf(o.dHq[ub][r], to_f32(hf.v[r]), hdot);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) o.lf.v[i] = from_f32<T>(g4 + i < E ? p.lam[row * E + g4 + i] * scale : 0.f);
    const float2 st = *reinterpret_cast<const float2*>(stats + row * 2);
    o.mx = st.x; o.inv = st.y;
    // rowsum(dP.P) = sum_k dP1.P (sweep 1) + dH[q].H[q]   (H = P.T_, saved)
    o.rowdot = qok ? p.rowdot_ws[row] : 0.f;
    if constexpr (!FINAL) o.rowdot += group_sum4(hdot);
    return o;
}
// One (key tile, query tile) pair of sweep 2: P^T, A'^T = (D.G'.P)^T and dS^T, all L(first = k, second = q)
template <typename T, int DT>
__device__ __forceinline__ void s2_tile(const S2Q<T, DT>& qo, const Frag4<T> (&kf)[DT], const Frag4<T> (&tf)[DT], const Frag4<T> (&vf)[DT],
                                        const Frag4<T>& mf, const f32x4& madd, const DropKey& dk, uint32_t dbase, int flags, float cscale,
                                        int kt, int qt, int lane, f32x4& P, f32x4& ap, f32x4& ds) {
    const int g4 = (lane >> 4) * 4, l15 = lane & 15, q = qt * 16 + l15;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const bool causal = (flags & MAU_CAUSAL) != 0;
    const f32x4 v = score_tile<T, DT>(kf, qo.qf, madd, cscale * 1.4426950408889634f, causal, kt * 16 + g4, q);
    const f32x4 gacc = mma16(mf, qo.lf, zero4);   // G' with the dropout scale
    f32x4 da = zero4;
#pragma unroll
    for (int vb = 0; vb < DT; ++vb) da = mma16(vf[vb], qo.dof[vb], da);
    const bool dtile = kt == qt && !(flags & MAU_NO_DIAG);
    const float dval = (flags & MAU_DIAG_ZERO) ? 0.0f : dk.scale;
    bool keep[4];
    keep4<T>(dk, dbase + kt * 16 + g4, keep);
    f32x4 a;   // dP = dP1 + dH.T_^T, dP1 = D . dA' . G'
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float gv = (dtile && g4 + r == l15) ? dval : gacc[r];
        P[r] = __builtin_amdgcn_exp2f(v[r] - qo.mx) * qo.inv;
        ap[r] = keep[r] ? gv * P[r] : 0.f;
        a[r] = keep[r] ? da[r] * gv : 0.f;
    }
#pragma unroll
    for (int ub = 0; ub < DT; ++ub) a = mma16(tf[ub], frag_from_acc<T>(qo.dHq[ub]), a);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        // tf.where(mask == 0, paddings, S) (temporal.py:425-426, 370-375) passes no gradient to a replaced score; keys k >= T have P = 0
        const bool replaced = madd[r] != 0.f || (causal && kt * 16 + g4 + r > q);
        ds[r] = replaced ? 0.f : P[r] * (a[r] - qo.rowdot) * cscale;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// backward, sweep 2, query side: dQ; writes the completed row term back for the key side
// ------------------------------------------------------------------------------------------------------------------
template <typename T, int DT>
__global__ __launch_bounds__(256) void stream_sweep2q_kernel(BwdP p, const float* stats, int nyp) {
    constexpr int dh = 16 * DT;
    const int NT = (p.T + 15) / 16, E = p.E;
    TileId id;
    if (!tile_of_wave(p.B, p.H, NT, id)) return;
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15;
    const long ldq = 4 * (long)p.C;
    const T* qkvt = reinterpret_cast<const T*>(p.qkvt) + (long)id.b * p.T * ldq + id.head * dh + g4;
    const int64_t* ids = p.ids + (long)id.b * p.T;
    const uint8_t* marks = p.marks + (long)id.b * p.T * E;
    const int qt = id.t, q = qt * 16 + l15;
    const float cscale = p.qk_scale > 0.f ? p.qk_scale : rsqrtf((float)dh);
    const DropKey dk = make_dropkey(p.rng, p.stream_id, p.rate);
    const Frag4<T> ident = identity_frag<T>(lane);
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const uint32_t dbase = (uint32_t)((id.bp * p.T + q) * p.T);
    const S2Q<T, DT> qo = load_s2q<T, DT, false>(p, stats, id, qt, nyp, dk.scale, lane);
    if (q < p.T && lane < 16) p.rowdot_ws[id.bp * p.T + q] = qo.rowdot;   // this wave is the row's only reader in this launch

    struct KOps { Frag4<T> kf[DT], tf[DT], vf[DT], mf; f32x4 madd; };
    auto load_k = [&](int kt) {
        KOps o;
        load_rows<T, DT>(o.kf, qkvt + p.C, ldq, kt * 16 + l15, p.T);
        load_rows<T, DT>(o.tf, qkvt + 3 * p.C, ldq, kt * 16 + l15, p.T);
        load_rows<T, DT>(o.vf, qkvt + 2 * p.C, ldq, kt * 16 + l15, p.T);
        o.mf = marks_row_frag<T>(marks, E, p.T, kt * 16 + l15, g4);
        o.madd = key_madd(ids, p.T, kt * 16 + g4);
        return o;
    };
    f32x4 dQ[DT];   // dQ^T[u][q]
#pragma unroll
    for (int ut = 0; ut < DT; ++ut) dQ[ut] = zero4;
    KOps cur = load_k(0);
    for (int kt = 0; kt < NT; ++kt) {
        KOps nxt;
        if constexpr (stream_pref<T, DT>()) nxt = load_k(min(kt + 1, NT - 1));
        f32x4 P, ap, ds;
        s2_tile<T, DT>(qo, cur.kf, cur.tf, cur.vf, cur.mf, cur.madd, dk, dbase, p.flags, cscale, kt, qt, lane, P, ap, ds);
        const Frag4<T> dsf = frag_from_acc<T>(ds);
#pragma unroll
        for (int ut = 0; ut < DT; ++ut) dQ[ut] = mma16(rows_to_contraction<T>(cur.kf[ut], ident), dsf, dQ[ut]);
        if constexpr (stream_pref<T, DT>()) cur = nxt;
        else if (kt + 1 < NT) cur = load_k(kt + 1);
    }
    if (q < p.T) {
        T* dst = reinterpret_cast<T*>(p.d_qkvt) + ((long)id.b * p.T + q) * ldq + id.head * dh + g4;
#pragma unroll
        for (int ut = 0; ut < DT; ++ut) st_frag<T>(dst + ut * 16, dQ[ut]);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// backward, sweep 2, key side: one wave per key tile, streaming the query tiles: dK, dT_, dV
// ------------------------------------------------------------------------------------------------------------------
template <typename T, int DT>
__global__ __launch_bounds__(256) void stream_sweep2k_kernel(BwdP p, const float* stats, int nyp) {
    constexpr int dh = 16 * DT;
    const int NT = (p.T + 15) / 16, E = p.E;
    TileId id;
    if (!tile_of_wave(p.B, p.H, NT, id)) return;
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15;
    const long ldq = 4 * (long)p.C;
    const T* qkvt = reinterpret_cast<const T*>(p.qkvt) + (long)id.b * p.T * ldq + id.head * dh + g4;
    const int kt = id.t, k = kt * 16 + l15;
    const float cscale = p.qk_scale > 0.f ? p.qk_scale : rsqrtf((float)dh);
    const DropKey dk = make_dropkey(p.rng, p.stream_id, p.rate);
    const Frag4<T> ident = identity_frag<T>(lane);
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    Frag4<T> kf[DT], tf[DT], vf[DT];
    load_rows<T, DT>(kf, qkvt + p.C, ldq, k, p.T);
    load_rows<T, DT>(tf, qkvt + 3 * p.C, ldq, k, p.T);
    load_rows<T, DT>(vf, qkvt + 2 * p.C, ldq, k, p.T);
    const Frag4<T> mf = marks_row_frag<T>(p.marks + (long)id.b * p.T * E, E, p.T, k, g4);
    const f32x4 madd = key_madd(p.ids + (long)id.b * p.T, p.T, kt * 16 + g4);

    f32x4 dKa[DT], dTa[DT], dVa[DT];   // L(first = u, second = k)
#pragma unroll
    for (int ut = 0; ut < DT; ++ut) { dKa[ut] = zero4; dTa[ut] = zero4; dVa[ut] = zero4; }
    S2Q<T, DT> cur = load_s2q<T, DT, true>(p, stats, id, 0, nyp, dk.scale, lane);
    for (int qt = 0; qt < NT; ++qt) {
        S2Q<T, DT> nxt;
        if constexpr (stream_pref<T, DT>()) nxt = load_s2q<T, DT, true>(p, stats, id, min(qt + 1, NT - 1), nyp, dk.scale, lane);
        const uint32_t dbase = (uint32_t)((id.bp * p.T + qt * 16 + l15) * p.T);
        f32x4 P, ap, ds;
        s2_tile<T, DT>(cur, kf, tf, vf, mf, madd, dk, dbase, p.flags, cscale, kt, qt, lane, P, ap, ds);
        if (qt * 16 + l15 >= p.T) {   // a query row past the sequence end contributes nothing
#pragma unroll
            for (int r = 0; r < 4; ++r) { P[r] = 0.f; ap[r] = 0.f; ds[r] = 0.f; }
        }
        // operands that contract over the query index: L(first = q, second = k) / L(first = q, second = u)
        const Frag4<T> dsT = frag_from_acc<T>(transpose_tile<T>(ds, ident));
        const Frag4<T> pT = frag_from_acc<T>(transpose_tile<T>(P, ident));
        const Frag4<T> apT = frag_from_acc<T>(transpose_tile<T>(ap, ident));
#pragma unroll
        for (int ut = 0; ut < DT; ++ut) {
            dKa[ut] = mma16(rows_to_contraction<T>(cur.qf[ut], ident), dsT, dKa[ut]);
            dTa[ut] = mma16(frag_from_acc<T>(transpose_tile<T>(cur.dHq[ut], ident)), pT, dTa[ut]);
            dVa[ut] = mma16(rows_to_contraction<T>(cur.dof[ut], ident), apT, dVa[ut]);
        }
        if constexpr (stream_pref<T, DT>()) cur = nxt;
        else if (qt + 1 < NT) cur = load_s2q<T, DT, true>(p, stats, id, qt + 1, nyp, dk.scale, lane);
    }
    if (k < p.T) {   // 4 consecutive channels of key row k
        T* dst = reinterpret_cast<T*>(p.d_qkvt) + ((long)id.b * p.T + k) * ldq + id.head * dh + g4;
#pragma unroll
        for (int ut = 0; ut < DT; ++ut) {
            st_frag<T>(dst + p.C + ut * 16, dKa[ut]);
            st_frag<T>(dst + 2 * p.C + ut * 16, dVa[ut]);
            st_frag<T>(dst + 3 * p.C + ut * 16, dTa[ut]);
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
inline unsigned tile_blocks(const int B, const int H, const int T) { return (unsigned)(((long)B * H * ((T + 15) / 16) + 3) / 4); }

template <typename T, int DT>
int fwd_stream(const FwdP& p, float* stats, int dtype, hipStream_t st) {
    const dim3 grid(tile_blocks(p.B, p.H, p.T));
    hipLaunchKernelGGL((stream_scores_kernel<T, DT>), grid, dim3(256), 0, st, p, stats);
    EDGL_LAUNCH_CHECK();
    const int rc = intensity_fwd_rows(p, dtype, st);   // z, lambda
    if (rc) return rc;
    hipLaunchKernelGGL((stream_values_kernel<T, DT>), grid, dim3(256), 0, st, p, (const float*)stats);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

template <typename T, int DT>
int bwd_stream(const BwdP& p, const float* stats, float* dW1, float* db1, float* dw, float* dsc, int dtype, hipStream_t st) {
    const dim3 grid(tile_blocks(p.B, p.H, p.T));
    const long dsc_rows = (long)p.B * p.H * ((p.T + 15) / 16);
    edgl_prof_begin(EDGL_KERNEL_BIMAU_BWD_ALL, st);
    hipLaunchKernelGGL((stream_sweep1_kernel<T, DT>), grid, dim3(256), 0, st, p, stats);
    EDGL_LAUNCH_CHECK();
    const int rc = DT <= 2 ? intensity_bwd_small(p, dsc_rows, dW1, db1, dw, dsc, dtype, st) : intensity_bwd_big(p, dsc_rows, dW1, db1, dw, dsc, dtype, st);
    if (rc) return rc;
    const int nyp = DT <= 2 ? KY_NY : 1;   // dH partial slabs the intensity backward leaves
    edgl_prof_begin(EDGL_KERNEL_BIMAU_BWD, st);
    hipLaunchKernelGGL((stream_sweep2q_kernel<T, DT>), grid, dim3(256), 0, st, p, stats, nyp);
    hipLaunchKernelGGL((stream_sweep2k_kernel<T, DT>), grid, dim3(256), 0, st, p, stats, nyp);
    edgl_prof_end(EDGL_KERNEL_BIMAU_BWD, st);
    edgl_prof_end(EDGL_KERNEL_BIMAU_BWD_ALL, st);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

}  // namespace

namespace bimau {

int stream_fwd(const FwdP& p, float* stats, int dtype, hipStream_t st) {
    if (!p.hin_out || !p.z_out || !stats) {
        edgl_set_error("edgl_bimau_fwd: the key-streamed form runs as three launches and needs `saved` (edgl_bimau_saved_bytes_ex) as "
                       "scratch, also for inference");
        return EDGL_ERR_WORKSPACE;
    }
    const int dh = p.C / p.H;
#define EDGL_STREAM_CASE(DT_)                                                              \
    case 16 * DT_:                                                                         \
        return dtype == EDGL_F32 ? fwd_stream<float, DT_>(p, stats, dtype, st) : fwd_stream<bf16, DT_>(p, stats, dtype, st);
    switch (dh) { EDGL_STREAM_CASE(1) EDGL_STREAM_CASE(2) EDGL_STREAM_CASE(4) EDGL_STREAM_CASE(8) }
#undef EDGL_STREAM_CASE
    edgl_set_error("edgl_bimau_fwd: head dim %d not supported (16, 32, 64 or 128)", dh);
    return EDGL_ERR_SHAPE;
}

int stream_bwd(const BwdP& p, const float* stats, float* dW1, float* db1, float* dw, float* dsc, int dtype, hipStream_t st) {
    const int dh = p.C / p.H;
#define EDGL_STREAM_CASE(DT_)                                                                                         \
    case 16 * DT_:                                                                                                    \
        return dtype == EDGL_F32 ? bwd_stream<float, DT_>(p, stats, dW1, db1, dw, dsc, dtype, st)                     \
                                 : bwd_stream<bf16, DT_>(p, stats, dW1, db1, dw, dsc, dtype, st);
    switch (dh) { EDGL_STREAM_CASE(1) EDGL_STREAM_CASE(2) EDGL_STREAM_CASE(4) EDGL_STREAM_CASE(8) }
#undef EDGL_STREAM_CASE
    edgl_set_error("edgl_bimau_bwd: head dim %d not supported (16, 32, 64 or 128)", dh);
    return EDGL_ERR_SHAPE;
}

}  // namespace bimau
