// K6c: evaluation on candidate lists — the sampled-negative protocol and re-ranking.  Every row r of the batch has its
// OWN list cand[r, :] of item ids, so there is no operand reuse for the matrix pipe: the op is a gather of R (N + 1) table rows.
//
//   v(r, c) = -inf                                  c < 0 (empty slot), c >= I (caller error: the address is clamped), c in seen[r, :]
//           = rows[r] . table_c[c] + bias_used[c]   otherwise; item 0 is the used table's zero row with bias -1000 (coding.py:56-57)
//   count[r] += #{ n : c = cand[r, n] >= 0, c != y, v(r, c) > v(r, y) or (v(r, c) == v(r, y) and c < y) },   y = labels[r]
//
//   score_cand_kernel    workgroup = (row, chunk of the row's list), 4 waves.  The query row stays in registers, spread over a lane
//                        group of G = min(64, pieces) lanes (a piece = 16 bytes of the row; G rounded up to a power of two, lanes past
//                        the row hold zeros; f32 rows longer than 1 KB: two pieces per lane).  One wave-instruction of
//                        global_load_dwordx4 fetches 64 / G candidate rows, UNROLL = 4 of them are in flight before the first is used,
//                        and the ids of the next step are fetched under the arithmetic of this one.
//                        cand_value (cand_gather.h, shared with the training loss of k_cand_ce.hip) IS the arithmetic rule:
//                        per lane the FMAs of its pieces in ascending channel order from +0, a fixed
//                        xor butterfly over the lane group (offsets 1, 2, .. G / 2: both partners form a + b, so every lane of the group
//                        ends with the same bits), then + bias.  It depends on rows[r], table_c[c] and the bias only — not on the slot, N,
//                        R, the chunk or the other candidates — and the label is one more slot through the same function, formed by
//                        every wave for itself.  The row's seen ids are staged once as int32 in LDS (<= 4 KB); a candidate is tested
//                        by its lane group striding over them.  Counts: one integer atomicAdd per workgroup (exact, order-independent);
//                        no float atomics, no workspace, no finish kernel; scratch 0.
//   sample_neg_kernel    cand[r, n] = the first of 32 counter-based draws from [lo, hi) that is neither one of the row's seen ids nor
//                        its label (the draw is specified in DESIGN 4.12 and replicated by tests/_cand_ref.py), else -1.
//   sample_neg_alias_kernel   the same draw with the id taken from an alias table: popularity-weighted negatives.
//   rank_metrics_rows_kernel   edgl_rank_metrics_from_rank with the rows added one by one in row order: sampled-negative steps give
//                        the same metric sums whatever the batch size.
#include <algorithm>

#include "edgl_common.h"
#include "cand_gather.h"

namespace evc {

using candg::UNROLL; using candg::RowRegs; using candg::load_pieces; using candg::unpack; using candg::cand_value; using candg::group_of;

constexpr int MAX_T = 1024;      // seen ids per row staged in LDS
constexpr int MAX_CHUNK = 1024;  // slots of one workgroup
constexpr int WG_TARGET = 1024;  // workgroups wanted on the chip (256 CUs x 4)

struct P {
    const void* rows; const void* table; const float* bias; const int32_t* cand; const int64_t* seen; const int64_t* labels;
    int T, R, C, I, N, chunk, nchunks;
    float* scores; float* label_val; int32_t* count;
};

// an id that the int32 LDS image can hold, else one that equals no candidate
__device__ __forceinline__ int seen_id32(int64_t v) { return (v < 0 || v > 0x7fffffffLL) ? -2 : (int)v; }

template <typename T, int G, int PPL>
__global__ __launch_bounds__(256) void score_cand_kernel(P p) {
    constexpr int RPW = 64 / G;               // candidate rows per wave-instruction
    constexpr int STEP = 4 * UNROLL * RPW;    // slots of one step of the workgroup
    __shared__ int sseen[MAX_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = lane / G, gl = lane % G;
    const int r = blockIdx.x / p.nchunks, chunk = blockIdx.x % p.nchunks;
    const int n_lo = chunk * p.chunk, n_hi = min(p.N, n_lo + p.chunk);
    const T* table = reinterpret_cast<const T*>(p.table);
    const int T_ = p.seen ? p.T : 0;
    for (int t = tid; t < T_; t += 256) sseen[t] = seen_id32(p.seen[(long)r * p.T + t]);
    RowRegs<T, PPL> xq;
    {
        uint4 w[PPL];
        load_pieces<T, G, PPL>(reinterpret_cast<const T*>(p.rows), r, p.C, gl, w);
#pragma unroll
        for (int pp = 0; pp < PPL; ++pp) unpack<T>(w[pp], gl + pp * 64 < p.C / (int)(16 / sizeof(T)), xq.x[pp]);
    }
    __syncthreads();
    // is id c (>= 0) one of the row's seen ids: the lane group strides over the LDS image
    auto seen_any = [&](int found) {
#pragma unroll
        for (int o = 1; o < G; o <<= 1) found |= __shfl_xor(found, o, 64);
        return found;
    };
    // ---- the label: one more slot, the same function, formed by every wave for itself ---------------------------------------------
    const bool with_label = p.labels != nullptr;
    int y = -1;
    float vy = -INFINITY;
    if (with_label) {                         // (block-uniform)
        const int64_t y64 = p.labels[r];
        const bool ok = y64 >= 0 && y64 < p.I;
        y = y64 < 0 ? -1 : (y64 > 0x7fffffffLL ? 0x7fffffff : (int)y64);
        const int ya = ok ? y : 0;
        uint4 w[PPL];
        load_pieces<T, G, PPL>(table, ya, p.C, gl, w);
        const float b = ya == 0 ? -1000.0f : p.bias[ya - 1];
        const float v = cand_value<T, G, PPL>(xq, w, ya, b, p.C, gl);
        int found = 0;
        for (int t = gl; t < T_; t += G) found |= sseen[t] == y ? 1 : 0;
        found = seen_any(found);
        vy = (!ok || found) ? -INFINITY : v;
        if (p.label_val && chunk == 0 && tid == 0) p.label_val[r] = vy;
    }
    // ---- the list -------------------------------------------------------------------------------------------------------------------
    const int32_t* crow = p.cand + (long)r * p.N;
    auto slot_of = [&](int base, int u) { return base + u * (4 * RPW) + wave * RPW + grp; };
    int cs[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        const int n = slot_of(n_lo, u);
        cs[u] = n < n_hi ? crow[n] : -1;
    }
    int cnt = 0;
    for (int base = n_lo; base < n_hi; base += STEP) {        // (block-uniform)
        uint4 w[UNROLL][PPL];
        float b[UNROLL];
        int c[UNROLL], ca[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            c[u] = cs[u];
            ca[u] = (c[u] >= 0 && c[u] < p.I) ? c[u] : 0;     // (addresses stay inside the table whatever the id)
            load_pieces<T, G, PPL>(table, ca[u], p.C, gl, w[u]);
            b[u] = p.bias[max(ca[u], 1) - 1];
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {                    // the next step's ids, under this step's arithmetic
            const int n = slot_of(base + STEP, u);
            cs[u] = n < n_hi ? crow[n] : -1;
        }
        int found[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) found[u] = 0;
        for (int t = gl; t < T_; t += G) {
            const int s = sseen[t];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) found[u] |= s == c[u] ? 1 : 0;
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const float vv = cand_value<T, G, PPL>(xq, w[u], ca[u], ca[u] == 0 ? -1000.0f : b[u], p.C, gl);
            const bool ok = c[u] >= 0 && c[u] < p.I;
            const int fnd = seen_any(found[u]);               // (every lane takes part: not behind the test of `ok`)
            const float v = (!ok || fnd) ? -INFINITY : vv;
            const int n = slot_of(base, u);
            if (gl == 0 && n < n_hi) {
                if (p.scores) p.scores[(long)r * p.N + n] = v;
                cnt += (c[u] >= 0 && c[u] != y && (v > vy || (v == vy && c[u] < y))) ? 1 : 0;
            }
        }
    }
    if (p.count) {                            // (block-uniform)  one atomic per workgroup: a short batch with long lists puts
        __shared__ int wcnt[4];               // hundreds of workgroups on one count (measured: per-wave atomics cost 8 x 4096 20 us)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (lane == 0) wcnt[wave] = cnt;
        __syncthreads();
        const int tot = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        if (tid == 0 && tot) atomicAdd(p.count + r, tot);
    }
}

struct SP {
    const int64_t* seen; const int64_t* labels; int32_t* cand;
    int T, R, n, lo, hi;
    uint32_t key, row0;
};

__global__ __launch_bounds__(256) void sample_neg_kernel(SP p) {
    __shared__ int sseen[MAX_T];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int T_ = p.seen ? p.T : 0;
    for (int t = tid; t < T_; t += 256) sseen[t] = seen_id32(p.seen[(long)r * p.T + t]);
    __syncthreads();
    const int64_t y64 = p.labels ? p.labels[r] : -1;
    const int y = seen_id32(y64);
    const uint32_t hrow = edgl_mix32(p.key ^ edgl_mix32(p.row0 + (uint32_t)r));
    const uint32_t span = (uint32_t)(p.hi - p.lo);
    for (int n = tid; n < p.n; n += 256) {
        const uint32_t hs = edgl_mix32(hrow + (uint32_t)n * 0x9E3779B1u);
        int out = -1;
        for (uint32_t att = 0; att < 32u && out < 0; ++att) {
            const uint32_t h = edgl_mix32(hs ^ (att * 0x85EBCA6Bu));
            const int id = p.lo + (int)(((uint64_t)h * (uint64_t)span) >> 32);
            bool hit = id == y;
            for (int t = 0; t < T_; ++t) hit |= sseen[t] == id;       // (no early exit: the LDS reads pipeline)
            if (!hit) out = id;
        }
        p.cand[(long)r * p.n + n] = out;
    }
}

// The weighted draw: sample_neg_kernel with one change — the map from the attempt's word h to an id goes through an
// alias table of span = hi - lo buckets (ops.build_neg_dist: Vose's method, uint32 thresholds).  bucket j = (h span) >> 32, a second
// word h2 = mix32(h + ALIAS_K), id = lo + (h2 < thr[j] || alias[j] == j ? j : alias[j]).  tab[j] = (thr[j], alias[j]): ONE 8-byte
// random read per attempt.  Keys, row / slot / attempt hashing, row0, 32 attempts, the LDS image of the seen ids and -1 on failure
// are sample_neg_kernel's.  The bucket index is < span by construction; an alias outside [0, span) (a caller's broken table) falls
// back to the bucket itself, so no id outside [lo, hi) is ever written.
constexpr uint32_t ALIAS_K = 0x68E31DA4u;

__global__ __launch_bounds__(256) void sample_neg_alias_kernel(SP p, const uint2* __restrict__ tab) {
    __shared__ int sseen[MAX_T];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int T_ = p.seen ? p.T : 0;
    for (int t = tid; t < T_; t += 256) sseen[t] = seen_id32(p.seen[(long)r * p.T + t]);
    __syncthreads();
    const int64_t y64 = p.labels ? p.labels[r] : -1;
    const int y = seen_id32(y64);
    const uint32_t hrow = edgl_mix32(p.key ^ edgl_mix32(p.row0 + (uint32_t)r));
    const uint32_t span = (uint32_t)(p.hi - p.lo);
    for (int n = tid; n < p.n; n += 256) {
        const uint32_t hs = edgl_mix32(hrow + (uint32_t)n * 0x9E3779B1u);
        int out = -1;
        for (uint32_t att = 0; att < 32u && out < 0; ++att) {
            const uint32_t h = edgl_mix32(hs ^ (att * 0x85EBCA6Bu));
            const uint32_t j = (uint32_t)(((uint64_t)h * (uint64_t)span) >> 32);
            const uint2 e = tab[j];
            const uint32_t h2 = edgl_mix32(h + ALIAS_K);
            const uint32_t a = e.y < span ? e.y : j;
            const int id = p.lo + (int)((h2 < e.x || a == j) ? j : a);
            bool hit = id == y;
            for (int t = 0; t < T_; ++t) hit |= sseen[t] == id;       // (no early exit: the LDS reads pipeline)
            if (!hit) out = id;
        }
        p.cand[(long)r * p.n + n] = out;
    }
}

// sums[0 .. nk) += H@k, sums[nk .. 2 nk) += N@k, sums[2 nk] += MRR, ONE lane per sum, the rows in ascending order: ((s + g_0) + g_1) + ..
// — the same f32 value however a split is cut into batches (k_eval_rank.hip's form adds a batch as a tree).  The gains of a block of
// rows are formed by all threads into LDS; only the additions are serial.
constexpr int MROWS = 1024;
__global__ __launch_bounds__(256) void rank_metrics_rows_kernel(const int32_t* rank, int R, const int32_t* ks, int nk, float* sums) {
    __shared__ int s_rk[MROWS];
    __shared__ float s_gain[MROWS], s_rr[MROWS];
    const int i = threadIdx.x;
    const bool owner = i <= 2 * nk;
    const int k = (owner && i < 2 * nk) ? ks[i % nk] : 0;
    float s = owner ? sums[i] : 0.0f;
    for (int r0 = 0; r0 < R; r0 += MROWS) {                   // (block-uniform)
        const int n = min(MROWS, R - r0);
        for (int j = i; j < n; j += 256) {
            const int rk = rank[r0 + j];
            s_rk[j] = rk;
            s_gain[j] = 1.0f / log2f((float)rk + 2.0f);
            s_rr[j] = 1.0f / ((float)rk + 1.0f);
        }
        __syncthreads();
        if (owner) {
            for (int j = 0; j < n; ++j) {
                const float g = i < nk ? 1.0f : (i < 2 * nk ? s_gain[j] : s_rr[j]);
                if (i == 2 * nk || s_rk[j] < k) s += g;
            }
        }
        __syncthreads();
    }
    if (owner) sums[i] = s;
}

template <typename T, int G, int PPL>
int launch(const P& p, hipStream_t st) {
    hipLaunchKernelGGL((score_cand_kernel<T, G, PPL>), dim3((unsigned)((long)p.R * p.nchunks)), dim3(256), 0, st, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

template <typename T>
int dispatch(const P& p, hipStream_t st) {
    const int pieces = p.C / (int)(16 / sizeof(T));
    if constexpr (sizeof(T) == 4) {           // (only f32 rows exceed 64 pieces; only bf16 rows have two)
        if (pieces > 64) return launch<T, 64, 2>(p, st);
    }
    switch (group_of(pieces)) {
        case 2:
            if constexpr (sizeof(T) == 2) return launch<T, 2, 1>(p, st);
        case 4: return launch<T, 4, 1>(p, st);
        case 8: return launch<T, 8, 1>(p, st);
        case 16: return launch<T, 16, 1>(p, st);
        case 32: return launch<T, 32, 1>(p, st);
        default: return launch<T, 64, 1>(p, st);
    }
}

}  // namespace evc

// Slots per workgroup for this shape (host arithmetic, no device work): enough workgroups to fill the chip when R is small, whole
// steps of the workgroup, at most 1024.  The values do not depend on it (cand_value); -1 for a shape not taken.
extern "C" int edgl_score_candidates_chunk(int R, int C, int N, int dtype) {
    if ((dtype != EDGL_F32 && dtype != EDGL_BF16) || C < 16 || C > 512 || C % 16 || R < 1 || N < 1 || (long)R * ((long)N + 1) >= (1L << 31))
        return -1;
    const int pieces = C / (dtype == EDGL_BF16 ? 8 : 4);
    const int unit = std::max(64, 4 * evc::UNROLL * (64 / evc::group_of(pieces)));
    const long want = ((long)R * N + evc::WG_TARGET - 1) / evc::WG_TARGET;
    const long chunk = (want + unit - 1) / unit * unit;
    return (int)std::min<long>(std::max<long>(chunk, unit), evc::MAX_CHUNK);
}

extern "C" int edgl_score_candidates(const void* rows, const void* table, const float* out_bias, const int32_t* cand, const int64_t* seen,
                                     int T, const int64_t* labels, int R, int C, int I, int N, float* scores, float* label_val,
                                     int32_t* count, int dtype, void* stream) {
    EDGL_REQUIRE(rows && table && out_bias && cand, EDGL_ERR_NULL, "edgl_score_candidates: null pointer");
    EDGL_REQUIRE(seen || T == 0, EDGL_ERR_NULL, "edgl_score_candidates: T > 0 without seen ids");
    EDGL_REQUIRE(labels || (!label_val && !count), EDGL_ERR_NULL, "edgl_score_candidates: label_val / count without labels");
    EDGL_REQUIRE(scores || label_val || count, EDGL_ERR_NULL, "edgl_score_candidates: no output wanted");
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_score_candidates: dtype %d (f32 = 0 or bf16 = 1)", dtype);
    EDGL_REQUIRE(C >= 16 && C <= 512 && C % 16 == 0, EDGL_ERR_SHAPE, "edgl_score_candidates: C=%d (16 <= C <= 512, a multiple of 16)", C);
    EDGL_REQUIRE(R >= 1 && N >= 1 && I > 1 && (long)R * ((long)N + 1) < (1L << 31), EDGL_ERR_SHAPE,
                 "edgl_score_candidates: R=%d N=%d I=%d (R >= 1, N >= 1, I > 1, R (N + 1) < 2^31)", R, N, I);
    EDGL_REQUIRE(T >= 0 && T <= evc::MAX_T, EDGL_ERR_SHAPE, "edgl_score_candidates: T=%d (0 <= T <= %d)", T, evc::MAX_T);
    EDGL_REQUIRE((((uintptr_t)rows | (uintptr_t)table) & 15) == 0, EDGL_ERR_SHAPE, "edgl_score_candidates: rows and table must be 16-byte aligned");
    evc::P p{};
    p.rows = rows; p.table = table; p.bias = out_bias; p.cand = cand; p.seen = T > 0 ? seen : nullptr; p.labels = labels;
    p.T = T; p.R = R; p.C = C; p.I = I; p.N = N;
    p.chunk = edgl_score_candidates_chunk(R, C, N, dtype);
    p.nchunks = (N + p.chunk - 1) / p.chunk;
    p.scores = scores; p.label_val = label_val; p.count = count;
    hipStream_t st = (hipStream_t)stream;
    return dtype == EDGL_BF16 ? evc::dispatch<bf16>(p, st) : evc::dispatch<float>(p, st);
}

extern "C" int edgl_sample_negatives(const int64_t* seen, int T, const int64_t* labels, int R, int n, int lo, int hi, int I,
                                     uint64_t seed, uint64_t step, int row0, int32_t* cand, void* stream) {
    EDGL_REQUIRE(cand, EDGL_ERR_NULL, "edgl_sample_negatives: null pointer");
    EDGL_REQUIRE(seen || T == 0, EDGL_ERR_NULL, "edgl_sample_negatives: T > 0 without seen ids");
    EDGL_REQUIRE(R >= 1 && n >= 1 && row0 >= 0 && (long)R * n < (1L << 31), EDGL_ERR_SHAPE,
                 "edgl_sample_negatives: R=%d n=%d row0=%d (R >= 1, n >= 1, row0 >= 0, R n < 2^31)", R, n, row0);
    EDGL_REQUIRE(T >= 0 && T <= evc::MAX_T, EDGL_ERR_SHAPE, "edgl_sample_negatives: T=%d (0 <= T <= %d)", T, evc::MAX_T);
    EDGL_REQUIRE(1 <= lo && lo < hi && hi <= I, EDGL_ERR_SHAPE, "edgl_sample_negatives: range [%d, %d) of %d items (1 <= lo < hi <= I)", lo, hi, I);
    EDGL_REQUIRE(2L * (T + 1) <= (long)hi - lo, EDGL_ERR_SHAPE,
                 "edgl_sample_negatives: range [%d, %d) holds %d ids, 2 (T + 1) = %d are needed (every draw is then rejected with "
                 "probability <= 1/2)", lo, hi, hi - lo, 2 * (T + 1));
    // key(seed, step) of DESIGN 4.12, on the host: mix32 as edgl_mix32
    auto mix = [](uint32_t h) { h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16; return h; };
    uint32_t k = mix((uint32_t)seed ^ 0xC4ED1DA7u);
    k = mix(k + (uint32_t)(seed >> 32));
    k = mix(k ^ (uint32_t)step);
    evc::SP p{};
    p.seen = T > 0 ? seen : nullptr; p.labels = labels; p.cand = cand; p.T = T; p.R = R; p.n = n; p.lo = lo; p.hi = hi;
    p.key = k; p.row0 = (uint32_t)row0;
    hipLaunchKernelGGL(evc::sample_neg_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

// edgl_sample_negatives with the weighted draw of DESIGN 4.16.  thr_alias: uint32 [hi - lo, 2], entry j = (acceptance threshold,
// alias bucket) of ops.build_neg_dist.  The weighted form of 2 (T + 1) <= hi - lo — the T + 1 heaviest ids hold at most half of the
// weight — is a property of the weights and is checked where the table is built.
extern "C" int edgl_sample_negatives_alias(const int64_t* seen, int T, const int64_t* labels, int R, int n, int lo, int hi, int I,
                                           const uint32_t* thr_alias, uint64_t seed, uint64_t step, int row0, int32_t* cand,
                                           void* stream) {
    EDGL_REQUIRE(cand && thr_alias, EDGL_ERR_NULL, "edgl_sample_negatives_alias: null pointer");
    EDGL_REQUIRE(seen || T == 0, EDGL_ERR_NULL, "edgl_sample_negatives_alias: T > 0 without seen ids");
    EDGL_REQUIRE(R >= 1 && n >= 1 && row0 >= 0 && (long)R * n < (1L << 31), EDGL_ERR_SHAPE,
                 "edgl_sample_negatives_alias: R=%d n=%d row0=%d (R >= 1, n >= 1, row0 >= 0, R n < 2^31)", R, n, row0);
    EDGL_REQUIRE(T >= 0 && T <= evc::MAX_T, EDGL_ERR_SHAPE, "edgl_sample_negatives_alias: T=%d (0 <= T <= %d)", T, evc::MAX_T);
    EDGL_REQUIRE(1 <= lo && lo < hi && hi <= I, EDGL_ERR_SHAPE, "edgl_sample_negatives_alias: range [%d, %d) of %d items (1 <= lo < hi <= I)",
                 lo, hi, I);
    EDGL_REQUIRE(((uintptr_t)thr_alias & 7) == 0, EDGL_ERR_SHAPE, "edgl_sample_negatives_alias: the table must be 8-byte aligned");
    // key(seed, step) of DESIGN 4.12, on the host: mix32 as edgl_mix32
    auto mix = [](uint32_t h) { h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16; return h; };
    uint32_t k = mix((uint32_t)seed ^ 0xC4ED1DA7u);
    k = mix(k + (uint32_t)(seed >> 32));
    k = mix(k ^ (uint32_t)step);
    evc::SP p{};
    p.seen = T > 0 ? seen : nullptr; p.labels = labels; p.cand = cand; p.T = T; p.R = R; p.n = n; p.lo = lo; p.hi = hi;
    p.key = k; p.row0 = (uint32_t)row0;
    hipLaunchKernelGGL(evc::sample_neg_alias_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, p,
                       reinterpret_cast<const uint2*>(thr_alias));
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_rank_metrics_from_rank_rows(const int32_t* rank, int R, const int32_t* ks, int nk, float* sums, void* stream) {
    EDGL_REQUIRE(rank && ks && sums, EDGL_ERR_NULL, "edgl_rank_metrics_from_rank_rows: null pointer");
    EDGL_REQUIRE(R > 0 && nk >= 1 && nk <= 8, EDGL_ERR_SHAPE, "edgl_rank_metrics_from_rank_rows: bad shape R=%d nk=%d (1 <= nk <= 8)", R, nk);
    hipLaunchKernelGGL(evc::rank_metrics_rows_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, rank, R, ks, nk, sums);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
