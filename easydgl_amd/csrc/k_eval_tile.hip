// K6 / K7: evaluation on a materialised [R, n] f32 logits tile (edgl_score_lse_fwd with `logits`, k_score.hip) — any dtype and
// width, where the fused sweeps of k_eval_topk.hip / k_eval_rank.hip do not apply.
//   mask_topk_kernel, mask_topk_reg_kernel<16|40|80>   K6: mask the seen items, per-row top-K (Base.py:156-163,181; topk_select.h)
//   topk_merge_kernel                                   K7: candidate lists of several item ranges -> one top-K
//   rank_metrics_kernel                                 HR / NDCG @ 10, 50, 100 from a top-K list (Base.py:181-201)
#include "edgl_common.h"
#include "topk_select.h"

namespace {

// one workgroup per row: 4-pass radix select of the K-th largest key, then ordered compaction (topk_select.h)
__global__ __launch_bounds__(256) void mask_topk_kernel(float* logits, int R, int n, int i0, const int64_t* seen,
                                                        int T, int K, float* out_val, int32_t* out_idx) {
    const int row = blockIdx.x, tid = threadIdx.x;
    float* x = logits + (long)row * n;
    if (seen) {
        for (int t = tid; t < T; t += blockDim.x) {
            const long id = seen[(long)row * T + t] - i0;
            if (id >= 0 && id < n) x[id] = -INFINITY;
        }
        __syncthreads();
    }
    radix_select_row(x, n, i0, K, out_val + (long)row * K, out_idx + (long)row * K);
}

// The same selection with the row in REGISTERS (n <= 256 * NJ): the 4-pass form above re-reads the row five times and builds its
// histograms with LDS atomics that pile up on a handful of bins (the logits of a row share their exponent bits) — 194 us for 512
// rows of 20 001 items, none of it memory time.  Here a thread keeps its NJ keys.
//   Fast path: the K-th largest of the 256 THREAD MAXIMA is a lower bound L of the K-th largest key (K distinct elements lie at or
//   above it), so the top K are among the elements >= L — a few hundred for any row without heavy ties.  They are compacted
//   into LDS and sorted there by (key descending, index ascending): no pass over all keys per bit, no tie logic.
//   Otherwise (more than TK_CAP candidates: tie blocks, degenerate rows) the K-th largest key is found bit by bit over ALL keys (32
//   rounds of "how many keys are >= prefix | bit": one compare per key, the wave total from the ballot's population count), then
//   the elements above it and the ties at it are gathered — ties in index order only when there are more of them than places left.
constexpr int TK_CAP = 1024;
template <int NJ>
__global__ __launch_bounds__(256) void mask_topk_reg_kernel(float* logits, int R, int n, int i0, const int64_t* seen,
                                                            int T, int K, float* out_val, int32_t* out_idx) {
    __shared__ int wcnt[2][4];
    __shared__ int cnt_gt, cnt_eq;
    __shared__ float cval[128];
    __shared__ int cidx[128];
    __shared__ int wave_eq[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float* x = logits + (long)row * n;
    if (seen) {
        for (int t = tid; t < T; t += 256) {
            const long id = seen[(long)row * T + t] - i0;
            if (id >= 0 && id < n) x[id] = -INFINITY;
        }
        __syncthreads();
    }
    // The row as aligned 16-byte pieces (a row of odd length starts anywhere): piece q = tid + 256 jq of the pieces from the aligned
    // address below the row's first element; register j = 4 jq + c holds element  i = 4 q + c - d  (d = the row's offset into its
    // first piece), or key 0 — below every float's key — outside the row.  (4-byte loads: 256 bytes per wave instruction, 1.3 TB/s.)
    static_assert(NJ % 4 == 0, "registers in groups of one piece");
    const long e0 = (long)row * n;
    const int d = (int)(e0 & 3);
    const float4* xa = reinterpret_cast<const float4*>(logits + (e0 - d));
    const int npiece = (n + d + 3) >> 2;
    auto elem = [&](int j) { return 4 * (tid + 256 * (j >> 2)) + (j & 3) - d; };
    uint32_t key[NJ];
#pragma unroll
    for (int jq = 0; jq < NJ / 4; ++jq) {
        const int q = tid + 256 * jq;
        const float4 v = xa[min(q, npiece - 1)];
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = 4 * q + c - d;
            key[4 * jq + c] = (i >= 0 && i < n) ? float_key(vv[c]) : 0u;
        }
    }
    const int Keff = min(K, n);
    // ---- fast path: candidates at or above the K-th largest thread maximum ----------------------------------------------------------
    __shared__ __attribute__((aligned(16))) uint32_t ckey[TK_CAP];
    __shared__ __attribute__((aligned(16))) int cix[TK_CAP];
    __shared__ int ccount;
    {
        uint32_t tmax = key[0];
#pragma unroll
        for (int j = 1; j < NJ; ++j) tmax = max(tmax, key[j]);
        // L = the Keff-th largest of the 256 maxima: ONE wave searches it bit by bit on four values per lane (ballots only, no
        // workgroup barrier per bit)
        __shared__ uint32_t tmx[256];
        __shared__ uint32_t Lsh;
        tmx[tid] = tmax;
        __syncthreads();
        if (w == 0) {
            const uint32_t m0 = tmx[lane], m1 = tmx[lane + 64], m2 = tmx[lane + 128], m3 = tmx[lane + 192];
            uint32_t Lw = 0u;
            for (int bit = 31; bit >= 0; --bit) {
                const uint32_t cand = Lw | (1u << bit);
                const int c = __popcll(__ballot(m0 >= cand)) + __popcll(__ballot(m1 >= cand)) + __popcll(__ballot(m2 >= cand)) +
                              __popcll(__ballot(m3 >= cand));
                if (c >= Keff) Lw = cand;
            }
            if (lane == 0) Lsh = Lw;
        }
        __syncthreads();
        const uint32_t L = Lsh;
        int c = 0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) c += __popcll(__ballot(key[j] >= L));
        if (tid == 0) ccount = 0;
        if (lane == 0) wcnt[0][w] = c;
        __syncthreads();
        const int C = wcnt[0][0] + wcnt[0][1] + wcnt[0][2] + wcnt[0][3];
        if (C <= TK_CAP) {
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (key[j] >= L) {
                    const int pos = atomicAdd(&ccount, 1);
                    ckey[pos] = key[j]; cix[pos] = elem(j);
                }
            __syncthreads();
            if (C <= 256) {
                // few candidates (the usual case): every thread ranks its own candidate against all of them — its rank in (key
                // descending, index ascending) is its place in the output; no sort, no further barrier
                for (int i = tid; i < K; i += 256) { if (i >= Keff) { out_val[(long)row * K + i] = -INFINITY; out_idx[(long)row * K + i] = -1; } }
                // (the list is read four candidates per LDS instruction, two such groups in flight: one 32-bit read per candidate
                //  and iteration was a chain of ~C LDS round trips)
                if (tid < 4) { ckey[C + tid] = 0u; cix[C + tid] = 0x7fffffff; }      // (C <= 256 < TK_CAP - 4) padding: precedes nobody
                __syncthreads();
                if (tid < C) {
                    const uint32_t a = ckey[tid];
                    const int ia = cix[tid];
                    int rank = 0;
#pragma unroll 2
                    for (int q = 0; q < C; q += 4) {
                        const uint4 b = *reinterpret_cast<const uint4*>(ckey + q);
                        const int4 ib = *reinterpret_cast<const int4*>(cix + q);
                        rank += ((b.x > a) || (b.x == a && ib.x < ia)) ? 1 : 0;
                        rank += ((b.y > a) || (b.y == a && ib.y < ia)) ? 1 : 0;
                        rank += ((b.z > a) || (b.z == a && ib.z < ia)) ? 1 : 0;
                        rank += ((b.w > a) || (b.w == a && ib.w < ia)) ? 1 : 0;
                    }
                    if (rank < Keff) { out_val[(long)row * K + rank] = key_float(a); out_idx[(long)row * K + rank] = ia + i0; }
                }
                return;
            }
            int P2 = 512;
            while (P2 < C) P2 <<= 1;
            for (int t = C + tid; t < P2; t += 256) { ckey[t] = 0u; cix[t] = 0x7fffffff; }
            __syncthreads();
            for (int k = 2; k <= P2; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int t = tid; t < P2; t += 256) {
                        const int ixj = t ^ j;
                        if (ixj > t) {
                            const uint32_t a = ckey[t], b = ckey[ixj];
                            const int ia = cix[t], ib = cix[ixj];
                            const bool a_first = (a > b) || (a == b && ia < ib);
                            const bool up = (t & k) == 0;
                            if (up ? !a_first : a_first) { ckey[t] = b; ckey[ixj] = a; cix[t] = ib; cix[ixj] = ia; }
                        }
                    }
                    __syncthreads();
                }
            for (int i = tid; i < K; i += 256) {
                out_val[(long)row * K + i] = i < Keff ? key_float(ckey[i]) : -INFINITY;
                out_idx[(long)row * K + i] = i < Keff ? cix[i] + i0 : -1;
            }
            return;
        }
        __syncthreads();
    }
    // ---- the K-th largest key: the largest P with |{key >= P}| >= K -------------------------------------------------------------
    uint32_t prefix = 0u;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = prefix | (1u << bit);
        int c = 0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) c += __popcll(__ballot(key[j] >= cand));     // wave total (scalar unit)
        if (lane == 0) wcnt[bit & 1][w] = c;
        __syncthreads();                                                             // (two buffers: one barrier per round)
        const int tot = wcnt[bit & 1][0] + wcnt[bit & 1][1] + wcnt[bit & 1][2] + wcnt[bit & 1][3];
        if (tot >= Keff) prefix = cand;
    }
    // ---- gather: keys above the prefix (any order), ties at the prefix (the `remaining` lowest indices) ----------------------------
    if (tid == 0) { cnt_gt = 0; cnt_eq = 0; }
    if (tid < 128) { cval[tid] = -INFINITY; cidx[tid] = 0x7fffffff; }
    int c_gt = 0, c_eq = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) { c_gt += __popcll(__ballot(key[j] > prefix)); c_eq += __popcll(__ballot(key[j] == prefix)); }
    __syncthreads();
    if (lane == 0) { atomicAdd(&cnt_gt, c_gt); atomicAdd(&cnt_eq, c_eq); }
    __syncthreads();
    const int n_gt = cnt_gt, n_eq = cnt_eq, remaining = Keff - n_gt;
    __syncthreads();
    if (tid == 0) { cnt_gt = 0; cnt_eq = 0; }
    __syncthreads();
    const bool all_ties = n_eq <= remaining;     // (n_eq >= remaining by construction: == means every tie is taken)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int i = elem(j);
        if (key[j] > prefix) {
            const int pos = atomicAdd(&cnt_gt, 1);
            if (pos < 128) { cval[pos] = key_float(key[j]); cidx[pos] = i; }
        } else if (all_ties && key[j] == prefix && i >= 0 && i < n) {
            const int pos = n_gt + atomicAdd(&cnt_eq, 1);
            if (pos < 128) { cval[pos] = key_float(key[j]); cidx[pos] = i; }
        }
    }
    if (!all_ties) {      // more ties than places: index order — one pass per 1024 consecutive elements (a thread's piece = 4 of them)
#pragma unroll 1
        for (int jq = 0; jq < NJ / 4; ++jq) {
            uint32_t k4[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int q = 0; q < NJ / 4; ++q)
#pragma unroll
                for (int c = 0; c < 4; ++c) k4[c] = q == jq ? key[4 * q + c] : k4[c];
            const int ibase = 4 * (tid + 256 * jq) - d;
            bool eq[4];
            int below = 0, wtot = 0, own = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                eq[c] = k4[c] == prefix && ibase + c >= 0 && ibase + c < n;
                const unsigned long long bal = __ballot(eq[c]);
                below += __popcll(bal & ((1ull << lane) - 1ull));
                wtot += __popcll(bal);
            }
            if (lane == 0) wave_eq[w] = wtot;
            __syncthreads();
            int offs = cnt_eq + below;
            for (int ww = 0; ww < w; ++ww) offs += wave_eq[ww];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (eq[c]) {
                    const int pos = offs + own;
                    if (pos < remaining) { cval[n_gt + pos] = key_float(prefix); cidx[n_gt + pos] = ibase + c; }
                    ++own;
                }
            }
            __syncthreads();
            if (tid == 0) cnt_eq += wave_eq[0] + wave_eq[1] + wave_eq[2] + wave_eq[3];
            __syncthreads();
        }
    }
    __syncthreads();
    // bitonic sort of 128 candidates by (value desc, index asc)
    for (int k = 2; k <= 128; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (tid < 128) {
                const int ixj = tid ^ j;
                if (ixj > tid) {
                    const float a = cval[tid], b = cval[ixj];
                    const int ia = cidx[tid], ib = cidx[ixj];
                    const bool a_first = (a > b) || (a == b && ia < ib);  // a should precede b
                    const bool up = (tid & k) == 0;
                    if (up ? !a_first : a_first) { cval[tid] = b; cval[ixj] = a; cidx[tid] = ib; cidx[ixj] = ia; }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < K; i += 256) {
        out_val[(long)row * K + i] = i < Keff ? cval[i] : -INFINITY;
        out_idx[(long)row * K + i] = i < Keff ? cidx[i] + i0 : -1;
    }
}

// candidates [S][R][K] -> global top-K by (value desc, index asc); S*K <= 1024
// counts (optional, [R]): the first counts[row] slots of a row's S*K (slot j = list j / K, place j % K) hold candidates, the rest
// is unwritten memory (the fused evaluation scoring appends candidates: k_eval_topk.hip); a row whose count exceeds S*K is left
// to that file's exact fallback kernel and not written here.
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* cand_val, const int32_t* cand_idx, int S, int R,
                                                         int K, float* out_val, int32_t* out_idx, const int32_t* counts) {
    __shared__ float v[1024];
    __shared__ int ix[1024];
    const int row = blockIdx.x, tid = threadIdx.x;
    int n = S * K;
    if (counts) {
        const int c = counts[row];
        if (c < 0 || c > n) return;
        n = c;
    }
    {   // the four slots of a thread: all eight loads out before the first use (slot index clamped: no load behind a branch)
        int id4[4]; float v4[4];
        const int SK = S * K;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = min(tid + 256 * j, SK - 1), s = i / K, k = i - s * K;
            id4[j] = cand_idx[((long)s * R + row) * K + k];
            v4[j] = cand_val[((long)s * R + row) * K + k];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(id4[j]), "+v"(v4[j]));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = tid + 256 * j;
            const bool ok = i < n && id4[j] >= 0;
            v[i] = ok ? v4[j] : -INFINITY;
            ix[i] = ok ? id4[j] : 0x7fffffff;
        }
    }
    // Fast path (any input order; as in mask_topk_reg_kernel): a thread looks at its <= 4 candidates, the K-th largest of the 256 thread
    // maxima is a lower bound of the K-th largest candidate, the candidates at or above it — a few hundred — are compacted and each
    // one's rank among them, in (value descending, index ascending), is its place in the output.  ~3 us instead of the 42 us of the
    // 1024-element bitonic sort below, which stays for inputs with more than 256 candidates above the bound (tie blocks).
    {
        __shared__ uint32_t tmx[256];
        __shared__ uint32_t Lsh;
        __shared__ __attribute__((aligned(16))) uint32_t ckey[264];
        __shared__ __attribute__((aligned(16))) int cix[264];
        __shared__ int ccount, wsum[4];
        const int lane = tid & 63, w = tid >> 6;
        const int Keff = min(K, n);
        uint32_t key[4];
        int kid[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + 256 * q;      // (n <= 1024)
            const bool ok = i < n && ix[i] != 0x7fffffff;
            key[q] = ok ? float_key(v[i]) : 0u;
            kid[q] = ok ? ix[i] : 0x7fffffff;
        }
        tmx[tid] = max(max(key[0], key[1]), max(key[2], key[3]));
        if (tid == 0) ccount = 0;
        __syncthreads();
        if (w == 0) {
            const uint32_t m0 = tmx[lane], m1 = tmx[lane + 64], m2 = tmx[lane + 128], m3 = tmx[lane + 192];
            uint32_t Lw = 0u;
            for (int bit = 31; bit >= 0; --bit) {
                const uint32_t cand = Lw | (1u << bit);
                const int c = __popcll(__ballot(m0 >= cand)) + __popcll(__ballot(m1 >= cand)) + __popcll(__ballot(m2 >= cand)) +
                              __popcll(__ballot(m3 >= cand));
                if (c >= Keff) Lw = cand;
            }
            if (lane == 0) Lsh = Lw;
        }
        __syncthreads();
        const uint32_t L = max(Lsh, 1u);      // (key 0: invalid / absent candidates never qualify)
        int c = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) c += __popcll(__ballot(key[q] >= L));
        if (lane == 0) wsum[w] = c;
        __syncthreads();
        const int C = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (C <= 256) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (key[q] >= L) {
                    const int pos = atomicAdd(&ccount, 1);
                    ckey[pos] = key[q]; cix[pos] = kid[q];
                }
            for (int i = tid; i < K; i += blockDim.x) { out_val[(long)row * K + i] = -INFINITY; out_idx[(long)row * K + i] = -1; }
            __syncthreads();
            if (tid < 4) { ckey[C + tid] = 0u; cix[C + tid] = 0x7fffffff; }
            __syncthreads();
            if (tid < C) {
                const uint32_t a = ckey[tid];
                const int ia = cix[tid];
                int rank = 0;
#pragma unroll 2
                for (int q = 0; q < C; q += 4) {
                    const uint4 b = *reinterpret_cast<const uint4*>(ckey + q);
                    const int4 ib = *reinterpret_cast<const int4*>(cix + q);
                    // (a repeated (value, index) pair: the copy that sits first in the list goes first)
                    rank += ((b.x > a) || (b.x == a && (ib.x < ia || (ib.x == ia && q < tid)))) ? 1 : 0;
                    rank += ((b.y > a) || (b.y == a && (ib.y < ia || (ib.y == ia && q + 1 < tid)))) ? 1 : 0;
                    rank += ((b.z > a) || (b.z == a && (ib.z < ia || (ib.z == ia && q + 2 < tid)))) ? 1 : 0;
                    rank += ((b.w > a) || (b.w == a && (ib.w < ia || (ib.w == ia && q + 3 < tid)))) ? 1 : 0;
                }
                if (rank < K) { out_val[(long)row * K + rank] = key_float(a); out_idx[(long)row * K + rank] = ia; }
            }
            return;
        }
        __syncthreads();
    }
    for (int k = 2; k <= 1024; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < 1024; t += blockDim.x) {
                const int ixj = t ^ j;
                if (ixj > t) {
                    const float a = v[t], b = v[ixj];
                    const int ia = ix[t], ib = ix[ixj];
                    const bool a_first = (a > b) || (a == b && ia < ib);
                    const bool up = (t & k) == 0;
                    if (up ? !a_first : a_first) { v[t] = b; v[ixj] = a; ix[t] = ib; ix[ixj] = ia; }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < K; i += blockDim.x) {
        out_val[(long)row * K + i] = v[i];
        out_idx[(long)row * K + i] = ix[i] == 0x7fffffff ? -1 : ix[i];
    }
}

__global__ void rank_metrics_kernel(const int32_t* topk, int R, int K, const int64_t* label, float* metrics) {
    __shared__ float red[8];
    float h10 = 0, h50 = 0, h100 = 0, n10 = 0, n50 = 0, n100 = 0;
    for (int r = threadIdx.x; r < R; r += blockDim.x) {
        const int lab = (int)label[r];
        int rank = -1;
        for (int k = 0; k < K && k < 100; ++k)
            if (topk[(long)r * K + k] == lab) { rank = k; break; }
        if (rank >= 0) {
            const float gain = 1.0f / log2f((float)rank + 2.0f);
            if (rank < 10) { h10 += 1; n10 += gain; }
            if (rank < 50) { h50 += 1; n50 += gain; }
            h100 += 1; n100 += gain;
        }
    }
    float vals[6] = {h10, h50, h100, n10, n50, n100};
    for (int i = 0; i < 6; ++i) {
        const float t = block_sum(vals[i], red);
        if (threadIdx.x == 0) metrics[i] += t;
    }
}

}  // namespace

extern "C" int edgl_mask_topk(float* logits, int R, int n, int i0, const int64_t* seen, int T, int K, float* out_val,
                              int32_t* out_idx, void* stream) {
    EDGL_REQUIRE(logits && out_val && out_idx, EDGL_ERR_NULL, "edgl_mask_topk: null pointer");
    EDGL_REQUIRE(R > 0 && n > 0 && K > 0 && K <= 128, EDGL_ERR_SHAPE, "edgl_mask_topk: bad shape R=%d n=%d K=%d", R, n, K);
    static const int reg_form = edgl_env_int("EDGL_TOPK_REG", 1);
    hipStream_t st = (hipStream_t)stream;
    if (reg_form && n <= 256 * 16 - 8) hipLaunchKernelGGL(mask_topk_reg_kernel<16>, dim3(R), dim3(256), 0, st, logits, R, n, i0, seen, T, K, out_val, out_idx);
    else if (reg_form && n <= 256 * 40 - 8) hipLaunchKernelGGL(mask_topk_reg_kernel<40>, dim3(R), dim3(256), 0, st, logits, R, n, i0, seen, T, K, out_val, out_idx);
    else if (reg_form && n <= 256 * 80 - 8) hipLaunchKernelGGL(mask_topk_reg_kernel<80>, dim3(R), dim3(256), 0, st, logits, R, n, i0, seen, T, K, out_val, out_idx);
    else hipLaunchKernelGGL(mask_topk_kernel, dim3(R), dim3(256), 0, st, logits, R, n, i0, seen, T, K, out_val, out_idx);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_topk_merge(const float* cand_val, const int32_t* cand_idx, int S, int R, int K, float* out_val,
                               int32_t* out_idx, void* stream) {
    EDGL_REQUIRE(cand_val && cand_idx && out_val && out_idx, EDGL_ERR_NULL, "edgl_topk_merge: null pointer");
    EDGL_REQUIRE(S > 0 && R > 0 && K > 0 && S * K <= 1024, EDGL_ERR_SHAPE, "edgl_topk_merge: S*K=%d > 1024", S * K);
    hipLaunchKernelGGL(topk_merge_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, cand_val, cand_idx, S, R, K, out_val, out_idx,
                       (const int32_t*)nullptr);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_rank_metrics(const int32_t* topk_idx, int R, int K, const int64_t* label, float* metrics, void* stream) {
    EDGL_REQUIRE(topk_idx && label && metrics, EDGL_ERR_NULL, "edgl_rank_metrics: null pointer");
    hipLaunchKernelGGL(rank_metrics_kernel, dim3(1), dim3(512), 0, (hipStream_t)stream, topk_idx, R, K, label, metrics);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
