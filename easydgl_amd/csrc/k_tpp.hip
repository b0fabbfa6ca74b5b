// The TPP likelihood regulariser (K8: temporal.py:317-333 + EasyDGL.py:157-175) as launches of its own: forward / backward pair,
// the one-launch forms with the gradient (per sequence, per masked slot, any number of marks), the normaliser, the slot data of
// the fused form (bimau_common.h: TppDesc) and the reduction of that form's partial sums.
#include "edgl_common.h"
#include "bimau_common.h"   // TppDesc / tpp_layout: slot data of the fused TPP form
#include "batch_prep.h"     // slot data of a sample (also run inside the encoder's launch)
#include "tpp_math.h"       // interval and mark count, shared with batch_prep.h

namespace {

constexpr int RED_BLOCKS = 256;   // per-block partials of edgl_tpp_fwd (one row per thread at the headline size)

struct TppP {
    const float* lam; const int64_t* mpos; const int64_t* labels; const float* ts; const uint8_t* mtab;
    int B, T, H, E, M; float coef;
};

using tpp_math::mark_word_count;
using tpp_math::raw_span;   // EasyDGL.py:161-162 on RAW seconds

// interval of position pos of sample b: masked-position mode (EasyDGL.py:157-175) or, with mpos == NULL, every position of the
// sequence (CTSMA.py:95-108: M == T, ts holds T+1 raw timestamps per row and the interval is the plain forward difference)
__device__ __forceinline__ float tpp_interval(const TppP& p, int b, int pos) {
    return p.mpos ? raw_span(p.ts + (long)b * p.T, pos, p.T)
                  : p.ts[(long)b * (p.T + 1) + pos + 1] - p.ts[(long)b * (p.T + 1) + pos];
}
// regulariser from the two sums and the normaliser c (temporal.py:331-332, EasyDGL.py:175); one thread
__device__ __forceinline__ void tpp_reg_store(float a, float b, float c, float coef, float* sums, float* reg_out, int accumulate) {
    sums[0] = a; sums[1] = b; sums[2] = c;
    const float reg = coef * (-(a - b) / c);
    reg_out[0] = accumulate ? reg_out[0] + reg : reg;
}

// per-row terms; returns (event_ll, non_event, n_marks); optionally the pieces needed by the backward
__device__ __forceinline__ void tpp_row(const TppP& p, long j, float& ev_ll, float& non_ev, float& nmk, float* ev_out,
                                        float* span_out, float* g_out, int* b_out, int* pos_out, int64_t* lab_out) {
    const long bp = j / p.M;
    const int m = (int)(j % p.M), b = (int)(bp % p.B);
    const int pos = p.mpos ? (int)p.mpos[(long)b * p.M + m] : m;
    const int64_t lab = p.labels[(long)b * p.M + m];
    const uint8_t* nm = p.mtab + lab * p.E;
    const float* lm = p.lam + (bp * p.T + pos) * p.E;
    float cnt = 0.f, ev = 0.f, ent = 0.f;
    for (int e = 0; e < p.E; ++e) { const float f = (float)nm[e]; cnt += f; ev += lm[e] * f; ent += lm[e]; }
    const float g = cnt > 0.f ? 1.f : 0.f;  // sign(sum nm), temporal.py:321
    ev *= g; ent *= g;
    const float sp = tpp_interval(p, b, pos);
    ev_ll = __logf(ev == 0.f ? 1.f : ev);  // :324
    non_ev = ent * sp * 0.5f;              // :327-328
    nmk = cnt;
    if (ev_out) { *ev_out = ev; *span_out = sp; *g_out = g; *b_out = b; *pos_out = pos; *lab_out = lab; }
}

__global__ __launch_bounds__(256) void tpp_partial_kernel(TppP p, float* part) {
    __shared__ float red[8];
    const long n = (long)p.H * p.B * p.M;
    float a = 0.f, bsum = 0.f, c = 0.f;
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (long)gridDim.x * blockDim.x) {
        float e, ne, k;
        tpp_row(p, j, e, ne, k, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        a += e; bsum += ne; c += k;
    }
    a = block_sum(a, red); bsum = block_sum(bsum, red); c = block_sum(c, red);
    if (threadIdx.x == 0) { part[blockIdx.x * 3] = a; part[blockIdx.x * 3 + 1] = bsum; part[blockIdx.x * 3 + 2] = c; }
}
__global__ void tpp_final_kernel(const float* part, int nblk, float coef, float* sums, float* reg_out, int accumulate) {
    // one wave: lane i adds partials i, i+64, ... in index order, then a fixed xor tree — deterministic
    float a = 0.f, b = 0.f, c = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 64) { a += part[i * 3]; b += part[i * 3 + 1]; c += part[i * 3 + 2]; }
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
    if (threadIdx.x != 0) return;
    tpp_reg_store(a, b, c, coef, sums, reg_out, accumulate);
}
__global__ __launch_bounds__(256) void tpp_bwd_kernel(TppP p, const float* sums, const float* gscale, float* d_lam) {
    const long n = (long)p.H * p.B * p.M;
    const float gs = gscale ? gscale[0] : 1.f;
    const float k = -gs * p.coef / sums[2];
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (long)gridDim.x * blockDim.x) {
        float e, ne, cnt, ev, sp, g; int b, pos; int64_t lab;
        tpp_row(p, j, e, ne, cnt, &ev, &sp, &g, &b, &pos, &lab);
        const long bp = j / p.M;
        const uint8_t* nm = p.mtab + lab * p.E;
        float* dst = d_lam + (bp * p.T + pos) * p.E;
        for (int q = 0; q < p.E; ++q) {
            const float dev = (ev != 0.f) ? (float)nm[q] / ev : 0.f;
            dst[q] = k * g * (dev - sp * 0.5f);
        }
    }
}

// Regulariser and its gradient for the training engine (edgl_tpp_fwd_bwd): d lambda is written for EVERY (b', position) row —
// zeros where the position is not masked, so the [H*B*T, E] gradient needs no memset, and the slots of a repeated masked
// position are summed (the gradient of tf.gather).  The normaliser c = sum of mark counts depends on the labels only and is
// computed first by one small workgroup (exact: integer counts), which removes the partial -> final -> gradient chain of
// launches.  (No last-workgroup-done reduction for the scalar sums: on this multi-XCD part every __threadfence() is an L2
// write-back — 2048 of them cost 50 us; a 64-thread final kernel costs 5.)
// one label per thread; integer atomics: exact and order-independent, hence deterministic
__global__ __launch_bounds__(256) void tpp_norm_kernel(TppP p, int* acc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int cnt = 0;
    if (i < p.B * p.M) {
        const uint8_t* nm = p.mtab + p.labels[i] * p.E;
        if (p.E == 16 && ((uintptr_t)p.mtab & 15) == 0) {
            const uint4 w = *reinterpret_cast<const uint4*>(nm);
            const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) cnt += (int)mark_word_count(ws[j]);
        } else {
            for (int e = 0; e < p.E; ++e) cnt += nm[e];
        }
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(acc, cnt);
}
// The same count by ONE workgroup (batches up to 64 K labels): strided labels per thread, integer block sum, a plain store — no
// memset launch in front of it and nothing stale to inherit (the memset of the atomic form was a 6 us launch of its own in the
// side-stream chain the first attention kernel waits for).
// (nz != NULL: also the number of labels != 0 — the weighted rows of the loss, EasyDGL.py:183-185 — for edgl_dp_counts)
__global__ __launch_bounds__(1024) void tpp_norm_one_kernel(TppP p, int* acc, int* nz) {
    __shared__ int red[16];
    int cnt = 0, cnz = 0;
    const int n = p.B * p.M;
    constexpr int NB = 8;   // labels per thread and round: all label loads of a round fly together, then all mark rows (two round
                            // trips per 8 K labels; one label -> one mark row at a time was a chain of 2 x 10 round trips: 20 us)
    for (int i0 = threadIdx.x; i0 < n; i0 += 1024 * NB) {
        int64_t lab[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) lab[j] = p.labels[min(i0 + j * 1024, n - 1)];
#pragma unroll
        for (int j = 0; j < NB; ++j) asm volatile("" : "+v"(lab[j]));
#pragma unroll
        for (int j = 0; j < NB; ++j) cnz += (i0 + j * 1024 < n && lab[j] != 0) ? 1 : 0;
        if (p.E == 16 && ((uintptr_t)p.mtab & 15) == 0) {
            uint4 w[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) w[j] = *reinterpret_cast<const uint4*>(p.mtab + lab[j] * 16);
#pragma unroll
            for (int j = 0; j < NB; ++j) asm volatile("" : "+v"(w[j].x), "+v"(w[j].y), "+v"(w[j].z), "+v"(w[j].w));
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                if (i0 + j * 1024 < n) {
                    const uint32_t ws[4] = {w[j].x, w[j].y, w[j].z, w[j].w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) cnt += (int)mark_word_count(ws[q]);
                }
            }
        } else {
            for (int j = 0; j < NB; ++j)
                if (i0 + j * 1024 < n) {
                    const uint8_t* nm = p.mtab + lab[j] * p.E;
                    for (int e = 0; e < p.E; ++e) cnt += nm[e];
                }
        }
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < 16; ++w) t += red[w];
        acc[0] = t;
    }
    if (nz) {
        __syncthreads();
        for (int o = 32; o > 0; o >>= 1) cnz += __shfl_xor(cnz, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnz;
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
            for (int w = 0; w < 16; ++w) t += red[w];
            nz[0] = t;
        }
    }
}

// ---- the 16-register forms (E <= 16: the marks of a slot unrolled over 16 registers) --------------------------------------------
// the first 16 lambda values of a row, clamped loads (E < 16: the last one repeats and is masked out in tpp_slot)
__device__ __forceinline__ void tpp_lam16(const TppP& p, long row, float lam[16]) {
#pragma unroll
    for (int e = 0; e < 16; ++e) { lam[e] = p.lam[row * p.E + min(e, p.E - 1)]; asm volatile("" : "+v"(lam[e])); }
}
// the E mark bytes of a label as four words: one 16-byte load (E == 16), else E clamped byte loads — all unconditional
// (a select around a load becomes a branch: dependent round trips)
__device__ __forceinline__ void tpp_mark_words(const TppP& p, const uint8_t* nm, uint32_t mw[4]) {
    if (p.E == 16 && ((uintptr_t)p.mtab & 15) == 0) {
        const uint4 w = *reinterpret_cast<const uint4*>(nm);
        mw[0] = w.x; mw[1] = w.y; mw[2] = w.z; mw[3] = w.w;
    } else {
        uint32_t by[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) { by[e] = nm[min(e, p.E - 1)]; asm volatile("" : "+v"(by[e])); }
#pragma unroll
        for (int j = 0; j < 4; ++j) mw[j] = by[4 * j] | (by[4 * j + 1] << 8) | (by[4 * j + 2] << 16) | (by[4 * j + 3] << 24);
    }
}
// terms of one slot: its event log-likelihood and non-event term; its gradient row is ADDED to gr (k = -coef / normaliser)
__device__ __forceinline__ void tpp_slot(const TppP& p, const uint32_t mw[4], const float lam[16], float sp, float k, float& ev_ll,
                                         float& non_ev, float gr[16]) {
    float cnt = 0.f, ev = 0.f, ent = 0.f, f[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        f[e] = e < p.E ? (float)((mw[e >> 2] >> (8 * (e & 3))) & 0xffu) : 0.f;
        cnt += f[e]; ev += lam[e] * f[e]; ent += e < p.E ? lam[e] : 0.f;
    }
    const float g = cnt > 0.f ? 1.f : 0.f;  // sign(sum nm), temporal.py:321
    ev *= g; ent *= g;
    ev_ll = __logf(ev == 0.f ? 1.f : ev);      // :324
    non_ev = ent * sp * 0.5f;                  // :327-328
    const float iev = ev != 0.f ? 1.0f / ev : 0.f, kg = k * g, hs = sp * 0.5f;
#pragma unroll
    for (int e = 0; e < 16; ++e) gr[e] += kg * (f[e] * iev - hs);
}

constexpr int TPP_MAXM = 256, TPP_MAXT = 1024, TPP_FUSED_BLOCKS = 2048;   // (4096 one-sequence workgroups measured slower: 24 vs 19 us)
__global__ __launch_bounds__(128) void tpp_fused_kernel(TppP p, const float* sums, float* part, float* d_lam) {
    __shared__ float red[8];
    __shared__ int s_pos[TPP_MAXM];
    __shared__ int s_lab[TPP_MAXM];
    __shared__ int s_head[TPP_MAXT];
    __shared__ __attribute__((aligned(16))) float s_out[2][64 * 16];   // per wave: 64 gradient rows, for coalesced stores
    const float c = (float)reinterpret_cast<const int*>(sums)[4] * (float)p.H;   // tpp_norm_kernel
    const float k = -p.coef / c;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float a = 0.f, bsum = 0.f;
    for (int bp = blockIdx.x; bp < p.H * p.B; bp += gridDim.x) {
        const int b = bp % p.B;
        __syncthreads();
        for (int m = threadIdx.x; m < p.M; m += blockDim.x) {
            s_pos[m] = p.mpos ? (int)p.mpos[(long)b * p.M + m] : m;
            s_lab[m] = (int)p.labels[(long)b * p.M + m];
        }
        for (int t = threadIdx.x; t < p.T; t += blockDim.x) s_head[t] = 0x7fffffff;
        __syncthreads();
        // first slot of every position (integer atomicMin: order-independent); unmasked positions — two thirds of the rows —
        // then skip the slot search altogether, and further slots of a repeated position are searched from the first one on
        for (int m = threadIdx.x; m < p.M; m += blockDim.x) {
            const int pos = s_pos[m];
            if (pos >= 0 && pos < p.T) atomicMin(&s_head[pos], m);
        }
        __syncthreads();
        for (int t0 = 0; t0 < p.T; t0 += blockDim.x) {
            const int t = t0 + threadIdx.x;
            const long row = (long)bp * p.T + min(t, p.T - 1);
            float lam[16], gr[16];
            bool loaded = false;
#pragma unroll
            for (int e = 0; e < 16; ++e) gr[e] = 0.f;
            // slots of this position: the search is a cheap LDS scan; the heavy part below runs once per FOUND slot, so the
            // lanes of a wave do their first (usually only) slot together instead of one lane per loop iteration
            const int m_hi = t >= p.T ? 0 : p.M;
            int m = -1, nxt = t < p.T ? s_head[t] : 0x7fffffff;
            for (;;) {
                if (nxt >= m_hi) break;
                m = nxt;
                nxt = 0x7fffffff;
                if (p.mpos)                              // another slot of the same position (rare; none in all-position mode)
                    for (int q = m + 1; q < m_hi; ++q)
                        if (s_pos[q] == t) { nxt = q; break; }
                if (!loaded) {
                    tpp_lam16(p, row, lam);
                    loaded = true;
                }
                uint32_t mw[4];
                tpp_mark_words(p, p.mtab + (long)s_lab[m] * p.E, mw);
                float ll, ne;
                tpp_slot(p, mw, lam, tpp_interval(p, b, t), k, ll, ne, gr);
                a += ll; bsum += ne;
            }
            if (d_lam) {
                if (p.E == 16) {
                    // 64 rows x 64 bytes of a wave are contiguous in d_lam: through LDS so that a store instruction
                    // writes 1 KB of consecutive bytes (lane = one 16-byte piece) instead of 64 scattered pieces
                    float* so = s_out[wave];
#pragma unroll
                    for (int e = 0; e < 16; e += 4)
                        *reinterpret_cast<float4*>(so + lane * 16 + e) = make_float4(gr[e], gr[e + 1], gr[e + 2], gr[e + 3]);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    const int row_w0 = t0 + wave * 64;                       // first position of this wave
                    const int nrows = min(64, p.T - row_w0);                 // <= 0: nothing to store
                    float* dst = d_lam + ((long)bp * p.T + row_w0) * 16;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int piece = i * 64 + lane;                     // 16-byte piece index in the wave's 4 KB
                        if (piece < nrows * 4) *reinterpret_cast<float4*>(dst + piece * 4) = *reinterpret_cast<const float4*>(so + piece * 4);
                    }
                    __builtin_amdgcn_wave_barrier();
                } else if (t < p.T) {
                    float* dst = d_lam + row * p.E;
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        if (e < p.E) dst[e] = gr[e];
                }
            }
        }
    }
    a = block_sum(a, red); bsum = block_sum(bsum, red);
    if (threadIdx.x == 0) { part[blockIdx.x * 2] = a; part[blockIdx.x * 2 + 1] = bsum; }
}
// The same regulariser and gradient with ONE THREAD PER MASKED SLOT (b', m), for a d lambda array that already holds zeros
// (edgl_bimau_fwd_zr fills it beside the lambda rows): only the rows of masked positions are written — 5 MB instead of the 26 MB
// of the headline step — and no position of the sequence is visited that carries no slot.  A position drawn into several slots
// (mask_random draws without replacement; padding rows can repeat position 0) is written once, by its FIRST slot, with the sum
// over its slots — the gradient of tf.gather; every slot adds its own term to the two loss sums.
__global__ __launch_bounds__(256) void tpp_rows_kernel(TppP p, const float* sums, float* part, float* d_lam) {
    __shared__ float red[8];
    __shared__ int s_pos[256], s_lab[256];
    const float c = (float)reinterpret_cast<const int*>(sums)[4] * (float)p.H;   // tpp_norm_kernel
    const float k = -p.coef / c;
    // M <= 256: a workgroup takes 256 / M whole (b', .) slot lists, positions and labels staged in LDS (the searches for the other
    // slots of a position are LDS reads; as global loads they were a chain of M dependent round trips: 17 us for 5 MB of work)
    const int G = p.M <= 256 ? 256 / p.M : 0;
    long bp; int m; bool active;
    if (G) {
        bp = (long)blockIdx.x * G + threadIdx.x / p.M; m = threadIdx.x % p.M;
        active = (int)threadIdx.x < G * p.M && bp < (long)p.H * p.B;
    } else {
        const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
        bp = j / p.M; m = (int)(j % p.M); active = j < (long)p.H * p.B * p.M;
    }
    const int b = (int)(bp % p.B);
    const int64_t* mp = (p.mpos && active) ? p.mpos + (long)b * p.M : nullptr;
    const int pos_in = !active ? 0 : (p.mpos ? (int)mp[m] : m);
    // a masked position outside [0, T) (malformed input, an uninitialised row after bind_batch): the slot is skipped, as the
    // fused kernel this one replaced did — never an out-of-bounds row of lambda / d lambda
    active = active && pos_in >= 0 && pos_in < p.T;
    const int pos = active ? pos_in : 0;
    const int lab = active ? (int)p.labels[(long)b * p.M + m] : 0;
    if (G) {
        s_pos[threadIdx.x] = active ? pos : -1 - (int)threadIdx.x;
        s_lab[threadIdx.x] = lab;
        __syncthreads();
    }
    float a = 0.f, bsum = 0.f;
    if (active) {
        const long row = bp * p.T + pos;
        float lam[16];
        if (p.E == 16) {
#pragma unroll
            for (int e = 0; e < 16; e += 4) {
                const float4 v = *reinterpret_cast<const float4*>(p.lam + row * 16 + e);
                lam[e] = v.x; lam[e + 1] = v.y; lam[e + 2] = v.z; lam[e + 3] = v.w;
            }
        } else {
            tpp_lam16(p, row, lam);
        }
        const float sp = tpp_interval(p, b, pos);
        // other slots of this position: any earlier one (then this slot is not the writer), any later one (rare)
        const int base = G ? (int)threadIdx.x - m : 0;
        bool head = true, later = false;
        if (p.mpos)
            for (int q = 0; q < p.M; ++q) {
                const bool same = (G ? s_pos[base + q] : (int)mp[q]) == pos;
                head = head && !(same && q < m);
                later = later || (same && q > m);
            }
        float gr[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) gr[e] = 0.f;
        // this slot, then (first slot of a repeated position only) the later slots of the same position
        const int q_end = (head && later) ? p.M : m + 1;
        for (int q = m; q < q_end; ++q) {
            if (q != m && (G ? s_pos[base + q] : (int)mp[q]) != pos) continue;
            const int lq = q == m ? lab : (G ? s_lab[base + q] : (int)p.labels[(long)b * p.M + q]);
            uint32_t mw[4];
            tpp_mark_words(p, p.mtab + (long)lq * p.E, mw);
            float ll, ne;
            tpp_slot(p, mw, lam, sp, k, ll, ne, gr);
            if (q == m) { a = ll; bsum = ne; }
        }
        if (head && d_lam) {
            float* dst = d_lam + row * p.E;
            if (p.E == 16) {
#pragma unroll
                for (int e = 0; e < 16; e += 4) *reinterpret_cast<float4*>(dst + e) = make_float4(gr[e], gr[e + 1], gr[e + 2], gr[e + 3]);
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (e < p.E) dst[e] = gr[e];
            }
        }
    }
    a = block_sum(a, red); bsum = block_sum(bsum, red);
    if (threadIdx.x == 0) { part[blockIdx.x * 2] = a; part[blockIdx.x * 2 + 1] = bsum; }
}
// tpp_rows_kernel for ANY number of mark types (the static engine with more than 16 marks: a data set's mark.pkl fixes E,
// EasyDGL.py:45-46): same contract — d lambda pre-zeroed, one thread per masked slot, a repeated position written once by its
// first slot with the sum over its slots — as plain loops over the marks (not the benchmarked shape: no staging, no vector loads).
__global__ __launch_bounds__(256) void tpp_rows_wide_kernel(TppP p, const float* sums, float* part, float* d_lam) {
    __shared__ float red[8];
    const float c = (float)reinterpret_cast<const int*>(sums)[4] * (float)p.H;
    const float k = -p.coef / c;
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool active = j < (long)p.H * p.B * p.M;
    const long bp = active ? j / p.M : 0;
    const int m = active ? (int)(j % p.M) : 0, b = (int)(bp % p.B);
    const int64_t* mp = p.mpos ? p.mpos + (long)b * p.M : nullptr;
    const int pos_in = !active ? 0 : (mp ? (int)mp[m] : m);
    active = active && pos_in >= 0 && pos_in < p.T;
    const int pos = active ? pos_in : 0;
    float a = 0.f, bsum = 0.f;
    if (active) {
        const long row = bp * p.T + pos;
        const float* lm = p.lam + row * p.E;
        const float sp = tpp_interval(p, b, pos);
        bool head = true;
        if (mp)
            for (int q = 0; q < m; ++q) head = head && (int)mp[q] != pos;
        for (int q = m; q < (head ? p.M : m + 1); ++q) {
            if (q != m && (!mp || (int)mp[q] != pos)) continue;
            const uint8_t* nm = p.mtab + p.labels[(long)b * p.M + q] * p.E;
            float cnt = 0.f, ev = 0.f, ent = 0.f;
            for (int e = 0; e < p.E; ++e) { const float f = (float)nm[e]; cnt += f; ev += lm[e] * f; ent += lm[e]; }
            const float g = cnt > 0.f ? 1.f : 0.f;
            ev *= g; ent *= g;
            if (q == m) { a = __logf(ev == 0.f ? 1.f : ev); bsum = ent * sp * 0.5f; }
            if (head && d_lam) {
                const float iev = ev != 0.f ? 1.0f / ev : 0.f, kg = k * g, hs = sp * 0.5f;
                float* dst = d_lam + row * p.E;
                for (int e = 0; e < p.E; ++e) dst[e] += kg * ((float)nm[e] * iev - hs);   // this thread owns the row
            }
        }
    }
    a = block_sum(a, red); bsum = block_sum(bsum, red);
    if (threadIdx.x == 0) { part[blockIdx.x * 2] = a; part[blockIdx.x * 2 + 1] = bsum; }
}
// Slot data of the fused TPP form (bimau_common.h: TppDesc): one workgroup per sample, one thread per masked slot.  A slot is
// EFFECTIVE when its position lies inside the sequence and its label's mark row is not empty (sign(sum nm) = 1, temporal.py:321) —
// the others add nothing to the regulariser or its gradient.  The first effective slot of a position fills the per-position
// arrays, further ones go to the sample's overflow list in slot order.  Labels, positions and timestamps only: runs ahead of
// the step's forward on a side stream.  E = 16 (one 16-byte mark row per label), M <= 256.
// Also the regulariser's normaliser, the mark count of ALL labels of the batch (temporal.py:330; what edgl_tpp_norm computes), as
// per-sample counts cntp[B] — every workgroup has its sample's mark rows in registers anyway; the consumers (one wave per (b, head) in
// sweep 1, the final reduction) add the B numbers up themselves: no launch, no memset, no atomics for it.
__global__ __launch_bounds__(256) void tpp_prep_kernel(const int64_t* mpos, const int64_t* labels, const float* ts, const uint8_t* mtab,
                                                       int B, int T, int M, char* desc) {
    extern __shared__ __attribute__((aligned(16))) char tpp_smem[];
    batch_prep::tpp_prep_sample(mpos, labels, ts, mtab, B, T, M, desc, (int)blockIdx.x, tpp_smem);
}
__global__ __launch_bounds__(256) void tpp_final2_kernel(const float* part, int nblk, float coef, int H, float* sums, float* reg_out,
                                                         int accumulate) {
    // one workgroup: thread i adds partials i, i+256, ... in index order, then the fixed block_sum tree — deterministic
    __shared__ float red[8];
    float a = 0.f, b = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 256) { a += part[i * 2]; b += part[i * 2 + 1]; }
    a = block_sum(a, red); b = block_sum(b, red);
    if (threadIdx.x != 0) return;
    const float c = (float)reinterpret_cast<const int*>(sums)[4] * (float)H;
    tpp_reg_store(a, b, c, coef, sums, reg_out, accumulate);
    reinterpret_cast<int*>(sums)[4] = 0;   // normaliser accumulator back to zero for the next call
}

// tpp_final2_kernel for the per-(b, head) partial sums of the fused form (thousands of pairs): 1024 threads, every thread's loads
// in flight together (the 256-thread loop above takes them one round trip at a time), the same fixed summation order per launch
// shape; the count slot is NOT cleared (sweep 1 of the same step reads it; edgl_tpp_norm stores it afresh every step).
__global__ __launch_bounds__(1024) void tpp_parts_kernel(const float* part, int nparts, float coef, int H, const int* cntp, int ncnt,
                                                         float* sums, float* reg_out, int accumulate) {
    __shared__ float red[16];
    __shared__ int redi[16];
    if (!cntp && ncnt < 0) {   // normaliser behind the partial sums, as edgl_bimau_bwd_tpp leaves it
        if (threadIdx.x == 0) reinterpret_cast<int*>(sums)[4] = reinterpret_cast<const int*>(part)[2 * nparts];
        __syncthreads();
    }
    if (cntp) {   // normaliser from the per-sample counts of edgl_tpp_prep (otherwise sums[4] holds it: edgl_tpp_norm, data parallel)
        int c = 0;
        for (int i = threadIdx.x; i < ncnt; i += 1024) c += cntp[i];
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if ((threadIdx.x & 63) == 0) redi[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
            for (int i = 0; i < 16; ++i) t += redi[i];
            reinterpret_cast<int*>(sums)[4] = t;
        }
        __syncthreads();
    }
    float a = 0.f, b = 0.f;
    for (int i0 = threadIdx.x; i0 < nparts; i0 += 1024 * 8) {
        float2 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = reinterpret_cast<const float2*>(part)[min(i0 + j * 1024, nparts - 1)];
#pragma unroll
        for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(v[j].x), "+v"(v[j].y));
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (i0 + j * 1024 < nparts) { a += v[j].x; b += v[j].y; }
    }
    a = block_sum(a, red); b = block_sum(b, red);
    if (threadIdx.x != 0) return;
    const float c = (float)reinterpret_cast<const int*>(sums)[4] * (float)H;
    tpp_reg_store(a, b, c, coef, sums, reg_out, accumulate);
}

// the arguments every launch of the regulariser itself shares: checked, then packed (`out`: reg_out, or d_lam of edgl_tpp_bwd)
int tpp_args(const char* who, const float* lam, const int64_t* masked_pos, const int64_t* labels, const float* ts_raw,
             const uint8_t* mark_table, int B, int T, int H, int E, int M, float coef, const float* sums, const float* out, TppP* p) {
    EDGL_REQUIRE(lam && labels && ts_raw && mark_table && sums && out, EDGL_ERR_NULL, "%s: null pointer", who);
    EDGL_REQUIRE(masked_pos || M == T, EDGL_ERR_SHAPE, "%s: all-position mode needs M == T", who);
    *p = TppP{lam, masked_pos, labels, ts_raw, mark_table, B, T, H, E, M, coef};
    return EDGL_OK;
}

}  // namespace

extern "C" int edgl_tpp_workspace(void) { return std::max(RED_BLOCKS * 3 + 4, 8 + 2 * 4096); }   // edgl_tpp_fwd_bwd: sums[8] + partial pairs

extern "C" int edgl_tpp_fwd(const float* lam, const int64_t* masked_pos, const int64_t* labels, const float* ts_raw,
                            const uint8_t* mark_table, int B, int T, int H, int E, int M, float coef, float* sums,
                            float* reg_out, int accumulate, void* stream) {
    TppP p;
    if (const int rc = tpp_args("edgl_tpp_fwd", lam, masked_pos, labels, ts_raw, mark_table, B, T, H, E, M, coef, sums, reg_out, &p)) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tpp_partial_kernel, dim3(RED_BLOCKS), dim3(256), 0, st, p, sums + 4);
    EDGL_LAUNCH_CHECK();
    hipLaunchKernelGGL(tpp_final_kernel, dim3(1), dim3(64), 0, st, sums + 4, RED_BLOCKS, coef, sums, reg_out, accumulate);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_tpp_bwd(const float* lam, const int64_t* masked_pos, const int64_t* labels, const float* ts_raw,
                            const uint8_t* mark_table, int B, int T, int H, int E, int M, float coef,
                            const float* sums, const float* gscale, float* d_lam, void* stream) {
    TppP p;
    if (const int rc = tpp_args("edgl_tpp_bwd", lam, masked_pos, labels, ts_raw, mark_table, B, T, H, E, M, coef, sums, d_lam, &p)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(d_lam, 0, (size_t)H * B * T * E * sizeof(float), st) != hipSuccess) {
        edgl_set_error("edgl_tpp_bwd: memset failed");
        return EDGL_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(tpp_bwd_kernel, dim3(grid_for((long)H * B * M)), dim3(256), 0, st, p, sums, gscale, d_lam);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

// The two batch sums that normalise the loss, in one launch — counts[0] = labels != 0 (weighted rows, EasyDGL.py:183-185), counts[1] =
// marks of all labels (temporal.py:330, what edgl_tpp_norm puts into sums[4]): what a data-parallel step all-reduces before it
// starts (8 bytes).  B * M <= 65536.
extern "C" int edgl_dp_counts(const int64_t* labels, const uint8_t* mark_table, int B, int M, int E, int32_t* counts, void* stream) {
    EDGL_REQUIRE(labels && mark_table && counts, EDGL_ERR_NULL, "edgl_dp_counts: null pointer");
    EDGL_REQUIRE(B > 0 && M > 0 && E > 0 && (long)B * M <= 65536, EDGL_ERR_SHAPE, "edgl_dp_counts: bad shape B=%d M=%d E=%d (B * M <= 65536)",
                 B, M, E);
    TppP p{nullptr, nullptr, labels, nullptr, mark_table, B, 0, 0, E, M, 0.f};
    hipLaunchKernelGGL(tpp_norm_one_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, p, counts + 1, counts);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
// normaliser of the regulariser: integer sum of the mark counts of the batch's labels into sums[4] (labels only: may run
// ahead of the step's forward, e.g. on a side stream)
extern "C" int edgl_tpp_norm(const int64_t* labels, const uint8_t* mark_table, int B, int M, int E, float* sums, void* stream) {
    EDGL_REQUIRE(labels && mark_table && sums, EDGL_ERR_NULL, "edgl_tpp_norm: null pointer");
    TppP p{nullptr, nullptr, labels, nullptr, mark_table, B, 0, 0, E, M, 0.f};
    if ((long)B * M <= 65536) {   // one workgroup, plain store
        hipLaunchKernelGGL(tpp_norm_one_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, p, reinterpret_cast<int*>(sums) + 4,
                           (int*)nullptr);
        EDGL_LAUNCH_CHECK();
        return EDGL_OK;
    }
    // the count is formed from zero every time: a step that aborted between this call and tpp_final2_kernel (which zeroes the slot
    // again) must not leave a stale count behind for the next one
    if (hipMemsetAsync(reinterpret_cast<int*>(sums) + 4, 0, sizeof(int), (hipStream_t)stream) != hipSuccess) {
        edgl_set_error("edgl_tpp_norm: memset failed");
        return EDGL_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(tpp_norm_kernel, dim3((B * M + 255) / 256), dim3(256), 0, (hipStream_t)stream, p, reinterpret_cast<int*>(sums) + 4);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
// with_norm = 0: edgl_tpp_norm has already run for this batch on the same `sums`
// (reports itself as edgl_tpp_fwd_bwd, the entry point the engine calls)
extern "C" int edgl_tpp_fwd_bwd_ex(const float* lam, const int64_t* masked_pos, const int64_t* labels, const float* ts_raw,
                                   const uint8_t* mark_table, int B, int T, int H, int E, int M, float coef, float* sums,
                                   float* reg_out, int accumulate, float* d_lam, int with_norm, void* stream) {
    TppP p;
    if (const int rc = tpp_args("edgl_tpp_fwd_bwd", lam, masked_pos, labels, ts_raw, mark_table, B, T, H, E, M, coef, sums, reg_out, &p)) return rc;
    EDGL_REQUIRE(E >= 1 && E <= 16, EDGL_ERR_SHAPE, "edgl_tpp_fwd_bwd: E=%d (1..16)", E);
    EDGL_REQUIRE(M <= TPP_MAXM && T <= TPP_MAXT, EDGL_ERR_SHAPE, "edgl_tpp_fwd_bwd: M=%d > %d or T=%d > %d", M, TPP_MAXM, T, TPP_MAXT);
    if (with_norm) {
        const int rc = edgl_tpp_norm(labels, mark_table, B, M, E, sums, stream);
        if (rc) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    const int nblk = std::min(TPP_FUSED_BLOCKS, H * B);
    hipLaunchKernelGGL(tpp_fused_kernel, dim3(nblk), dim3(128), 0, st, p, sums, sums + 8, d_lam);
    EDGL_LAUNCH_CHECK();
    hipLaunchKernelGGL(tpp_final2_kernel, dim3(1), dim3(256), 0, st, sums + 8, nblk, coef, H, sums, reg_out, accumulate);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
// edgl_tpp_fwd_bwd_ex (with_norm = 0) for a d_lam array that ALREADY HOLDS ZEROS (edgl_bimau_fwd_zr): one thread per masked
// slot, only the rows of masked positions are written.  `sums` needs edgl_tpp_rows_workspace(B, H, M) floats.
static long tpp_rows_blocks(int B, int H, int M) {   // (also an upper bound of the one-slot-per-thread grid of the wide form)
    return M <= 256 ? ((long)H * B + 256 / M - 1) / (256 / M) : ((long)H * B * M + 255) / 256;
}
extern "C" long edgl_tpp_rows_workspace(int B, int H, int M) {
    return (B > 0 && H > 0 && M > 0) ? 8 + 2 * std::max(tpp_rows_blocks(B, H, M), ((long)H * B * M + 255) / 256) : -1;
}
extern "C" int edgl_tpp_fwd_bwd_rows(const float* lam, const int64_t* masked_pos, const int64_t* labels, const float* ts_raw,
                                     const uint8_t* mark_table, int B, int T, int H, int E, int M, float coef, float* sums,
                                     float* reg_out, int accumulate, float* d_lam, void* stream) {
    TppP p;
    if (const int rc = tpp_args("edgl_tpp_fwd_bwd_rows", lam, masked_pos, labels, ts_raw, mark_table, B, T, H, E, M, coef, sums, reg_out, &p)) return rc;
    EDGL_REQUIRE(E >= 1 && E <= 256 && B > 0 && H > 0 && M > 0, EDGL_ERR_SHAPE, "edgl_tpp_fwd_bwd_rows: bad shape E=%d B=%d H=%d M=%d", E, B, H, M);
    hipStream_t st = (hipStream_t)stream;
    int nblk = (int)tpp_rows_blocks(B, H, M);
    if (E <= 16) {
        hipLaunchKernelGGL(tpp_rows_kernel, dim3(nblk), dim3(256), 0, st, p, sums, sums + 8, d_lam);
    } else {   // more than 16 mark types: plain loops over the marks, one slot per thread
        nblk = (int)(((long)H * B * M + 255) / 256);
        hipLaunchKernelGGL(tpp_rows_wide_kernel, dim3(nblk), dim3(256), 0, st, p, sums, sums + 8, d_lam);
    }
    EDGL_LAUNCH_CHECK();
    hipLaunchKernelGGL(tpp_final2_kernel, dim3(1), dim3(256), 0, st, sums + 8, nblk, coef, H, sums, reg_out, accumulate);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
// ---- fused TPP form: the regulariser inside the attention kernels (bimau_common.h: TppDesc) -----------------------------------
extern "C" long edgl_tpp_prep_bytes(int B, int T, int M) {
    return (B > 0 && T > 0 && M > 0) ? (long)bimau::tpp_layout(B, T, M).bytes : -1;
}
// slot data of one batch for edgl_bimau_bwd_tpp: `desc` = edgl_tpp_prep_bytes(B, T, M) bytes, 16-byte aligned
extern "C" int edgl_tpp_prep(const int64_t* masked_pos, const int64_t* labels, const float* ts_raw, const uint8_t* mark_table,
                             int B, int T, int E, int M, void* desc, void* stream) {
    EDGL_REQUIRE(masked_pos && labels && ts_raw && mark_table && desc, EDGL_ERR_NULL, "edgl_tpp_prep: null pointer");
    EDGL_REQUIRE(B > 0 && T > 0 && T <= 2048 && E == 16 && M > 0 && M <= 256, EDGL_ERR_SHAPE,
                 "edgl_tpp_prep: bad shape B=%d T=%d E=%d M=%d (E = 16, M <= 256, T <= 2048)", B, T, E, M);
    EDGL_REQUIRE((((uintptr_t)mark_table | (uintptr_t)desc) & 15) == 0, EDGL_ERR_SHAPE, "edgl_tpp_prep: mark_table / desc must be 16-byte aligned");
    const size_t smem = (size_t)T * 16 + 2 * 256 * sizeof(int);
    hipLaunchKernelGGL(tpp_prep_kernel, dim3(B), dim3(256), smem, (hipStream_t)stream, masked_pos, labels, ts_raw, mark_table, B, T, M,
                       (char*)desc);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
// reduction of the per-(b, head) partial sums edgl_bimau_bwd_tpp left in `part` ([nparts, 2]) into the regulariser
// reg_out (=|+=) coef * (-(sum log ev - sum non-event) / (count * H))  (temporal.py:331-332, EasyDGL.py:175); `sums` = the array
// edgl_tpp_norm wrote the batch's mark count into (sums[0..2] receive the two sums and the normaliser, as edgl_tpp_fwd_bwd leaves
// them).  The normaliser: tpp_desc != NULL — the per-sample counts of edgl_tpp_prep(B, T, M), whose total also goes to sums[4];
// tpp_desc == NULL — sums[4] as edgl_tpp_norm (or a data-parallel all-reduce) left it; the slot is not cleared.
extern "C" int edgl_tpp_finish_parts(const float* part, int nparts, float coef, int H, const void* tpp_desc, int B, int T, int M,
                                     float* sums, float* reg_out, int accumulate, void* stream) {
    EDGL_REQUIRE(part && sums && reg_out, EDGL_ERR_NULL, "edgl_tpp_finish_parts: null pointer");
    EDGL_REQUIRE(nparts > 0 && H > 0 && (!tpp_desc || (B > 0 && T > 0 && M > 0)), EDGL_ERR_SHAPE,
                 "edgl_tpp_finish_parts: bad shape nparts=%d H=%d B=%d T=%d M=%d", nparts, H, B, T, M);
    const int* cntp = tpp_desc ? reinterpret_cast<const int*>((const char*)tpp_desc + bimau::tpp_layout(B, T, M).off_cntp) : nullptr;
    hipLaunchKernelGGL(tpp_parts_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, part, nparts, coef, H, cntp, B, sums, reg_out,
                       accumulate);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
// edgl_tpp_finish_parts with the normaliser edgl_bimau_bwd_tpp left behind the partial sums (part: [nparts + 1, 2]; the count it
// used — the per-sample counts' total or the data-parallel sums[4] — as an int in the last pair): reads nothing of the batch.
extern "C" int edgl_tpp_finish_parts_n(const float* part, int nparts, float coef, int H, float* sums, float* reg_out, int accumulate,
                                       void* stream) {
    EDGL_REQUIRE(part && sums && reg_out, EDGL_ERR_NULL, "edgl_tpp_finish_parts_n: null pointer");
    EDGL_REQUIRE(nparts > 0 && H > 0, EDGL_ERR_SHAPE, "edgl_tpp_finish_parts_n: bad shape nparts=%d H=%d", nparts, H);
    hipLaunchKernelGGL(tpp_parts_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, part, nparts, coef, H, (const int*)nullptr, -1, sums,
                       reg_out, accumulate);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
extern "C" int edgl_tpp_fwd_bwd(const float* lam, const int64_t* masked_pos, const int64_t* labels, const float* ts_raw,
                                const uint8_t* mark_table, int B, int T, int H, int E, int M, float coef, float* sums,
                                float* reg_out, int accumulate, float* d_lam, void* stream) {
    return edgl_tpp_fwd_bwd_ex(lam, masked_pos, labels, ts_raw, mark_table, B, T, H, E, M, coef, sums, reg_out, accumulate, d_lam, 1,
                               stream);
}
