// K5c: sampled-softmax training — cross-entropy over per-row candidate lists.  The write side of k_eval_cand.hip:
// every weighted row r (label y = labels[r] != 0) is scored against ITS OWN list cand[r, 0 .. N) instead of the catalogue.
//
//   slots of row r : slot 0 = the label, slot 1 + n = cand[r, n]
//   v(r, c)        = cand_value (cand_gather.h): rows[r] . table_c[c] + bias_used[c], the bits edgl_score_candidates gives
//   a list slot is DEAD (-inf; no part in loss or gradient) when it is empty (c < 0), at or past I (the address is clamped), or
//   equal to the row's label (accidental-hit removal: the sampler never draws the label, a caller's list may hold it)
//   lse[r]         = log sum exp v over the label and the live slots;  loss and coef[r] come from edgl_ce_loss_fwd(lse, label_val)
//   dv(r, s)       = g coef[r] (exp(v_s - lse) - [s == 0])
//   d_rows[r]      = sum_s dv table_c[c_s]     (item 0 adds nothing)        d_table[c_s] += dv rows[r] (row 0 stays zero)
//   d_bias[c_s - 1] += dv  (c_s >= 1)
// Uniform negatives over [1, hi): the log-Q correction of sampled softmax is one constant for every slot and cancels.  A weighted
// sampler hands logq [I] to edgl_cand_ce_fwd_q: the label and every live slot then read v - logq[c] — one f32
// subtraction on the finished value, so logq = 0 or NULL gives the bits above; the backward forms dv from the saved vals and lse
// and is the same code either way.
//
//   cand_ce_fwd_kernel   one workgroup (4 waves) per row; the structure of score_cand_kernel: query row in registers over a lane group,
//                        UNROLL gathered table rows in flight, the next step's ids fetched under this step's arithmetic.  Writes
//                        vals [R, N + 1], label_val, lse.  Reduction order, a function of N alone: every lane runs (max, sum) over its
//                        slots in ascending order, a fixed xor butterfly joins the lane groups of a wave (lane 0's result is used), then
//                        (label, wave 0, 1, 2, 3) are joined in that order through LDS.  No atomics; two calls give the same bits and a
//                        row's outputs do not depend on R or on the other rows.
//   cand_ce_bwd_kernel   same decomposition.  dv from (vals, lse, coef), written as f32 [R, N + 1]; the listed table rows are gathered
//                        again and d_rows[r] accumulates in registers (every lane the partial sums of its own pieces; the lane groups of
//                        a wave are joined by a fixed butterfly, the four waves in wave order through LDS): one store per row.
//                        Table gradient (d_table != NULL): f32 atomicAdd into the ZERO-FILLED d_table / d_bias in a second sweep over
//                        the row's slots with the query row re-laid so that one wave-instruction adds 256 contiguous bytes of one table
//                        row (C >= 64; narrower rows: 64 / C whole rows) — the shape that runs at the chip-wide atomic rate, so the
//                        cost model is R (N + 1) C 4 bytes / 1.3 TB/s.
//   edgl_cand_ce_table_det   the same sums without float atomics: a k_segsum.hip plan over the flattened slot keys (0 for dead slots and
//                        rows of weight 0), one ordered sum per distinct id, one writer per table row.
// Rows with label 0 leave by a block-uniform exit (no compaction: a row's list never depends on which other rows are weighted); their
// vals read -inf, their lse / label_val 0 and their d_rows / dv are written as zeros.  A label outside [0, I) is a caller error and
// the row is skipped the same way.
//
// Other objectives over the same slots (sampled_dv.h): the forward is unchanged (its lse is not used), the row losses come
// from k_sampled_loss.hip, and cand_ce_bwd_kernel<.., FORM> forms dv by the form's rule in its two sweeps — everything behind dv
// is the code above.  FORM = softmax is today's kernel, bit for bit.
#include "edgl_common.h"
#include "sampled_dv.h"
#include "cand_gather.h"

namespace cce {

using candg::UNROLL; using candg::RowRegs; using candg::load_pieces; using candg::unpack; using candg::cand_value; using candg::group_of;

constexpr int MAX_N = 8192;

struct P {
    const void* rows; const void* table; const float* bias; const int32_t* cand; const int64_t* labels;
    const float* logq;                                               // forward only: [I] or NULL
    int R, C, I, N;
    float* vals; float* label_val; float* lse;                       // forward: outputs; backward: vals / lse are inputs (lse: the
                                                                     // row auxiliary of a form other than softmax)
    const float* coef; const float* gscale;
    void* d_rows; float* dv; float* d_table; float* d_bias;
};

// (m, s) <- (m, s) joined with (m2, s2): running maximum and sum of exp(v - m); (-inf, 0) is the empty set
__device__ __forceinline__ void lse_join(float& m, float& s, float m2, float s2) {
    const float M = fmaxf(m, m2);
    s = M == -INFINITY ? 0.0f : s * __expf(m - M) + s2 * __expf(m2 - M);
    m = M;
}

// Q: with the log-Q term (p.logq != NULL); Q = false compiles to the kernel without it
template <typename T, int G, int PPL, bool Q>
__global__ __launch_bounds__(256) void cand_ce_fwd_kernel(P p) {
    constexpr int RPW = 64 / G;               // candidate rows per wave-instruction
    constexpr int STEP = 4 * UNROLL * RPW;    // slots of one step of the workgroup
    __shared__ float red[4][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = lane / G, gl = lane % G;
    const int r = blockIdx.x, N = p.N;
    float* vrow = p.vals + (long)r * (N + 1);
    const int64_t y64 = p.labels[r];
    if (y64 < 1 || y64 >= p.I) {              // (block-uniform) weight 0
        for (int n = tid; n <= N; n += 256) vrow[n] = -INFINITY;
        if (tid == 0) { p.label_val[r] = 0.0f; p.lse[r] = 0.0f; }
        return;
    }
    const int y = (int)y64;
    const T* table = reinterpret_cast<const T*>(p.table);
    RowRegs<T, PPL> xq;
    {
        uint4 w[PPL];
        load_pieces<T, G, PPL>(reinterpret_cast<const T*>(p.rows), r, p.C, gl, w);
#pragma unroll
        for (int pp = 0; pp < PPL; ++pp) unpack<T>(w[pp], gl + pp * 64 < p.C / (int)(16 / sizeof(T)), xq.x[pp]);
    }
    float vy;                                 // the label: one more slot, the same function, formed by every wave for itself
    {
        uint4 w[PPL];
        load_pieces<T, G, PPL>(table, y, p.C, gl, w);
        vy = cand_value<T, G, PPL>(xq, w, y, p.bias[y - 1], p.C, gl);
        if constexpr (Q) vy -= p.logq[y];     // the log-Q correction: one f32 subtraction on the finished value
    }
    const int32_t* crow = p.cand + (long)r * N;
    auto slot_of = [&](int base, int u) { return base + u * (4 * RPW) + wave * RPW + grp; };
    int cs[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        const int n = slot_of(0, u);
        cs[u] = n < N ? crow[n] : -1;
    }
    float m = -INFINITY, s = 0.0f;
    for (int base = 0; base < N; base += STEP) {              // (block-uniform)
        uint4 w[UNROLL][PPL];
        float b[UNROLL], q[Q ? UNROLL : 1];
        int c[UNROLL], ca[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            c[u] = cs[u];
            ca[u] = (c[u] >= 0 && c[u] < p.I) ? c[u] : 0;     // (addresses stay inside the table whatever the id)
            load_pieces<T, G, PPL>(table, ca[u], p.C, gl, w[u]);
            b[u] = p.bias[max(ca[u], 1) - 1];
            if constexpr (Q) q[u] = p.logq[ca[u]];            // (logq[0] = 0: item 0 keeps its -1000)
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {                    // the next step's ids, under this step's arithmetic
            const int n = slot_of(base + STEP, u);
            cs[u] = n < N ? crow[n] : -1;
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            float vv = cand_value<T, G, PPL>(xq, w[u], ca[u], ca[u] == 0 ? -1000.0f : b[u], p.C, gl);
            if constexpr (Q) vv -= q[u];
            const bool live = c[u] >= 0 && c[u] < p.I && c[u] != y;
            const float v = live ? vv : -INFINITY;
            const int n = slot_of(base, u);
            if (n < N) {
                if (gl == 0) vrow[1 + n] = v;
                if (live) {                                   // this lane's slots in ascending order
                    if (v > m) { s = s * __expf(m - v) + 1.0f; m = v; }
                    else s += __expf(v - m);
                }
            }
        }
    }
#pragma unroll
    for (int o = G; o < 64; o <<= 1) {                        // the lane groups of the wave (the lanes of a group hold the same pair)
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        lse_join(m, s, m2, s2);
    }
    if (lane == 0) { red[wave][0] = m; red[wave][1] = s; }
    __syncthreads();
    if (tid == 0) {
        float M = vy, S = 1.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) lse_join(M, S, red[w][0], red[w][1]);
        vrow[0] = vy;
        p.label_val[r] = vy;
        p.lse[r] = M + logf(S);
    }
}

// FORM: the objective whose dv is formed (sampled_dv.h); L is lse[r] (softmax) or the row auxiliary (bpr: sum_s sigma(v_s - v_0))
template <typename T, int G, int PPL, int FORM>
__global__ __launch_bounds__(256) void cand_ce_bwd_kernel(P p) {
    constexpr int VEC = 16 / sizeof(T);
    constexpr int RPW = 64 / G;
    constexpr int STEP = 4 * UNROLL * RPW;
    constexpr int NA = PPL * VEC;             // partial sums of one lane
    __shared__ float red[4][G][NA];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = lane / G, gl = lane % G;
    const int r = blockIdx.x, N = p.N, np = p.C / VEC;
    const float* vrow = p.vals + (long)r * (N + 1);
    float* dvrow = p.dv + (long)r * (N + 1);
    T* drow = reinterpret_cast<T*>(p.d_rows) + (long)r * p.C;
    const int64_t y64 = p.labels[r];
    if (y64 < 1 || y64 >= p.I) {              // (block-uniform) weight 0
        for (int n = tid; n <= N; n += 256) dvrow[n] = 0.0f;
        if (tid < np) st16<T>(drow + tid * VEC, zero16<T>());
        return;
    }
    const int y = (int)y64;
    const T* table = reinterpret_cast<const T*>(p.table);
    const float gc = (p.gscale ? p.gscale[0] : 1.0f) * p.coef[r];
    const float L = p.lse[r];
    float acc[PPL][VEC];
#pragma unroll
    for (int pp = 0; pp < PPL; ++pp)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[pp][e] = 0.0f;
    auto add_row = [&](const uint4 (&w)[PPL], bool keep, float d) {
#pragma unroll
        for (int pp = 0; pp < PPL; ++pp) {
            float z[VEC];
            unpack<T>(w[pp], keep && gl + pp * 64 < np, z);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[pp][e] = fmaf(d, z[e], acc[pp][e]);
        }
    };
    const float v0 = vrow[0];
    const float dv0 = sdv::dv_label<FORM>(gc, v0, L);
    if (wave == 0 && grp == 0) {              // the label slot: the first term of wave 0's first lane group
        uint4 w[PPL];
        load_pieces<T, G, PPL>(table, y, p.C, gl, w);
        add_row(w, true, dv0);
        if (gl == 0) dvrow[0] = dv0;
    }
    const int32_t* crow = p.cand + (long)r * N;
    auto slot_of = [&](int base, int u) { return base + u * (4 * RPW) + wave * RPW + grp; };
    int cs[UNROLL];
    float vs[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        const int n = slot_of(0, u);
        cs[u] = n < N ? crow[n] : -1;
        vs[u] = n < N ? vrow[1 + n] : -INFINITY;
    }
    for (int base = 0; base < N; base += STEP) {              // (block-uniform)
        uint4 w[UNROLL][PPL];
        int c[UNROLL];
        float v[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            c[u] = cs[u];
            v[u] = vs[u];
            const int ca = (c[u] >= 0 && c[u] < p.I) ? c[u] : 0;
            load_pieces<T, G, PPL>(table, ca, p.C, gl, w[u]);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {                    // the next step's ids and values, under this step's arithmetic
            const int n = slot_of(base + STEP, u);
            cs[u] = n < N ? crow[n] : -1;
            vs[u] = n < N ? vrow[1 + n] : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const bool live = v[u] > -INFINITY;               // (the forward's test: empty, past I and accidental hits read -inf)
            const float d = live ? sdv::dv_slot<FORM>(gc, v[u], v0, L) : 0.0f;
            add_row(w[u], live && c[u] > 0, d);
            const int n = slot_of(base, u);
            if (gl == 0 && n < N) dvrow[1 + n] = d;
        }
    }
#pragma unroll
    for (int o = G; o < 64; o <<= 1)                          // the lane groups of the wave: both partners form a + b
#pragma unroll
        for (int pp = 0; pp < PPL; ++pp)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[pp][e] += __shfl_xor(acc[pp][e], o, 64);
    if (grp == 0) {
#pragma unroll
        for (int pp = 0; pp < PPL; ++pp)
#pragma unroll
            for (int e = 0; e < VEC; ++e) red[wave][gl][pp * VEC + e] = acc[pp][e];
    }
    __syncthreads();
    if (tid < G) {                                            // the four waves in wave order; one store per piece of the row
#pragma unroll
        for (int pp = 0; pp < PPL; ++pp) {
            if (tid + pp * 64 >= np) continue;
            Vec16<T> o;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const int k = pp * VEC + e;
                o.v[e] = from_f32<T>(((red[0][tid][k] + red[1][tid][k]) + red[2][tid][k]) + red[3][tid][k]);
            }
            st16<T>(drow + (tid + pp * 64) * VEC, o);
        }
    }
    if (!p.d_table) return;                   // (block-uniform) dv only: the table gradient is summed over a plan
    // ---- the table gradient: one wave-instruction adds LR contiguous floats of one table row, 64 / LR rows at a time -------------
    int LR = 16;
    while (LR < p.C && LR < 64) LR <<= 1;
    const int rpi = 64 / LR, al = lane % LR, ag = lane / LR;
    const T* xrow = reinterpret_cast<const T*>(p.rows) + (long)r * p.C;
    float xr[8];                              // C <= 512: at most 8 floats per lane
#pragma unroll
    for (int j = 0; j < 8; ++j) xr[j] = j * LR + al < p.C ? to_f32(xrow[j * LR + al]) : 0.0f;
    for (int s0 = wave * rpi + ag; s0 <= N; s0 += 4 * rpi) {
        const float v = vrow[s0];
        const int c = s0 == 0 ? y : crow[s0 - 1];
        if (!(v > -INFINITY) || c < 1 || c >= p.I) continue;  // dead slot, or item 0 (its table row and bias are no parameters)
        const float d = s0 == 0 ? dv0 : sdv::dv_slot<FORM>(gc, v, v0, L);     // (the bits written to dv)
        float* dst = p.d_table + (long)c * p.C;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j * LR + al < p.C) atomicAdd(dst + j * LR + al, d * xr[j]);
        if (al == 0) atomicAdd(p.d_bias + c - 1, d);
    }
}

// keys[r (N + 1) + s] = the item of slot s of row r, 0 for a dead slot and for a row of weight 0 (the plan drops key 0)
__global__ __launch_bounds__(256) void cand_ce_keys_kernel(const int32_t* cand, const int64_t* labels, int R, int N, int I, int64_t* keys) {
    const long n = (long)R * (N + 1);
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const int r = (int)(e / (N + 1)), s = (int)(e % (N + 1));
        const int64_t y = labels[r];
        int64_t k = 0;
        if (y >= 1 && y < I) {
            const int c = s == 0 ? (int)y : cand[(long)r * N + s - 1];
            k = (s == 0 || (c >= 1 && c < I && c != y)) ? c : 0;
        }
        keys[e] = k;
    }
}

template <typename T, int G, int PPL>
int launch(const P& p, bool bwd, int form, hipStream_t st) {
    if (bwd && form == sdv::BCE) hipLaunchKernelGGL((cand_ce_bwd_kernel<T, G, PPL, sdv::BCE>), dim3((unsigned)p.R), dim3(256), 0, st, p);
    else if (bwd && form == sdv::BPR) hipLaunchKernelGGL((cand_ce_bwd_kernel<T, G, PPL, sdv::BPR>), dim3((unsigned)p.R), dim3(256), 0, st, p);
    else if (bwd) hipLaunchKernelGGL((cand_ce_bwd_kernel<T, G, PPL, sdv::SOFTMAX>), dim3((unsigned)p.R), dim3(256), 0, st, p);
    else if (p.logq) hipLaunchKernelGGL((cand_ce_fwd_kernel<T, G, PPL, true>), dim3((unsigned)p.R), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((cand_ce_fwd_kernel<T, G, PPL, false>), dim3((unsigned)p.R), dim3(256), 0, st, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

template <typename T>
int dispatch(const P& p, bool bwd, int form, hipStream_t st) {
    const int pieces = p.C / (int)(16 / sizeof(T));
    if constexpr (sizeof(T) == 4) {           // (only f32 rows exceed 64 pieces; only bf16 rows have two)
        if (pieces > 64) return launch<T, 64, 2>(p, bwd, form, st);
    }
    switch (group_of(pieces)) {
        case 2:
            if constexpr (sizeof(T) == 2) return launch<T, 2, 1>(p, bwd, form, st);
        case 4: return launch<T, 4, 1>(p, bwd, form, st);
        case 8: return launch<T, 8, 1>(p, bwd, form, st);
        case 16: return launch<T, 16, 1>(p, bwd, form, st);
        case 32: return launch<T, 32, 1>(p, bwd, form, st);
        default: return launch<T, 64, 1>(p, bwd, form, st);
    }
}

// the shape rule of the three entry points
int check_shape(const char* who, const void* rows, const void* table, int R, int C, int I, int N, int dtype) {
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "%s: dtype %d (f32 = 0 or bf16 = 1)", who, dtype);
    EDGL_REQUIRE(C >= 16 && C <= 512 && C % 16 == 0, EDGL_ERR_SHAPE, "%s: C=%d (16 <= C <= 512, a multiple of 16)", who, C);
    EDGL_REQUIRE(R >= 1 && N >= 1 && N <= MAX_N && I > 1 && (long)R * ((long)N + 1) < (1L << 31), EDGL_ERR_SHAPE,
                 "%s: R=%d N=%d I=%d (R >= 1, 1 <= N <= %d, I > 1, R (N + 1) < 2^31)", who, R, N, I, MAX_N);
    EDGL_REQUIRE((((uintptr_t)rows | (uintptr_t)table) & 15) == 0, EDGL_ERR_SHAPE, "%s: rows and table must be 16-byte aligned", who);
    return EDGL_OK;
}

}  // namespace cce

// logq (f32 [I], or NULL): every live slot and the label read v - logq[c]; NULL subtracts nothing
extern "C" int edgl_cand_ce_fwd_q(const void* rows, const void* table, const float* out_bias, const float* logq, const int32_t* cand,
                                  const int64_t* labels, int R, int C, int I, int N, float* vals, float* label_val, float* row_lse,
                                  int dtype, void* stream) {
    const int rc = cce::check_shape("edgl_cand_ce_fwd", rows, table, R, C, I, N, dtype);      // (first: an empty list has no address)
    if (rc) return rc;
    EDGL_REQUIRE(rows && table && out_bias && cand && labels && vals && label_val && row_lse, EDGL_ERR_NULL, "edgl_cand_ce_fwd: null pointer");
    cce::P p{};
    p.rows = rows; p.table = table; p.bias = out_bias; p.cand = cand; p.labels = labels; p.R = R; p.C = C; p.I = I; p.N = N;
    p.logq = logq;
    p.vals = vals; p.label_val = label_val; p.lse = row_lse;
    hipStream_t st = (hipStream_t)stream;
    return dtype == EDGL_BF16 ? cce::dispatch<bf16>(p, false, 0, st) : cce::dispatch<float>(p, false, 0, st);
}

extern "C" int edgl_cand_ce_fwd(const void* rows, const void* table, const float* out_bias, const int32_t* cand, const int64_t* labels,
                                int R, int C, int I, int N, float* vals, float* label_val, float* row_lse, int dtype, void* stream) {
    return edgl_cand_ce_fwd_q(rows, table, out_bias, nullptr, cand, labels, R, C, I, N, vals, label_val, row_lse, dtype, stream);
}

// form: EDGL_LOSS_SOFTMAX (row_aux = row_lse; edgl_cand_ce_bwd forwards here), EDGL_LOSS_BCE, EDGL_LOSS_BPR (row_aux of
// edgl_sampled_row_loss)
extern "C" int edgl_cand_ce_bwd_form(const void* rows, const void* table, const float* out_bias, const int32_t* cand,
                                     const int64_t* labels, const float* vals, const float* row_aux, const float* coef,
                                     const float* gscale, int R, int C, int I, int N, void* d_rows, float* dv, float* d_table,
                                     float* d_bias, int form, int dtype, void* stream) {
    const float* row_lse = row_aux;
    const int rc = cce::check_shape("edgl_cand_ce_bwd", rows, table, R, C, I, N, dtype);
    if (rc) return rc;
    EDGL_REQUIRE(form >= sdv::SOFTMAX && form <= sdv::BPR, EDGL_ERR_SHAPE, "edgl_cand_ce_bwd: form %d (0 <= form <= %d: softmax, bce, bpr)",
                 form, sdv::BPR);
    EDGL_REQUIRE(rows && table && out_bias && cand && labels && vals && row_lse && coef && d_rows && dv, EDGL_ERR_NULL,
                 "edgl_cand_ce_bwd: null pointer");
    EDGL_REQUIRE(!d_table == !d_bias, EDGL_ERR_NULL, "edgl_cand_ce_bwd: d_table and d_bias go together (both NULL: dv only)");
    EDGL_REQUIRE(((uintptr_t)d_rows & 15) == 0, EDGL_ERR_SHAPE, "edgl_cand_ce_bwd: d_rows must be 16-byte aligned");
    cce::P p{};
    p.rows = rows; p.table = table; p.bias = out_bias; p.cand = cand; p.labels = labels; p.R = R; p.C = C; p.I = I; p.N = N;
    p.vals = const_cast<float*>(vals); p.lse = const_cast<float*>(row_lse); p.coef = coef; p.gscale = gscale;
    p.d_rows = d_rows; p.dv = dv; p.d_table = d_table; p.d_bias = d_bias;
    hipStream_t st = (hipStream_t)stream;
    return dtype == EDGL_BF16 ? cce::dispatch<bf16>(p, true, form, st) : cce::dispatch<float>(p, true, form, st);
}

extern "C" int edgl_cand_ce_bwd(const void* rows, const void* table, const float* out_bias, const int32_t* cand, const int64_t* labels,
                                const float* vals, const float* row_lse, const float* coef, const float* gscale, int R, int C, int I,
                                int N, void* d_rows, float* dv, float* d_table, float* d_bias, int dtype, void* stream) {
    return edgl_cand_ce_bwd_form(rows, table, out_bias, cand, labels, vals, row_lse, coef, gscale, R, C, I, N, d_rows, dv, d_table,
                                 d_bias, EDGL_LOSS_SOFTMAX, dtype, stream);
}

extern "C" int edgl_cand_ce_table_det(const void* rows, const int32_t* cand, const int64_t* labels, const float* dv, int R, int C, int I,
                                      int N, float* d_table, float* d_bias, int64_t* keys, void* plan, int dtype, void* stream) {
    const int rc = cce::check_shape("edgl_cand_ce_table_det", rows, d_table, R, C, I, N, dtype);
    if (rc) return rc;
    EDGL_REQUIRE(rows && cand && labels && dv && d_table && d_bias && keys && plan, EDGL_ERR_NULL, "edgl_cand_ce_table_det: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const long n = (long)R * (N + 1);
    hipLaunchKernelGGL(cce::cand_ce_keys_kernel, dim3((unsigned)grid_for(n)), dim3(256), 0, st, cand, labels, R, N, I, keys);
    EDGL_LAUNCH_CHECK();
    return edgl_segsum_cand(rows, keys, dv, n, N + 1, C, I, d_table, d_bias, plan, dtype, st);
}
