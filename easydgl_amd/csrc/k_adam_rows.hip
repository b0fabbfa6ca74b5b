// Lazy row-wise Adam for the item table of sampled-softmax training: the TF-form update of k_optim.hip on the rows a
// step used and on no other — TensorFlow's LazyAdamOptimizer.  The gradient of the table is complete in `grad` before the launch
// (the embedding scatter and the sampled loss's table gradient ADD into the table's view of the gradient arena, which is all zeros
// between steps); this launch consumes it row by row and leaves the zeros behind.
//
//   entries      e in [0, n_ids)                    : ids[e]                                  (the batch's input ids)
//                e = n_ids + r (N + 1) + s          : s == 0 ? labels[r] : cand[r, s - 1]     (rows with 1 <= labels[r] < I only: the
//                                                     slots of a row of weight 0 name nothing, the dead-slot rule of k_cand_ce.hip)
//   touched      an entry with 1 <= id < I touches row id; the set is a function of the integer inputs alone
//   claim        every lane holds one entry and raises stamp[id] to the step count of step_state with ONE returning integer
//                atomic; the entry that saw a smaller value owns the row (duplicates, in the launch or in the wave, leave at once:
//                exactly one entry per row sees the old value).  Any owner computes the same update, so the winner does not matter.
//   update       the owners of a wave are compacted to its first lanes (one lane permute) and the WHOLE wave then walks them:
//                a row is C / 4 pieces of 16 bytes, a lane group of G = 1 .. 64 lanes (the power of two >= C / 4) holds one row,
//                64 / G rows per wave-instruction; at C = 256 one dwordx4 per lane and array, at C = 512 two.  Per row
//                4 loads (w, g, m, v) and 4 stores (w, m, v, g := 0) of C f32 plus the bf16 shadow: 8.5 C 4 bytes.
//   grid         persistent waves striding over chunks of 64 entries (grid_for's cap of 4096 workgroups): the claim is one
//                wave-instruction per 64 entries whatever the duplicate rate, and the memory-level parallelism comes from the
//                resident waves, not from unrolling one.  (Smaller chunks for launches with few entries — 16 per wave at 218 K
//                entries, so that the waves fill the chip — measured 0.420 against 0.467 ms on a machine whose dense Adam ran 7 %
//                faster as well: not kept.)
// No float atomics, no sort, no host read-back; one writer per row, hence bitwise reproducible.
// The element update is a third text beside adam_kernel / adam_ex_kernel of k_optim.hip (see the comment there: a shared function
// moved instructions of the kernel the training step launches).
#include "edgl_common.h"

namespace {

struct RowsP {
    float* w; float* g; float* m; float* v; bf16* shadow;
    int I, C;
    const int64_t* ids; long n_ids;
    const int64_t* labels; const int32_t* cand; int R, N;
    int32_t* stamp;
    float b1, b2, eps;
    const uint64_t* st;
    float l2;
};

template <bool SHADOW>
__global__ __launch_bounds__(256) void adam_rows_kernel(RowsP p) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwave = (long)gridDim.x * 4;
    const long total = p.n_ids + (long)p.R * (p.N + 1);
    const int step = (int)p.st[0];
    const float lr_t = reinterpret_cast<const float*>(p.st + 1)[0];
    const int pieces = p.C / 4;
    int G = 1;
    while (G < pieces && G < 64) G <<= 1;
    const int rpw = 64 / G, grp = lane / G, gl = lane % G;
    const uint32_t np1 = (uint32_t)p.N + 1u;
    for (long base = wave * 64; base < total; base += nwave * 64) {      // (wave-uniform)
        const long e = base + lane;
        int id = 0;
        if (e < total) {
            int64_t x = 0;
            if (e < p.n_ids) {
                x = p.ids[e];
            } else {
                const uint32_t q = (uint32_t)(e - p.n_ids), r = q / np1, s = q - r * np1;      // (R (N + 1) < 2^31)
                const int64_t y = p.labels[r];
                if (y >= 1 && y < p.I) x = s == 0 ? y : (int64_t)p.cand[(long)r * p.N + (s - 1)];
            }
            id = (x >= 1 && x < p.I) ? (int)x : 0;
        }
        bool owner = false;
        if (id > 0) owner = atomicMax(p.stamp + id, step) < step;
        const unsigned long long mask = __ballot(owner);
        const int count = __popcll(mask);
        if (count == 0) continue;
        // owners to lanes 0 .. count - 1 in lane order, the others behind them: a permutation of the wave
        const unsigned long long below = (1ull << lane) - 1ull;
        const int dest = owner ? __popcll(mask & below) : count + __popcll(~mask & below);
        const int packed = __builtin_amdgcn_ds_permute(dest << 2, id);
        for (int j0 = 0; j0 < count; j0 += rpw) {                        // (wave-uniform)
            const int j = j0 + grp;
            const int row = __shfl(packed, j & 63, 64);
            if (j >= count || row < 1 || row >= p.I) continue;           // (addresses stay inside the table whatever was read)
            for (int pc = gl; pc < pieces; pc += G) {
                const long o = (long)row * p.C + pc * 4;
                const float4 w4 = *reinterpret_cast<const float4*>(p.w + o), g4 = *reinterpret_cast<const float4*>(p.g + o);
                const float4 m4 = *reinterpret_cast<const float4*>(p.m + o), v4 = *reinterpret_cast<const float4*>(p.v + o);
                const float wi[4] = {w4.x, w4.y, w4.z, w4.w}, go[4] = {g4.x, g4.y, g4.z, g4.w};
                const float mo[4] = {m4.x, m4.y, m4.z, m4.w}, vo[4] = {v4.x, v4.y, v4.z, v4.w};
                float wn[4], mn[4], vn[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float gi = p.l2 != 0.f ? go[k] + p.l2 * wi[k] : go[k];
                    mn[k] = p.b1 * mo[k] + (1.f - p.b1) * gi;
                    vn[k] = p.b2 * vo[k] + (1.f - p.b2) * gi * gi;
                    wn[k] = wi[k] - lr_t * mn[k] / (sqrtf(vn[k]) + p.eps);
                }
                *reinterpret_cast<float4*>(p.m + o) = make_float4(mn[0], mn[1], mn[2], mn[3]);
                *reinterpret_cast<float4*>(p.v + o) = make_float4(vn[0], vn[1], vn[2], vn[3]);
                *reinterpret_cast<float4*>(p.w + o) = make_float4(wn[0], wn[1], wn[2], wn[3]);
                *reinterpret_cast<float4*>(p.g + o) = make_float4(0.f, 0.f, 0.f, 0.f);
                if (SHADOW) {
                    const Frag4<bf16> f = frag_from_acc<bf16>(f32x4{wn[0], wn[1], wn[2], wn[3]});
                    *reinterpret_cast<uint2*>(p.shadow + o) = *reinterpret_cast<const uint2*>(&f);
                }
            }
        }
    }
}

}  // namespace

extern "C" int edgl_adam_rows(float* table, float* grad, float* m, float* v, void* shadow, int I, int C, const int64_t* ids, long n_ids,
                              const int64_t* labels, const int32_t* cand, int R, int N, int32_t* stamp, float beta1, float beta2,
                              float eps, const uint64_t* step_state, float l2, void* stream) {
    // (the shape rule first, before any pointer is looked at: an empty list has no address)
    EDGL_REQUIRE(C >= 4 && C <= 512 && C % 4 == 0, EDGL_ERR_SHAPE, "edgl_adam_rows: C=%d (4 <= C <= 512, a multiple of 4)", C);
    EDGL_REQUIRE(I > 1 && R >= 0 && N >= 0 && n_ids >= 0 && (long)R * ((long)N + 1) < (1L << 31), EDGL_ERR_SHAPE,
                 "edgl_adam_rows: I=%d R=%d N=%d n_ids=%ld (I > 1, R >= 0, N >= 0, n_ids >= 0, R (N + 1) < 2^31)", I, R, N, n_ids);
    EDGL_REQUIRE(table && grad && m && v && stamp && step_state, EDGL_ERR_NULL, "edgl_adam_rows: null pointer");
    EDGL_REQUIRE((n_ids == 0 || ids) && (R == 0 || labels) && (R == 0 || N == 0 || cand), EDGL_ERR_NULL,
                 "edgl_adam_rows: null list (ids with n_ids > 0, labels with R > 0, cand with R > 0 and N > 0)");
    EDGL_REQUIRE((((uintptr_t)table | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v | (uintptr_t)shadow) & 15) == 0, EDGL_ERR_SHAPE,
                 "edgl_adam_rows: table, grad, m, v and shadow must be 16-byte aligned");
    const long total = n_ids + (long)R * (N + 1);
    if (total == 0) return EDGL_OK;
    const dim3 grid((unsigned)grid_for(total));      // (256 entries per workgroup and pass)
    const RowsP p{table, grad, m, v, (bf16*)shadow, I, C, ids, n_ids, labels, cand, R, N, stamp, beta1, beta2, eps, step_state, l2};
    if (shadow) hipLaunchKernelGGL(adam_rows_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(adam_rows_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
