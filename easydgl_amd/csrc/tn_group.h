// The grouped weight-gradient (TN) launch of k_gemm2.hip, host side: the queue entry, the launch parameters and the index arithmetic
// that lays a queue out as workgroups — shared by the stand-alone grouped launch (tn_flush) and by the hand-over of the queue to the
// QKVT dX GEMM's launch (edgl_gemm_dw_ride, DESIGN rule 79).  No device code and no runtime call in here: tools/tn_ride_layout_check.hip
// runs these functions on the host under the address / undefined-behaviour sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include "red_batch.h"

namespace gemm2 {

constexpr int T_NT = 256, T_BR = 64, T_LD = 128 + 16;   // T_BR rows per step (128-row steps measured: grouped dW 70 -> 81 us)

struct TnP {
    const bf16* X; const bf16* Y; int R, Kf, N, ldx, ldy;
    int rows_per_split;
    float* partial;   // [splits][Kf + 1][N]  (row Kf = column sums of Y)
    int with_colsum;
    int tiles_n, tiles_k, nblocks;   // tn_gemm_kernel: 1-D grid (padded to a multiple of 8 with the XCD-aware order)
};

constexpr int TN_MAX_JOBS = 8;
struct TnGroupP { TnP job[TN_MAX_JOBS]; int tiles_n[TN_MAX_JOBS], tiles_k[TN_MAX_JOBS], blk0[TN_MAX_JOBS + 1]; int n; };
struct TnQueued { TnP p; float* C; float* dbias; int accumulate, max_splits; };

// Row splits of a TN product (or of a group of them: `tiles` output tiles in all, `out_elems` f32 of output in all, `flop` =
// 2 R sum(Kf N)) on a part of `cus` compute units.  The chip takes workgroups in rounds of its CU count: 192 tiles x 2 splits = 384
// workgroups run as TWO rounds (the 512-unit QKVT weight gradient: 229 us), x 4 = 768 as three of half the length (143 us) — but
// every split leaves a [Kf+1, N] f32 slab that a second kernel sums (384 workgroups over a 128 x 128 output meant 25 MB of partials
// for a 64 KB result).  Both sides priced (rates measured on the part: ~0.6 PFLOP/s of this kernel when every round is full, 3 us
// of prologue / slab write per workgroup, x1.25 below two resident workgroups per CU, ~4 TB/s of slab reduction), the
// cheapest split count wins: 4 for that product (768 workgroups), 28 for the headline's grouped launch (504, as before).
static inline int tn_choose_splits_on(int cus, int R, int tiles, double flop, double out_elems, int cap) {
    const int smax = std::max(1, std::min(cap, R / 128));
    int best = 1;
    double best_t = 1e30;
    for (int sp = 1; sp <= smax; ++sp) {
        const long wg = (long)tiles * sp;
        const long rounds = (wg + cus - 1) / cus;
        double t = (double)rounds * (flop / (double)wg / (0.6e15 / cus) + 3e-6);   // + a workgroup's fixed part (its 64 KB slab)
        if (4 * wg < 7L * cus) t *= 1.25;   // fewer than ~two workgroups per CU: nothing hides a workgroup's barriers
        if (sp > 1) t += (double)sp * out_elems * 4.0 / 4e12 + 3e-6;
        if (t < best_t * 0.999) { best_t = t; best = sp; }
    }
    return best;
}

// The queue q[0..n) as one grouped launch: tile counts, ONE split count for the whole group (row ranges of similar length), capped by
// what each job's workspace was sized for, rows_per_split (written into the queue entries too), first block of every job.  Returns
// the number of workgroups (g->blk0[n]); splits[i] = partial slabs of job i.
static inline int tn_group_layout(TnQueued* q, int n, int cus, TnGroupP* g, int* splits) {
    g->n = n;
    int total_tiles = 0;
    for (int i = 0; i < n; ++i) {
        g->tiles_n[i] = (q[i].p.N + 127) / 128;
        g->tiles_k[i] = (q[i].p.Kf + 127) / 128;
        total_tiles += g->tiles_n[i] * g->tiles_k[i];
    }
    double flop = 0.0, elems = 0.0;
    int rmin = 1 << 30;
    for (int i = 0; i < n; ++i) {
        const TnP& p = q[i].p;
        flop += 2.0 * p.R * p.Kf * p.N;
        elems += (double)(p.Kf + 1) * p.N;
        rmin = std::min(rmin, p.R);
    }
    const int group_splits = tn_choose_splits_on(cus, rmin, total_tiles, flop, elems, 1 << 20);
    int blocks = 0;
    for (int i = 0; i < n; ++i) {
        TnP& p = q[i].p;
        int sp = std::max(1, std::min(std::min(group_splits, q[i].max_splits), p.R / 128));
        const int rps = ((p.R + sp - 1) / sp + T_BR - 1) / T_BR * T_BR;
        sp = (p.R + rps - 1) / rps;
        p.rows_per_split = rps;
        splits[i] = sp;
        g->job[i] = p;
        g->blk0[i] = blocks;
        blocks += g->tiles_n[i] * g->tiles_k[i] * sp;
    }
    g->blk0[n] = blocks;
    return blocks;
}

// Hand-over of the queue to the QKVT dX GEMM's launch (dx_encode_kernel): the group as tn_group_layout lays it out, and its slab
// reductions as jobs of the vector-form list that follows that launch, behind the caller's `nown` own jobs — (dW, db) contiguous, as in
// the flat gradient arena: one job, else one each.
struct TnRidePlan { TnGroupP g; int blocks, splits[TN_MAX_JOBS]; RedJob red[RED_MAX_JOBS]; int nred; };
// 1 = the group rides (plan filled, red[0..nown) left for the caller's jobs); 0 = it does not: an empty queue, an accumulating job
// (its read-modify-write reduction is ordered by the flush), a slab or output the vector form of the reductions does not take, or more
// reduction jobs than one RedBatch holds with the caller's.  (Only bf16 products in 128-tiles are ever queued: edgl_gemm2_try_tn.)
static inline int tn_ride_plan(TnQueued* q, int n, int cus, int nown, TnRidePlan* out) {
    if (n <= 0 || n > TN_MAX_JOBS) return 0;
    int nred = nown;
    for (int i = 0; i < n; ++i) {
        const TnP& p = q[i].p;
        if (q[i].accumulate) return 0;
        const bool one = !q[i].dbias || q[i].dbias == q[i].C + (long)p.Kf * p.N;
        if ((((uintptr_t)p.partial | (uintptr_t)q[i].C | (uintptr_t)q[i].dbias) & 15) || (p.N & 3)) return 0;
        nred += one ? 1 : 2;
    }
    if (nred > RED_MAX_JOBS) return 0;
    out->blocks = tn_group_layout(q, n, cus, &out->g, out->splits);
    int k = nown;
    for (int i = 0; i < n; ++i) {
        const TnP& p = q[i].p;
        const long slab = (long)(p.Kf + 1) * p.N;
        const bool with_db = q[i].dbias && q[i].dbias == q[i].C + (long)p.Kf * p.N;
        out->red[k++] = RedJob{p.partial, q[i].C, slab, out->splits[i], (with_db ? p.Kf + 1 : p.Kf) * p.N, 0, 0};
        if (q[i].dbias && !with_db) out->red[k++] = RedJob{p.partial + (long)p.Kf * p.N, q[i].dbias, slab, out->splits[i], p.N, 0, 0};
    }
    out->nred = k;
    return 1;
}

}  // namespace gemm2
