// Host-only check of the queue hand-over behind edgl_gemm_dw_ride (easydgl_amd/csrc/tn_group.h): the layout of a riding group —
// blocks, first block of every job, splits, rows per split — and its reduction jobs, for the engine's five weight-gradient shapes at
// the row counts of tests/test_gpu_dw_ride.py.  No kernel is launched and no device is touched: every workgroup id is decoded the way
// the kernel decodes it, and the first and last float of the slab it would write, the rows it would read, are touched in host
// buffers of exactly the sizes the library asks for — under the address sanitizer a wrong extent is a report, not a wrong number.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/tn_ride_layout_check.hip -o tools/tn_ride_layout_check && tools/tn_ride_layout_check
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../easydgl_amd/csrc/tn_group.h"

using namespace gemm2;

#define CHECK(c)                                                                      \
    do {                                                                              \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } \
    } while (0)

static const int CUS = 256;
static const int SHAPES[5][2] = {{384, 512}, {128, 128}, {256, 128}, {128, 256}, {128, 128}};

// what edgl_gemm2_try_tn queues for one product: the split count its workspace was sized for
static int own_splits(int R, int Kf, int N, long* ws_floats) {
    const int tiles = ((Kf + 127) / 128) * ((N + 127) / 128);
    int sp = tn_choose_splits_on(CUS, R, tiles, 2.0 * R * Kf * N, (double)(Kf + 1) * N, 1 << 20);
    *ws_floats = (long)sp * (Kf + 1) * N;
    const int rps = ((R + sp - 1) / sp + T_BR - 1) / T_BR * T_BR;
    return (R + rps - 1) / rps;
}

struct Group {
    std::vector<std::vector<float>> ws, out, db;
    std::vector<std::vector<char>> rows;      // one byte per row of the operands: the rows a split reads
    TnQueued q[TN_MAX_JOBS];
    int n;
};

static void make_group(Group& g, int R, int n, bool split_db) {
    g.n = n;
    g.ws.resize(n); g.out.resize(n); g.db.resize(n); g.rows.resize(n);
    for (int i = 0; i < n; ++i) {
        const int Kf = SHAPES[i % 5][0], N = SHAPES[i % 5][1];
        long wsf = 0;
        const int sp = own_splits(R, Kf, N, &wsf);
        g.ws[i].assign(wsf, 0.f);
        g.out[i].assign((long)(Kf + 1) * N, 0.f);
        g.db[i].assign(N, 0.f);
        g.rows[i].assign(R, 0);
        float* db = split_db && i == n - 1 ? g.db[i].data() : g.out[i].data() + (long)Kf * N;
        g.q[i] = TnQueued{TnP{nullptr, nullptr, R, Kf, N, Kf, N, 0, g.ws[i].data(), 1, 0, 0, 0}, g.out[i].data(), db, 0, sp};
    }
}

static void check_group(int R, int n, bool split_db, int nown) {
    Group g;
    make_group(g, R, n, split_db);
    TnRidePlan plan;
    CHECK(tn_ride_plan(g.q, n, CUS, nown, &plan) == 1);
    const TnGroupP& G = plan.g;
    CHECK(G.n == n && G.blk0[0] == 0 && G.blk0[n] == plan.blocks && plan.blocks > 0);
    for (int i = 0; i < n; ++i) {
        const TnP& p = G.job[i];
        const int sp = plan.splits[i];
        CHECK(sp >= 1 && sp <= g.q[i].max_splits && sp <= std::max(1, R / 128));
        CHECK(p.rows_per_split % T_BR == 0 && (long)p.rows_per_split * sp >= R && (long)p.rows_per_split * (sp - 1) < R);
        CHECK(G.tiles_n[i] == (p.N + 127) / 128 && G.tiles_k[i] == (p.Kf + 127) / 128);
        CHECK(G.blk0[i + 1] - G.blk0[i] == G.tiles_n[i] * G.tiles_k[i] * sp);
        CHECK(g.q[i].p.rows_per_split == p.rows_per_split);
    }
    // every workgroup id of the padded grid, decoded as dx_encode_kernel / tn_gemm_group_kernel decode it
    const int grid = (plan.blocks + 7) / 8 * 8;
    std::vector<int> seen(plan.blocks, 0);
    for (int b = 0; b < grid; ++b) {
        const int vid = (b & 7) * (grid >> 3) + (b >> 3);
        if (vid >= plan.blocks) continue;
        int j = 0;
        for (int i = 1; i < G.n; ++i)
            if (vid >= G.blk0[i]) j = i;
        const int local = vid - G.blk0[j], tn = G.tiles_n[j], tk = G.tiles_k[j];
        const int bx = local % tn, by = (local / tn) % tk, bz = local / (tn * tk);
        const TnP& p = G.job[j];
        CHECK(bz < plan.splits[j] && bx * 128 < p.N && by * 128 < p.Kf);
        const int r_lo = bz * p.rows_per_split, r_hi = std::min(p.R, r_lo + p.rows_per_split);
        CHECK(r_lo < r_hi);
        if (bx == 0 && by == 0)
            for (int r = r_lo; r < r_hi; ++r) g.rows[j][r]++;
        float* slab = p.partial + (long)bz * (p.Kf + 1) * p.N;
        slab[(long)(by * 128) * p.N + bx * 128] += 1.f;                                   // first element of the tile
        slab[(long)(std::min(p.Kf, by * 128 + 128) - 1) * p.N + std::min(p.N, bx * 128 + 128) - 1] += 1.f;
        if (by == 0) slab[(long)p.Kf * p.N + std::min(p.N, bx * 128 + 128) - 1] += 1.f;   // the column sums' row
        seen[vid]++;
    }
    for (int v = 0; v < plan.blocks; ++v) CHECK(seen[v] == 1);
    for (int i = 0; i < n; ++i)
        for (int r = 0; r < R; ++r) CHECK(g.rows[i][r] == 1);      // the splits cover every row once
    // the reduction jobs behind the caller's own
    int k = nown;
    for (int i = 0; i < n; ++i) {
        const TnP& p = G.job[i];
        const bool two = g.q[i].dbias != g.q[i].C + (long)p.Kf * p.N;
        const RedJob& a = plan.red[k++];
        CHECK(a.part == p.partial && a.out == g.q[i].C && a.P == plan.splits[i] && a.ld == (long)(p.Kf + 1) * p.N && a.f64 == 0);
        CHECK(a.N == (two ? p.Kf : p.Kf + 1) * p.N);
        for (int s = 0; s < a.P; ++s) const_cast<float*>(a.part)[(long)s * a.ld + a.N - 1] += 1.f;
        a.out[a.N - 1] += 1.f;
        if (two) {
            const RedJob& b = plan.red[k++];
            CHECK(b.part == p.partial + (long)p.Kf * p.N && b.out == g.q[i].dbias && b.P == plan.splits[i] && b.N == p.N && b.ld == a.ld);
            for (int s = 0; s < b.P; ++s) const_cast<float*>(b.part)[(long)s * b.ld + b.N - 1] += 1.f;
            b.out[b.N - 1] += 1.f;
        }
    }
    CHECK(k == plan.nred && k <= RED_MAX_JOBS);
    // the stand-alone grouped launch lays the same queue out the same way
    TnGroupP g2;
    int sp2[TN_MAX_JOBS];
    CHECK(tn_group_layout(g.q, n, CUS, &g2, sp2) == plan.blocks);
    for (int i = 0; i < n; ++i) CHECK(sp2[i] == plan.splits[i] && g2.blk0[i] == G.blk0[i] && g2.job[i].rows_per_split == G.job[i].rows_per_split);
    std::printf("R=%6d jobs=%d split_db=%d: %4d workgroups, splits", R, n, (int)split_db, plan.blocks);
    for (int i = 0; i < n; ++i) std::printf(" %d", plan.splits[i]);
    std::printf(", %d reduction jobs\n", plan.nred);
}

int main() {
    const int Bs[3] = {120, 128, 250}, Ts[3] = {1, 17, 101};
    for (int B : Bs)
        for (int T : Ts) {
            check_group(B * T, 5, false, 2);
            check_group(B * T, 5, true, 2);
        }
    check_group(512 * 101, 5, false, 2);      // the headline step
    check_group(128 * 17, 1, false, 1);
    check_group(128 * 17, 8, true, 2);
    // groups that do not ride
    {
        Group g;
        make_group(g, 128 * 17, 5, false);
        TnRidePlan plan;
        CHECK(tn_ride_plan(g.q, 0, CUS, 2, &plan) == 0);
        g.q[2].accumulate = 1;
        CHECK(tn_ride_plan(g.q, 5, CUS, 2, &plan) == 0);
        g.q[2].accumulate = 0;
        g.q[1].C += 1;      // an output the vector form of the reductions does not take
        CHECK(tn_ride_plan(g.q, 5, CUS, 2, &plan) == 0);
        g.q[1].C -= 1;
        CHECK(tn_ride_plan(g.q, 5, CUS, RED_MAX_JOBS - 4, &plan) == 0);      // 5 + 20 jobs: more than one list holds
        CHECK(tn_ride_plan(g.q, 5, CUS, RED_MAX_JOBS - 5, &plan) == 1 && plan.nred == RED_MAX_JOBS);
    }
    std::printf("ok\n");
    return 0;
}
