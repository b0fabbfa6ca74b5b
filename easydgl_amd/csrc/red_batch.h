// The deferred partial reductions (k_reduce.hip): the job list of one launch and the body of its vector-form kernel.  Shared with
// the embedding backward's MFMA scatter launch (k_encode.hip), which can carry the list as extra workgroups (edgl_reduce_ride).
#pragma once
#include "edgl_common.h"

constexpr int RED_MAX_JOBS = 24;
constexpr int RED_COL_P = 32;      // jobs with at most this many partial rows run in the column form of the vector kernel
struct RedJob { const float* part; float* out; long ld; int P, N, blk0, f64; };      // f64: the sums of the job in double precision (vector form only)
struct RedBatch { RedJob j[RED_MAX_JOBS]; int n, blocks; };

// k_reduce.hip: hand the calling thread's queue (+ the caller's own jobs) to the scatter launch; 0 = nothing rides, nothing changed; < 0 = a launch failed
int edgl_reduce_ride_take(const RedJob* own, int nown, const float* lo0, const float* hi0, const float* lo1, const float* hi1,
                          RedBatch* out, int* first_blocks, hipStream_t st);

// k_reduce.hip: the vector-form jobs `jobs` as ONE launch on `st` now, whatever the deferred mode holds (the reductions of a launch that
// carried the queue itself: its own partials cannot ride with it); jobs outside the vector form go through edgl_reduce_rows
int edgl_reduce_rows_now(const RedJob* jobs, int n, hipStream_t st);
// k_reduce.hip: edgl_reduce_rows (overwrite) with the sums formed in double precision and rounded once: for partials that are themselves
// long sums (the 128-sample column sums of dx_encode_kernel).  Queued in deferred mode; a job outside the vector form runs in f32.
int edgl_reduce_rows_f64(const float* part, int P, int N, long ld, float* out, hipStream_t st);

// Workgroup `bid` (256 threads) of a list whose blk0 were laid out in the vector form; sm: 32 x 9 float4 (4.6 KB) of LDS.
__device__ __forceinline__ void reduce_rows_vec_block(const RedBatch& b, int bid, float4 (*sm)[9]) {
    int ji = 0;
    for (int i = 1; i < b.n; ++i)
        if (bid >= b.j[i].blk0) ji = i;
    const RedJob& jb = b.j[ji];
    const int P = jb.P, N = jb.N;
    const long ld = jb.ld;
    if (jb.f64) {      // (block-uniform) row-lane layout for any P, double accumulators, two components per pass through the scratch
        const int tx = threadIdx.x & 7, ty = threadIdx.x >> 3;
        const int n = (bid - jb.blk0) * 32 + 4 * tx;
        double a[4] = {0., 0., 0., 0.};
        if (n < N)
            for (int p = ty; p < P; p += 32) {
                const float4 v = *reinterpret_cast<const float4*>(jb.part + n + (long)p * ld);
                a[0] += v.x; a[1] += v.y; a[2] += v.z; a[3] += v.w;
            }
        double2 (*sd)[9] = reinterpret_cast<double2(*)[9]>(sm);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            sd[ty][tx] = make_double2(a[2 * h], a[2 * h + 1]);
            __syncthreads();
            if (ty < 2 && n < N) {
                double s = 0.;
#pragma unroll
                for (int i = 0; i < 32; ++i) s += ty == 0 ? sd[i][tx].x : sd[i][tx].y;
                jb.out[n + 2 * h + ty] = (float)s;
            }
            __syncthreads();
        }
        return;
    }
    if (P <= RED_COL_P) {
        // few partial rows (the row splits of a weight-gradient GEMM: 2-24 slabs of up to 3 M elements): a thread owns one
        // float4 column and adds its P values — 4 KB of consecutive bytes per row and workgroup, 32x fewer workgroups than the
        // row-lane form, whose 32 lanes per column would mostly idle (the 512-unit recipe's lists took 213 us for 143 MB)
        const int n = ((bid - jb.blk0) * 256 + (int)threadIdx.x) * 4;
        if (n >= N) return;
        const float* base = jb.part + n;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        int p0 = 0;
        for (; p0 + 8 <= P; p0 += 8) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(base + (long)(p0 + u) * ld);
#pragma unroll
            for (int u = 0; u < 8; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
        }
        for (; p0 < P; ++p0) {
            const float4 v = *reinterpret_cast<const float4*>(base + (long)p0 * ld);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        *reinterpret_cast<float4*>(jb.out + n) = acc;
        return;
    }
    const int tx = threadIdx.x & 7, ty = threadIdx.x >> 3;          // float4 column group, row lane
    const int n = (bid - jb.blk0) * 32 + 4 * tx;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n < N) {
        const float* base = jb.part + n;
        int p = ty;
        for (; p + 7 * 32 < P; p += 8 * 32) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(base + (long)(p + 32 * u) * ld);
#pragma unroll
            for (int u = 0; u < 8; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
        }
        for (; p < P; p += 32) {
            const float4 v = *reinterpret_cast<const float4*>(base + (long)p * ld);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
    }
    sm[ty][tx] = acc;
    __syncthreads();
    if (ty < 4 && n < N) {       // 32 threads finish the 32 columns: thread (ty, tx) takes component ty of group tx
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const float4 v = sm[i][tx];
            s += ty == 0 ? v.x : (ty == 1 ? v.y : (ty == 2 ? v.z : v.w));
        }
        jb.out[n + ty] = s;
    }
}
