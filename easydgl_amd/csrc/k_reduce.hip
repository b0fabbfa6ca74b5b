// Partial-sum reductions out[n] (+)= sum_p part[p * ld + n] in a fixed summation order, and the queue that collects them in
// deferred mode so that one launch (or the embedding scatter's / the dX-encode launch, red_batch.h) runs the whole list.
#include "edgl_common.h"
#include "red_batch.h"      // job list of the deferred reductions (also run inside the embedding scatter's launch)

namespace {

// 32 columns x 8 row lanes per block; each thread keeps 4 independent partial sums in flight
// (reduce_rows_multi_kernel<8> below on a single job, plus `accumulate`: kept as two texts — a body shared between them moved
// instructions of the list kernels)
__global__ __launch_bounds__(256) void reduce_rows_kernel(const float* part, int P, int N, long ld, float* out, int accumulate) {
    __shared__ float sm[8][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int n = blockIdx.x * 32 + tx;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (n < N) {
        int p = ty;
        for (; p + 24 < P; p += 32) {
            a0 += part[(long)p * ld + n];
            a1 += part[(long)(p + 8) * ld + n];
            a2 += part[(long)(p + 16) * ld + n];
            a3 += part[(long)(p + 24) * ld + n];
        }
        for (; p < P; p += 8) a0 += part[(long)p * ld + n];
    }
    sm[ty][tx] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (ty == 0 && n < N) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) s += sm[i][tx];
        out[n] = accumulate ? out[n] + s : s;
    }
}

}  // namespace

// ---- deferred reductions ------------------------------------------------------------------------------------------
// Every backward kernel that produces per-workgroup partials ends with one of these reductions; each is a few
// microseconds of work behind a full kernel launch.  In deferred mode (edgl_reduce_defer(1)) the calls are collected on
// the host and edgl_reduce_flush() runs all of them in ONE launch.  The caller must then keep every partial buffer
// alive (distinct workspaces) until the flush.  Jobs that accumulate into `out` flush first and run immediately, so the
// order of read-modify-write updates is preserved.
static inline int red_blocks_scalar(const RedJob& j) { return (j.N + 31) / 32; }
static inline int red_blocks_vec(const RedJob& j) { return j.P <= RED_COL_P && !j.f64 ? (j.N + 1023) / 1024 : (j.N + 31) / 32; }
static inline bool red_job_vec(const RedJob& j) {
    return (j.N & 3) == 0 && (j.ld & 3) == 0 && (((uintptr_t)j.part | (uintptr_t)j.out) & 15) == 0;
}
// first-block index of every job of the list, and the list's block count, for the kernel form chosen
static void red_assign_blocks(RedBatch& b, bool vec) {
    int blocks = 0;
    for (int i = 0; i < b.n; ++i) {
        b.j[i].blk0 = blocks;
        blocks += vec ? red_blocks_vec(b.j[i]) : red_blocks_scalar(b.j[i]);
    }
    b.blocks = blocks;
}
thread_local bool g_red_defer = false;
thread_local RedBatch g_red_batch = {};
thread_local int g_red_ride = 0;       // edgl_reduce_ride: 1 / 2 = the queue may leave with the embedding scatter's launch (in front of / behind its blocks)

// 32 columns per workgroup.  Scalar form: one column per thread x RL partial-row lanes (RL = 8, or 32 when a list holds a deep job:
// the 1616 partial rows of the mark-embedding gradient were a chain of 50 dependent loads per thread with 8 lanes).
// Vector form (every job of the list has N, ld and both pointers multiples of four floats — the layouts of all producers here):
// 8 float4 column groups x 32 row lanes in 256 threads, eight loads in flight per thread: a 512-row job is two rounds of loads
// instead of sixteen (the scalar list of the headline step took 26 us for ~12 MB: latency, not bandwidth).
template <int RL>
__global__ __launch_bounds__(32 * RL) void reduce_rows_multi_kernel(RedBatch b) {
    __shared__ float sm[RL][33];
    int ji = 0;
    for (int i = 1; i < b.n; ++i)
        if ((int)blockIdx.x >= b.j[i].blk0) ji = i;
    const RedJob& jb = b.j[ji];
    const float* part = jb.part;
    const int P = jb.P, N = jb.N;
    const long ld = jb.ld;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int n = ((int)blockIdx.x - jb.blk0) * 32 + tx;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (n < N) {
        int p = ty;
        for (; p + 3 * RL < P; p += 4 * RL) {
            a0 += part[(long)p * ld + n];
            a1 += part[(long)(p + RL) * ld + n];
            a2 += part[(long)(p + 2 * RL) * ld + n];
            a3 += part[(long)(p + 3 * RL) * ld + n];
        }
        for (; p < P; p += RL) a0 += part[(long)p * ld + n];
    }
    sm[ty][tx] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (ty == 0 && n < N) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < RL; ++i) s += sm[i][tx];
        jb.out[n] = s;
    }
}

__global__ __launch_bounds__(256) void reduce_rows_multi_vec_kernel(RedBatch b) {
    __shared__ float4 sm[32][9];
    reduce_rows_vec_block(b, (int)blockIdx.x, sm);      // (red_batch.h: the body is shared with the embedding scatter's launch)
}

int edgl_reduce_flush_impl(hipStream_t st) {
    if (g_red_batch.n == 0) return EDGL_OK;
    int maxp = 0;
    bool vec = true;
    for (int i = 0; i < g_red_batch.n; ++i) {
        const RedJob& j = g_red_batch.j[i];
        maxp = std::max(maxp, j.P);
        vec = vec && red_job_vec(j);
    }
    red_assign_blocks(g_red_batch, vec);
    if (vec) hipLaunchKernelGGL(reduce_rows_multi_vec_kernel, dim3(g_red_batch.blocks), dim3(256), 0, st, g_red_batch);
    else if (maxp > 1024) hipLaunchKernelGGL(reduce_rows_multi_kernel<32>, dim3(g_red_batch.blocks), dim3(1024), 0, st, g_red_batch);
    else hipLaunchKernelGGL(reduce_rows_multi_kernel<8>, dim3(g_red_batch.blocks), dim3(256), 0, st, g_red_batch);
    g_red_batch.n = 0;
    g_red_batch.blocks = 0;
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

int edgl_reduce_rows(const float* part, int P, int N, long ld, float* out, int accumulate, hipStream_t st) {
    if (g_red_defer && !accumulate) {
        if (g_red_batch.n == RED_MAX_JOBS) {
            const int rc = edgl_reduce_flush_impl(st);
            if (rc) return rc;
        }
        RedJob& j = g_red_batch.j[g_red_batch.n++];
        j.part = part; j.out = out; j.ld = ld; j.P = P; j.N = N; j.blk0 = g_red_batch.blocks; j.f64 = 0;
        g_red_batch.blocks += (N + 31) / 32;
        return EDGL_OK;
    }
    if (g_red_defer) {   // read-modify-write job: everything queued before it must have landed
        const int rc = edgl_reduce_flush_impl(st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(reduce_rows_kernel, dim3((N + 31) / 32), dim3(256), 0, st, part, P, N, ld, out, accumulate);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

// Hand-over of the queue to the embedding backward's MFMA scatter launch (k_encode.hip), which runs the jobs as extra workgroups:
// `own` = the caller's d_pos / d_mark jobs, not yet queued; lo / hi = the two address ranges its atomics add into.  Returns the number
// of reduction workgroups (*first_blocks: in front of the scatter's) with the list in *out and the queue empty, a negative error
// code when the launch below failed, or 0 with everything as it was: riding not requested, not in deferred mode, a job outside the vector form (the form, and with it the order of the
// additions, is chosen per list), or a job whose output lies inside a range — the flush assigns it BEHIND the scatter.  A list too
// long for one batch with the caller's jobs is launched here, in the vector form it would have had anyway.
int edgl_reduce_ride_take(const RedJob* own, int nown, const float* lo0, const float* hi0, const float* lo1, const float* hi1,
                          RedBatch* out, int* first_blocks, hipStream_t st) {
    if (!g_red_defer || !g_red_ride) return 0;
    auto rides = [&](const RedJob& j) {
        const float* o0 = j.out;
        const float* o1 = j.out + j.N;
        return red_job_vec(j) && !(o0 < hi0 && lo0 < o1) && !(o0 < hi1 && lo1 < o1);
    };
    for (int i = 0; i < g_red_batch.n; ++i)
        if (!rides(g_red_batch.j[i])) return 0;
    for (int i = 0; i < nown; ++i)
        if (!rides(own[i])) return 0;
    if (g_red_batch.n + nown > RED_MAX_JOBS) {
        const int rc = edgl_reduce_flush_impl(st);
        if (rc) return rc;
    }
    for (int i = 0; i < nown; ++i) g_red_batch.j[g_red_batch.n++] = own[i];
    red_assign_blocks(g_red_batch, true);
    const int blocks = g_red_batch.blocks;
    *out = g_red_batch;
    *first_blocks = g_red_ride == 1;
    g_red_batch.n = 0;
    g_red_batch.blocks = 0;
    return blocks;
}

int edgl_reduce_rows_now(const RedJob* jobs, int n, hipStream_t st) {
    if (n <= 0) return EDGL_OK;
    bool vec = n <= RED_MAX_JOBS;
    for (int i = 0; i < n && vec; ++i) vec = red_job_vec(jobs[i]);
    if (!vec) {
        for (int i = 0; i < n; ++i) {
            const int rc = edgl_reduce_rows(jobs[i].part, jobs[i].P, jobs[i].N, jobs[i].ld, jobs[i].out, 0, st);
            if (rc) return rc;
        }
        return EDGL_OK;
    }
    RedBatch b;
    b.n = n;
    for (int i = 0; i < n; ++i) b.j[i] = jobs[i];
    red_assign_blocks(b, true);
    hipLaunchKernelGGL(reduce_rows_multi_vec_kernel, dim3(b.blocks), dim3(256), 0, st, b);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

int edgl_reduce_rows_f64(const float* part, int P, int N, long ld, float* out, hipStream_t st) {
    const RedJob j{part, out, ld, P, N, g_red_batch.blocks, 1};
    if (!red_job_vec(j)) return edgl_reduce_rows(part, P, N, ld, out, 0, st);
    if (!g_red_defer) return edgl_reduce_rows_now(&j, 1, st);
    if (g_red_batch.n == RED_MAX_JOBS) {
        const int rc = edgl_reduce_flush_impl(st);
        if (rc) return rc;
    }
    g_red_batch.j[g_red_batch.n] = j;
    g_red_batch.j[g_red_batch.n++].blk0 = g_red_batch.blocks;
    g_red_batch.blocks += (N + 31) / 32;
    return EDGL_OK;
}

extern "C" int edgl_reduce_ride(int on) {
    EDGL_REQUIRE(on >= 0 && on <= 2, EDGL_ERR_SHAPE, "edgl_reduce_ride: on = %d (0: off, 1: in front of the scatter's workgroups, 2: behind)", on);
    g_red_ride = on;
    return EDGL_OK;
}

extern "C" int edgl_reduce_partials(const float* part, int P, int N, long ld, float* out, int accumulate, void* stream) {
    EDGL_REQUIRE(part && out, EDGL_ERR_NULL, "edgl_reduce_partials: null pointer");
    EDGL_REQUIRE(P > 0 && N > 0 && ld >= N, EDGL_ERR_SHAPE, "edgl_reduce_partials: bad shape P=%d N=%d ld=%ld", P, N, ld);
    return edgl_reduce_rows(part, P, N, ld, out, accumulate, (hipStream_t)stream);
}

extern "C" int edgl_reduce_defer(int on, void* stream) {
    if (on <= 0) g_red_ride = 0;      // (a riding request ends with the deferred mode it belongs to)
    if (on < 0) {   // abort: forget the queued jobs (their partial buffers may be gone) and leave deferred mode
        g_red_batch.n = 0;
        g_red_batch.blocks = 0;
        g_red_defer = false;
        return EDGL_OK;
    }
    if (!on && g_red_defer) {
        const int rc = edgl_reduce_flush_impl((hipStream_t)stream);
        if (rc) return rc;
    }
    g_red_defer = on != 0;
    return EDGL_OK;
}

extern "C" int edgl_reduce_flush(void* stream) { return edgl_reduce_flush_impl((hipStream_t)stream); }
