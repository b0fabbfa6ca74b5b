// Deterministic scatter-add into the item table: the gradient of the embedding lookup (coding.py:60-64:
// d_item[id] += sqrt(C) dX0[row, :C]) and the one-hot term of the tied table's scoring gradient (EasyDGL.py:177-185:
// d_table[label] -= coef rows, d_bias[label - 1] -= coef) WITHOUT f32 atomics.  The table gradient of the sampled-softmax loss
// (k_cand_ce.hip, DESIGN §4.13: one entry per list slot, d_table[c] += dv rows[r]) runs through the same plan and sums.
//
//   (a) the plan: a stable LSD radix sort of the row indices by item id — per pass a per-block digit histogram, one scan over
//       [digit][block] and a scatter with stable in-block ranks (wave match + fixed (round, wave) order).  Integer LDS atomics
//       only count digits; where a row lands follows from the counts and the ranks alone.  Dropped entries (key 0, rows
//       behind the device row count, keys outside [i0, i1)) sort as key 0 and are cut off in front.  Equal ids keep ascending rows.
//   (b) the ordered sum: the sorted positions are cut into windows of SUB positions; a thread group walks one window in plan
//       order.  A segment (the rows of one id) inside one window is added to its table row by that group; a segment that
//       crosses windows leaves one partial per window, and the group of the window it starts in adds them up in window order
//       (8 interleaved accumulators, joined in a fixed tree).  One writer per table row per call, plain loads and stores; the
//       order of every sum is a function of the keys (and n, the row count, the range) — never of timing.
// No host read-back: grids are sized from n, the kernels read nseg / the kept-row count from the plan and exit past them.
#include "edgl_common.h"

namespace segsum {

constexpr int TILE = 1024;   // keys of one sort block: 256 threads x 4 rounds
constexpr int SUB = 64;      // sorted positions of one sequential walk
constexpr int CMAX = 512;    // widest row the partial area of a plan is sized for

// Plan buffer, in 32-bit words (easydgl_hip.h documents the caller-visible front: header, perm, seg_key, seg_start)
struct Layout {
    long hdr, perm, seg_key, seg_start, seg_id, keyA, idxA, keyB, idxB, hist, bheads, bzeros, part, partb, total;
    int nblk, nsub;
};
static inline long up4(long x) { return (x + 3) & ~3L; }
static Layout layout(long n) {
    Layout L;
    const long n4 = up4(n);
    L.nblk = (int)((n + TILE - 1) / TILE);
    L.nsub = (int)((n + SUB - 1) / SUB);
    long o = 0;
    L.hdr = o; o += 4;
    L.perm = o; o += n4;
    L.seg_key = o; o += n4;
    L.seg_start = o; o += n4 + 4;
    L.seg_id = o; o += n4;
    L.keyA = o; o += n4;
    L.idxA = o; o += n4;
    L.keyB = o; o += n4;
    L.idxB = o; o += n4;
    L.hist = o; o += 256L * L.nblk;
    L.bheads = o; o += up4(L.nblk);
    L.bzeros = o; o += up4(L.nblk);
    L.part = o; o += (long)L.nsub * 2 * CMAX;
    L.partb = o; o += up4((long)L.nsub * 2);
    L.total = o;
    return L;
}

struct SortP {
    const int64_t* keys; const int32_t* nvalid; int n, i0, i1;      // first pass: the caller's keys
    int kofs;                                                       // ... sorted as keys[e] + kofs (1: a table whose row 0 counts)
    const uint32_t* kin; const int32_t* iin;                        // later passes: the previous pass' output
    uint32_t* kout; int32_t* iout;
    int32_t* hist; int nblk; int shift;
};

// key / source row of element e (< n) as this pass reads it
template <bool FIRST>
__device__ __forceinline__ uint32_t sort_load(const SortP& p, int e, int nlive, int32_t& idx) {
    if constexpr (FIRST) {
        idx = e;
        const int64_t k = p.keys[e] + p.kofs;
        const bool keep = e < nlive && k != 0 && k >= p.i0 && k < p.i1;
        return keep ? (uint32_t)k : 0u;
    } else {
        idx = p.iin[e];
        return p.kin[e];
    }
}
__device__ __forceinline__ int sort_nlive(const SortP& p) { return p.nvalid ? min(p.n, max(p.nvalid[0], 0)) : p.n; }

// hist[digit][block] = number of the block's keys with that digit
template <bool FIRST>
__global__ __launch_bounds__(256) void sort_hist_kernel(SortP p) {
    __shared__ int h[256];
    const int tid = threadIdx.x, blk = blockIdx.x;
    h[tid] = 0;
    __syncthreads();
    const int nlive = sort_nlive(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = blk * TILE + j * 256 + tid;
        if (e < p.n) {
            int32_t ix;
            const uint32_t k = sort_load<FIRST>(p, e, nlive, ix);
            atomicAdd(&h[(k >> p.shift) & 255u], 1);      // a count: its value does not depend on the order of the adds
        }
    }
    __syncthreads();
    p.hist[tid * p.nblk + blk] = h[tid];
}

// all threads get the exclusive prefix of v over the block (threads in index order); red: blockDim / 64 ints
__device__ __forceinline__ int block_excl_scan(int v, int* red, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) red[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int i = 0; i < nw; ++i) {
        const int r = red[i];
        if (i < w) base += r;
        tot += r;
    }
    total = tot;
    return base + inc - v;
}

// exclusive scan of hist in [digit][block] order, in place (one workgroup: 256 * nblk counts)
__global__ __launch_bounds__(1024) void sort_scan_kernel(int32_t* hist, int M) {
    __shared__ int red[16];
    const int tid = threadIdx.x;
    const int per = (M + 1023) / 1024;
    const int lo = min(M, tid * per), hi = min(M, lo + per);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += hist[i];
    int total;
    int run = block_excl_scan(s, red, total);
    for (int i = lo; i < hi; ++i) {
        const int v = hist[i];
        hist[i] = run;
        run += v;
    }
}

// position = scanned hist[digit][block] + (keys of the block with the same digit in front of this one).  The in-block order is
// (round, wave, lane) = ascending element index: a wave finds its equal digits with eight ballots, the (round, wave) counts are
// prefixed per digit by one thread each.
template <bool FIRST>
__global__ __launch_bounds__(256) void sort_scatter_kernel(SortP p) {
    __shared__ int cnt[16][256];
    const int tid = threadIdx.x, blk = blockIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int s = 0; s < 16; ++s) cnt[s][tid] = 0;
    __syncthreads();
    const int nlive = sort_nlive(p);
    uint32_t k[4]; int32_t ix[4]; int rk[4], dg[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = blk * TILE + j * 256 + tid;
        const bool valid = e < p.n;
        k[j] = 0u; ix[j] = 0;
        if (valid) k[j] = sort_load<FIRST>(p, e, nlive, ix[j]);
        const int d = valid ? (int)((k[j] >> p.shift) & 255u) : 0;
        unsigned long long m = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1;
            const unsigned long long bal = __ballot(bit);
            m &= bit ? bal : ~bal;
        }
        dg[j] = valid ? d : -1;
        rk[j] = __popcll(m & ((1ull << lane) - 1ull));
        if (valid && rk[j] == 0) cnt[j * 4 + wave][d] = __popcll(m);      // one writer per (round, wave, digit)
    }
    __syncthreads();
    {
        int run = 0;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int v = cnt[s][tid];
            cnt[s][tid] = run;
            run += v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (dg[j] < 0) continue;
        const int pos = p.hist[dg[j] * p.nblk + blk] + cnt[j * 4 + wave][dg[j]] + rk[j];      // < n: the counts cover valid keys only
        p.kout[pos] = k[j];
        p.iout[pos] = ix[j];
    }
}

__device__ __forceinline__ int wave_isum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// all threads get the block-wide sums of a and b (256 threads)
__device__ __forceinline__ void block_isum2(int& a, int& b, int (*red)[2]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    a = wave_isum(a); b = wave_isum(b);
    __syncthreads();
    if (lane == 0) { red[w][0] = a; red[w][1] = b; }
    __syncthreads();
    a = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    b = red[0][1] + red[1][1] + red[2][1] + red[3][1];
}

// per sort block of the SORTED keys: segment heads (a nonzero key that differs from its predecessor) and dropped entries (key 0)
__global__ __launch_bounds__(256) void seg_count_kernel(const uint32_t* ks, int n, int32_t* bheads, int32_t* bzeros) {
    __shared__ int red[4][2];
    int h = 0, z = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = blockIdx.x * TILE + threadIdx.x * 4 + j;
        if (q < n) {
            const uint32_t k = ks[q];
            z += k == 0u;
            h += k != 0u && (q == 0 || ks[q - 1] != k);
        }
    }
    block_isum2(h, z, red);
    if (threadIdx.x == 0) { bheads[blockIdx.x] = h; bzeros[blockIdx.x] = z; }
}

// the plan's caller-visible arrays: perm (kept rows in sorted order), seg_key / seg_start per distinct id, the segment of every
// kept position, and the header (nseg, kept rows)
__global__ __launch_bounds__(256) void seg_write_kernel(const uint32_t* ks, const int32_t* is, int n, int nblk, const int32_t* bheads,
                                                        const int32_t* bzeros, int32_t* hdr, int32_t* perm, int32_t* seg_key,
                                                        int32_t* seg_start, int32_t* seg_id) {
    __shared__ int red[4][2];
    __shared__ int red2[4][2];
    __shared__ int sred[4];
    const int tid = threadIdx.x, blk = blockIdx.x;
    int hbase = 0, htot = 0, ztot = 0, dummy = 0;
    for (int i = tid; i < nblk; i += 256) {
        const int h = bheads[i];
        htot += h;
        if (i < blk) hbase += h;
        ztot += bzeros[i];
    }
    block_isum2(htot, ztot, red);
    block_isum2(hbase, dummy, red2);
    uint32_t k[4]; bool head[4]; int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = blk * TILE + tid * 4 + j;
        k[j] = q < n ? ks[q] : 0u;
        head[j] = q < n && k[j] != 0u && (q == 0 || ks[q - 1] != k[j]);
        c += head[j];
    }
    int total;
    int seen = hbase + block_excl_scan(c, sred, total);      // heads in front of this thread's first position
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = blk * TILE + tid * 4 + j;
        if (q >= n || k[j] == 0u) continue;
        const int pos = q - ztot;      // the dropped entries sort in front
        if (head[j]) {
            seg_key[seen] = (int32_t)k[j];
            seg_start[seen] = pos;
            ++seen;
        }
        seg_id[pos] = seen - 1;
        perm[pos] = is[q];
    }
    if (blk == 0 && tid == 0) {
        hdr[0] = htot;
        hdr[1] = n - ztot;
        seg_start[htot] = n - ztot;
    }
}

// ---- (b) the ordered sum ------------------------------------------------------------------------------------------------------
struct SumP {
    const int32_t* hdr; const int32_t* perm; const int32_t* seg_key; const int32_t* seg_start; const int32_t* seg_id;
    float* part; float* partb;      // [nsub][2][C], [nsub][2]: slot 0 = the segment that came in from the left, 1 = the one that leaves
    int C;
    const void* src; const void* add1; const void* add2;      // embedding rows: dX0 (leading dimension 3C), optional [rows, C] terms
    long ld;                                                  // item rows (ROWS): leading dimension of src, C or 2C
    float sq; float rate; const uint64_t* rng; uint32_t stream_id;
    const float* coef; const float* gscale;                   // label rows: src = the compacted head rows [R, C]
    const float* dv; int np1;                                 // list slots (CAND_ROWS): entry e = slot e % np1 of row e / np1, src = rows [R, C]
    float* d_item; float* d_bias;
};

__device__ __forceinline__ void add4(float* dst, const float (&a)[4]) {
    float4 v = *reinterpret_cast<float4*>(dst);
    v.x += a[0]; v.y += a[1]; v.z += a[2]; v.w += a[3];
    *reinterpret_cast<float4*>(dst) = v;
}

// x + a + b rounded ONCE (two error-free additions, the two errors added back): the residual branches may cancel against dX0, and a
// plain f32 chain then carries the rounding of x + a — an error relative to |x| + |a|, not to the term the sum contributes
__device__ __forceinline__ float sum3(float x, float a, float b) {
    const float s = x + a, bs = s - x, e1 = (x - (s - bs)) + (a - bs);
    const float t = s + b, bt = t - s, e2 = (s - (t - bt)) + (b - bt);
    return t + (e1 + e2);
}

// EMBED: term = sqrt(C_true) * drop(dX0[row, c] (+ add1 + add2)), the mask of element row * 3C + c (encode_scatter_kernel)
// LABEL: term = -gscale coef[row] rows[row, c];  bias term -gscale coef[row]
// ROWS : term = sq * drop(src[row * ld + c]), the mask of element row * ld + c (embed_pos_bwd_kernel; rate 0: embedding_bwd_kernel)
// CAND : the plan's entries are the slots of per-row candidate lists (k_cand_ce.hip): term = dv[e] rows[e / np1, c];
//        bias term dv[e]
enum { EMBED = 0, LABEL_ROWS = 1, ROWS = 2, CAND_ROWS = 3 };
template <typename T, int ROLE>
__global__ __launch_bounds__(256) void segsum_walk_kernel(SumP p) {
    constexpr bool LABEL = ROLE == LABEL_ROWS, CAND = ROLE == CAND_ROWS, BIAS = LABEL || CAND;
    const int cpr = p.C >> 2, rows_par = 256 / cpr;
    const int tid = threadIdx.x, cv = tid % cpr, rl = tid / cpr, c0 = cv * 4;
    if (rl >= rows_par) return;
    const int nkept = p.hdr[1];
    const long u = (long)blockIdx.x * rows_par + rl;
    const long p0 = u * SUB;
    if (p0 >= nkept) return;
    const int p1 = (int)min(p0 + (long)SUB, (long)nkept);
    const DropKey dk = make_dropkey(p.rng, p.stream_id, BIAS ? 0.f : p.rate);
    const float gs = LABEL ? (p.gscale ? p.gscale[0] : 1.0f) : 0.f;
    const T* src = reinterpret_cast<const T*>(p.src);
    const long ld = BIAS ? p.C : (ROLE == ROWS ? p.ld : 3L * p.C);
    const bool adds = ROLE == EMBED && p.add1;
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, accb = 0.f;
    int s_cur = p.seg_id[p0];
    auto flush = [&]() {
        const int a = p.seg_start[s_cur], b = p.seg_start[s_cur + 1];
        if (a >= p0 && b <= p0 + SUB) {      // the whole segment lies in this window: its only writer
            const long key = p.seg_key[s_cur];
            add4(p.d_item + key * p.C + c0, acc);
            if (BIAS && cv == 0) p.d_bias[key - 1] += accb;
        } else {
            const int slot = a < p0 ? 0 : 1;
            float* dst = p.part + (u * 2 + slot) * p.C + c0;
            *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            if (BIAS && cv == 0) p.partb[u * 2 + slot] = accb;
        }
    };
    for (int pb = (int)p0; pb < p1; pb += 8) {
        int row[8], sid[8];
        Frag4<T> g[8], ga[8], gb[8];
        float cf[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int q = min(pb + k, p1 - 1);
            row[k] = p.perm[q];
            sid[k] = p.seg_id[q];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (CAND) {      // (the entry's coefficient first: `row` then becomes the row the slot belongs to)
                cf[k] = p.dv[row[k]];
                row[k] /= p.np1;
            }
            g[k] = frag_ld<T>(src + row[k] * ld + c0);
            if (adds) {
                ga[k] = frag_ld<T>(reinterpret_cast<const T*>(p.add1) + (long)row[k] * p.C + c0);
                gb[k] = frag_ld<T>(reinterpret_cast<const T*>(p.add2) + (long)row[k] * p.C + c0);
            }
            if (LABEL) cf[k] = p.coef[row[k]];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (pb + k >= p1) break;
            if (sid[k] != s_cur) {
                flush();
                s_cur = sid[k];
                acc[0] = acc[1] = acc[2] = acc[3] = 0.f; accb = 0.f;
            }
            float gv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) gv[j] = to_f32(g[k].v[j]);
            if (adds) {
#pragma unroll
                for (int j = 0; j < 4; ++j) gv[j] = sum3(gv[j], to_f32(ga[k].v[j]), to_f32(gb[k].v[j]));
            }
            if (BIAS) {
                const float w = CAND ? cf[k] : -(gs * cf[k]);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] += w * gv[j];
                accb += w;
            } else {
                drop_apply4(dk, (uint64_t)row[k] * ld + c0, gv);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] += p.sq * gv[j];
            }
        }
    }
    flush();
}

// the segments that cross windows: the group of the window a segment STARTS in adds its partials in window order
template <bool LABEL>
__global__ __launch_bounds__(256) void segsum_join_kernel(SumP p) {
    const int cpr = p.C >> 2, rows_par = 256 / cpr;
    const int tid = threadIdx.x, cv = tid % cpr, rl = tid / cpr, c0 = cv * 4;
    if (rl >= rows_par) return;
    const int nkept = p.hdr[1];
    const long u = (long)blockIdx.x * rows_par + rl;
    const long p0 = u * SUB;
    if (p0 >= nkept) return;
    const int pl = (int)min(p0 + (long)SUB, (long)nkept) - 1;
    const int s = p.seg_id[pl];
    const int a = p.seg_start[s], b = p.seg_start[s + 1];
    if (a < p0 || b <= p0 + SUB) return;      // came in from the left (its start window owns it), or complete inside this window
    const int np = (b - 1) / SUB - (int)u + 1;      // partials: slot 1 of this window, slot 0 of the following ones
    float acc[8][4], accb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.f; accb[i] = 0.f; }
    for (int j0 = 0; j0 < np; j0 += 8) {
        float4 v[8]; float vb[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int j = j0 + i;
            const long sl = (u + min(j, np - 1)) * 2 + (j == 0 ? 1 : 0);
            v[i] = *reinterpret_cast<const float4*>(p.part + sl * p.C + c0);
            vb[i] = LABEL ? p.partb[sl] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (j0 + i >= np) break;
            acc[i][0] += v[i].x; acc[i][1] += v[i].y; acc[i][2] += v[i].z; acc[i][3] += v[i].w;
            accb[i] += vb[i];
        }
    }
    float t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        t[j] = ((acc[0][j] + acc[1][j]) + (acc[2][j] + acc[3][j])) + ((acc[4][j] + acc[5][j]) + (acc[6][j] + acc[7][j]));
    const long key = p.seg_key[s];
    add4(p.d_item + key * p.C + c0, t);
    if (LABEL && cv == 0)
        p.d_bias[key - 1] += ((accb[0] + accb[1]) + (accb[2] + accb[3])) + ((accb[4] + accb[5]) + (accb[6] + accb[7]));
}

static int bits_of(long x) {
    int b = 0;
    while (x > 0) { ++b; x >>= 1; }
    return b;
}

}  // namespace segsum

extern "C" int edgl_segsum_passes(int I) {
    if (I < 2) return -1;
    return (segsum::bits_of((long)I - 1) + 7) / 8;
}

extern "C" long edgl_segsum_plan_bytes(int n, int I) {
    if (n < 1 || I < 2) return -1;
    return segsum::layout(n).total * 4;
}

// the plan of keys[e] + kofs (kofs = 1 with [i0, i1) = [1, I): key 0 of the caller is kept, as key 1)
static int segsum_plan_ofs(const int64_t* keys, int n, const int32_t* nvalid, int I, int i0, int i1, int kofs, void* plan, void* stream);

extern "C" int edgl_segsum_plan(const int64_t* keys, int n, const int32_t* nvalid, int I, int i0, int i1, void* plan, void* stream) {
    return segsum_plan_ofs(keys, n, nvalid, I, i0, i1, 0, plan, stream);
}

static int segsum_plan_ofs(const int64_t* keys, int n, const int32_t* nvalid, int I, int i0, int i1, int kofs, void* plan, void* stream) {
    using namespace segsum;
    EDGL_REQUIRE(keys && plan, EDGL_ERR_NULL, "edgl_segsum_plan: null pointer");
    EDGL_REQUIRE(n > 0 && I > 1 && i0 >= 0 && i1 <= I && i0 < i1, EDGL_ERR_SHAPE, "edgl_segsum_plan: bad shape n=%d I=%d [%d,%d)", n, I, i0, i1);
    EDGL_REQUIRE(((uintptr_t)plan & 15) == 0, EDGL_ERR_SHAPE, "edgl_segsum_plan: the plan buffer must be 16-byte aligned");
    const Layout L = layout(n);
    int32_t* w = reinterpret_cast<int32_t*>(plan);
    hipStream_t st = (hipStream_t)stream;
    uint32_t* kb[2] = {reinterpret_cast<uint32_t*>(w + L.keyA), reinterpret_cast<uint32_t*>(w + L.keyB)};
    int32_t* ib[2] = {w + L.idxA, w + L.idxB};
    const int passes = edgl_segsum_passes(I);
    SortP p{};
    p.keys = keys; p.nvalid = nvalid; p.n = n; p.i0 = i0; p.i1 = i1; p.kofs = kofs; p.hist = w + L.hist; p.nblk = L.nblk;
    for (int ps = 0; ps < passes; ++ps) {
        p.shift = 8 * ps;
        p.kin = ps ? kb[(ps - 1) & 1] : nullptr; p.iin = ps ? ib[(ps - 1) & 1] : nullptr;
        p.kout = kb[ps & 1]; p.iout = ib[ps & 1];
        if (ps == 0) hipLaunchKernelGGL(sort_hist_kernel<true>, dim3(L.nblk), dim3(256), 0, st, p);
        else hipLaunchKernelGGL(sort_hist_kernel<false>, dim3(L.nblk), dim3(256), 0, st, p);
        hipLaunchKernelGGL(sort_scan_kernel, dim3(1), dim3(1024), 0, st, p.hist, 256 * L.nblk);
        if (ps == 0) hipLaunchKernelGGL(sort_scatter_kernel<true>, dim3(L.nblk), dim3(256), 0, st, p);
        else hipLaunchKernelGGL(sort_scatter_kernel<false>, dim3(L.nblk), dim3(256), 0, st, p);
        EDGL_LAUNCH_CHECK();
    }
    const uint32_t* ks = kb[(passes - 1) & 1];
    const int32_t* is = ib[(passes - 1) & 1];
    hipLaunchKernelGGL(seg_count_kernel, dim3(L.nblk), dim3(256), 0, st, ks, n, w + L.bheads, w + L.bzeros);
    hipLaunchKernelGGL(seg_write_kernel, dim3(L.nblk), dim3(256), 0, st, ks, is, n, L.nblk, w + L.bheads, w + L.bzeros, w + L.hdr,
                       w + L.perm, w + L.seg_key, w + L.seg_start, w + L.seg_id);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

// the two ordered sums over a plan this call builds first (called from k_encode.hip / k_score.hip)
static int segsum_run(int role, const int64_t* keys, int n, const int32_t* nvalid, int I, int i0, int i1, int kofs, segsum::SumP p,
                      void* plan, int dtype, hipStream_t st) {
    using namespace segsum;
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_segsum: bad dtype %d", dtype);
    EDGL_REQUIRE(p.C > 0 && p.C % 4 == 0 && p.C <= CMAX, EDGL_ERR_SHAPE, "edgl_segsum: C=%d unsupported (a multiple of 4 up to %d)", p.C, CMAX);
    const uintptr_t al = (uintptr_t)p.src | (uintptr_t)p.add1 | (uintptr_t)p.add2;
    EDGL_REQUIRE((al & (dtype == EDGL_F32 ? 15 : 7)) == 0 && ((uintptr_t)p.d_item & 15) == 0, EDGL_ERR_SHAPE,
                 "edgl_segsum: operands must be 16-byte (bf16 rows: 8-byte) aligned");
    const int rc = segsum_plan_ofs(keys, n, nvalid, I, i0, i1, kofs, plan, st);
    if (rc) return rc;
    const Layout L = layout(n);
    int32_t* w = reinterpret_cast<int32_t*>(plan);
    p.hdr = w + L.hdr; p.perm = w + L.perm; p.seg_key = w + L.seg_key; p.seg_start = w + L.seg_start; p.seg_id = w + L.seg_id;
    p.part = reinterpret_cast<float*>(w + L.part); p.partb = reinterpret_cast<float*>(w + L.partb);
    const int rows_par = 256 / (p.C / 4);
    const dim3 grid((unsigned)((L.nsub + rows_par - 1) / rows_par));
    if (role == LABEL_ROWS) {      // (bf16 only: in f32 the scoring product pass contains the one-hot term and the entry point is a no-op)
        hipLaunchKernelGGL((segsum_walk_kernel<bf16, LABEL_ROWS>), grid, dim3(256), 0, st, p);
        hipLaunchKernelGGL(segsum_join_kernel<true>, grid, dim3(256), 0, st, p);
    } else if (role == CAND_ROWS) {
        if (dtype == EDGL_F32) hipLaunchKernelGGL((segsum_walk_kernel<float, CAND_ROWS>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((segsum_walk_kernel<bf16, CAND_ROWS>), grid, dim3(256), 0, st, p);
        hipLaunchKernelGGL(segsum_join_kernel<true>, grid, dim3(256), 0, st, p);
    } else if (role == ROWS) {
        if (dtype == EDGL_F32) hipLaunchKernelGGL((segsum_walk_kernel<float, ROWS>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((segsum_walk_kernel<bf16, ROWS>), grid, dim3(256), 0, st, p);
        hipLaunchKernelGGL(segsum_join_kernel<false>, grid, dim3(256), 0, st, p);
    } else {
        if (dtype == EDGL_F32) hipLaunchKernelGGL((segsum_walk_kernel<float, EMBED>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((segsum_walk_kernel<bf16, EMBED>), grid, dim3(256), 0, st, p);
        hipLaunchKernelGGL(segsum_join_kernel<false>, grid, dim3(256), 0, st, p);
    }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

int edgl_segsum_embed(const int64_t* ids, long rows, int C, int I, const void* dx0, const void* add1, const void* add2, float sq, float rate,
                      const uint64_t* rng, uint32_t stream_id, float* d_item, void* plan, int dtype, hipStream_t st) {
    EDGL_REQUIRE(plan, EDGL_ERR_NULL, "edgl_encode_bwd_add_det: null plan buffer");
    EDGL_REQUIRE(rows > 0 && rows < (1L << 30), EDGL_ERR_SHAPE, "edgl_encode_bwd_add_det: %ld rows unsupported", rows);
    segsum::SumP p{};
    p.C = C; p.src = dx0; p.add1 = add1; p.add2 = add2; p.sq = sq; p.rate = rate; p.rng = rng; p.stream_id = stream_id; p.d_item = d_item;
    return segsum_run(segsum::EMBED, ids, (int)rows, nullptr, I, 0, I, 0, p, plan, dtype, st);
}

int edgl_segsum_label(const void* rows, const int64_t* labels, const float* coef, const float* gscale, int R, int C, int I, int i0, int i1,
                      const int32_t* nvalid, float* d_table, float* d_bias, void* plan, int dtype, hipStream_t st) {
    EDGL_REQUIRE(plan, EDGL_ERR_NULL, "edgl_score_flash_label_term_det: null plan buffer");
    EDGL_REQUIRE(dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_score_flash_label_term_det: the ordered label sum takes bf16 rows (dtype %d)", dtype);
    segsum::SumP p{};
    p.C = C; p.src = rows; p.coef = coef; p.gscale = gscale; p.d_item = d_table; p.d_bias = d_bias;
    return segsum_run(segsum::LABEL_ROWS, labels, R, nvalid, I, i0, i1, 0, p, plan, dtype, st);
}

// the table gradient of the sampled-softmax loss (k_cand_ce.hip: edgl_cand_ce_table_det): keys int64 [n = R np1], one per list slot
// (0: a dead slot); d_table[key] += sum in plan order of dv[e] rows[e / np1], d_bias[key - 1] += sum dv[e]
int edgl_segsum_cand(const void* rows, const int64_t* keys, const float* dv, long n, int np1, int C, int I, float* d_table, float* d_bias,
                     void* plan, int dtype, hipStream_t st) {
    EDGL_REQUIRE(plan, EDGL_ERR_NULL, "edgl_cand_ce_table_det: null plan buffer");
    EDGL_REQUIRE(n > 0 && n < (1L << 31) && np1 >= 2, EDGL_ERR_SHAPE, "edgl_cand_ce_table_det: %ld list slots unsupported", n);
    segsum::SumP p{};
    p.C = C; p.src = rows; p.dv = dv; p.np1 = np1; p.d_item = d_table; p.d_bias = d_bias;
    return segsum_run(segsum::CAND_ROWS, keys, (int)n, nullptr, I, 0, I, 0, p, plan, dtype, st);
}

// d_table[key] = sum over the rows with that key, in plan order, of sq * drop(src[row * ld + c]) into the ZERO-FILLED d_table
// (k_data.hip: edgl_embed_pos_bwd_det, k_coding.hip: edgl_embedding_bwd_det).  keep_zero: key 0 is a table row like the others
// (a lookup without zero padding) — the keys are sorted one up and the sums land one row down.
int edgl_segsum_rows(const int64_t* ids, long rows, int C, int I, const void* src, long ld, float sq, float rate, const uint64_t* rng,
                     uint32_t stream_id, int keep_zero, float* d_table, void* plan, int dtype, hipStream_t st) {
    EDGL_REQUIRE(plan, EDGL_ERR_NULL, "edgl_segsum_rows: null plan buffer");
    EDGL_REQUIRE(rows > 0 && rows < (1L << 30) && I >= 1 && I < (1 << 30), EDGL_ERR_SHAPE, "edgl_segsum_rows: %ld rows / %d keys unsupported", rows, I);
    EDGL_REQUIRE(ld >= C && ld % 4 == 0, EDGL_ERR_SHAPE, "edgl_segsum_rows: bad leading dimension %ld (C=%d)", ld, C);
    segsum::SumP p{};
    p.C = C; p.src = src; p.ld = ld; p.sq = sq; p.rate = rate; p.rng = rng; p.stream_id = stream_id;
    const int k = keep_zero ? 1 : 0;
    p.d_item = d_table - (long)k * C;
    return segsum_run(segsum::ROWS, ids, (int)rows, nullptr, I + k, k, I + k, k, p, plan, dtype, st);
}
