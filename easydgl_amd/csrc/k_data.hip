// Batch construction on the device — MAUPostProcessor of the reference (src/dataloader.py:159-206) without its
// per-example Python py_func: `choice(seqslen - ignore_head, masklen) + ignore_head` (dataloader.py:34-36,183-186),
// token := MASK at the drawn positions, labels = original tokens there (:188-201); evaluation masks the last position
// (:166-179).  One workgroup (256 threads) per sequence.
#include "edgl_common.h"

namespace {

// M DISTINCT positions in [1, T) per row, uniformly at random (any M-subset equally likely, in random order — the
// semantics of np.random.choice(T-1, M, replace=False) + 1): every position gets a counter-based 32-bit key from
// (seed, step, stream, row, position); the M positions with the smallest (key, position) are taken, rank = output slot.
// The key and the rank are these two functions and nothing else: mask_random_kernel and the resident-split loader
// (loader_batch_kernel) both call them, so a batch row gets the same draws from either.
// keys: LDS [T] (entry 0 unused: position 0 is never drawn, ignore_head = 1); called by the whole workgroup, ends in a barrier.
__device__ __forceinline__ void mask_keys_fill(uint32_t* keys, const DropKey& dk, int b, int T) {
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        uint32_t h = ((uint32_t)(b * T + t) ^ dk.k0) * 0x9E3779B1u + dk.k1;
        h ^= h >> 15; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
        keys[t] = h;
    }
    __syncthreads();
}
// rank of position t (>= 1) among the positions [1, T) by (key, position): t is drawn iff rank < M, into output slot `rank`
__device__ __forceinline__ int mask_rank(const uint32_t* keys, int t, int T) {
    const uint32_t k = keys[t];
    int rank = 0;
    for (int j = 1; j < T; ++j) {
        const uint32_t kj = keys[j];
        rank += (kj < k) || (kj == k && j < t);
    }
    return rank;
}

__global__ __launch_bounds__(256) void mask_random_kernel(const int64_t* tokens, int T, int M, int64_t mask_id,
                                                          const uint64_t* rng, uint32_t stream_id, int64_t* masked,
                                                          int64_t* mpos, int64_t* labels) {
    extern __shared__ uint32_t keys[];   // [T]
    const int b = blockIdx.x;
    const int64_t* row = tokens + (long)b * T;
    const DropKey dk = make_dropkey(rng, stream_id, 0.f);
    mask_keys_fill(keys, dk, b, T);
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        int64_t tok = row[t];
        if (t >= 1) {
            const int rank = mask_rank(keys, t, T);
            if (rank < M) {
                mpos[(long)b * M + rank] = t;
                labels[(long)b * M + rank] = tok;
                tok = mask_id;
            }
        }
        masked[(long)b * T + t] = tok;
    }
}

// ---- Resident training split -> batch.  tokens int64 [N,T] / times f32 [N,T] stay on the device for the whole run;
//      one workgroup assembles output row b from source row perm[cursor + b] (perm NULL: cursor + b) in one of four forms:
//      MASK_RANDOM (mask_random_kernel's draws for batch row b), MASK_LAST (mask_last_kernel), REG_TRAIN / REG_EVAL
//      (train.regressive_batch).  state = uint64 {seed, step, cursor, reserved}: the first two words ARE the masker's rng_state.
//      Everything that changes from batch to batch is READ from `state`, so the launch is the same in every replay of a captured
//      graph; loader_advance_kernel moves step / cursor in a launch of its own behind it (other workgroups of the batch launch
//      still read them).  A source position outside [0, N) — the host cannot see a device cursor — or a permutation entry outside
//      [0, N) gives an EMPTY row: ids 0, times 0, labels 0, and (MASK_RANDOM) the M drawn positions, which are valid by themselves.
struct LoaderP {
    const int64_t* tokens; const float* times; const int32_t* perm; long N; int T, M, mode; int64_t mask_id;
    const uint64_t* state; uint32_t stream_id; int64_t* seqs_i; float* seqs_t; int64_t* mpos; int64_t* labels;
};
__global__ __launch_bounds__(256) void loader_batch_kernel(LoaderP p) {
    extern __shared__ uint32_t keys[];   // [T] (MASK_RANDOM only)
    const int b = blockIdx.x, T = p.T, M = p.M;
    const uint64_t cursor = p.state[2];
    long src = -1;
    if (cursor < (uint64_t)p.N && cursor + (uint64_t)b < (uint64_t)p.N) {
        const long pos = (long)cursor + b;
        src = p.perm ? (long)p.perm[pos] : pos;
        if (src < 0 || src >= p.N) src = -1;
    }
    const int64_t* row = src >= 0 ? p.tokens + src * T : nullptr;
    const float* trow = src >= 0 ? p.times + src * T : nullptr;
    for (int t = threadIdx.x; t < T; t += blockDim.x) p.seqs_t[(long)b * T + t] = trow ? trow[t] : 0.f;
    if (p.mode == EDGL_LOADER_MASK_RANDOM) {
        const DropKey dk = make_dropkey(p.state, p.stream_id, 0.f);
        mask_keys_fill(keys, dk, b, T);
        for (int t = threadIdx.x; t < T; t += blockDim.x) {
            int64_t tok = row ? row[t] : 0;
            if (t >= 1) {
                const int rank = mask_rank(keys, t, T);
                if (rank < M) {
                    p.mpos[(long)b * M + rank] = t;
                    p.labels[(long)b * M + rank] = tok;
                    if (row) tok = p.mask_id;
                }
            }
            p.seqs_i[(long)b * T + t] = tok;
        }
    } else if (p.mode == EDGL_LOADER_MASK_LAST) {
        for (int t = threadIdx.x; t < T; t += blockDim.x) {
            const int64_t tok = row ? row[t] : 0;
            p.labels[(long)b * T + t] = tok;
            p.seqs_i[(long)b * T + t] = (row && t == T - 1) ? p.mask_id : tok;
        }
    } else {   // REG_TRAIN / REG_EVAL: seqs_i = tokens[:-1]; labels = tokens[1:] (training) or the whole record (evaluation)
        const bool train = p.mode == EDGL_LOADER_REG_TRAIN;
        for (int t = threadIdx.x; t < T; t += blockDim.x) {
            const int64_t tok = row ? row[t] : 0;
            if (t < T - 1) p.seqs_i[(long)b * (T - 1) + t] = tok;
            if (!train) p.labels[(long)b * T + t] = tok;
            else if (t >= 1) p.labels[(long)b * (T - 1) + t - 1] = tok;
        }
    }
}
__global__ void loader_advance_kernel(uint64_t* state, int count) {
    state[1] += 1;
    state[2] += (uint64_t)count;
}

__global__ void mask_last_kernel(const int64_t* tokens, long n, int T, int64_t mask_id, int64_t* masked) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        masked[i] = (i % T == T - 1) ? mask_id : tokens[i];
}

// ---- CTSMA input encoding (CTSMA.py:48-58): X0 = dropout(concat(item_tab[ids] * sqrt(C), pos_tab[0..T))) [B,T,2C],
//      spans[t] = ts[t+1]/scale - ts[t]/scale (float32, no clipping), marks = mark_table[ids].  Thread = 4 channels.
struct EmbP {
    const int64_t* ids; const float* ts; const void* item_tab; const float* pos_tab; const uint8_t* mark_table;
    int B, T, C, E; float time_scale; float rate; const uint64_t* rng; uint32_t stream_id;
    void* x0; float* spans; uint8_t* marks;
    const void* dx0; float* d_item; float* d_pos;
    int srows;   // rows per block of the backward (<= ESROWS; fewer when ESROWS*C floats exceed the LDS)
    float sq;    // coding.py:62-63 sqrt(num_units): of the TRUE width for a channel-padded model (the _ct entry points)
};
template <typename T>
__global__ __launch_bounds__(256) void embed_pos_fwd_kernel(EmbP p) {
    const int cpr = p.C >> 2;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long row = gid / cpr;
    if (row >= (long)p.B * p.T) return;
    const int cv = (int)(gid % cpr), c0 = cv * 4, t = (int)(row % p.T);
    const long b = row / p.T;
    const int64_t id = p.ids[row];
    if (cv == 0 && p.spans) {
        const float* tr = p.ts + b * (p.T + 1) + t;
        p.spans[row] = tr[1] / p.time_scale - tr[0] / p.time_scale;   // CTSMA.py:50-51
        for (int e = 0; e < p.E; ++e) p.marks[row * p.E + e] = p.mark_table[id * p.E + e];   // :54
    }
    const int nseg = p.pos_tab ? 2 : 1;   // item | position (CTSMA) or the item embedding alone (TGAT.py:49, TiSASREC.py:52)
    const long ldo = (long)nseg * p.C;
    const float sq = p.sq;   // coding.py:62-63
    float v[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (id != 0) {   // coding.py:56-57 zero-padded row 0
        const Frag4<T> it = frag_ld<T>(reinterpret_cast<const T*>(p.item_tab) + id * p.C + c0);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[0][j] = to_f32(it.v[j]) * sq;
    }
    if (p.pos_tab) {
        const float4 pp = *reinterpret_cast<const float4*>(p.pos_tab + (long)t * p.C + c0);
        v[1][0] = pp.x; v[1][1] = pp.y; v[1][2] = pp.z; v[1][3] = pp.w;
    }
    const DropKey dk = make_dropkey(p.rng, p.stream_id, p.rate);
    T* out = reinterpret_cast<T*>(p.x0) + row * ldo;
    for (int s2 = 0; s2 < nseg; ++s2) {
        Frag4<T> o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o.v[j] = from_f32<T>(drop_apply(dk, (uint64_t)row * ldo + s2 * p.C + c0 + j, v[s2][j]));
        if constexpr (sizeof(T) == 4) *reinterpret_cast<uint4*>(out + s2 * p.C + c0) = *reinterpret_cast<uint4*>(&o);
        else *reinterpret_cast<uint2*>(out + s2 * p.C + c0) = *reinterpret_cast<uint2*>(&o);
    }
}
// d_item[id] += sqrt(C) * dropmask * dx[:, :C] (rows with id != 0), d_pos[t] += dropmask * dx[:, C:2C] into zero-filled tables.
// Item popularity is heavy-tailed, so raw global atomics serialise on the hot rows: a block takes ESROWS consecutive (b,t)
// rows, finds for every row the first row of the block with the same id (its leader), accumulates per leader in LDS and
// issues ONE global atomic per distinct id and channel (the scheme of k_encode.hip's encode_scatter_kernel).
constexpr int ESROWS = 128;
template <typename T>
__global__ __launch_bounds__(256) void embed_pos_bwd_kernel(EmbP p) {
    extern __shared__ float acc[];  // [ESROWS][C]
    __shared__ int s_id[ESROWS];
    __shared__ int s_lead[ESROWS];
    const int SR = p.srows;
    const long rows = (long)p.B * p.T, r0 = (long)blockIdx.x * SR;
    const int tid = threadIdx.x;
    if (tid < SR) s_id[tid] = (r0 + tid < rows) ? (int)p.ids[r0 + tid] : -1;
    for (int i = tid; i < SR * p.C; i += 256) acc[i] = 0.f;
    __syncthreads();
    if (tid < SR) {
        const int id = s_id[tid];
        int lead = tid;
        for (int j = 0; j < tid; ++j)
            if (s_id[j] == id) { lead = j; break; }
        s_lead[tid] = lead;
    }
    __syncthreads();
    const int cpr = p.C >> 2, rows_par = 256 / cpr;
    const int cv = tid % cpr, rl = tid / cpr, c0 = cv * 4;
    const DropKey dk = make_dropkey(p.rng, p.stream_id, p.rate);
    const float sq = p.sq;
    const long ldo = p.d_pos ? 2L * p.C : (long)p.C;
    if (tid < rows_par * cpr)
        for (int r = rl; r < SR; r += rows_par) {
            if (s_id[r] < 0) continue;   // past the end
            const long row = r0 + r;
            const T* d = reinterpret_cast<const T*>(p.dx0) + row * ldo;
            if (s_id[r] != 0) {          // coding.py:56-57: row 0 is a constant
                const Frag4<T> g0 = frag_ld<T>(d + c0);
                float* dst = acc + s_lead[r] * p.C + c0;
#pragma unroll
                for (int j = 0; j < 4; ++j) atomicAdd(dst + j, sq * drop_apply(dk, (uint64_t)row * ldo + c0 + j, to_f32(g0.v[j])));
            }
            if (p.d_pos) {
                const Frag4<T> g1 = frag_ld<T>(d + p.C + c0);
                const int t = (int)(row % p.T);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    atomicAdd(p.d_pos + (long)t * p.C + c0 + j, drop_apply(dk, (uint64_t)row * ldo + p.C + c0 + j, to_f32(g1.v[j])));
            }
        }
    __syncthreads();
    for (int i = tid; i < SR * p.C; i += 256) {
        const int r = i / p.C, c = i % p.C;
        if (s_lead[r] == r && s_id[r] > 0) atomicAdd(p.d_item + (long)s_id[r] * p.C + c, acc[i]);
    }
}

// Deterministic form of the position half: d_pos[t][c] = sum_b dropmask * dx[b, t, C + c] with b ascending.  One
// thread per (t, 4 channels) is the only writer of its elements; eight rows are in flight, the adds stay in order.
template <typename T>
__global__ __launch_bounds__(256) void embed_pos_dpos_kernel(EmbP p) {
    const int cpr = p.C >> 2;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)p.T * cpr) return;
    const int t = (int)(gid / cpr), c0 = (int)(gid % cpr) * 4;
    const DropKey dk = make_dropkey(p.rng, p.stream_id, p.rate);
    const long ldo = 2L * p.C;
    const T* d = reinterpret_cast<const T*>(p.dx0) + p.C + c0;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b0 = 0; b0 < p.B; b0 += 8) {
        Frag4<T> g[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) g[k] = frag_ld<T>(d + ((long)min(b0 + k, p.B - 1) * p.T + t) * ldo);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (b0 + k >= p.B) break;
            const long row = (long)(b0 + k) * p.T + t;
            float gv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) gv[j] = to_f32(g[k].v[j]);
            drop_apply4(dk, (uint64_t)row * ldo + p.C + c0, gv);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += gv[j];
        }
    }
    *reinterpret_cast<float4*>(p.d_pos + (long)t * p.C + c0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

}  // namespace

extern "C" int edgl_embed_pos_fwd_ct(const int64_t* ids, const float* ts, const void* item_tab, const float* pos_tab,
                                  const uint8_t* mark_table, int B, int T, int C, int E, float time_scale, float drop_rate,
                                  const uint64_t* rng_state, uint32_t stream_id, void* x0, float* spans, uint8_t* marks,
                                  int c_true, int dtype, void* stream) {
    EDGL_REQUIRE(ids && item_tab && x0, EDGL_ERR_NULL, "edgl_embed_pos_fwd: null pointer");
    EDGL_REQUIRE((spans != nullptr) == (marks != nullptr) && (!spans || (ts && mark_table)), EDGL_ERR_NULL,
                 "edgl_embed_pos_fwd: spans and marks go together and need ts and mark_table");
    EDGL_REQUIRE(B > 0 && T > 0 && C > 0 && C % 4 == 0 && (E >= 1 || !spans), EDGL_ERR_SHAPE, "edgl_embed_pos_fwd: bad shape B=%d T=%d C=%d E=%d", B, T, C, E);
    EDGL_REQUIRE(c_true >= 0 && c_true <= C, EDGL_ERR_SHAPE, "edgl_embed_pos_fwd: true width %d exceeds C=%d", c_true, C);
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_embed_pos_fwd: bad dtype %d", dtype);
    EDGL_REQUIRE(drop_rate == 0.f || rng_state, EDGL_ERR_NULL, "edgl_embed_pos_fwd: dropout without rng_state");
    EmbP p{ids, ts, item_tab, pos_tab, mark_table, B, T, C, E, time_scale, drop_rate, rng_state, stream_id, x0, spans, marks,
           nullptr, nullptr, nullptr, 0, sqrtf((float)(c_true > 0 ? c_true : C))};
    const long total = (long)B * T * (C / 4);
    dim3 grid((unsigned)((total + 255) / 256));
    if (dtype == EDGL_F32) hipLaunchKernelGGL((embed_pos_fwd_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((embed_pos_fwd_kernel<bf16>), grid, dim3(256), 0, (hipStream_t)stream, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_embed_pos_fwd(const int64_t* ids, const float* ts, const void* item_tab, const float* pos_tab,
                                  const uint8_t* mark_table, int B, int T, int C, int E, float time_scale, float drop_rate,
                                  const uint64_t* rng_state, uint32_t stream_id, void* x0, float* spans, uint8_t* marks,
                                  int dtype, void* stream) {
    return edgl_embed_pos_fwd_ct(ids, ts, item_tab, pos_tab, mark_table, B, T, C, E, time_scale, drop_rate, rng_state, stream_id, x0,
                                 spans, marks, 0, dtype, stream);
}

extern "C" int edgl_embed_pos_bwd_ct(const int64_t* ids, const void* dx0, int B, int T, int C, int I, float drop_rate,
                                  const uint64_t* rng_state, uint32_t stream_id, float* d_item, float* d_pos, int c_true,
                                  int dtype, void* stream) {
    EDGL_REQUIRE(ids && dx0 && d_item, EDGL_ERR_NULL, "edgl_embed_pos_bwd: null pointer");
    EDGL_REQUIRE(B > 0 && T > 0 && C > 0 && C % 4 == 0 && C / 4 <= 256 && I > 1,
                 EDGL_ERR_SHAPE, "edgl_embed_pos_bwd: bad shape B=%d T=%d C=%d", B, T, C);
    EDGL_REQUIRE(c_true >= 0 && c_true <= C, EDGL_ERR_SHAPE, "edgl_embed_pos_bwd: true width %d exceeds C=%d", c_true, C);
    int srows = ESROWS;
    while (srows > 8 && (size_t)srows * C * sizeof(float) > 150 * 1024) srows >>= 1;   // C = 512: 64 rows per block
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_embed_pos_bwd: bad dtype %d", dtype);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(d_item, 0, (size_t)I * C * sizeof(float), st) != hipSuccess ||
        (d_pos && hipMemsetAsync(d_pos, 0, (size_t)T * C * sizeof(float), st) != hipSuccess)) {
        edgl_set_error("edgl_embed_pos_bwd: memset failed");
        return EDGL_ERR_LAUNCH;
    }
    EmbP p{ids, nullptr, nullptr, nullptr, nullptr, B, T, C, 0, 1.f, drop_rate, rng_state, stream_id, nullptr, nullptr, nullptr,
           dx0, d_item, d_pos, srows, sqrtf((float)(c_true > 0 ? c_true : C))};
    const size_t smem = (size_t)srows * C * sizeof(float);
    dim3 grid((unsigned)(((long)B * T + srows - 1) / srows));
    if (dtype == EDGL_F32) {
        EDGL_LDS_LIMIT(embed_pos_bwd_kernel<float>, smem, "edgl_embed_pos_bwd");
        hipLaunchKernelGGL((embed_pos_bwd_kernel<float>), grid, dim3(256), smem, st, p);
    } else {
        EDGL_LDS_LIMIT(embed_pos_bwd_kernel<bf16>, smem, "edgl_embed_pos_bwd");
        hipLaunchKernelGGL((embed_pos_bwd_kernel<bf16>), grid, dim3(256), smem, st, p);
    }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

// edgl_embed_pos_bwd_ct without f32 atomics: the item rows as ordered sums over a plan of ids that this call builds in `plan`
// (k_segsum.hip; key 0 is cut off), the position rows summed over b in order.  Same masks, same scale, every sum in an order
// that follows from ids and the shape alone.
extern "C" int edgl_embed_pos_bwd_det(const int64_t* ids, const void* dx0, int B, int T, int C, int I, float drop_rate,
                                      const uint64_t* rng_state, uint32_t stream_id, float* d_item, float* d_pos, int c_true,
                                      void* plan, int dtype, void* stream) {
    EDGL_REQUIRE(ids && dx0 && d_item && plan, EDGL_ERR_NULL, "edgl_embed_pos_bwd_det: null pointer");
    EDGL_REQUIRE(B > 0 && T > 0 && C > 0 && C % 4 == 0 && C <= 512 && I > 1 && (long)B * T < (1L << 30),
                 EDGL_ERR_SHAPE, "edgl_embed_pos_bwd_det: bad shape B=%d T=%d C=%d (a multiple of 4 up to 512) I=%d", B, T, C, I);
    EDGL_REQUIRE(c_true >= 0 && c_true <= C, EDGL_ERR_SHAPE, "edgl_embed_pos_bwd_det: true width %d exceeds C=%d", c_true, C);
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "edgl_embed_pos_bwd_det: bad dtype %d", dtype);
    EDGL_REQUIRE(((uintptr_t)plan & 15) == 0 && ((uintptr_t)d_pos & 15) == 0, EDGL_ERR_SHAPE,
                 "edgl_embed_pos_bwd_det: plan and d_pos must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(d_item, 0, (size_t)I * C * sizeof(float), st) != hipSuccess) {
        edgl_set_error("edgl_embed_pos_bwd_det: memset failed");
        return EDGL_ERR_LAUNCH;
    }
    const float sq = sqrtf((float)(c_true > 0 ? c_true : C));
    const long ldo = d_pos ? 2L * C : (long)C;
    if (int rc = edgl_segsum_rows(ids, (long)B * T, C, I, dx0, ldo, sq, drop_rate, rng_state, stream_id, 0, d_item, plan, dtype, st))
        return rc;
    if (!d_pos) return EDGL_OK;
    EmbP p{ids, nullptr, nullptr, nullptr, nullptr, B, T, C, 0, 1.f, drop_rate, rng_state, stream_id, nullptr, nullptr, nullptr,
           dx0, d_item, d_pos, 0, sq};
    const dim3 grid((unsigned)(((long)T * (C / 4) + 255) / 256));
    if (dtype == EDGL_F32) hipLaunchKernelGGL((embed_pos_dpos_kernel<float>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((embed_pos_dpos_kernel<bf16>), grid, dim3(256), 0, st, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_embed_pos_bwd(const int64_t* ids, const void* dx0, int B, int T, int C, int I, float drop_rate,
                                  const uint64_t* rng_state, uint32_t stream_id, float* d_item, float* d_pos, int dtype,
                                  void* stream) {
    return edgl_embed_pos_bwd_ct(ids, dx0, B, T, C, I, drop_rate, rng_state, stream_id, d_item, d_pos, 0, dtype, stream);
}

extern "C" int edgl_mask_random(const int64_t* tokens, int B, int T, int M, int64_t mask_id, const uint64_t* rng_state,
                                uint32_t stream_id, int64_t* masked_tokens, int64_t* masked_pos, int64_t* labels,
                                void* stream) {
    EDGL_REQUIRE(tokens && rng_state && masked_tokens && masked_pos && labels, EDGL_ERR_NULL, "edgl_mask_random: null pointer");
    EDGL_REQUIRE(B > 0 && T > 1 && M >= 1 && M <= T - 1, EDGL_ERR_SHAPE,
                 "edgl_mask_random: need 1 <= masklen <= T-1 (B=%d T=%d M=%d)", B, T, M);
    EDGL_REQUIRE((size_t)T * sizeof(uint32_t) <= 64 * 1024, EDGL_ERR_SHAPE, "edgl_mask_random: T=%d too long", T);
    hipLaunchKernelGGL(mask_random_kernel, dim3(B), dim3(256), (size_t)T * sizeof(uint32_t), (hipStream_t)stream, tokens, T,
                       M, mask_id, rng_state, stream_id, masked_tokens, masked_pos, labels);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_mask_last(const int64_t* tokens, int B, int T, int64_t mask_id, int64_t* masked_tokens, void* stream) {
    EDGL_REQUIRE(tokens && masked_tokens, EDGL_ERR_NULL, "edgl_mask_last: null pointer");
    EDGL_REQUIRE(B > 0 && T > 0, EDGL_ERR_SHAPE, "edgl_mask_last: bad shape B=%d T=%d", B, T);
    const long n = (long)B * T;
    hipLaunchKernelGGL(mask_last_kernel, dim3((unsigned)std::min<long>((n + 255) / 256, 2048)), dim3(256), 0,
                       (hipStream_t)stream, tokens, n, T, mask_id, masked_tokens);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_loader_state_words(void) { return 4; }

extern "C" int edgl_loader_batch(const int64_t* tokens, const float* times, const int32_t* perm, long N, int T, int count, int mode,
                                 int M, int64_t mask_id, const uint64_t* state, uint32_t stream_id, int64_t* seqs_i, float* seqs_t,
                                 int64_t* masked_pos, int64_t* labels, void* stream) {
    EDGL_REQUIRE(mode >= EDGL_LOADER_MASK_RANDOM && mode <= EDGL_LOADER_REG_EVAL, EDGL_ERR_SHAPE, "edgl_loader_batch: unknown mode %d", mode);
    EDGL_REQUIRE(tokens && times && state && seqs_i && seqs_t && labels, EDGL_ERR_NULL, "edgl_loader_batch: null pointer");
    EDGL_REQUIRE(mode != EDGL_LOADER_MASK_RANDOM || masked_pos, EDGL_ERR_NULL, "edgl_loader_batch: null pointer (masked_pos)");
    EDGL_REQUIRE(N >= 1 && N <= 0x7fffffffL, EDGL_ERR_SHAPE, "edgl_loader_batch: bad split size N=%ld", N);
    EDGL_REQUIRE(T >= 2, EDGL_ERR_SHAPE, "edgl_loader_batch: need T >= 2 (T=%d)", T);
    EDGL_REQUIRE(count >= 1, EDGL_ERR_SHAPE, "edgl_loader_batch: need count >= 1 (count=%d)", count);
    EDGL_REQUIRE(mode != EDGL_LOADER_MASK_RANDOM || (M >= 1 && M <= T - 1), EDGL_ERR_SHAPE,
                 "edgl_loader_batch: need 1 <= masklen <= T-1 (T=%d masklen=%d)", T, M);
    EDGL_REQUIRE((size_t)T * sizeof(uint32_t) <= 64 * 1024, EDGL_ERR_SHAPE, "edgl_loader_batch: T=%d too long", T);
    LoaderP p{tokens, times, perm, N, T, M, mode, mask_id, state, stream_id, seqs_i, seqs_t, masked_pos, labels};
    const size_t smem = mode == EDGL_LOADER_MASK_RANDOM ? (size_t)T * sizeof(uint32_t) : 0;
    hipLaunchKernelGGL(loader_batch_kernel, dim3(count), dim3(256), smem, (hipStream_t)stream, p);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

extern "C" int edgl_loader_advance(uint64_t* state, int count, void* stream) {
    EDGL_REQUIRE(state, EDGL_ERR_NULL, "edgl_loader_advance: null pointer");
    EDGL_REQUIRE(count >= 1, EDGL_ERR_SHAPE, "edgl_loader_advance: need count >= 1 (count=%d)", count);
    hipLaunchKernelGGL(loader_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, count);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
