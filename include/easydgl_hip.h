/*
 * libeasydgl_hip.so — C ABI of the MI355X (gfx950) kernels for EasyDGL's temporal-point-process
 * self-modulating-attention hot path.
 *
 * The reference (cchao0116/EasyDGL) has NO FFI: its hot path is a TensorFlow-1.x graph.  Each entry
 * point below therefore replaces a *group of TF ops*; the comment on each cites the reference lines
 * (paths relative to the reference repo root) whose arithmetic it reproduces.  INTEGRATION.md shows
 * the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the name ends in _host; the caller owns all buffers;
 *    kernels never allocate, never synchronise, and launch on `stream` (a hipStream_t);
 *  - returns 0 on success, a negative EDGL_ERR_* otherwise (edgl_last_error() gives the text);
 *  - activations / GEMM operands are `dtype` (EDGL_F32 exact-f32 MFMA path, or EDGL_BF16 with f32
 *    accumulation); statistics, losses, gradients of parameters and optimizer state are always f32;
 *  - tensors are dense row-major; B = batch, T = positions (= seqslen+1), C = num_units,
 *    H = num_heads, dh = C/H, E = num_events, I = item-table rows (= num_items+1), M = masklen;
 *  - head-major stacking b' = head*B + b for every [H*B, ...] tensor (temporal.py:413-416);
 *  - dropout masks are a pure function of (rng_state[0]=seed, rng_state[1]=step, stream_id, element
 *    index); backward kernels regenerate them.  rng_state may be NULL when the rate is 0.
 */
#ifndef EASYDGL_HIP_H
#define EASYDGL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { EDGL_F32 = 0, EDGL_BF16 = 1 } edgl_dtype;

enum {
    EDGL_OK = 0,
    EDGL_ERR_SHAPE = -1,       /* unsupported / inconsistent shape */
    EDGL_ERR_DTYPE = -2,
    EDGL_ERR_LAUNCH = -3,      /* hipGetLastError() != hipSuccess after a launch */
    EDGL_ERR_NULL = -4,
    EDGL_ERR_WORKSPACE = -5
};

/* GEMM epilogue flags */
enum {
    EDGL_EPI_BIAS = 1,        /* + bias[n]                                   */
    EDGL_EPI_GELU = 2,        /* erf-GELU (EasyDGL.py:19-32)                 */
    EDGL_EPI_SAVE_PRE = 4,    /* aux[m,n] = pre-activation (dtype)           */
    EDGL_EPI_MUL_DGELU = 8,   /* *= gelu'(aux[m,n])                          */
    EDGL_EPI_ACCUM = 16,      /* C += result                                 */
    EDGL_EPI_OUT_F32 = 32,    /* C is f32 regardless of dtype                */
    EDGL_EPI_RELU = 64        /* max(x, 0) (FeedForward inner layer, Base.py:73) */
};

const char* edgl_last_error(void);
int edgl_version(void);

/* Profiling hook (measurement only): the NEXT launch of kernel (group) `kernel_id` on the calling thread records the two
 * hipEvent_t handles immediately before / after it on its launch stream, then the slot clears.
 *   SCORE_BWD_ROWS : the row-side scoring pass (K5);  BIMAU_BWD : sweep 2 of the BiMAU backward alone;
 *   BIMAU_FWD      : every kernel of one edgl_bimau_fwd call (K3 forward: temporal.py:404-452 + 281-315);
 *   BIMAU_BWD_ALL  : the three backward passes X, Y, Z of one edgl_bimau_bwd call (without the parameter-partial reductions) */
enum { EDGL_KERNEL_SCORE_BWD_ROWS = 0, EDGL_KERNEL_BIMAU_BWD = 1, EDGL_KERNEL_BIMAU_FWD = 2, EDGL_KERNEL_BIMAU_BWD_ALL = 3 };
int edgl_profile_next(int kernel_id, void* ev_start, void* ev_stop);

/* ---- dropout RNG state ----------------------------------------------------------------------- */
/* rng_state[1] += 1 on the device (one launch per training step, graph-capturable). */
int edgl_rng_advance(uint64_t* rng_state, void* stream);

/* ---- K0: batch construction — MAUPostProcessor, dataloader.py:159-206 (choice: :34-36) -----------
 * tokens int64 [B,T] (T = seqslen + 1).  edgl_mask_random: per row `masklen` = M DISTINCT positions
 * drawn uniformly from [1, T) (ignore_head = 1, dataloader.py:183-186) by a counter-based generator
 * keyed on (rng_state, stream_id, row); masked_tokens = tokens with MASK = mask_id at those positions
 * (:188-193), masked_pos int64 [B,M], labels int64 [B,M] = the original tokens there (:194-201).
 * edgl_mask_last: evaluation batches — position T-1 := MASK (:166-179); labels are the input tokens. */
int edgl_mask_random(const int64_t* tokens, int B, int T, int M, int64_t mask_id, const uint64_t* rng_state,
                     uint32_t stream_id, int64_t* masked_tokens, int64_t* masked_pos, int64_t* labels,
                     void* stream);
int edgl_mask_last(const int64_t* tokens, int B, int T, int64_t mask_id, int64_t* masked_tokens, void* stream);

/* ---- K0b: batches from a split that lives on the device ---------------------------
 * tokens int64 [N,T] / times f32 [N,T]: a whole split, uploaded once.  perm int32 [N] or NULL (identity): the epoch's order.
 * state: device uint64[edgl_loader_state_words()] = { seed, step, cursor, reserved } — words 0..1 are the rng_state of
 * edgl_mask_random.  edgl_loader_batch writes `count` rows (one workgroup each); output row b takes source row
 * perm[cursor + b].  cursor and step are READ FROM THE DEVICE, never passed by value: the same launch serves every replay of a
 * captured graph.  edgl_loader_advance (one thread: step += 1, cursor += count) follows it in stream order; the batch launch
 * never advances them itself (its other workgroups still read them).
 *   EDGL_LOADER_MASK_RANDOM  seqs_i [count,T], seqs_t [count,T], masked_pos [count,M], labels [count,M] — bit for bit what
 *                            edgl_mask_random(tokens[perm[cursor..]], ..., state, stream_id) gives: the draws of BATCH row b
 *   EDGL_LOADER_MASK_LAST    seqs_i [count,T] with position T-1 := mask_id, seqs_t, labels [count,T] = the record (masked_pos unused)
 *   EDGL_LOADER_REG_TRAIN    seqs_i [count,T-1] = tokens[:, :-1], seqs_t [count,T], labels [count,T-1] = tokens[:, 1:]
 *   EDGL_LOADER_REG_EVAL     seqs_i [count,T-1] = tokens[:, :-1], seqs_t [count,T], labels [count,T] = the record
 * A row whose source position cursor + b is >= N (or whose permutation entry is outside [0,N)) comes out EMPTY: ids 0, times 0,
 * labels 0, masked_pos the M distinct drawn positions in [1,T) — the host cannot check a device-side cursor, the kernel does.
 * Refused before any launch: null pointers, T < 2, masklen < 1 or > T-1 (MASK_RANDOM), count < 1, N < 1, an unknown mode. */
enum { EDGL_LOADER_MASK_RANDOM = 0, EDGL_LOADER_MASK_LAST = 1, EDGL_LOADER_REG_TRAIN = 2, EDGL_LOADER_REG_EVAL = 3 };
int edgl_loader_state_words(void);
int edgl_loader_batch(const int64_t* tokens, const float* times, const int32_t* perm, long N, int T, int count, int mode,
                      int M, int64_t mask_id, const uint64_t* state, uint32_t stream_id, int64_t* seqs_i, float* seqs_t,
                      int64_t* masked_pos, int64_t* labels, void* stream);
int edgl_loader_advance(uint64_t* state, int count, void* stream);

/* ---- K1: input encoding — EasyDGL.py:70-95, coding.py:60-64,76-79,137-149 ---------------------
 * x0[b,t,:]   = [ item_tab[id]*sqrt(C) + sincos(ts/time_scale) | pos_tab[t] | nmarks*mark_emb[1] ]
 *               followed by hidden dropout (EasyDGL.py:92);
 * spans[b,t]  = clip(ts'[t]-ts'[t-1],0,100), spans[b,0]=spans[b,1] with ts' = ts/time_scale (:73-74);
 * marks[b,t,:] = mark_table[id (MASK->0)] (:76-77); item row 0 and mark_emb row 0 act as zeros
 *               (coding.py:56-57).
 * item_tab is `dtype` (master f32 or its bf16 shadow); pos_tab / mark_emb are f32; mark_table holds
 * 0/1 bytes [>= num_items, E]; tscale f32 [C/2] = float32(10000^(2j/C)) (coding.py:134-135, computed on
 * the host exactly as the reference does). */
int edgl_encode_fwd(const int64_t* ids, const float* ts, const void* item_tab, const float* pos_tab,
                    const float* mark_emb, const uint8_t* mark_table, const float* tscale, int B, int T, int C,
                    int E, int I, int64_t mask_id, float time_scale, float drop_rate,
                    const uint64_t* rng_state, uint32_t stream_id, void* x0, float* spans, uint8_t* marks,
                    int dtype, void* stream);

/* Backward of K1 (SURVEY Appendix C "Embedding side"): d_item[id] += sqrt(C)*dX0[:, :C] for id != 0
 * (f32 atomics into d_item, which must be pre-initialised by the caller), d_pos[t] and d_mark_emb[1]
 * are written via per-block partials reduced deterministically (d_mark_emb [E,C]: only row 1 is
 * non-zero).  workspace: edgl_encode_bwd_workspace(B,T,C) floats. */
long edgl_encode_bwd_workspace(int B, int T, int C);
int edgl_encode_bwd(const int64_t* ids, const uint8_t* marks, const void* dx0, int B, int T, int C, int E,
                    int I, float drop_rate, const uint64_t* rng_state, uint32_t stream_id, float* d_item,
                    float* d_pos, float* d_mark_emb, float* workspace, int dtype, void* stream);
/* The same with two optional [B*T, C] terms (activation dtype; both or neither) added in f32 to the item section dX0[:, :C]
 * before the scatter: the residual branches of the first block, which the training engine would otherwise add with a
 * separate pass over dX0 (edgl_add_cols). */
int edgl_encode_bwd_add(const int64_t* ids, const uint8_t* marks, const void* dx0, const void* add1, const void* add2, int B,
                        int T, int C, int E, int I, float drop_rate, const uint64_t* rng_state, uint32_t stream_id,
                        float* d_item, float* d_pos, float* d_mark_emb, float* workspace, int dtype, void* stream);
/* Channel-padded models (a model width whose head dim the attention kernels do not tile — the reference's default --num_units 50
 * --num_heads 1, main.py:35-37 — runs at the next supported head dim with zero-padded channels; channel c of a C-wide section is
 * real iff c % dh_pad < dh_true): edgl_encode_fwd / edgl_encode_bwd_add with coding.py:62-63's sqrt(C) taken of the TRUE width and
 * the time code of the padded channels zeroed (dh_pad = dh_true = 0 / c_true = 0: no padding). */
int edgl_encode_fwd_ct(const int64_t* ids, const float* ts, const void* item_tab, const float* pos_tab, const float* mark_emb,
                       const uint8_t* mark_table, const float* tscale, int B, int T, int C, int E, int I, int64_t mask_id,
                       float time_scale, float drop_rate, const uint64_t* rng_state, uint32_t stream_id, void* x0, float* spans,
                       uint8_t* marks, int dh_pad, int dh_true, int dtype, void* stream);
/* edgl_encode_fwd_ct with the batch preparation of a training step as the first workgroups of its launch (EasyDGL.py:70-95 encoder;
 * EasyDGL.py:177-185: which rows the loss weights — edgl_compact_scan_labels(labels [B * M]); EasyDGL.py:157-175 / temporal.py:317-333:
 * the slots of the TPP term — edgl_tpp_prep(masked_pos, labels, ts, mark_table) into tpp_desc, NULL: none).  Same results as the
 * three calls; what it writes is ordered in front of the stream's later kernels without a second stream and its join. */
int edgl_encode_fwd_prep(const int64_t* ids, const float* ts, const void* item_tab, const float* pos_tab, const float* mark_emb,
                         const uint8_t* mark_table, const float* tscale, int B, int T, int C, int E, int I, int64_t mask_id,
                         float time_scale, float drop_rate, const uint64_t* rng_state, uint32_t stream_id, void* x0, float* spans,
                         uint8_t* marks, int dh_pad, int dh_true, const int64_t* labels, int M, int32_t* perm, int32_t* inv,
                         int32_t* nvalid, int64_t* labels_c, const int64_t* masked_pos, void* tpp_desc, int dtype, void* stream);
int edgl_encode_bwd_add_ct(const int64_t* ids, const uint8_t* marks, const void* dx0, const void* add1, const void* add2, int B,
                           int T, int C, int E, int I, float drop_rate, const uint64_t* rng_state, uint32_t stream_id,
                           float* d_item, float* d_pos, float* d_mark_emb, float* workspace, int c_true, int dtype, void* stream);
/* edgl_encode_bwd_add_ct that also applies the one-hot term of the tied table's scoring gradient which
 * edgl_score_flash_bwd_ex(defer_label_term = 1) left out (EasyDGL.py:177-185: dl = coef (softmax - onehot)):
 * d_item[label[r]] -= coef[r] rows[r], d_bias[label[r] - 1] -= coef[r] over the first min(lab_R, *lab_nvalid) compacted rows — as
 * extra blocks of the embedding scatter's launch (the same segmented sum over equal ids), instead of the launch and stream fork
 * of edgl_score_flash_label_term.  edgl_encode_bwd_label_fused(C, dtype) says whether this shape has the fused form. */
int edgl_encode_bwd_label_fused(int C, int dtype);
int edgl_encode_bwd_add_label(const int64_t* ids, const uint8_t* marks, const void* dx0, const void* add1, const void* add2, int B,
                              int T, int C, int E, int I, float drop_rate, const uint64_t* rng_state, uint32_t stream_id,
                              float* d_item, float* d_pos, float* d_mark_emb, float* workspace, int c_true, const void* lab_rows,
                              const int64_t* lab_ids, const float* lab_coef, const int32_t* lab_nvalid, int lab_R, float* d_bias,
                              int dtype, void* stream);
/* The QKVT dX GEMM of the first block with edgl_encode_bwd_add_label as its epilogue (csrc/k_gemm2.hip: dx_encode_kernel; DESIGN
 * rule 78): dX0[B*T, 3C] = dqkvt[B*T, 4C] . W[3C, 4C]^T — edgl_gemm's dX call (A = dqkvt with row stride lda, Bm = W k-contiguous
 * with row stride ldb) — is consumed tile by tile where it is produced and never written: a row tile holds 128 samples at one
 * position, so d_pos / d_mark_emb are column sums inside the tile and the item section of the tile is the row image of the scatter.
 * The label job and the thread's queued reductions (edgl_reduce_ride) are extra workgroups of the same launch; the call's own two
 * reductions follow in one launch (deferred mode without riding: queued).  dx0_out (NULL in the engine): when given, [B*T, 3C]
 * receives dX0, bit-identical to edgl_gemm.  The other arguments are those of edgl_encode_bwd_add_label, same workspace.
 * edgl_dx_encode_supported(B, T, C, dtype) = 1 for EDGL_BF16, C = 128, B <= 2048 and at most B / 8 padded samples in the last
 * chunk of 128 (B = 120, 128, 250, 512: yes; 4, 129: no), else 0: the unfused pair remains the path for everything else. */
int edgl_dx_encode_supported(int B, int T, int C, int dtype);
int edgl_dx_encode_bwd_label(const void* dqkvt, const void* W, int lda, int ldb, void* dx0_out, const int64_t* ids,
                             const uint8_t* marks, const void* add1, const void* add2, int B, int T, int C, int E, int I,
                             float drop_rate, const uint64_t* rng_state, uint32_t stream_id, float* d_item, float* d_pos,
                             float* d_mark_emb, float* workspace, int c_true, const void* lab_rows, const int64_t* lab_ids,
                             const float* lab_coef, const int32_t* lab_nvalid, int lab_R, float* d_bias, int dtype, void* stream);

/* ---- Deterministic item-table scatter (csrc/k_segsum.hip) — coding.py:60-64, EasyDGL.py:177-185 ---------------------
 * The f32 atomics of the embedding scatter and of the one-hot term of the scoring gradient make the item-table gradient differ in
 * its last bits from run to run.  The _det entry points below compute the same sums without atomics: a stable radix sort of the
 * row indices by item id (the plan), then one ordered f32 sum per id, added to its table row with plain loads and stores (one writer
 * per row per call).  The summation order is a function of the keys alone; two calls on the same inputs give the same bits.
 *
 * A plan is built in a caller-provided device buffer of edgl_segsum_plan_bytes bytes (16-byte aligned; sized for n rows at any
 * C <= 512, scratch of the sort and of the sums included).  Its front, in 32-bit words with n4 = n rounded up to a multiple of 4:
 *   [0] nseg   [1] kept rows   [4, 4 + n) perm   [4 + n4, ..) seg_key   [4 + 2 n4, ..) seg_start (nseg + 1 entries)
 * keys int64 [n]; entries with key 0, entries at or behind min(n, *nvalid) (nvalid may be NULL) and keys outside [i0, i1) are
 * dropped.  perm holds the kept row indices sorted by key, ascending rows inside one key; seg_key are the distinct keys in
 * ascending order, seg_start[s] the first position of segment s in perm, seg_start[nseg] = kept rows.  The sort runs
 * edgl_segsum_passes = ceil(bits(I - 1) / 8) passes of 8-bit digits.  No host read-back anywhere: every call can be captured in
 * a HIP graph.  The two size queries are host functions (no GPU needed); they return -1 for bad arguments. */
int edgl_segsum_passes(int I);
long edgl_segsum_plan_bytes(int n, int I);
int edgl_segsum_plan(const int64_t* keys, int n, const int32_t* nvalid, int I, int i0, int i1, void* plan, void* stream);
/* edgl_encode_bwd_add_ct with the item scatter through a plan over ids (built by the call in `plan`, edgl_segsum_plan_bytes of
 * (B * T, I) bytes): the position / mark stage and its reductions are the same launches, d_item += the ordered sums.  The
 * three-way sum dX0 + add1 + add2 is kept in f32.  C % 4 == 0, C <= 512. */
int edgl_encode_bwd_add_det(const int64_t* ids, const uint8_t* marks, const void* dx0, const void* add1, const void* add2, int B,
                            int T, int C, int E, int I, float drop_rate, const uint64_t* rng_state, uint32_t stream_id,
                            float* d_item, float* d_pos, float* d_mark_emb, float* workspace, int c_true, void* plan, int dtype,
                            void* stream);

/* ---- K1b: CTSMA input encoding — CTSMA.py:48-58, coding.py:60-79 ----------------------------------
 * ids int64 [B,T] (tokens[:-1]), ts f32 [B,T+1] raw seconds.  x0 [B,T,2C] `dtype` =
 * dropout(concat(item_tab[ids] * sqrt(C) (row 0 reads as zeros), pos_tab[0..T))) (PositionCoding.__call__
 * concatenates); spans f32 [B,T] = ts[t+1]/time_scale - ts[t]/time_scale (no clipping); marks u8 [B,T,E] =
 * mark_table[ids].  bwd: d_item f32 [I,C] and d_pos f32 [T,C] are overwritten.
 * pos_tab == NULL (d_pos == NULL in the backward): x0 is [B,T,C], the item embedding alone (TGAT.py:49-56,
 * TiSASREC.py:52-65); spans and marks may be NULL together (then ts and mark_table are not read). */
int edgl_embed_pos_fwd(const int64_t* ids, const float* ts, const void* item_tab, const float* pos_tab,
                       const uint8_t* mark_table, int B, int T, int C, int E, float time_scale, float drop_rate,
                       const uint64_t* rng_state, uint32_t stream_id, void* x0, float* spans, uint8_t* marks,
                       int dtype, void* stream);
int edgl_embed_pos_bwd(const int64_t* ids, const void* dx0, int B, int T, int C, int I, float drop_rate,
                       const uint64_t* rng_state, uint32_t stream_id, float* d_item, float* d_pos, int dtype,
                       void* stream);
/* The same for a channel-padded model (TGAT / TiSASRec / CTSMA at a head dim the attention kernels do not tile, e.g. the
 * reference's default --num_units 50, main.py:35): c_true (0: = C) is the TRUE model width whose square root scales the item
 * embedding (coding.py:62-63); the padded channels of the tables are zero. */
int edgl_embed_pos_fwd_ct(const int64_t* ids, const float* ts, const void* item_tab, const float* pos_tab,
                          const uint8_t* mark_table, int B, int T, int C, int E, float time_scale, float drop_rate,
                          const uint64_t* rng_state, uint32_t stream_id, void* x0, float* spans, uint8_t* marks,
                          int c_true, int dtype, void* stream);
int edgl_embed_pos_bwd_ct(const int64_t* ids, const void* dx0, int B, int T, int C, int I, float drop_rate,
                          const uint64_t* rng_state, uint32_t stream_id, float* d_item, float* d_pos, int c_true,
                          int dtype, void* stream);
/* edgl_embed_pos_bwd_ct without f32 atomics: the item rows are summed over a plan of ids that the call builds in
 * `plan` (edgl_segsum_plan_bytes of (B * T, I) bytes, 16-byte aligned; key 0 is cut off), d_pos[t] is the sum over b in
 * ascending order.  Same masks and scale; d_item and d_pos are overwritten; one writer per element.  C % 4 == 0, C <= 512. */
int edgl_embed_pos_bwd_det(const int64_t* ids, const void* dx0, int B, int T, int C, int I, float drop_rate,
                           const uint64_t* rng_state, uint32_t stream_id, float* d_item, float* d_pos, int c_true, void* plan,
                           int dtype, void* stream);

/* ---- K2/K4: dense layers — tf.layers.dense (temporal.py:409, EasyDGL.py:113,120,125,138) ------
 * C[M,N] = epilogue( sum_k A(m,k) * B(k,n) ).
 * a_kc != 0: A stored [M, lda] with k contiguous; else stored [K, lda] with m contiguous.
 * b_kc != 0: B stored [N, ldb] with k contiguous; else stored [K, ldb] with n contiguous.
 * A, B are `dtype`; C is `dtype` unless EDGL_EPI_OUT_F32.  bias f32[N].  aux is `dtype` [M,ldc].
 * splitk > 1 needs workspace >= splitk*M*N floats (partials reduced by a second launch). */
int edgl_gemm(const void* A, const void* Bm, void* Cm, int M, int N, int K, int lda, int ldb, int ldc,
              int a_kc, int b_kc, const float* bias, void* aux, int epi_flags, int splitk, float* workspace,
              int dtype, void* stream);

/* Weight / bias gradients of a dense layer: dW[Kf,N] (+)= X[R,Kf]^T . dY[R,N] (f32), and if dbias != NULL
 * dbias[N] (+)= colsum(dY).  workspace >= edgl_gemm_dw_workspace floats; per-split partials are reduced in a
 * fixed order. */
long edgl_gemm_dw_workspace(int R, int Kf, int N, int dtype);
int edgl_gemm_dw(const void* X, const void* dY, float* dW, float* dbias, int R, int Kf, int N, int ldx, int ldy,
                 int accumulate, float* workspace, int dtype, void* stream);
/* Grouped mode of edgl_gemm_dw (bf16): after edgl_gemm_dw_defer(1, stream) the calls are queued on the calling host thread;
 * edgl_gemm_dw_defer(0, stream) runs all of them as ONE launch (up to 8 products, row splits of similar length) followed by
 * their slab reductions.  Operands and workspaces of queued calls must stay untouched until then.  on < 0: drop the queue
 * without launching (error exit). */
int edgl_gemm_dw_defer(int on, void* stream);
/* edgl_gemm_dw_ride(1), in grouped mode: the next edgl_dx_encode_bwd_label call of this thread takes the queued products along as
 * workgroups of ITS launch (DESIGN rule 79) — the two are independent and each runs far below the chip's limits by itself — and issues
 * their slab reductions with its own two, behind that launch; a following edgl_gemm_dw_defer(0) finds the queue empty.  Same dW / db
 * bits as the grouped launch.  A queue that cannot ride (an accumulating product, outputs the vector-form reduction does not take,
 * more reduction jobs than one list holds) is run in front of the call as edgl_gemm_dw_defer(0) would.  edgl_gemm_dw_ride(0), or
 * edgl_gemm_dw_defer(0 | -1), withdraws the request. */
int edgl_gemm_dw_ride(int on);

/* out[n] (+)= sum_m X[m, n]  — bias gradients.  X `dtype` (or f32 if x_f32) [M, ld]; out f32[N]. */
int edgl_colsum(const void* X, int M, int N, int ld, float* out, int accumulate, float* workspace,
                int x_f32, int dtype, void* stream);

/* ---- K3: fused BiMAU attention — temporal.py:404-452 + MAU.intensity temporal.py:281-315 -------
 * qkvt [B,T,4C] = dense(x) already computed (K2), split order Q,K,V,T (temporal.py:410).  Per
 * (b, head): S=QK^T/sqrt(dh), key mask (ids[b,k]==0 -> -2^32+1), softmax, H=P.T_, intensity MLP ->
 * lam[b',q,:E], G=lam.marks^T with diag:=1, attention dropout, O=(G*P).V;
 * out[b,q,head*dh+:] = O + resid[b,q,head*dh+:] (:447); resid has row stride ld_res (first C channels
 * of the block input).  The intensity weights W1 [dh+1, dh*E], b1 [dh*E], w [E,dh], scaling [E] (f32)
 * are first packed by edgl_bimau_pack into `pack` (edgl_bimau_pack_bytes bytes, reusable by fwd and
 * bwd until the weights change).  lam_out f32 [H*B,T,E].  `saved` (edgl_bimau_saved_bytes bytes, or
 * NULL for inference) receives what the backward re-uses: the H rows fed to the intensity MLP and its
 * pre-softplus output z.  `flags`: 0 = BiMAU as above; EDGL_MAU_CAUSAL adds the future-blinding mask of
 * MAU.__call__(causality=True) (temporal.py:370-375: keys k > q scored -2^32+1 like padded keys, no gradient
 * through them); EDGL_MAU_NO_DIAG keeps the modulation on the diagonal (MAU, temporal.py:383; BiMAU overwrites
 * it with 1, :438-439); EDGL_MAU_DIAG_ZERO writes 0 there instead of 1 — for a unit with more than 16 mark types, run as
 * groups of <= 16 marks whose outputs are summed (G is linear in the marks: group 0 carries the diagonal 1 and the
 * residual, the later groups 0 and a zero residual).  The caller may fill the Q and K|V|T_ column blocks of qkvt from different inputs
 * (MAU: Q = dense(LN(x)), K,V,T_ = dense(x), temporal.py:352-355).  Supported: dh in {16,32,64,128}, E<=16, T<=1024.
 *
 * Two kernel families serve the unit.  The in-register kernels keep the whole key row of a (sample, head) job in registers and
 * take T <= 208 at head dim 16, T <= 208 (bf16) / 128 (f32) at head dim 32, T <= 128 / 112 at head dim 64 and T <= 128 / 64 at head
 * dim 128.  Every other shape up to T = 1024 runs the key-streamed kernels (flash style: the keys are walked in tiles, the softmax
 * statistics of every row are kept in `saved`), which compute the same function, take the same dropout decisions from the same
 * (rng_state, stream_id) and need `saved` also for inference.  edgl_bimau_form tells which family a shape gets (0 in-register,
 * 1 key-streamed, negative: unsupported; a host function, no GPU needed).  EDGL_MAU_STREAM is a host-side hint like
 * EDGL_MAU_NO_SKIP: it forces the key-streamed family at a shape the in-register kernels also take; the forward, its backward and
 * the size queries (the _ex forms below, which take the flags) must all see the same flag.  The key-streamed family has no fused TPP
 * form and ignores dropbits, order and EDGL_MAU_NO_SKIP (results do not depend on them anywhere). */
#define EDGL_MAU_CAUSAL 1
#define EDGL_MAU_NO_DIAG 2
#define EDGL_MAU_DIAG_ZERO 4
/* host-side hint, not a semantic flag: launch the kernels that walk every key tile.  The bf16 / head dim 16 / 16 marks family
 * otherwise leaves out the all-padding key tiles in front of a sequence's first real key (exact); a caller whose batches cannot
 * have any — training batches of the reference's masker carry MASK tokens on padded positions, dataloader.py:187-191 — saves the
 * skip variant's per-tile scalar branch.  Results are identical either way. */
#define EDGL_MAU_NO_SKIP 8
#define EDGL_MAU_STREAM 16
int edgl_bimau_form(int T, int C, int H, int dtype, int flags);
long edgl_bimau_pack_bytes(int C, int H, int E, int dtype);
/* bytes of `saved` for the family the shape gets without / with the hint flags (the _ex form with flags = 0 is the plain one) */
long edgl_bimau_saved_bytes(int B, int T, int C, int H, int dtype);
long edgl_bimau_saved_bytes_ex(int B, int T, int C, int H, int dtype, int flags);
/* largest mark count (<= 16) one launch takes at this head dim / dtype (LDS of the intensity backward); -1: bad arguments */
int edgl_bimau_mark_group(int C, int H, int dtype);
int edgl_bimau_pack(const float* W1, const float* b1, const float* w, const float* scaling, int C, int H, int E,
                    void* pack, int dtype, void* stream);
int edgl_bimau_fwd(const void* qkvt, const void* resid, int ld_res, const int64_t* ids, const float* spans,
                   const uint8_t* marks, const void* pack, int B, int T, int C, int H, int E, float drop_rate,
                   const uint64_t* rng_state, uint32_t stream_id, void* out, float* lam_out, void* saved,
                   int flags, int dtype, void* stream);
/* edgl_bimau_fwd that also fills `zero_rows` (f32 [H*B,T,E], may be NULL) with zeros — the training engine's d lambda buffer, of
 * which edgl_tpp_fwd_bwd_rows then writes the masked positions only (the forward is VALU bound: the extra stores are free). */
int edgl_bimau_fwd_zr(const void* qkvt, const void* resid, int ld_res, const int64_t* ids, const float* spans,
                      const uint8_t* marks, const void* pack, int B, int T, int C, int H, int E, float drop_rate,
                      const uint64_t* rng_state, uint32_t stream_id, void* out, float* lam_out, void* saved,
                      float* zero_rows, int flags, int dtype, void* stream);

/* Attention dropout as stored keep bits (temporal.py:442; the three kernels of a training step — forward and the two backward
 * sweeps — take the same decisions): edgl_bimau_dropbits evaluates the counter hash of (rng_state, stream_id, element (b', q, k))
 * ONCE and stores the decisions in the kernels' register layout — edgl_bimau_dropbits_bytes(B, T, H) bytes (0: no stored-bits form
 * at this T, the kernels hash) —, edgl_bimau_fwd_db / edgl_bimau_bwd_db are edgl_bimau_fwd_zr / edgl_bimau_bwd reading them
 * (dropbits NULL = hash).  Identical masks either way: a kernel without a stored-bits form (head dims other than 16, E != 16, MAU
 * flags, f32) ignores the argument and hashes.  qk_scale: the score scale of temporal.py:422 (0 = 1 / sqrt(dh)); a model whose
 * head dim d is none of {16, 32, 64, 128} — the reference's default --num_units 50 --num_heads 1 (main.py:35-37) — runs with
 * zero-padded channels at the next supported head dim and qk_scale = 1 / sqrt(d) (exact: padded Q / K / V / T_ columns are 0). */
long edgl_bimau_dropbits_bytes(int B, int T, int H);
int edgl_bimau_dropbits(int B, int T, int H, float drop_rate, const uint64_t* rng_state, uint32_t stream_id, uint32_t* bits,
                        void* stream);
int edgl_bimau_fwd_db(const void* qkvt, const void* resid, int ld_res, const int64_t* ids, const float* spans,
                      const uint8_t* marks, const void* pack, int B, int T, int C, int H, int E, float drop_rate,
                      const uint64_t* rng_state, uint32_t stream_id, const uint32_t* dropbits, float qk_scale, void* out,
                      float* lam_out, void* saved, float* zero_rows, int flags, int dtype, void* stream);

/* Launch order of the attention kernels' (sample, head) jobs (temporal.py:404-452 computes every head of every sample; the order
 * only decides WHEN a job runs).  The bf16 / head dim 16 / 16 marks kernels leave out the key tiles that hold nothing but the
 * left padding of a sequence (data/linkpred.py:142-157; temporal.py:425-429: their probabilities are exactly 0), so a job's time
 * falls with its padding; edgl_bimau_job_order lists the samples by falling key-tile count (first B entries of `order`, ties by index) and
 * edgl_bimau_fwd_ord / edgl_bimau_bwd_ord launch the long jobs first.  order == NULL: index order (= edgl_bimau_fwd_db /
 * edgl_bimau_bwd_db / edgl_bimau_bwd_tpp).  edgl_bimau_bwd_ord: tpp_desc == NULL -> d_lam_ext as in edgl_bimau_bwd_db;
 * tpp_desc != NULL -> the fused TPP form of edgl_bimau_bwd_tpp (d_lam_ext must be NULL).  Results do not depend on the order. */
int edgl_bimau_job_order(const int64_t* ids, int B, int T, int32_t* order, void* stream);   /* order: int32 [2 * B] (order | scratch); B <= 16384 */
int edgl_bimau_fwd_ord(const void* qkvt, const void* resid, int ld_res, const int64_t* ids, const float* spans,
                       const uint8_t* marks, const void* pack, int B, int T, int C, int H, int E, float drop_rate,
                       const uint64_t* rng_state, uint32_t stream_id, const uint32_t* dropbits, float qk_scale, void* out,
                       float* lam_out, void* saved, float* zero_rows, const int32_t* order, int flags, int dtype, void* stream);
int edgl_bimau_bwd_ord(const void* qkvt, const int64_t* ids, const float* spans, const uint8_t* marks, const void* pack,
                       const void* d_out, const float* d_lam_ext, const void* tpp_desc, int M, const float* tpp_sums, float coef,
                       float* tpp_part, const float* lam, const void* saved, int B, int T, int C, int H, int E, float drop_rate,
                       const uint64_t* rng_state, uint32_t stream_id, const uint32_t* dropbits, float qk_scale, void* d_qkvt,
                       float* dW1, float* db1, float* dw, float* dscaling, void* workspace, const int32_t* order, int flags,
                       int dtype, void* stream);

/* Backward.  d_out [B,T,C] `dtype`; d_lam_ext f32 [H*B,T,E] or NULL (gradient
 * from the TPP regulariser); lam / saved: the forward's lam_out and `saved` buffer.  Writes d_qkvt [B,T,4C] `dtype` and the f32 weight gradients dW1
 * [dh+1,dh*E], db1 [dh*E], dw [E,dh], dscaling [E] (overwritten; per-workgroup partials in
 * `workspace` — edgl_bimau_bwd_workspace BYTES — are reduced in a fixed order).  The residual
 * gradient (d_out itself) is NOT added here — the caller routes it. */
long edgl_bimau_bwd_workspace(int B, int T, int C, int H, int E, int dtype);
long edgl_bimau_bwd_workspace_ex(int B, int T, int C, int H, int E, int dtype, int flags);   /* for the family that `flags` selects */
int edgl_bimau_bwd(const void* qkvt, const int64_t* ids, const float* spans, const uint8_t* marks,
                   const void* pack, const void* d_out, const float* d_lam_ext, const float* lam,
                   const void* saved, int B, int T, int C, int H, int E, float drop_rate,
                   const uint64_t* rng_state, uint32_t stream_id, void* d_qkvt, float* dW1, float* db1,
                   float* dw, float* dscaling, void* workspace, int flags, int dtype, void* stream);
int edgl_bimau_bwd_db(const void* qkvt, const int64_t* ids, const float* spans, const uint8_t* marks,
                      const void* pack, const void* d_out, const float* d_lam_ext, const float* lam,
                      const void* saved, int B, int T, int C, int H, int E, float drop_rate,
                      const uint64_t* rng_state, uint32_t stream_id, const uint32_t* dropbits, float qk_scale, void* d_qkvt,
                      float* dW1, float* db1, float* dw, float* dscaling, void* workspace, int flags, int dtype, void* stream);

/* ---- K4-LN: y = layernorm_joint(dropout(x) + resid) — Base.py:12-67 (moments over (T,C) per
 * sample, eps 1e-12), EasyDGL.py:114-116,126-128,139.  resid may be NULL (ld_res ignored).
 * stats f32 [B,2] = (mean, rstd).  If gather_pos != NULL (int64 [B,Mg]) only rows
 * y_g[b*Mg+j,:] = y[b, gather_pos[b,j], :] are written (EasyDGL.py:142-146 batch_gather). */
int edgl_add_layernorm_fwd(const void* x, const void* resid, int ld_res, const float* gamma,
                           const float* beta, int B, int T, int C, float drop_rate,
                           const uint64_t* rng_state, uint32_t stream_id, const int64_t* gather_pos,
                           int Mg, void* y, float* stats, int dtype, void* stream);

/* Backward: given dy (dense [B,T,C], or gathered [B*Mg,C] when gather_pos != NULL), recomputes
 * xhat from (x, resid, stats) and writes dx (gradient w.r.t. dropout(x)+resid input sum, i.e. the
 * caller uses it for the residual; d_x_pre = dx * dropmask is written to dx_drop) and per-sample
 * partials of dgamma/dbeta into workspace [B,2,C] reduced into dgamma/dbeta (overwritten).
 * Gathered rows naming the same position add up.  dy_rowmap (int32 [B*Mg], may be NULL) redirects
 * gathered row r to row dy_rowmap[r] of dy (-1: the row carries no gradient) — the `inv` map of
 * edgl_compact_rows. */
int edgl_add_layernorm_bwd(const void* x, const void* resid, int ld_res, const float* gamma,
                           const float* stats, const void* dy, int B, int T, int C, float drop_rate,
                           const uint64_t* rng_state, uint32_t stream_id, const int64_t* gather_pos,
                           int Mg, const int32_t* dy_rowmap, void* dsum, void* dx_drop, float* dgamma,
                           float* dbeta, float* workspace, int dtype, void* stream);
/* The same with a fused activation backward: x is gelu(act_pre) (the head transform, EasyDGL.py:136-139); the emitted
 * gradients (dsum, dx_drop) are multiplied by gelu'(act_pre) — the gradient w.r.t. the dense layer's pre-activation. */
int edgl_add_layernorm_bwd_act(const void* x, const void* resid, int ld_res, const float* gamma,
                               const float* stats, const void* dy, int B, int T, int C, float drop_rate,
                               const uint64_t* rng_state, uint32_t stream_id, const int64_t* gather_pos,
                               int Mg, const int32_t* dy_rowmap, const void* act_pre, void* dsum, void* dx_drop,
                               float* dgamma, float* dbeta, float* workspace, int dtype, void* stream);
/* The joint LayerNorm of a channel-padded model (see edgl_encode_fwd_ct): moments over the REAL channels only (divisor T * true
 * width; the padded channels hold exact zeros and stay out of the centred second moment), the input gradient of a padded channel
 * is zero — so nothing ever flows into the padded rows / columns of the dense kernels (Base.py:12-67 on the true width). */
int edgl_add_layernorm_fwd_ct(const void* x, const void* resid, int ld_res, const float* gamma, const float* beta, int B, int T,
                              int C, float drop_rate, const uint64_t* rng_state, uint32_t stream_id, const int64_t* gather_pos,
                              int Mg, void* y, float* stats, int dh_pad, int dh_true, int dtype, void* stream);
int edgl_add_layernorm_bwd_act_ct(const void* x, const void* resid, int ld_res, const float* gamma, const float* stats,
                                  const void* dy, int B, int T, int C, float drop_rate, const uint64_t* rng_state,
                                  uint32_t stream_id, const int64_t* gather_pos, int Mg, const int32_t* dy_rowmap,
                                  const void* act_pre, void* dsum, void* dx_drop, float* dgamma, float* dbeta, float* workspace,
                                  int dh_pad, int dh_true, int dtype, void* stream);

/* ---- K5: tied-embedding scoring + cross-entropy — EasyDGL.py:149-155,177-185, Base.py:106-110 --
 * rows [R,C] `dtype`; table [I,C] `dtype` (row 0 acts as zeros, column 0 logit == -1000); out_bias
 * f32 [I-1]; labels int64 [R] (may be NULL for eval).  The item range [i0, i1) lets a rank score its
 * shard only.  The [R, I] logits are never materialised unless `logits` (f32 [R, i1-i0]) is given.
 * fwd: online (max, sumexp) per row and item chunk -> row_lse f32 [R] (log-sum-exp over [i0,i1)),
 * label_logit f32 [R] (written only for rows whose label lies in [i0,i1); pre-zero when sharded).
 * workspace >= 2*R*edgl_score_chunks(R, i1-i0) floats.  C: power of two, 32..256 (bf16) / 32..128 (f32);
 * i0 must be a multiple of 8. */
int edgl_score_chunks(int R, int n_items);
/* Rows with label 0 have weight 0 in the loss (EasyDGL.py:180) and therefore no effect on the loss
 * or on any gradient.  edgl_compact_rows orders the weighted rows first: perm int32 [R] (original
 * row of compact row j, -1 past the end), inv int32 [R] (compact index of row r, or -1), nvalid
 * int32 [1] (device), rows_c [R,C] / labels_c [R] the gathered copies (zero past nvalid).  The
 * scoring entry points take `nvalid` (device pointer or NULL): rows >= *nvalid are skipped (their
 * row_lse is 0, their d_rows undefined).  edgl_scatter_rows undoes the compaction:
 * rows[r] = inv[r] >= 0 ? rows_c[inv[r]] : 0. */
int edgl_compact_rows(const void* rows, const int64_t* labels, int R, int C, int32_t* perm, int32_t* inv,
                      int32_t* nvalid, void* rows_c, int64_t* labels_c, int dtype, void* stream);
/* The two halves of edgl_compact_rows: the scan needs the labels only (it may run before the rows exist), the gather the rows. */
int edgl_compact_scan(const int64_t* labels, int R, int32_t* perm, int32_t* inv, int32_t* nvalid, void* stream);
/* ... the scan that also writes the compacted labels (labels_c int64 [R]: weighted rows first, 0 behind them) */
int edgl_compact_scan_labels(const int64_t* labels, int R, int32_t* perm, int32_t* inv, int32_t* nvalid, int64_t* labels_c,
                             void* stream);
int edgl_compact_gather(const void* rows, const int64_t* labels, const int32_t* perm, int R, int C, void* rows_c,
                        int64_t* labels_c, int dtype, void* stream);
int edgl_scatter_rows(const void* rows_c, const int32_t* inv, int R, int C, void* rows, int dtype,
                      void* stream);
/* (row_lse may be NULL when logits is given: the evaluation path wants the logits tile only — Base.py:150-163) */
int edgl_score_lse_fwd(const void* rows, const void* table, const float* out_bias, const int64_t* labels,
                       int R, int C, int I, int i0, int i1, const int32_t* nvalid, float* row_lse,
                       float* label_logit, float* logits, float* workspace, int dtype, void* stream);
/* loss = sum_r w_r * (-log(p_y + 1e-5)) / (sum w + 1e-5), w_r = [label != 0]; also writes the
 * per-row coefficient coef[r] = (w_r/W) * p_y/(p_y+1e-5) used by the backward.  loss_out f32[1]. */
int edgl_ce_loss_fwd(const float* row_lse, const float* label_logit, const int64_t* labels, int R,
                     float* loss_out, float* coef, void* stream);
/* The same with loss_out[0] = cross-entropy + add_in[0] + add_in2[0] (device scalars holding the regularisation terms of
 * the step — two, so that terms produced on different streams need no common accumulator; either may be NULL): saves the
 * training engine a separate one-element add launch. */
int edgl_ce_loss_fwd_add(const float* row_lse, const float* label_logit, const int64_t* labels, int R, float* loss_out,
                         float* coef, const float* add_in, const float* add_in2, void* stream);
/* ... with the denominator of the GLOBAL batch (`wtotal`, device int32 or NULL; see edgl_score_flash_fwd_coef_w): loss_out[0] is
 * then this rank's share of the global cross-entropy (+ the terms added in). */
int edgl_ce_loss_fwd_add_w(const float* row_lse, const float* label_logit, const int64_t* labels, int R, float* loss_out,
                           float* coef, const float* add_in, const float* add_in2, const int32_t* wtotal, void* stream);
/* backward of the CE: dl[r,j] = g * coef[r] * (p[r,j] - [j==label_r]) (g = d loss, device scalar or
 * NULL for 1), never materialised:  d_rows[R,C] (`dtype`) = dl . table ;  d_table[I,C] (f32,
 * overwritten for rows [i0,i1), row 0 := 0) = dl^T . rows ;  d_bias[I-1] f32 = colsum(dl)[1:].
 * workspace >= edgl_score_bwd_workspace(R, C, I, i1-i0, dtype) floats (holds the per-chunk partial slabs, reduced in a
 * fixed order, and — f32 only — the transposed operand images rowsT/tableT; the bf16 kernels read the transposed
 * operand out of their row-major LDS tiles). */
long edgl_score_bwd_workspace(int R, int C, int I, int n_items, int dtype);
int edgl_score_ce_bwd(const void* rows, const void* table, const float* out_bias, const int64_t* labels,
                      const float* row_lse, const float* coef, const float* gscale, int R, int C, int I,
                      int i0, int i1, const int32_t* nvalid, void* d_rows, float* d_table, float* d_bias,
                      float* workspace, int dtype, void* stream);

/* ---- K6: evaluation — Base.py:150-207 ----------------------------------------------------------
 * logits f32 [R, n] for the item range starting at i0; seen [R,T] int64 item ids to mask with -inf
 * (Base.py:156-163; NULL = no masking); top-K by (value desc, index asc) (tf.nn.top_k tie rule).
 * out_val f32 [R,K], out_idx int32 [R,K] (GLOBAL item ids = i0 + local). K <= 128. */
int edgl_mask_topk(float* logits, int R, int n, int i0, const int64_t* seen, int T, int K, float* out_val,
                   int32_t* out_idx, void* stream);
/* Fused evaluation scoring (Base.py:150-181 + EasyDGL.py:149-151): logits = rows . table[i0:i1]^T + [-1000, out_bias] -> -inf at the
 * row's seen ids (seen [R,T] int64, may be NULL with T = 0) -> top-K by (value desc, global index asc), WITHOUT the [R, i1-i0] logits
 * tile in HBM: the logits are computed twice on the matrix pipe — group maxima give every row a lower bound of its K-th best unseen
 * logit, the second sweep appends the few hundred elements above it to the row's candidate list, one more launch ranks
 * them; rows whose list overflows (heavy ties) are redone exactly from the row's logits in a scratch row.  bf16; C in {64, 128, 256};
 * K <= 128; 4096 <= i1 - i0 <= 262144 per call (larger catalogues: item chunks + edgl_topk_merge).  edgl_score_topk_fused_supported
 * = 1 when the shape is taken — otherwise the call returns EDGL_ERR_SHAPE (no silent fallback): run edgl_score_lse_fwd +
 * edgl_mask_topk.  workspace: edgl_score_topk_fused_workspace BYTES.  out_val f32 [R,K], out_idx int32 [R,K] (global ids). */
int edgl_score_topk_fused_supported(int R, int C, int n_items, int T, int K, int dtype);
long edgl_score_topk_fused_workspace(int R, int C, int n_items, int T, int K);
int edgl_score_topk_fused(const void* rows, const void* table, const float* out_bias, const int64_t* seen, int T, int R, int C,
                          int I, int i0, int i1, int K, float* out_val, int32_t* out_idx, void* workspace, int dtype, void* stream);
/* ---- K7: merge of per-shard candidates (after an RCCL all-gather): cand_val/idx [S, R, K] ->
 * global top-K per row by (value desc, global index asc); entries with index < 0 are ignored; S*K <= 1024.  (Candidates above the
 * K-th largest thread maximum are ranked by counting; inputs with more than 256 of them — tie blocks — are sorted.) */
int edgl_topk_merge(const float* cand_val, const int32_t* cand_idx, int S, int R, int K, float* out_val,
                    int32_t* out_idx, void* stream);
/* HR@k / NDCG@k sums for k in {10,50,100} (Base.py:181-201): metrics f32 [6] += per-batch sums in
 * the order H10,H50,H100,N10,N50,N100; label int64 [R]. */
int edgl_rank_metrics(const int32_t* topk_idx, int R, int K, const int64_t* label, float* metrics,
                      void* stream);

/* ---- K6r: evaluation by label rank — Base.py:150-201 without a top-K list.  For row r with label y = labels[r] (int64, 0 <= y < I)
 * and v_j = -inf at the row's seen ids, else rows[r] . table[j] + [-1000, out_bias][j] (table row 0 reads as zeros):
 *     count[r] += #{ j in [i0, i1), j != y : v_j > v_y  or  (v_j == v_y and j < y) }          (-0.0 == +0.0)
 * Over [0, I) that is the index of y in the (value desc, id asc) order of edgl_mask_topk / edgl_score_topk_fused, so HR@k, NDCG@k
 * and MRR follow for any k; counts over disjoint ranges (item chunks, table shards) add.  label_val f32 [R] holds v_y (-inf when the
 * label is itself seen) and MUST be the bits the counting pass forms for the pair (r, y): the tie rule on duplicated items depends
 * on it.  Fused form (Base.py:150-201): bf16, C in {64, 128, 256}, 1 <= i1 - i0 <= 262144 per call, i0 % 8 == 0, seen 16-byte
 * aligned; edgl_score_label_value runs the sweep's own MFMA chain on gathered label rows (once per batch), edgl_score_rank_fused is
 * one sweep on the matrix pipe with the seen ids as an LDS bitmap and integer atomics into count (exact, order-independent).  The
 * three host queries (Base.py:150-201: no device work) answer: shape taken (1 / 0), workspace BYTES (0 for every shape taken — the
 * workspace argument may then be NULL; -1 for a shape not taken), item slices of the plan (-1 likewise).  A shape not taken is
 * refused with EDGL_ERR_SHAPE and the bound in the text: no silent fallback. */
int edgl_score_rank_supported(int R, int C, int n_items, int T, int dtype);
long edgl_score_rank_workspace(int R, int C, int n_items, int T);
int edgl_score_rank_slices(int R, int C, int n_items, int T);
int edgl_score_label_value(const void* rows, const void* table, const float* out_bias, const int64_t* seen, int T,
                           const int64_t* labels, int R, int C, int I, float* label_val, int dtype, void* stream);
int edgl_score_rank_fused(const void* rows, const void* table, const float* out_bias, const int64_t* seen, int T,
                          const int64_t* labels, const float* label_val, int R, int C, int I, int i0, int i1, int32_t* count,
                          void* workspace, int dtype, void* stream);
/* Tile form (Base.py:150-201; any dtype and width): logits f32 [R, n] of the item range starting at i0 (i0 % 8 == 0), read and NOT
 * modified.  edgl_label_value_tile writes label_val[r] for the rows whose label lies in [i0, i0 + n) (the tile's own value, -inf when
 * the label is seen) and leaves the others untouched; edgl_rank_count_tile adds the tile's share of the count. */
int edgl_label_value_tile(const float* logits, int R, int n, int i0, const int64_t* seen, int T, const int64_t* labels,
                          float* label_val, void* stream);
int edgl_rank_count_tile(const float* logits, int R, int n, int i0, const int64_t* seen, int T, const int64_t* labels,
                         const float* label_val, int32_t* count, void* stream);
/* Metric sums from ranks (Base.py:150-201 for any k): rank int32 [R], ks int32 [nk <= 8] (device);
 * sums f32 [2 nk + 1] += H@k.., N@k.., MRR with H = [rank < k], N = H / log2(rank + 2), MRR = 1 / (rank + 1); fixed summation order. */
int edgl_rank_metrics_from_rank(const int32_t* rank, int R, const int32_t* ks, int nk, float* sums, void* stream);

/* ---- K6c: evaluation on candidate lists (k_eval_cand.hip): the sampled-negative protocol and re-ranking.
 * Every row scores its OWN list cand int32 [R, N] — a gather of R (N + 1) table rows, no sweep over the catalogue.  The order and the
 * used table are those of the rank sweep above (Base.py:150-201: item 0 is the zero row with bias -1000):
 *   v(r, c) = -inf for c < 0 (an empty slot), for c >= I (a caller error: nothing is read out of bounds) and for c in seen[r, :];
 *           = rows[r] . table[c] + bias_used[c] otherwise, f32 accumulation;
 *   count[r] += #{ n : c = cand[r, n] >= 0, c != y, v(r, c) > v(r, y) or (v(r, c) == v(r, y) and c < y) },  y = labels[r].
 * v(r, c) is a pure function of rows[r], table[c] and the bias — the same bits whatever the slot, N, R or the other candidates — and
 * v(r, y) comes out of the same code: ties between items with identical table rows and biases resolve by id alone.  The label need
 * not be in the list; its own slots are not counted; a repeated id is counted once per slot.
 * rows [R, C] and table [I, C] in `dtype` (f32 or bf16; 16-byte aligned), out_bias f32 [I - 1], seen int64 [R, T] (NULL with T = 0),
 * labels int64 [R] (NULL when neither label_val nor count is wanted).  Outputs, each may be NULL: scores f32 [R, N], label_val f32
 * [R], count int32 [R] (ADDED into: the caller zeroes it).  16 <= C <= 512 and C % 16 == 0; R >= 1; N >= 1 with R (N + 1) < 2^31;
 * 0 <= T <= 1024; anything else is EDGL_ERR_SHAPE with the bound in the text.  No workspace.  edgl_score_candidates_chunk: the
 * slots one workgroup takes for this shape (host arithmetic; -1 for a shape not taken) — the values do not depend on it. */
int edgl_score_candidates_chunk(int R, int C, int N, int dtype);
int edgl_score_candidates(const void* rows, const void* table, const float* out_bias, const int32_t* cand, const int64_t* seen,
                          int T, const int64_t* labels, int R, int C, int I, int N, float* scores, float* label_val,
                          int32_t* count, int dtype, void* stream);
/* cand int32 [R, n]: per row n ids drawn uniformly from [lo, hi), with replacement between slots, never one of seen[r, :] (int64
 * [R, T], NULL with T = 0) and never labels[r] (int64 [R], may be NULL).  Counter-based (all arithmetic mod 2^32, mix32 = the
 * murmur3 finaliser of the dropout generator):
 *   k = mix32((u32)seed ^ 0xC4ED1DA7); k = mix32(k + (u32)(seed >> 32)); k = mix32(k ^ (u32)step)
 *   h = mix32(k ^ mix32((u32)(row0 + r))); h = mix32(h + slot * 0x9E3779B1); h = mix32(h ^ (att * 0x85EBCA6B))
 *   id = lo + (((u64)h * (u64)(hi - lo)) >> 32);  the slot takes the first att in 0..31 whose id is accepted, else -1.
 * row0 = index of the batch's first sequence in its split: a sequence's list does not depend on the batch size.  Needs
 * 1 <= lo < hi <= I and 2 (T + 1) <= hi - lo (a draw is then rejected with probability <= 1/2), 0 <= T <= 1024, else EDGL_ERR_SHAPE. */
int edgl_sample_negatives(const int64_t* seen, int T, const int64_t* labels, int R, int n, int lo, int hi, int I,
                          uint64_t seed, uint64_t step, int row0, int32_t* cand, void* stream);
/* edgl_sample_negatives with a weighted draw: everything above stands but the last line.  thr_alias: uint32
 * [hi - lo, 2], 8-byte aligned, entry j = (acceptance threshold thr[j], alias bucket alias[j]) of an alias table over the ids
 * lo + j (Vose's method; a full bucket stores alias[j] = j).  With n = hi - lo:
 *   j = ((u64)h * n) >> 32;  h2 = mix32(h + 0x68E31DA4);  id = lo + (h2 < thr[j] || alias[j] == j ? j : alias[j])
 * one 8-byte random read per attempt.  The weighted form of 2 (T + 1) <= hi - lo is a property of the weights — the T + 1
 * heaviest ids hold at most half of the total weight — and is the table builder's to check (easydgl_amd.ops.build_neg_dist). */
int edgl_sample_negatives_alias(const int64_t* seen, int T, const int64_t* labels, int R, int n, int lo, int hi, int I,
                                const uint32_t* thr_alias, uint64_t seed, uint64_t step, int row0, int32_t* cand, void* stream);
/* edgl_rank_metrics_from_rank with the rows added to every sum one by one, in row order: the f32 sums of a split do not depend on
 * how it is cut into batches (the steps on candidate lists use it; a batch costs one lane-loop over its rows). */
int edgl_rank_metrics_from_rank_rows(const int32_t* rank, int R, const int32_t* ks, int nk, float* sums, void* stream);

/* ---- K5c: sampled-softmax training — cross-entropy over per-row candidate lists (csrc/k_cand_ce.hip) -------------
 * The training side of edgl_score_candidates: row r (label y = labels[r]) is scored against slot 0 = its label and slots 1 + n =
 * cand[r, n] (int32 [R, N]) by the SAME arithmetic (cand_gather.h), so vals[r, 1 + n] and label_val carry the bits
 * edgl_score_candidates gives.  A list slot reads -inf and takes no part in loss or gradient when it is empty (-1), at or past I,
 * or equal to the row's label (accidental hits).  Rows with label 0 have weight 0: vals -inf, label_val = row_lse = 0, gradients 0.
 *   edgl_cand_ce_fwd   vals f32 [R, N + 1], label_val f32 [R], row_lse f32 [R] = log sum exp over the label and the live slots, in
 *                      an order that is a function of N alone (no atomics; a row's outputs do not depend on R or on other rows).
 *                      Loss and coef come from edgl_ce_loss_fwd(row_lse, label_val, labels, ..).
 *   edgl_cand_ce_bwd   dv f32 [R, N + 1] = g coef[r] (exp(vals - row_lse) - [slot 0]) (gscale: device scalar or NULL = 1);
 *                      d_rows [R, C] (`dtype`) = sum_s dv table[c_s], one store per row, no atomics; d_table f32 [I, C] / d_bias f32
 *                      [I - 1] are ADDED into with f32 atomics (the caller zero-fills them; row 0 is never touched), or both NULL:
 *                      dv only.  R (N + 1) C 4 bytes of atomic adds, whole contiguous row segments per wave-instruction.
 *   edgl_cand_ce_table_det   the same table / bias sums without float atomics: ordered sums over a plan of the slot keys (the call
 *                      builds keys int64 [R (N + 1)] and the plan, edgl_segsum_plan_bytes of (R (N + 1), I) bytes, 16-byte aligned):
 *                      one writer per table row, the order of every sum a function of (cand, labels) alone.  Adds into d_table / d_bias.
 * rows / table in `dtype` (f32 or bf16), 16-byte aligned; 16 <= C <= 512 and C % 16 == 0; R >= 1; 1 <= N <= 8192 with
 * R (N + 1) < 2^31; I > 1; anything else is EDGL_ERR_SHAPE with the bound in the text. */
int edgl_cand_ce_fwd(const void* rows, const void* table, const float* out_bias, const int32_t* cand, const int64_t* labels, int R,
                     int C, int I, int N, float* vals, float* label_val, float* row_lse, int dtype, void* stream);
/* edgl_cand_ce_fwd with the log-Q correction of a weighted sampler: logq f32 [I] (log of each id's draw probability,
 * 0 where none is defined) — the label and every live slot read v - logq[c], one f32 subtraction on the finished value.  logq of
 * zeros, or NULL, gives the bits of edgl_cand_ce_fwd (which forwards here with NULL).  edgl_cand_ce_bwd serves both. */
int edgl_cand_ce_fwd_q(const void* rows, const void* table, const float* out_bias, const float* logq, const int32_t* cand,
                       const int64_t* labels, int R, int C, int I, int N, float* vals, float* label_val, float* row_lse, int dtype,
                       void* stream);
int edgl_cand_ce_bwd(const void* rows, const void* table, const float* out_bias, const int32_t* cand, const int64_t* labels,
                     const float* vals, const float* row_lse, const float* coef, const float* gscale, int R, int C, int I, int N,
                     void* d_rows, float* dv, float* d_table, float* d_bias, int dtype, void* stream);
int edgl_cand_ce_table_det(const void* rows, const int32_t* cand, const int64_t* labels, const float* dv, int R, int C, int I, int N,
                           float* d_table, float* d_bias, int64_t* keys, void* plan, int dtype, void* stream);

/* ---- K5d: sampled-softmax training on ONE negative list per step (csrc/k_shared_ce.hip) ---------------------------
 * The definition of edgl_cand_ce_* with cand[r, :] = shared[:] (int32 [S]) for every row: the label is kept apart (label_val) and
 * vals f32 [R, S] holds slot s = shared[s]; a slot reads -inf for row r when shared[s] < 0, shared[s] >= I or shared[s] == labels[r].
 * Rows of weight 0 (label outside [1, I), or at / past nvalid[0]; nvalid: device int32 of a compacted batch, or NULL = R): vals
 * -inf, label_val = row_lse = 0, d_rows 0.
 *   edgl_shared_ce_fwd   the [R, C] x [C, S] product on MFMA with the listed table rows gathered into the LDS image; an online
 *                        (max, sum) per row in an order that is a function of (dtype, C, S) alone: no atomics, a row's outputs do not
 *                        depend on R or on the other rows.  Loss and coef come from edgl_ce_loss_fwd(row_lse, label_val, labels, ..).
 *   edgl_shared_ce_bwd   d_rows [R, C] (`dtype`) = dv W_S + dv_label table[y] without atomics; the slab dv^T rows [S, C] is summed
 *                        over fixed row splits in order and ADDED into d_table f32 [I, C] / d_bias f32 [I - 1] (row 0 is never
 *                        touched), as is the label term.  keys / plan NULL: both with f32 atomics, (R + S) C 4 bytes.  keys (int64
 *                        [2 R]) and plan (edgl_segsum_plan_bytes(2 R, I) bytes, 16-byte aligned) given: no float atomics — the first
 *                        slot of a repeated id sums its repeats in slot order, the label term is an ordered sum over the plan.
 *                        workspace: edgl_shared_ce_workspace(R, C, S, dtype) floats, 16-byte aligned.
 * rows / table in `dtype`, 16-byte aligned; 16 <= C <= 512 with C % 8 == 0 (bf16) or C % 4 == 0 (f32); R >= 1; 1 <= S <= 8192 with
 * R (S + 8) < 2^31; I > 1; anything else is EDGL_ERR_SHAPE with the bound in the text, checked before any pointer is read. */
long edgl_shared_ce_workspace(int R, int C, int S, int dtype);
int edgl_shared_ce_fwd(const void* rows, const void* table, const float* out_bias, const int32_t* shared, const int64_t* labels,
                       const int32_t* nvalid, int R, int C, int I, int S, float* vals, float* label_val, float* row_lse, int dtype,
                       void* stream);
/* edgl_shared_ce_fwd with the log-Q correction: logq f32 [I] as in edgl_cand_ce_fwd_q; zeros or NULL give the bits
 * of edgl_shared_ce_fwd (which forwards here with NULL).  edgl_shared_ce_bwd serves both. */
int edgl_shared_ce_fwd_q(const void* rows, const void* table, const float* out_bias, const float* logq, const int32_t* shared,
                         const int64_t* labels, const int32_t* nvalid, int R, int C, int I, int S, float* vals, float* label_val,
                         float* row_lse, int dtype, void* stream);
int edgl_shared_ce_bwd(const void* rows, const void* table, const int32_t* shared, const int64_t* labels, const float* vals,
                       const float* label_val, const float* row_lse, const float* coef, const float* gscale, const int32_t* nvalid,
                       int R, int C, int I, int S, void* d_rows, float* d_table, float* d_bias, float* workspace, int64_t* keys,
                       void* plan, int dtype, void* stream);

/* ---- K5e: binary cross-entropy and BPR over the same sampled slots (csrc/k_sampled_loss.hip, sampled_dv.h) ---------
 * The slots, their liveness and their values are those of edgl_cand_ce_fwd[_q] / edgl_shared_ce_fwd[_q]: the forwards are the same
 * calls (their row_lse output is not used).  Row r is weighted iff 1 <= labels[r] < I and r < nvalid[0] (nvalid NULL = R); v0 is the
 * label's value, L_r the live list slots, n_r their number, W the number of weighted rows.
 *   EDGL_LOSS_BCE   l_r = softplus(-v0) + sum_{s in L_r} softplus(v_s)       dl/dv0 = sigma(v0) - 1       dl/dv_s = sigma(v_s)
 *   EDGL_LOSS_BPR   l_r = (1 / n_r) sum_{s in L_r} softplus(v_s - v0)        dl/dv_s = sigma(v_s - v0) / n_r,  dl/dv0 = -sum_s dl/dv_s
 *                   (n_r = 0: l_r = 0 and every derivative 0)
 *   loss = sum over the weighted rows of l_r / (W + 1e-5), the denominator of edgl_ce_loss_fwd; rows of weight 0 add nothing.
 *   With a log-Q term in the values, bce is tf.nn.nce_loss up to its constant log N, which is not applied.
 *   edgl_sampled_row_loss     per row: row_loss = l_r, row_aux (bpr: sum_s sigma(v_s - v0); bce: 0), row_scale (bce: 1; bpr: 1 / n_r
 *                             or 0), all f32 [R]; zeros for a row of weight 0.  label_val NULL: vals is f32 [R, S + 1] with slot 0 the
 *                             label (edgl_cand_ce_fwd's, S = N); label_val given: vals is f32 [R, S] (edgl_shared_ce_fwd's).  One wave
 *                             per row, no atomics, the order of every sum a function of S alone: a row's outputs depend on neither
 *                             R nor the other rows.
 *   edgl_sampled_loss_finish  loss_out[0] and coef f32 [R] = row_scale[r] / (W + 1e-5) (0 for a row of weight 0), one workgroup,
 *                             a fixed order.
 *   edgl_cand_ce_bwd_form / edgl_shared_ce_bwd_form   edgl_cand_ce_bwd / edgl_shared_ce_bwd with dv = g coef[r] dl_r/dv of `form`;
 *                             row_aux stands where row_lse went (EDGL_LOSS_SOFTMAX: it IS row_lse, and the call is the one without
 *                             _form, bit for bit).  Everything behind dv — d_rows, the table / bias sums in both modes, dv f32
 *                             [R, N + 1], the zero pad columns of the shared path — is unchanged.
 * edgl_sampled_row_loss: R >= 1, 1 <= S <= 8192, R (S + 8) < 2^31, I > 1, form bce or bpr; the _form calls: the shape rule of their
 * family and 0 <= form <= 2; anything else is EDGL_ERR_SHAPE with the bound in the text, before any launch. */
#define EDGL_LOSS_SOFTMAX 0
#define EDGL_LOSS_BCE 1
#define EDGL_LOSS_BPR 2
int edgl_sampled_row_loss(const float* vals, const float* label_val, const int64_t* labels, const int32_t* nvalid, int R, int S, int I,
                          int form, float* row_loss, float* row_aux, float* row_scale, void* stream);
int edgl_sampled_loss_finish(const float* row_loss, const float* row_scale, const int64_t* labels, const int32_t* nvalid, int R, int I,
                             float* loss_out, float* coef, void* stream);
int edgl_cand_ce_bwd_form(const void* rows, const void* table, const float* out_bias, const int32_t* cand, const int64_t* labels,
                          const float* vals, const float* row_aux, const float* coef, const float* gscale, int R, int C, int I, int N,
                          void* d_rows, float* dv, float* d_table, float* d_bias, int form, int dtype, void* stream);
int edgl_shared_ce_bwd_form(const void* rows, const void* table, const int32_t* shared, const int64_t* labels, const float* vals,
                            const float* label_val, const float* row_aux, const float* coef, const float* gscale, const int32_t* nvalid,
                            int R, int C, int I, int S, void* d_rows, float* d_table, float* d_bias, float* workspace, int64_t* keys,
                            void* plan, int form, int dtype, void* stream);

/* ---- K5, "flash" form (used by the static training engine): the forward scoring pass already accumulates the row
 * gradients, so the [R, I] logits are computed twice per step instead of three times.
 * edgl_score_flash_fwd: one pass over the item rows [i0, i1) gives row_lse (as edgl_score_lse_fwd), label_logit, and keeps
 * sum_z exp(logit_z - max) table[z] per weighted row (flash-style running maxima) in `workspace`.
 * edgl_score_flash_bwd: d_rows = gscale * coef * (that sum / row sum - table[label]) — i.e. dl . table with
 * dl = coef (softmax - onehot), SURVEY Appendix C — then d_table / d_bias exactly as edgl_score_ce_bwd.  `workspace`:
 * edgl_score_flash_workspace floats, untouched between the two calls.  Other arguments as edgl_score_lse_fwd /
 * edgl_score_ce_bwd (EasyDGL.py:149-155,177-185).
 * Item ranges (the item table row-sharded over ranks; i0 a multiple of 8): edgl_score_flash_fwd over [i0, i1) gives the
 * log-sum-exp of the RANGE's logits (the pad item's -1000 only where the range holds item 0) and label_logit where i0 <= label < i1;
 * edgl_score_flash_bwd over the same range takes the GLOBAL row_lse / coef (merged over the ranges by the caller) and returns the
 * range's share of d_rows — its label row subtracted only by the range that owns the label — and writes rows [i0, i1) of d_table /
 * entries [max(i0,1) - 1, i1 - 1) of d_bias, nothing else: the shares add up to the unsharded result (tests/test_gpu_score_strip.py). */
long edgl_score_flash_workspace(int R, int C, int I, int n_items, int dtype);
int edgl_score_flash_fwd(const void* rows, const void* table, const float* out_bias, const int64_t* labels, int R, int C,
                         int I, int i0, int i1, const int32_t* nvalid, float* row_lse, float* label_logit,
                         float* workspace, int dtype, void* stream);
/* f32: the transposed operand image of the item table depends on the weights only: edgl_score_prepare_table writes it into
 * the flash workspace ahead of the forward (same R, C, I, [i0, i1), workspace, dtype), and edgl_score_flash_fwd_pre with
 * table_ready != 0 skips it (table_ready == 0: identical to edgl_score_flash_fwd).  bf16 needs no such image:
 * edgl_score_prepare_table returns at once and table_ready is ignored. */
int edgl_score_prepare_table(const void* table, int R, int C, int I, int i0, int i1, float* workspace, int dtype, void* stream);
int edgl_score_flash_fwd_pre(const void* rows, const void* table, const float* out_bias, const int64_t* labels, int R, int C,
                             int I, int i0, int i1, const int32_t* nvalid, float* row_lse, float* label_logit,
                             float* workspace, int table_ready, int dtype, void* stream);
/* edgl_score_flash_fwd over the whole table for COMPACTED rows (edgl_compact_*: the *nvalid weighted rows first, labels 0 behind)
 * that also writes the loss coefficients coef[r] = (1 / (n + 1e-5)) * p_y / (p_y + 1e-5), n = *nvalid — exactly what
 * edgl_ce_loss_fwd computes after its reduction over the rows (EasyDGL.py:177-185); the backward then does not wait for the loss
 * kernel, which may be given coef = NULL. */
int edgl_score_flash_fwd_coef(const void* rows, const void* table, const float* out_bias, const int64_t* labels, int R, int C,
                              int I, const int32_t* nvalid, float* row_lse, float* label_logit, float* coef, float* workspace,
                              int dtype, void* stream);
/* Data-parallel form: `wtotal` (device int32, may be NULL = the local count) is the number of weighted rows of the
 * GLOBAL batch — the denominator of EasyDGL.py:183-185 summed over the ranks — so that the ranks' gradients add up to the gradient
 * of the global-batch loss. */
int edgl_score_flash_fwd_coef_w(const void* rows, const void* table, const float* out_bias, const int64_t* labels, int R, int C,
                                int I, const int32_t* nvalid, const int32_t* wtotal, float* row_lse, float* label_logit, float* coef,
                                float* workspace, int dtype, void* stream);
/* ... that also finishes the rows: d_rows [R, C] `dtype` (= gscale * d loss / d rows; gscale device scalar or NULL = 1) is written by
 * the launch that forms lse / label logits / coefficients (one kernel instead of two between the two product passes);
 * edgl_score_flash_bwd is then called with d_rows = NULL and computes d_table / d_bias only. */
int edgl_score_flash_fwd_rows_w(const void* rows, const void* table, const float* out_bias, const int64_t* labels, int R, int C,
                                int I, const int32_t* nvalid, const int32_t* wtotal, const float* gscale, float* row_lse,
                                float* label_logit, float* coef, void* d_rows, float* workspace, int dtype, void* stream);
/* edgl_score_flash_fwd_rows_w that also leaves the loss numerator — sum over the weighted rows of -log(p_label + 1e-5),
 * EasyDGL.py:181-185 — as edgl_score_ce_nparts(R, C) per-workgroup sums in ce_part, the weighted-row count behind them (nparts + 1
 * floats; 0 parts: this width has no one-launch row finish; ce_part NULL: none).  edgl_ce_loss_parts forms the loss from them: sum / (weighted rows + 1e-5) + add_in + add_in2; it
 * reads nothing else of the batch, so it may run any time before the next forward rewrites ce_part. */
int edgl_score_ce_nparts(int R, int C);
int edgl_score_flash_fwd_rows_wp(const void* rows, const void* table, const float* out_bias, const int64_t* labels, int R, int C,
                                 int I, const int32_t* nvalid, const int32_t* wtotal, const float* gscale, float* row_lse,
                                 float* label_logit, float* coef, void* d_rows, float* ce_part, float* workspace, int dtype,
                                 void* stream);
int edgl_ce_loss_parts(const float* ce_part, int nparts, float* loss_out, const float* add_in, const float* add_in2,
                       const int32_t* wtotal, void* stream);      /* ce_part: nparts + 1 floats (the weighted-row count rides last) */
int edgl_score_flash_bwd(const void* rows, const void* table, const float* out_bias, const int64_t* labels,
                         const float* row_lse, const float* coef, const float* gscale, int R, int C, int I, int i0,
                         int i1, const int32_t* nvalid, void* d_rows, float* d_table, float* d_bias, float* workspace,
                         int dtype, void* stream);
/* The one-hot part of dl = coef (p - onehot(label)) as a call of its own: d_table[label[r]] -= gscale coef[r] rows[r], d_bias[label[r]-1]
 * -= gscale coef[r] over the weighted rows (f32 atomics: commutes with every other accumulation into the two arrays).
 * edgl_score_flash_bwd_ex(defer_label_term = 1) leaves exactly this out where its product pass does not contain it (bf16, C = 128 / 256 / 512: the strip kernels);
 * edgl_score_flash_label_term then applies it — and is a no-op for every other configuration.  A training loop may run it off the
 * critical path (any time after the table-side reduction of edgl_score_flash_bwd_ex wrote d_table / d_bias).
 * Bit 1 (value 2) of defer_label_term, the form that adds the row chunks into a zero-filled d_table / d_bias with f32 atomics, is no
 * longer used by the training engine. */
int edgl_score_flash_bwd_ex(const void* rows, const void* table, const float* out_bias, const int64_t* labels,
                            const float* row_lse, const float* coef, const float* gscale, int R, int C, int I, int i0,
                            int i1, const int32_t* nvalid, void* d_rows, float* d_table, float* d_bias, float* workspace,
                            int defer_label_term, int dtype, void* stream);
int edgl_score_flash_label_term(const void* rows, const int64_t* labels, const float* coef, const float* gscale, int R, int C, int I,
                                int i0, int i1, const int32_t* nvalid, float* d_table, float* d_bias, int dtype, void* stream);
/* The same term without f32 atomics (deterministic mode): an ordered sum over a plan of the labels, built by the call in `plan`
 * (edgl_segsum_plan_bytes of (R, I) bytes) — same contract, same no-op where the product pass already contains the one-hot term. */
int edgl_score_flash_label_term_det(const void* rows, const int64_t* labels, const float* coef, const float* gscale, int R, int C,
                                    int I, int i0, int i1, const int32_t* nvalid, float* d_table, float* d_bias, void* plan, int dtype,
                                    void* stream);

/* ---- deferred partial reductions ------------------------------------------------------------------
 * The weight-gradient entry points (edgl_gemm_dw, edgl_add_layernorm_bwd, edgl_encode_bwd,
 * edgl_bimau_bwd, edgl_colsum) finish with a small fixed-order reduction of per-workgroup partials.
 * After edgl_reduce_defer(1, stream) those reductions are queued on the calling host thread instead
 * of launched, and edgl_reduce_flush(stream) (or edgl_reduce_defer(0, stream)) runs all of them in
 * one launch.  While deferred, every call must be given its OWN workspace, kept until the flush,
 * and the gradient outputs are not valid before it.  Accumulating calls flush and run immediately.
 * edgl_reduce_defer(-1, stream) is the error exit: it drops the queued jobs WITHOUT launching them and
 * leaves deferred mode (a caller whose launch sequence failed half-way must not leave the thread deferred). */
int edgl_reduce_defer(int on, void* stream);
int edgl_reduce_flush(void* stream);
/* The reduction of one set of partials by itself: out[n] (+)= sum over p < P of part[p * ld + n], fixed order — launched at once, or
 * queued in deferred mode (accumulate = 0), exactly as the entry points above do with their own partials. */
int edgl_reduce_partials(const float* part, int P, int N, long ld, float* out, int accumulate, void* stream);
/* edgl_reduce_ride(1) (2: behind instead of in front of the scatter's workgroups), in deferred mode: the next edgl_encode_bwd* call
 * of this thread that launches the MFMA scatter kernel (bf16, C = 64 / 128; not edgl_encode_bwd_add_det) takes the queued jobs,
 * its own two included, into that launch as extra workgroups and leaves the queue empty — same sums, bit for bit, no reduction
 * launch.  The jobs must not depend on the scatter: a list with a job outside the vector form (N, ld multiples of 4, 16-byte
 * aligned pointers) or with an output inside d_item [I * C] / d_bias [I - 1] does not ride and stays queued for the flush.
 * edgl_reduce_ride(0), or leaving deferred mode, withdraws the request. */
int edgl_reduce_ride(int on);

/* ---- K8: TPP likelihood regulariser — temporal.py:317-333 + EasyDGL.py:157-175 -----------------
 * lam f32 [H*B,T,E]; masked_pos int64 [B,M]; labels int64 [B,M]; ts_raw f32 [B,T] (raw seconds);
 * mark_table uint8 [NI,E].  reg_out f32[1] (+)= coef * biased_mle with coef = ct_reg/H;
 * sums f32[edgl_tpp_workspace()] scratch (sums[0..2] = event-ll, non-event, #marks are reused by
 * the backward).  bwd zero-fills and writes d_lam f32 [H*B,T,E] (zero except at masked positions), scaled by
 * the device scalar gscale (NULL = 1).
 * masked_pos == NULL selects the all-position form of CTSMA.train (CTSMA.py:95-108): M == T, labels [B,T] (next
 * items), ts_raw f32 [B,T+1] and the interval of position t is ts[t+1]-ts[t] (raw, unclipped). */
int edgl_tpp_workspace(void);
int edgl_tpp_fwd(const float* lam, const int64_t* masked_pos, const int64_t* labels, const float* ts_raw,
                 const uint8_t* mark_table, int B, int T, int H, int E, int M, float coef, float* sums,
                 float* reg_out, int accumulate, void* stream);
int edgl_tpp_bwd(const float* lam, const int64_t* masked_pos, const int64_t* labels, const float* ts_raw,
                 const uint8_t* mark_table, int B, int T, int H, int E, int M, float coef,
                 const float* sums, const float* gscale, float* d_lam, void* stream);
/* edgl_tpp_fwd + edgl_tpp_bwd as one call (three small launches instead of four + a memset): reg_out (+)= regulariser, sums[0..2] as edgl_tpp_fwd, and (d_lam != NULL) the
 * FULL gradient d_lam[H*B*T, E] — zero rows where the position is not masked (no memset needed), contributions of repeated
 * masked positions summed.  sums: edgl_tpp_workspace() floats; sums[4] must be zero before the first call (integer normaliser
 * accumulator; left zero). */
int edgl_tpp_fwd_bwd(const float* lam, const int64_t* masked_pos, const int64_t* labels, const float* ts_raw,
                     const uint8_t* mark_table, int B, int T, int H, int E, int M, float coef, float* sums,
                     float* reg_out, int accumulate, float* d_lam, void* stream);
/* The normaliser alone (labels only; integer sum into sums[4]) and edgl_tpp_fwd_bwd with it optional (with_norm == 0: edgl_tpp_norm
 * already ran for this batch on the same `sums`). */
int edgl_tpp_norm(const int64_t* labels, const uint8_t* mark_table, int B, int M, int E, float* sums, void* stream);
int edgl_tpp_fwd_bwd_ex(const float* lam, const int64_t* masked_pos, const int64_t* labels, const float* ts_raw,
                        const uint8_t* mark_table, int B, int T, int H, int E, int M, float coef, float* sums,
                        float* reg_out, int accumulate, float* d_lam, int with_norm, void* stream);
/* edgl_tpp_fwd_bwd_ex(with_norm = 0) for a d_lam array that ALREADY HOLDS ZEROS (edgl_bimau_fwd_zr): one thread per masked slot,
 * only the rows of masked positions are written (repeated positions: once, summed).  sums: max(edgl_tpp_workspace(),
 * edgl_tpp_rows_workspace(B, H, M)) floats; edgl_tpp_norm must have run on the same `sums`. */
long edgl_tpp_rows_workspace(int B, int H, int M);
int edgl_tpp_fwd_bwd_rows(const float* lam, const int64_t* masked_pos, const int64_t* labels, const float* ts_raw,
                          const uint8_t* mark_table, int B, int T, int H, int E, int M, float coef, float* sums,
                          float* reg_out, int accumulate, float* d_lam, void* stream);   /* E <= 256 (E > 16: plain loops over the marks) */

/* Fused TPP form (bf16, head dim 16, E = 16, T <= 128, M <= 256): the regulariser of MAU.biased_likelihood (temporal.py:317-333)
 * evaluated at the masked positions (EasyDGL.py:157-175) INSIDE sweep 1 of the attention backward, which holds lambda in registers —
 * no [H*B,T,E] d lambda array and no TPP launch between the attention forward and the block tail (the forward runs as
 * edgl_bimau_fwd_db with zero_rows = NULL).
 *   edgl_tpp_prep         slot data of a batch (labels / positions / raw timestamps only, runs ahead of the forward): per position
 *                         the next-mark bytes of its first effective slot (a slot whose label's mark row is not empty:
 *                         temporal.py:321) and the raw span (EasyDGL.py:161-162), further effective slots of a taken position
 *                         in a per-sample overflow list, and the marks of all labels of a sample (their total is the regulariser's
 *                         normaliser, temporal.py:330); desc = edgl_tpp_prep_bytes(B, T, M) bytes, 16-byte aligned.
 *   edgl_bimau_bwd_tpp    edgl_bimau_bwd_db with the regulariser's d lambda (coef = ct_reg / H; count: tpp_sums[4] as edgl_tpp_norm or a
 *                         data-parallel all-reduce left it, tpp_sums == NULL: the total of the slot data's per-sample counts)
 *                         computed by sweep 1 from the slot data, and the two loss sums of the wave's (b, head) in tpp_part f32
 *                         [B*H + 1, 2] — the last pair's first word = the count it used (int32)
 *   edgl_tpp_finish_parts their reduction: reg_out (+)= coef * (-(sum log ev - sum non-event) / (count * H)); sums as edgl_tpp_fwd_bwd
 *                         (count: tpp_desc != NULL — from the slot data (B, T, M), also stored into sums[4]; NULL — sums[4] as given)
 *   edgl_tpp_finish_parts_n  the same with the count edgl_bimau_bwd_tpp left behind the sums (part [nparts + 1, 2]): it reads nothing
 *                         of the batch, a training loop may launch it any time before the next edgl_bimau_bwd_tpp on that array */
/* data parallel: counts[0] = labels != 0, counts[1] = marks of all labels — the two normalisers a step all-reduces (B * M <= 65536) */
int edgl_dp_counts(const int64_t* labels, const uint8_t* mark_table, int B, int M, int E, int32_t* counts, void* stream);
long edgl_tpp_prep_bytes(int B, int T, int M);
int edgl_tpp_prep(const int64_t* masked_pos, const int64_t* labels, const float* ts_raw, const uint8_t* mark_table, int B, int T,
                  int E, int M, void* desc, void* stream);
int edgl_bimau_bwd_tpp(const void* qkvt, const int64_t* ids, const float* spans, const uint8_t* marks, const void* pack,
                       const void* d_out, const void* tpp_desc, int M, const float* tpp_sums, float coef, float* tpp_part,
                       const float* lam, const void* saved, int B, int T, int C, int H, int E, float drop_rate,
                       const uint64_t* rng_state, uint32_t stream_id, const uint32_t* dropbits, float qk_scale, void* d_qkvt, float* dW1,
                       float* db1, float* dw, float* dscaling, void* workspace, int flags, int dtype, void* stream);
int edgl_tpp_finish_parts(const float* part, int nparts, float coef, int H, const void* tpp_desc, int B, int T, int M, float* sums,
                          float* reg_out, int accumulate, void* stream);
int edgl_tpp_finish_parts_n(const float* part, int nparts, float coef, int H, float* sums, float* reg_out, int accumulate, void* stream);

/* ---- optimizer — tf.train.AdamOptimizer (Base.py:142-144) over a flat f32 arena ----------------
 * step_state: device uint64[2]: [0] = step count (incremented by this call, so the first call is
 * t = 1), [1] = scratch holding lr_t = lr*sqrt(1-b2^t)/(1-b1^t).  theta -= lr_t * m/(sqrt(v)+eps).
 * l2 (coding.py:34-40) enters as grad += l2 * w on the element ranges [seg[2s], seg[2s+1]) (device
 * int64 pairs).  If shadow != NULL the updated weights are also written there as bf16. */
int edgl_adam_step(float* param, const float* grad, float* m, float* v, long n, float lr, float beta1,
                   float beta2, float eps, uint64_t* step_state, float l2, const int64_t* seg, int nseg,
                   void* shadow, void* stream);
/* Training-step form of the two state updates: edgl_step_begin = edgl_rng_advance + the step / learning-rate half of
 * edgl_adam_step in ONE single-thread launch at the start of the step; edgl_adam_apply = the parameter-update half (reads
 * the learning rate edgl_step_begin left in step_state). */
int edgl_step_begin(uint64_t* rng_state, uint64_t* adam_state, float lr, float beta1, float beta2, void* stream);
int edgl_adam_apply(float* param, const float* grad, float* m, float* v, long n, float beta1, float beta2, float eps,
                    const uint64_t* step_state, float l2, const int64_t* seg, int nseg, void* shadow, void* stream);
/* l2 part of the loss: out[0] (+)= 0.5*l2*sum(w[seg]^2)  (EasyDGL.py:158); workspace >= 1024 floats. */
/* edgl_adam_apply that also leaves the per-block sums of squares of the UPDATED parameters inside the l2 segments in l2_part
 * (edgl_adam_l2_parts(n) floats): the next step's L2 loss term (coding.py:40) is then edgl_l2_from_parts(l2_part, nparts, l2_reg, ...)
 * = l2_reg / 2 * sum — one tiny launch that reads nothing of the parameter arena. */
int edgl_adam_l2_parts(long n);
int edgl_adam_apply_l2p(float* param, const float* grad, float* m, float* v, long n, float beta1, float beta2, float eps,
                        const uint64_t* step_state, float l2, const int64_t* seg, int nseg, void* shadow, float* l2_part, void* stream);
/* The eager engine's optimizer launch: edgl_adam_apply_l2p that also (a) adds the sum of `nslab` partial-gradient slabs to two ranges of
 * the gradient arena — grad[lo .. hi) += sum_s slabs[s * stride + (i - lo)]; the first `zero_first_a` elements of range a take none (row 0
 * of the used item table is the zero constant, coding.py:56-57): the row-chunk slabs that edgl_score_flash_bwd_ex(defer_label_term & 4)
 * leaves in its workspace (edgl_score_flash_slab_info), so that no slab-reduction launch stands between the scoring and the block-tail
 * backward — and (b) writes the counters of the NEXT step (edgl_step_begin's update: dropout step + 1, Adam step + 1, its bias-corrected
 * learning rate) into step_next / rng_next, buffers OTHER than step_state / rng_cur, which the launch reads: no single-thread launch at
 * the end of a step and no last-workgroup ticket; the caller swaps the buffer pairs behind the launch.  With slabs given, the two ranges
 * of `grad` are ZEROED behind their use: the next step's embedding scatter / one-hot term add into them (no zero-fill launch).  slabs_* / the three counter
 * pointers may be NULL (then that part is left out); l2_part may be NULL.  A non-NULL slabs_a or slabs_b needs nslab >= 1
 * (EDGL_ERR_SHAPE otherwise).  Base.py:142-144. */
int edgl_adam_apply_ex(float* param, float* grad, float* m, float* v, long n, float beta1, float beta2, float eps,
                       const uint64_t* step_state, float l2, const int64_t* seg, int nseg, void* shadow, float* l2_part,
                       const float* slabs_a, long stride_a, long lo_a, long hi_a, long zero_first_a,
                       const float* slabs_b, long stride_b, long lo_b, long hi_b, int nslab,
                       const uint64_t* rng_cur, uint64_t* step_next, uint64_t* rng_next, float lr, void* stream);
/* Lazy row-wise Adam for the item table of sampled-softmax training (k_adam_rows.hip; TensorFlow's LazyAdamOptimizer):
 * edgl_adam_apply's update on the TOUCHED rows of table f32 [I, C] and on no other.  Row i in [1, I) is touched when it occurs in
 * ids (int64 [n_ids]: the batch's input ids; NULL with n_ids = 0), or is labels[r] (int64 [R]) of a row with 1 <= labels[r] < I, or
 * is cand[r, n] (int32 [R, N]; NULL with N = 0) of such a row; ids <= 0 or >= I are skipped, the list of a row of weight 0 touches
 * nothing, row 0 is never touched — a function of the integer inputs alone.  A touched row is updated exactly ONCE however often it
 * is listed: g' = g + l2 w, m = b1 m + (1 - b1) g', v = b2 v + (1 - b2) g'^2, w -= lr_t m / (sqrt(v) + eps) with lr_t read from
 * step_state as edgl_adam_apply reads it (the caller has advanced the step: edgl_adam_step / edgl_step_begin), shadow (bf16 [I, C] or
 * NULL) = bf16(w), and its row of grad is written back as ZEROS; an untouched row keeps every bit of w, m, v, shadow and grad.
 * stamp: int32 [I], caller-owned, zero before the first call (and again whenever the step count is set back): the step count is
 * raised into stamp[id] with one returning integer atomic per entry and the entry that raised it owns the row.  No float atomics,
 * no sort, no read-back.  f32 masters, C % 4 == 0, 4 <= C <= 512, I > 1, R (N + 1) < 2^31, arrays 16-byte aligned; anything else is
 * EDGL_ERR_SHAPE, checked before any pointer is read.  Base.py:142-144 on the rows of the step. */
int edgl_adam_rows(float* table, float* grad, float* m, float* v, void* shadow, int I, int C, const int64_t* ids, long n_ids,
                   const int64_t* labels, const int32_t* cand, int R, int N, int32_t* stamp, float beta1, float beta2, float eps,
                   const uint64_t* step_state, float l2, void* stream);
/* out[0] / out[1]: float offsets of the d_table [nslab][I * C] / d_bias [nslab][I - 1] slabs inside the edgl_score_flash_workspace
 * buffer, out[2] = nslab — what edgl_score_flash_bwd_ex leaves there with (defer_label_term & 4) (requires & 1, the whole item range
 * and gscale == NULL; otherwise the flag is ignored and the slabs are reduced as usual).  EasyDGL.py:149-151 backward. */
int edgl_score_flash_slab_info(int R, int C, int I, int n_items, int dtype, long* out);
int edgl_l2_from_parts(const float* l2_part, int nparts, float l2, float* out, int accumulate, void* stream);
int edgl_l2_loss(const float* param, const int64_t* seg, int nseg, float l2, float* out, int accumulate,
                 float* workspace, void* stream);
/* element-wise helpers on `dtype` buffers */
int edgl_cast(const float* src, void* dst, long n, int dtype, void* stream);                 /* dst = (dtype)src      */
int edgl_cast_back(const void* src, float* dst, long n, int accumulate, int dtype, void* stream); /* dst (+)= (f32)src */
int edgl_add(const void* a, const void* b, void* out, long n, int dtype, void* stream);      /* out = a + b           */
/* y = x * keep / (1 - rate) with the counter-based keep mask of (rng_state, stream_id, element index): tf.layers.dropout
 * (Base.py:80,83); calling it on dy with the same arguments is the backward. */
int edgl_dropout(const void* x, void* y, long n, float drop_rate, const uint64_t* rng_state, uint32_t stream_id, int dtype,
                 void* stream);
/* FeedForward tail in one pass (Base.py:83-86, then `seqs_outs *= seqs_masks`, TGAT.py:70 / TiSASREC.py:73):
 * out[r,:] = (dropout(a[r,:]) + b[r,:]) * (ids[r] != 0); b and ids may be NULL (no residual / no row mask).  The dropout
 * mask is the one edgl_dropout draws for the same (rng_state, stream_id, element index).  Backward of the `a` branch:
 * the same call on the upstream gradient with b == NULL; of the `b` branch: edgl_mask_rows. */
int edgl_ff_tail(const void* a, const void* b, const int64_t* ids, long rows, int C, float drop_rate,
                 const uint64_t* rng_state, uint32_t stream_id, void* out, int dtype, void* stream);
int edgl_relu_bwd(const void* dy, const void* y, void* dz, long n, int dtype, void* stream);   /* dz = dy*[y>0] (Base.py:73) */
int edgl_gelu_bwd(const void* dy, const void* pre, void* dz, long n, int dtype, void* stream); /* dz = dy*gelu'(pre), EasyDGL.py:19-32 */
int edgl_add_cols(void* dst, int ld_dst, const void* src, const void* src2, int ld_src, long rows, int ncols,
                  int dtype, void* stream);                                                             /* dst[:, :n] += src[:, :n] (+ src2[:, :n] if not NULL; same ld_src) */

/* ---- K11: causal attention with a time feature map (config 5: TGAT) ---------------------------------
 * Replaces TfMultiHeadAttention.__call__ (src/module/temporal.py:126-184) after its three dense layers, with
 * TimeFunctionCoding.code (src/module/coding.py:104-122) folded into the operands.
 *
 * edgl_timefn_fwd: q [B,T,C] (row stride ldq), k [B,T,C] (ldk), pos_tab f32 [T,C] (pcoding_K), ts f32 [B,T+1] raw seconds
 * (RegressivePostProcessor layout, dataloader.py:95-108), omega/phi f32 [C] (basis_freq, phase) ->
 *   qx [B,T,H,3*dh] = [ Q | Q*cos(a w + phi) | Q*sin(a w + phi) ],  kx [B,T,H,3*dh] = [ K + pos | cos(b w) | sin(b w) ]
 * with a[t] = ts[t+1]/time_scale - base, b[t] = ts[t]/time_scale - base, base = ts[T]/time_scale, so that
 *   qx[q] . kx[k] = sum_d Q[q,d] (K[k,d] + pos[k,d] + cos((ts'[q+1]-ts'[k]) w_d + phi_d))       (temporal.py:143-148)
 * which is the reference's score wherever its max(.,0) clamp (TGAT.py:54) is inactive: every unmasked (k <= q) pair of a
 * sequence with non-decreasing timestamps.  *violations (int32, device) += number of unpadded positions t with
 * ts[t+1] < ts[t]; the caller must treat a non-zero count as an input error.
 * edgl_timefn_bwd: d_qx, d_kx -> d_q (ld_dq), d_k (ld_dk; this is also d(pos_tab) before the sum over the batch),
 * d_omega, d_phi f32 [C] (overwritten).  workspace >= edgl_timefn_bwd_workspace(C) floats.
 *
 * edgl_tattn_fwd: generic masked attention per (sample, head): S = scale * qx_h . kx_h^T with head slices
 * qx[:, :, h*Dq:(h+1)*Dq] (same for kx; v and out use Dv); scores of padded keys (ids == 0) and, with EDGL_TATTN_CAUSAL,
 * of keys k > q are REPLACED by float32(-2^32+1) (temporal.py:153-166: a fully masked row is uniform over all T keys);
 * P = softmax(S); out = dropout(P) . v_h + resid (temporal.py:169-181).  Dv in {16,32,64,128}, Dq in {Dv, 3*Dv}.
 * saved (NULL for inference): edgl_tattn_saved_bytes bytes = row max / sum / dO.O [H*B*T] f32 each + O before the
 * residual [B,T,H*Dv] f32.  edgl_tattn_bwd (Dq in {Dv, 3*Dv}): d_out -> d_qx, d_kx, d_v (the residual gradient is d_out
 * itself); no gradient flows into a replaced score. */
#define EDGL_TATTN_CAUSAL 1
long edgl_tattn_saved_bytes(int B, int T, int H, int Dv);
int edgl_tattn_fwd(const void* qx, int ldq, const void* kx, int ldk, const void* v, int ldv, const void* resid, int ldr,
                   const int64_t* ids, int B, int T, int H, int Dq, int Dv, float scale, float drop_rate,
                   const uint64_t* rng_state, uint32_t stream_id, void* out, int ldo, void* saved, int flags, int dtype,
                   void* stream);
int edgl_tattn_bwd(const void* qx, int ldq, const void* kx, int ldk, const void* v, int ldv, const int64_t* ids,
                   const void* d_out, int ld_do, void* saved, int B, int T, int H, int Dq, int Dv, float scale,
                   float drop_rate, const uint64_t* rng_state, uint32_t stream_id, void* d_qx, int ld_dq, void* d_kx,
                   int ld_dk, void* d_v, int ld_dv, int flags, int dtype, void* stream);
int edgl_timefn_fwd(const void* q, int ldq, const void* k, int ldk, const float* pos_tab, const float* ts,
                    const int64_t* ids, const float* omega, const float* phi, int B, int T, int C, int H,
                    float time_scale, void* qx, void* kx, int* violations, int dtype, void* stream);
long edgl_timefn_bwd_workspace(int C);
int edgl_timefn_bwd(const void* q, int ldq, const float* ts, const float* omega, const float* phi, const void* d_qx,
                    const void* d_kx, int B, int T, int C, int H, float time_scale, void* d_q, int ld_dq, void* d_k,
                    int ld_dk, float* d_omega, float* d_phi, float* workspace, int dtype, void* stream);
/* y = x * (ids != 0) per row: `seqs_outs *= seqs_masks` (TGAT.py:58,70; TiSASREC.py:73); its own backward. */
int edgl_mask_rows(const void* x, const int64_t* ids, void* y, long rows, int C, int dtype, void* stream);

/* ---- K11b: causal attention with interval buckets (config 5: TiSASRec) ------------------------------
 * Replaces TiMultiHeadAttention.__call__ (src/module/temporal.py:36-105) after its three dense layers.
 * q [B,T,H*dh] (ldq); k, v = K + pcoding_K[t], V + pcoding_V[t] (edgl_add_pos2; temporal.py:50-51,57,94), strides ldk, ldv;
 * ts f32 [B,T+1] raw seconds; ktime, vtime [tab_rows, H*dh] in `dtype` (tcoding_K / tcoding_V tables, head slice
 * h*dh..); bucket(q,k) = int(clip(ts[q+1]/time_scale - ts[k]/time_scale, 0, timelen)) (TiSASREC.py:58-62), a bucket
 * >= tab_rows reads a zero row (the GPU embedding lookup of the reference for the index `timelen` of a [timelen, C]
 * table).  S[q,k] = scale * (q.k + q.ktime[bucket]); masks and softmax as edgl_tattn_fwd; out = dropout(P) . (v +
 * vtime[bucket]) + resid.  The query mask of temporal.py:84-88 is the identity for LayerNorm-ed queries and is not
 * applied.  T <= 256.  saved: edgl_tattn_saved_bytes(B,T,H,dh) bytes; wbuf: edgl_tiattn_bucket_elems elements of `dtype` (binned
 * probabilities, read by the backward); both NULL for inference.  timelen <= 256.
 * edgl_tiattn_bwd: d_q, d_k, d_v; d_ktime, d_vtime f32 [tab_rows, H*dh] (overwritten); dgbuf: workspace like wbuf
 * (binned score gradients).
 * flags: EDGL_TATTN_CAUSAL, and EDGL_TATTN_ORDERED: the forward and the query sweep of the backward fill their
 * per-query interval bins in a fixed order (ascending key) with plain loads and stores instead of f32 atomics — out, wbuf, dgbuf
 * and d_q are then the same bits in every call.
 * edgl_tiattn_bwd_det: edgl_tiattn_bwd with the ordered query sweep and the interval-table gradients without atomics: every
 * row split stores its partial tile to its own slab of `workspace` (edgl_tiattn_det_workspace floats, 16-byte aligned, as
 * d_ktime and d_vtime), one more launch adds the slabs in split order.  The size query is a host function; -1 for bad shapes. */
#define EDGL_TATTN_ORDERED 2
long edgl_tiattn_det_workspace(int H, int dh, int timelen);
int edgl_tiattn_bwd_det(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const int64_t* ids,
                        const float* ts, const void* ktime, const void* vtime, int tab_rows, const void* d_out, int ld_do,
                        void* saved, void* wbuf, int B, int T, int H, int dh, float scale, float time_scale, int timelen,
                        float drop_rate, const uint64_t* rng_state, uint32_t stream_id, void* d_q, int ld_dq, void* d_k,
                        int ld_dk, void* d_v, int ld_dv, void* dgbuf, float* d_ktime, float* d_vtime, float* workspace,
                        int flags, int dtype, void* stream);
long edgl_tiattn_bucket_elems(int B, int T, int H, int timelen);
int edgl_tiattn_fwd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* resid, int ldr,
                    const int64_t* ids, const float* ts, const void* ktime, const void* vtime, int tab_rows, int B, int T,
                    int H, int dh, float scale, float time_scale, int timelen, float drop_rate, const uint64_t* rng_state,
                    uint32_t stream_id, void* out, int ldo, void* saved, void* wbuf, int flags, int dtype, void* stream);
int edgl_tiattn_bwd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const int64_t* ids,
                    const float* ts, const void* ktime, const void* vtime, int tab_rows, const void* d_out, int ld_do,
                    void* saved, void* wbuf, int B, int T, int H, int dh, float scale, float time_scale, int timelen,
                    float drop_rate, const uint64_t* rng_state, uint32_t stream_id, void* d_q, int ld_dq, void* d_k,
                    int ld_dk, void* d_v, int ld_dv, void* dgbuf, float* d_ktime, float* d_vtime, int flags, int dtype,
                    void* stream);
/* out[b,t,:] = kv[b,t,:] + concat(posK[t], posV[t]); kv, out [B,T,2C] `dtype`, posK/posV f32 [>=T, C]. */
int edgl_add_pos2(const void* kv, const float* posK, const float* posV, int B, int T, int C, void* out, int dtype,
                  void* stream);

/* ---- operator-level forms of src/module/coding.py (the classes' own __call__ / code methods) ------
 * The model kernels fuse these (edgl_encode_fwd, edgl_embed_pos_fwd, edgl_timefn_fwd, edgl_tiattn_fwd); the entry
 * points below are what `C.Embedding(...)(ids)`, `C.PositionCoding(...).code(x)`, `C.TimeIntervalCoding(...).code(x)`,
 * `C.TimeSinusoidCoding(C).code(x)` and `C.TimeFunctionCoding(C).code(x)` bind to when called on their own.
 * edgl_embedding_fwd — Embedding.__call__, coding.py:60-64: out[r,:] = scale * table[ids[r],:] over n flat indices;
 *   table [rows, C] in `dtype`; zero_pad != 0: row 0 acts as a zero constant (coding.py:56-57); an index outside
 *   [0, rows) reads zeros (tf.nn.embedding_lookup on the GPU).  scale = sqrt(num_units) or 1 (coding.py:62-63).
 *   PositionCoding.code (coding.py:76-79) is this gather on ids = tile(range(T)); TimeIntervalCoding.code
 *   (coding.py:93-94) on the integer intervals.
 * edgl_embedding_bwd: d_table f32 [rows, C] (overwritten) += scale * d_out at the gathered rows.
 * edgl_time_sinusoid — TimeSinusoidCoding.code, coding.py:137-149: x f32 [n]; out[r, 2j] = sin(x[r] / tscale[j]),
 *   out[r, 2j+1] = cos(same); tscale f32 [C/2] = 10000^(2j/C) (coding.py:134).
 * edgl_time_function_fwd — TimeFunctionCoding.code, coding.py:113-122: out[r, c] = cos(x[r] * freq[c] + phase[c]).
 * edgl_time_function_bwd: d_freq, d_phase f32 [C] (overwritten); workspace: edgl_time_function_bwd_workspace(C) floats. */
int edgl_embedding_fwd(const int64_t* ids, long n, const void* table, int rows, int C, int zero_pad, float scale, void* out,
                       int dtype, void* stream);
int edgl_embedding_bwd(const int64_t* ids, long n, const void* d_out, int rows, int C, int zero_pad, float scale,
                       float* d_table, int dtype, void* stream);
/* edgl_embedding_bwd without f32 atomics: ordered sums over a plan of ids built by the call in `plan`
 * (edgl_segsum_plan_bytes of (n, rows + 1) bytes, 16-byte aligned).  zero_pad cuts index 0 off; C % 4 == 0, C <= 512. */
int edgl_embedding_bwd_det(const int64_t* ids, long n, const void* d_out, int rows, int C, int zero_pad, float scale,
                           float* d_table, void* plan, int dtype, void* stream);
int edgl_time_sinusoid(const float* x, long n, const float* tscale, int C, void* out, int dtype, void* stream);
int edgl_time_function_fwd(const float* x, long n, const float* freq, const float* phase, int C, void* out, int dtype,
                           void* stream);
long edgl_time_function_bwd_workspace(int C);
int edgl_time_function_bwd(const float* x, long n, const float* freq, const float* phase, int C, const void* d_out,
                           float* d_freq, float* d_phase, float* workspace, int dtype, void* stream);

/* ---- fused per-sample block tail — EasyDGL.py:110-139 in ONE launch (csrc/k_tail_fwd.hip, csrc/k_tail_bwd.hip) ----------------
 * The reference's LayerNorm is joint over (T, C) per sample (Base.py:12-67), so a workgroup owning a sample runs
 *   ao = att.Wo + bo ; a1 = LN1(dropout(ao) + x_in) ; f = gelu(a1.Wi + bi) ; o = f.Wout + bout ; y = LN2(dropout(o) + a1)
 *   head != 0:  so = gelu(y.Wt + bt) ; hrows[b*M + j] = LN3(so)[masked_pos[b, j]]                     (EasyDGL.py:136-146)
 *               hrow_map (optional, int32 [B*M]): the row goes to hrows[hrow_map[b*M + j]] instead, rows with a negative entry
 *               are dropped — with edgl_compact_scan_labels' `inv` the weighted rows land compacted, no edgl_compact_gather
 * with the activations in LDS between the steps; every intermediate the backward reads is written once:
 * ao, a1, o, y, pre_t, so [B,T,C]; pre_f, f [B,T,2C]; st1/st2/st3 f32 [B,2] = (mean, rstd).  pre_f and pre_t receive
 * gelu'(pre-activation), not the pre-activation: the derivative is all edgl_tail_bwd needs them for, and the forward has the
 * erf at hand (the unfused kernels save the pre-activation itself — do not mix the two paths within a block).  Otherwise the
 * same arithmetic, the same dropout element indices (streams sid1 / sid2) and the same saved tensors as edgl_gemm +
 * edgl_add_layernorm_fwd, which remain the path for every other shape: edgl_tail_supported(T, C, dtype) != 0 iff dtype is EDGL_BF16, C in {64, 128},
 * T <= 112.  att [B,T,C]; xin = the block input's first C channels, row stride ld_x.
 * pack: edgl_tail_pack_elems(C) elements of `dtype` written by edgl_tail_pack from the four [in, out] kernels (compute
 * copies) — their [out][in] images, the MFMA operand layout. */
long edgl_tail_pack_elems(int C);
int edgl_tail_supported(int T, int C, int dtype);
/* Launch form of edgl_tail_fwd / edgl_tail_bwd at C = 128, T <= 101 (same results, bit for bit): 1 (default) = TWO 8-wave
 * workgroups per CU (three unpadded, swizzled LDS images = 80 KB, <= 128 registers: a second independent chain of dependent
 * phases on every CU), 0 = one workgroup per CU (four padded images + an f32 image, 256 registers — the form of every other
 * shape; the backward also where the head gathers more than 112 rows per sample).  variant < 0 only queries.  Returns the
 * previous value.  Initial value: environment EDGL_TAIL2 (unset = 1).  Process-wide, not thread-safe against concurrent
 * launches: a development / A-B switch. */
int edgl_tail_variant(int variant);
int edgl_tail_pack(const void* Wo, const void* Wi, const void* Wout, const void* Wt, int C, void* pack, void* stream);
int edgl_tail_fwd(const void* att, const void* xin, int ld_x, const void* pack, const float* bo, const float* bi,
                  const float* bout, const float* bt, const float* g1, const float* b1, const float* g2,
                  const float* b2, const float* g3, const float* b3, int B, int T, int C, float drop_rate,
                  const uint64_t* rng_state, uint32_t sid1, uint32_t sid2, const int64_t* masked_pos, int M, int head,
                  void* ao, void* a1, float* st1, void* pre_f, void* f, void* o, void* y, float* st2, void* pre_t,
                  void* so, float* st3, void* hrows, const int32_t* hrow_map, int dtype, void* stream);
/* The same for a channel-padded model (head dim dh_true stored as dh_pad, a power of two; padded channels of every operand exactly
 * zero: model/easydgl.py): the three LayerNorms take their joint (T, C) moments over the REAL channels — divisor T * C_true, padded
 * entries left out of the centred second moment — as edgl_add_layernorm_fwd_ct does.  0, 0 = edgl_tail_fwd. */
int edgl_tail_fwd_ct(const void* att, const void* xin, int ld_x, const void* pack, const float* bo, const float* bi,
                     const float* bout, const float* bt, const float* g1, const float* b1, const float* g2,
                     const float* b2, const float* g3, const float* b3, int B, int T, int C, float drop_rate,
                     const uint64_t* rng_state, uint32_t sid1, uint32_t sid2, const int64_t* masked_pos, int M, int head,
                     void* ao, void* a1, float* st1, void* pre_f, void* f, void* o, void* y, float* st2, void* pre_t,
                     void* so, float* st3, void* hrows, const int32_t* hrow_map, int dh_pad, int dh_true, int dtype,
                     void* stream);

/* Backward of the same chain, one launch per block: given the gradient of the gathered head rows (head != 0: d_rows [*, C]
 * compact, masked_pos [B, M], dy_rowmap = the `inv` map of edgl_compact_rows or NULL) or of y (head == 0: d_y_in [B,T,C]),
 * recomputes the three LayerNorm inputs from the saved tensors (pre_f / pre_t as edgl_tail_fwd wrote them: gelu') and writes
 * what the weight-gradient GEMMs consume:
 * d_pre_t, d_o, d_ao [B,T,C] and d_pre_f [B,T,2C] (gradients w.r.t. the four dense outputs), d_res1 (gradient into the LN1
 * residual x_in[:, :, :C]) and d_att (gradient w.r.t. the block-tail input); LayerNorm parameter gradients dg*, db*
 * (overwritten; reduced from per-sample partials in `workspace`, edgl_tail_bwd_workspace(B, C) floats).  Wo, Wi, Wout, Wt: the
 * [in, out] kernels' compute copies (no packed image needed: dX contracts over the output index). */
long edgl_tail_bwd_workspace(int B, int C);
int edgl_tail_bwd(const void* xin, int ld_x, const void* ao, const void* a1, const void* pre_f, const void* o,
                  const void* pre_t, const void* so, const float* st1, const float* st2, const float* st3,
                  const void* Wo, const void* Wi, const void* Wout, const void* Wt, const float* g1, const float* g2,
                  const float* g3, int B, int T, int C, float drop_rate, const uint64_t* rng_state, uint32_t sid1,
                  uint32_t sid2, int head, const void* d_rows, const int64_t* masked_pos, int M,
                  const int32_t* dy_rowmap, const void* d_y_in, void* d_pre_t, void* d_o, void* d_pre_f, void* d_ao,
                  void* d_res1, void* d_att, float* dg1, float* db1, float* dg2, float* db2, float* dg3, float* db3,
                  float* workspace, int dtype, void* stream);
/* ... of a channel-padded model: the LayerNorm backward divides by T * C_true and returns nothing into a padded channel
 * (edgl_add_layernorm_bwd_act_ct's rule), so every gradient tensor keeps exact zeros there. */
int edgl_tail_bwd_ct(const void* xin, int ld_x, const void* ao, const void* a1, const void* pre_f, const void* o,
                     const void* pre_t, const void* so, const float* st1, const float* st2, const float* st3,
                     const void* Wo, const void* Wi, const void* Wout, const void* Wt, const float* g1, const float* g2,
                     const float* g3, int B, int T, int C, float drop_rate, const uint64_t* rng_state, uint32_t sid1,
                     uint32_t sid2, int head, const void* d_rows, const int64_t* masked_pos, int M,
                     const int32_t* dy_rowmap, const void* d_y_in, void* d_pre_t, void* d_o, void* d_pre_f, void* d_ao,
                     void* d_res1, void* d_att, float* dg1, float* db1, float* dg2, float* db2, float* dg3, float* db3,
                     float* workspace, int dh_pad, int dh_true, int dtype, void* stream);

/* ---- GRU sequence recurrence (S2PNM's recurrent layer) -------------------------------------
 * One unidirectional GRU layer in cuDNN's form (gate order r, z, n; linear input; zero initial state; every position is a step):
 *   r = s(xp_r + h R_r + b_Rr)   z = s(xp_z + h R_z + b_Rz)   n = tanh(xp_n + r * (h R_n + b_Rn))   h' = (1 - z) n + z h
 * xp [B,T,3C] `dtype` = x [W_r|W_z|W_n] + b_W (a plain edgl_gemm), R [C,3C] `dtype` (gate blocks as column blocks), b_R f32 [3C].
 * edgl_gru_seq_fwd: h [B,T,C] `dtype`; saved f32 [B,T,5C] = r | z | n | h R_n + b_Rn | h_prev per position (NULL: inference);
 * hprev_c [B,T,C] `dtype` (may be NULL) = the state BEFORE each step, the A operand of dR = H_prev^T dG_h (in f32 mode the
 * h_prev block of `saved` is that operand already, row stride 5C).  `pack`: edgl_gru_seq_pack_bytes(C, dtype) bytes, 16-byte
 * aligned, written by the call (R as MFMA fragments).
 * edgl_gru_seq_bwd: d_h [B,T,C] -> d_xp [B,T,3C] (gradient of xp) and d_gh [B,T,3C] (gradient of h R + b_R: the n block times r);
 * dh is carried in f32; dR = H_prev^T d_gh and db_R = colsum(d_gh) are ONE edgl_gemm_dw over the B*T rows afterwards.
 * One workgroup owns 16 samples for all T steps; no atomics: the same bits in every call.  C a multiple of 16 in [16, 512],
 * B >= 1, T >= 1; anything else is EDGL_ERR_SHAPE before a launch.  edgl_gru_seq_resident: 1 if R stays in LDS for the whole
 * launch at this width (bf16: C <= 128, f32: C <= 80), 0 if it is streamed from L2 every step, -1 for a bad shape. */
long edgl_gru_seq_pack_bytes(int C, int dtype);
int edgl_gru_seq_resident(int C, int dtype);
int edgl_gru_seq_fwd(const void* xp, const void* R, const float* b_R, int B, int T, int C, void* h, float* saved,
                     void* hprev_c, void* pack, int dtype, void* stream);
int edgl_gru_seq_bwd(const void* d_h, const void* R, const float* saved, int B, int T, int C, void* d_xp, void* d_gh,
                     void* pack, int dtype, void* stream);

/* ---- S2PNM's element-wise pieces (S2PNM.py:52-66) and gradient clipping (k_s2pnm.hip) -----------------
 * edgl_cat_pos_mask_fwd: out [B,T,2C] = [h[b,t] | pos[t]] * (ids[b,t] != 0); h `dtype` [B,T,C], pos f32 [>=T, C].
 * edgl_cat_pos_mask_bwd: d_h [B,T,C] = d_out[:, :, :C] * mask; d_pos f32 [T,C] (overwritten) = sum over b, in ascending b, of the
 *   masked d_out[:, :, C:] — one thread per element, no atomics.
 * edgl_dict_feat_fwd: out [rows,4C] = [g, h, g - h, g * h]; edgl_dict_feat_bwd: d_g = d0 + d2 + d3 * h, d_h = d1 - d2 + d3 * g.
 * edgl_sigmoid_fwd: y = 1 / (1 + exp(-x)); edgl_sigmoid_bwd: dx = dy * y * (1 - y).
 * edgl_clip_scale: grad[0..n) *= clip / max(sqrt(sumsq[0]), clip) with sumsq a DEVICE scalar (edgl_l2_loss of the gradient
 *   with l2 = 2): clip_by_global_norm without a host read; the factor is exactly 1 while the norm is below the clip. */
int edgl_cat_pos_mask_fwd(const void* h, const float* pos, const int64_t* ids, int B, int T, int C, void* out, int dtype,
                          void* stream);
int edgl_cat_pos_mask_bwd(const void* d_out, const int64_t* ids, int B, int T, int C, void* d_h, float* d_pos, int dtype,
                          void* stream);
int edgl_dict_feat_fwd(const void* g, const void* h, long rows, int C, void* out, int dtype, void* stream);
int edgl_dict_feat_bwd(const void* g, const void* h, const void* d_feat, long rows, int C, void* d_g, void* d_h, int dtype,
                       void* stream);
int edgl_sigmoid_fwd(const void* x, void* y, long n, int dtype, void* stream);
int edgl_sigmoid_bwd(const void* dy, const void* y, void* dx, long n, int dtype, void* stream);
int edgl_clip_scale(float* grad, long n, const float* sumsq, float clip, void* stream);

/* ---- TimelyREC: multi-aspect time encoder and time-aware history encoder (k_mate.hip, k_tahe.hip) -------------
 * MATE — calendar slots, slot attention and the gated combination (TimelyREC.py:57-77,108-135; sequential.py:220-237) in one op.
 * Granularities month, day, weekday, hour: ranges M = 12, 31, 7, 24, tables E_g [M_g, C] `dtype`, windows W_g = w_month .. w_hour
 * (max(int(M * window_ratio + 0.5), 1) + 1 with window_ratio in (0, 0.5]: 2 <= W_g <= M_g / 2 + 2).
 *   idx int64 [4][B][T]: the calendar index of every position, month - 1 | day - 1 | weekday | hour; an index outside [0, M) reads a
 *     zero row for e (the padding's -1) and enters the window rows by floor-mod M;
 *   u [B,T,4C] = U [Wu_month | Wu_day | Wu_weekday | Wu_hour], pq [B,T,C] = U Wc (plain GEMMs);
 *   cs[s][w] = sum_{s' <= s} E[(f[s'] + w) mod M] + E[(f[s'] - w) mod M], slot_0 = e, slot_w = (e + cs_w) / (2w + 1),
 *   p = softmax_w((e * u) . (slot_w * u) / sqrt(C)), period = sum_w p_w slot_w * u, R = sum_g sigmoid(pq . period_g) period_g.
 * edgl_mate_fwd: R [B,T,C]; saved f32 [B,T,edgl_mate_saved_floats] (NULL: inference) = p of the four granularities, then the four gates.
 * edgl_mate_bwd: d_u [B,T,4C], d_pq [B,T,C] `dtype`; d_tables f32 [74, C] (overwritten): rows 0-11 month, 12-42 day, 43-49 weekday,
 *   50-73 hour.  workspace: edgl_mate_bwd_workspace floats.  The slots are recomputed; the table gradient is accumulated per
 *   workgroup in LDS over 64-channel slices and summed from slabs in a fixed order: no atomics, the same bits in every call.
 * 1 <= T <= 128, C a power of two in [32, 512]; anything else is EDGL_ERR_SHAPE before a launch.
 * TAHE — hist[q] = sum_{k <= q} ((1 + n_q . n_k) / 2) Hs[k], n = l2_normalize(R) (x * rsqrt(max(sum x^2, 1e-12))); R, Hs, hist
 * [B,T,C] `dtype`; same T and C range.  edgl_tahe_bwd: d_R (both operands of the cosine, one gradient) and d_Hs.  No atomics.
 * edgl_tahe_mix_fwd: out [rows,C] = (emb + te_weight[0] * tcode) * (ids != 0); edgl_tahe_mix_bwd: d_emb = d_out * mask and
 *   d_te f32 [1] = sum d_out * tcode over the unmasked rows, from per-workgroup partials (workspace: edgl_tahe_mix_bwd_workspace
 *   floats) in a fixed order. */
int edgl_mate_saved_floats(int w_month, int w_day, int w_weekday, int w_hour);
int edgl_mate_fwd(const int64_t* idx, const void* month_tab, const void* day_tab, const void* weekday_tab, const void* hour_tab,
                  const void* u, const void* pq, int B, int T, int C, int w_month, int w_day, int w_weekday, int w_hour, void* R,
                  float* saved, int dtype, void* stream);
long edgl_mate_bwd_workspace(int B, int T, int C, int w_month, int w_day, int w_weekday, int w_hour);
int edgl_mate_bwd(const int64_t* idx, const void* month_tab, const void* day_tab, const void* weekday_tab, const void* hour_tab,
                  const void* u, const void* pq, const float* saved, const void* d_R, int B, int T, int C, int w_month, int w_day,
                  int w_weekday, int w_hour, void* d_u, void* d_pq, float* d_tables, float* workspace, int dtype, void* stream);
int edgl_tahe_fwd(const void* R, const void* Hs, int B, int T, int C, void* hist, int dtype, void* stream);
int edgl_tahe_bwd(const void* R, const void* Hs, const void* d_hist, int B, int T, int C, void* d_R, void* d_Hs, int dtype,
                  void* stream);
int edgl_tahe_mix_fwd(const void* emb, const void* tcode, const float* te_weight, const int64_t* ids, long rows, int C, void* out,
                      int dtype, void* stream);
/* cat [rows,3C] = [a | b | c] (split == 0: the head's input, TimelyREC.py:150) or a, b, c <- the three blocks of cat (split != 0). */
int edgl_cat3(void* a, void* b, void* c, long rows, int C, void* cat, int split, int dtype, void* stream);
long edgl_tahe_mix_bwd_workspace(long rows);
int edgl_tahe_mix_bwd(const void* d_out, const void* tcode, const int64_t* ids, long rows, int C, void* d_emb, float* d_te,
                      float* workspace, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EASYDGL_HIP_H */
