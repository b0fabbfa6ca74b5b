// The embedding backward's MFMA scatter (coding.py:60-64): per-workgroup segmented sum over equal ids as ONE matrix product with a
// one-hot operand, leaders add their rows to the table gradient.  Shared by the stand-alone scatter launch (k_encode.hip:
// encode_scatter_mfma_kernel) and by the QKVT dX GEMM whose epilogue runs it on its own output tile (k_gemm2.hip: dx_encode_kernel).
#pragma once
#include "edgl_common.h"
#include "red_batch.h"

namespace enc_scatter {

struct EncBwdP {
    const int64_t* ids; const uint8_t* marks; const void* dx0;
    int B, T, C, E, I; float rate; const uint64_t* rng; uint32_t stream_id;
    float* d_item; float* part_pos; float* part_mk; int nchunk;
    int srows;
    const void* add1; const void* add2;   // optional [B*T, C] terms added to the item section of dX0 (residual branches)
    float sq;             // sqrt(true model width): coding.py:62-63 (== sqrt(C) without channel padding)
    // Optional second job of the MFMA scatter launch (encode_scatter_mfma_kernel): the one-hot term of the tied table's scoring
    // gradient, d_table[label[r]] -= coef[r] rows[r], d_bias[label[r] - 1] -= coef[r] over the weighted rows (Appendix C; what
    // edgl_score_flash_label_term applies as a launch of its own) — the same segmented sum over equal ids, on blocks behind the
    // embedding's: lab_blk0 = first such block (0: none)
    const void* lab_rows; const int64_t* lab_ids; const float* lab_coef; const int32_t* lab_nvalid; int lab_R; int lab_blk0;
    float* d_bias;
    int red_blk0;         // first workgroup of the reduction list that rides in the MFMA scatter launch (RedBatch::blocks of them; 0: in front)
    float* d_mark_zero;   // [E*C]: cleared by block (0, 0) of the position / mark stage (only row 1 is ever written afterwards)   // rows per block of the scatter stage (<= SROWS; fewer when SROWS*C floats exceed the LDS)
};

constexpr int SROWS = 128;
constexpr int ENC_NCHUNK = 16;      // chunks of the batch in the position / mark partial sums (edgl_encode_bwd_workspace)

typedef __attribute__((ext_vector_type(4))) short enc_s16x4;
__device__ __forceinline__ uint2 enc_tr_read(const bf16* tile, int ld, int k0, int z0, int lane) {
    const int G = lane >> 4, s = lane & 15;
    const bf16* p = tile + (k0 + 4 * G + (s >> 2)) * ld + z0 + 4 * (s & 3);
    enc_s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) enc_s16x4*)p);
    return *reinterpret_cast<uint2*>(&v);
}

// leader of row `tid` = first row of the block with the same id: branch-free scan over int4 groups (a per-element scan with an
// early exit is a chain of up to 127 dependent LDS reads)
__device__ __forceinline__ int scatter_leader(const int* s_id, int tid) {
    const int id = s_id[tid];
    int lead = tid;
    for (int j4 = (tid >> 2); j4 >= 0; --j4) {
        const int4 v = *reinterpret_cast<const int4*>(s_id + 4 * j4);
        const int j = 4 * j4;
        if (v.w == id && j + 3 < tid) lead = j + 3;
        if (v.z == id && j + 2 < tid) lead = j + 2;
        if (v.y == id && j + 1 < tid) lead = j + 1;
        if (v.x == id && j < tid) lead = j;
    }
    return lead;
}

// acc[leader][c] = sum_row onehot[leader][row] * Gs[row][c] over the SROWS rows of the image (Gs: [SROWS][C + 8] bf16, masked
// rows; s_lead: first row with the same id, -1: padding), then leaders add sqs * their sums to d_item[s_id[leader]][coff + c].
// wave w: leaders [32 w, 32 w + 32) x all channels; the block's sums are formed in one fixed order.
template <int CT>
__device__ __forceinline__ void scatter_onehot_sum(const bf16* Gs, const int* s_id, const int* s_lead, float* d_item, int CF, int coff,
                                                   float sqs) {
    constexpr int C = 16 * CT, LDG = C + 8, SR = SROWS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, G = lane >> 4, g4 = G * 4, l15 = lane & 15;
    f32x4 acc[2][CT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[mt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bf16 one = from_f32<bf16>(1.f), zero = from_f32<bf16>(0.f);
#pragma unroll
    for (int kb = 0; kb < SR / 32; ++kb) {
        // k-slot order of the transpose-read fragments: slots 0-3 <-> row 32 kb + 4G + j, slots 4-7 <-> 32 kb + 16 + 4G + j
        const int4 la = *reinterpret_cast<const int4*>(s_lead + kb * 32 + g4);
        const int4 lb = *reinterpret_cast<const int4*>(s_lead + kb * 32 + 16 + g4);
        const int lk[8] = {la.x, la.y, la.z, la.w, lb.x, lb.y, lb.z, lb.w};
        bf16x8 af[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int lead = wave * 32 + mt * 16 + l15;
#pragma unroll
            for (int i = 0; i < 8; ++i) af[mt][i] = lk[i] == lead ? one : zero;
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            bf16x8 bfr;
            *reinterpret_cast<uint2*>(&bfr) = enc_tr_read(Gs, LDG, kb * 32, ct * 16, lane);
            *(reinterpret_cast<uint2*>(&bfr) + 1) = enc_tr_read(Gs, LDG, kb * 32 + 16, ct * 16, lane);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) acc[mt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[mt], bfr, acc[mt][ct], 0, 0, 0);
        }
    }
    // acc[mt][ct][r] = sum for leader 32 w + 16 mt + 4G + r, channel 16 ct + l15
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int lead = wave * 32 + mt * 16 + g4 + r;
            if (s_lead[lead] != lead) continue;   // not a leader (or padding)
            float* dst = d_item + (long)s_id[lead] * CF + coff + l15;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) atomicAdd(dst + ct * 16, sqs * acc[mt][ct][r]);
        }
}

// One workgroup (256 threads) of the scatter over SROWS consecutive rows: bx = workgroup index among the scatter's own (embedding
// blocks first, label blocks from p.lab_blk0 on), by = channel slice (C = 16 CT channels starting at by * C of the p.C-wide rows:
// the 256 / 512-unit recipes run as 2 / 4 slices of 128).  Gs: [SROWS][C + 8]; s_id, s_lead, s_cf, s_cb: [SROWS].
template <int CT>
__device__ __forceinline__ void scatter_block(const EncBwdP& p, int bx, int by, bf16* Gs, int* s_id, int* s_lead, float* s_cf, float* s_cb) {
    constexpr int C = 16 * CT, LDG = C + 8, SR = SROWS;
    const int CF = p.C, coff = by * C;      // full row width, first channel of this slice
    // label job (block-uniform): rows = the compacted head rows, ids = their labels, every row scaled by its loss coefficient
    const bool lab = p.lab_blk0 > 0 && bx >= p.lab_blk0;
    const long rows = lab ? (long)(p.lab_nvalid ? min(p.lab_R, p.lab_nvalid[0]) : p.lab_R) : (long)p.B * p.T;
    const long r0 = (long)(bx - (lab ? p.lab_blk0 : 0)) * SR;
    if (lab && r0 >= rows) return;
    const int tid = threadIdx.x;
    if (tid < SR) {
        const bool in = r0 + tid < rows;
        if (lab) {
            const float cf = in ? p.lab_coef[r0 + tid] : 0.f;
            s_id[tid] = (in && cf != 0.f) ? (int)p.lab_ids[r0 + tid] : 0;      // label 0: weight 0 (EasyDGL.py:180)
            s_cf[tid] = cf;
            s_cb[tid] = 0.f;
        } else {
            s_id[tid] = in ? (int)p.ids[r0 + tid] : 0;
        }
    }
    // gradient fragments of this thread's rows, all in flight before anything else (rows clamped)
    constexpr int cpr = C / 4, rows_par = 256 / cpr, NR = SR / rows_par;
    const int cv = tid % cpr, rl = tid / cpr, c0 = cv * 4;
    const bf16* dx0 = reinterpret_cast<const bf16*>(lab ? p.lab_rows : p.dx0);
    const long ldrow = lab ? CF : 3 * CF;
    const bool adds = p.add1 && !lab;
    Frag4<bf16> g[NR], ga[NR], gb[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const long row = min(r0 + rl + (long)k * rows_par, rows - 1);
        g[k] = frag_ld<bf16>(dx0 + row * ldrow + coff + c0);
        if (adds) {
            ga[k] = frag_ld<bf16>(reinterpret_cast<const bf16*>(p.add1) + row * CF + coff + c0);
            gb[k] = frag_ld<bf16>(reinterpret_cast<const bf16*>(p.add2) + row * CF + coff + c0);
        }
    }
    __syncthreads();
    if (tid < SR) {
        const int id = s_id[tid];
        const int lead = scatter_leader(s_id, tid);
        s_lead[tid] = id == 0 ? -1 : lead;
        if (lab && id != 0 && by == 0) atomicAdd(&s_cb[lead], s_cf[tid]);     // bias term of the leader's label
    }
    const DropKey dk = make_dropkey(p.rng, p.stream_id, p.rate);
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int r = rl + k * rows_par;
        const long row = r0 + r;
        Frag4<bf16> v = g[k];
        if (adds) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v.v[j] = from_f32<bf16>(to_f32(v.v[j]) + to_f32(ga[k].v[j]) + to_f32(gb[k].v[j]));
        }
        if (lab) {   // coef[r] * rows[r], rounded to the operand dtype of the segmented sum (as the product pass rounds its P)
            const float cf = s_cf[r];
#pragma unroll
            for (int j = 0; j < 4; ++j) v.v[j] = from_f32<bf16>(cf * to_f32(v.v[j]));
        } else if (dk.thresh != 0u) {
            const uint32_t keep = drop_keep4(dk, (uint64_t)row * 3 * CF + coff + c0);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (!((keep >> j) & 1u)) v.v[j] = from_f32<bf16>(0.f);
        }
        *reinterpret_cast<uint2*>(Gs + r * LDG + c0) = *reinterpret_cast<const uint2*>(&v);
    }
    __syncthreads();
    scatter_onehot_sum<CT>(Gs, s_id, s_lead, p.d_item, CF, coff, lab ? -1.0f : p.sq * dk.scale);
    if (lab && by == 0 && tid < SR && s_lead[tid] == tid) atomicAdd(p.d_bias + s_id[tid] - 1, -s_cb[tid]);
}

}  // namespace enc_scatter
