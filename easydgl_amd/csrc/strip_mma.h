// The hand-placed MFMA slots of the K5 strip kernels (k_score_strip.hip: C = 128, namespace strip; k_score_stripw.hip: C = 256 and
// 512, namespace stripw): everything the pipelines write the same way — the slot statements, the bare MFMAs and the LDS operand
// reads.  Both files pull it in with a using-directive inside their namespace.  What a width's pipeline shapes (ring depth,
// staging, settle_s / settle_o, Carry, unit_iter*, main_pass*, epilogue*) stays in its file.
//
// Why the MFMAs and the per-logit VALU work are asm statements:
// (1) Register FILES: with 512 registers per wave the compiler selects the AGPR form for every builtin MFMA and then moves each
//     logit through v_accvgpr_read before the VALU can touch it (144 moves per 32 MFMAs in the first build of the C = 128 kernel;
//     -amdgpu-mfma-vgpr-form crashes hipcc 7.2 there).  Fixed here:  logits S in VGPRs (exponentiated in place), x fragments XF
//     in AGPRs (only ever an MFMA B operand; loaded straight into them), output O in AGPRs (only touched by MFMAs until the
//     epilogue), P and the Z fragments in VGPRs.
// (2) Placement: one wave per SIMD issues one instruction per ~4 cycles, so a 32-cycle MFMA hides ~7 other instructions and only
//     if they sit next to it.  IR passes otherwise sink the conversions to the end of the iteration and pack the row sums into
//     v_pk_add_f32 (slow beside MFMAs).  asm volatile statements keep their program order.
// Hazards (guide §5.7): the compiler neither sees nor pads an instruction inside asm.  Every consumer of an MFMA result here is
// either the next MFMA of the same accumulator chain (no wait states) or more than a full slot group later; a v_exp result is
// first read one slot later (no trans -> VALU forwarding hazard); the places that read MFMA results directly (prologue maxima,
// epilogue) sit behind the pipelines' settle_s() / settle_o().  tests/test_strip_isa.py audits the assembly of both files.
#pragma once

#include "edgl_common.h"

namespace strip_mma {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef int v4i __attribute__((ext_vector_type(4)));

constexpr float L2E = 1.4426950408889634f;
// Reference of the row exponentials (ROLE_YF).  A flash-style running maximum would have to rescale the accumulator whenever it
// moves — code that touches O outside an MFMA, which drags the accumulators through VGPRs in every iteration (128 v_accvgpr moves
// + spills in the first build).  Instead the reference of a row is FIXED per item chunk: the maximum of the chunk's first 32
// logits.  exp(logit - ref) then exceeds 1 for larger logits, which f32 (and bf16: same exponent range, relative precision)
// absorbs up to 2^100; a row sum beyond that makes the WORKGROUP redo its chunk with the exact row maxima from an S-only sweep
// (fallback_exact*: exp <= 1, cannot overflow).  The finish kernels merge chunks from (reference, sum) pairs and do not care which
// reference a chunk used.
constexpr float LSUM_LIMIT = 1.2676506e30f;   // 2^100

enum { ROLE_YF = 0, ROLE_W = 1 };

// LDS rotation of row / block z: ((z&3)<<2) | ((z>>2)&3) 16-byte columns
__device__ __forceinline__ int rot16(int z) { return (((z & 3) << 2) | ((z >> 2) & 3)) * 16; }

#define SPIN() __builtin_amdgcn_sched_barrier(0)

__device__ __forceinline__ v4i lds_b128(const char* p) { return *reinterpret_cast<const v4i*>(p); }
__device__ __forceinline__ f32x4 lds_f4(const char* p) { return *reinterpret_cast<const f32x4*>(p); }
// B operand of a 32x32x16 MFMA contracting along the rows of the tile / unit: two transpose reads (slots 0-3: rows +0..3, slots
// 4-7: rows +8..11 of this lane half's row group — the order in which P is packed from the logit registers).  STRIDE: LDS bytes
// from row z to row z + 1 (512 in the C = 128 image, the block size BLKB in the wide ones); rows + 8 sit at rot + 2.
template <int STRIDE>
__device__ __forceinline__ v4i lds_tr(const char* p) {
    typedef __attribute__((ext_vector_type(4))) short s4;
    const s4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)p);
    const s4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(p + 8 * STRIDE + 32));
    const uint2 a = __builtin_bit_cast(uint2, v0), b = __builtin_bit_cast(uint2, v1);
    return v4i{(int)a.x, (int)a.y, (int)b.x, (int)b.y};
}

// Per-lane LDS offsets (bytes, relative to a unit's first row / block); filled by the pipelines' lane_off*()
struct LaneOff {
    int zf;   // row-fragment read: row l&31, k-slot hi        (+ ks*32)
    int tr;   // transpose read: row 4hi + (s>>2), columns 16*(G&1) + 4*(s&3)   (+ the k-slot / channel-tile offsets of the image)
    int ci;   // C operand of the logit rows: info floats 4hi .. 4hi+3   (+ g*32)
};

// a quarter (g = 0..3) of the C operand of a unit's logit rows
__device__ __forceinline__ void fetch_ci_part(f32x16& ci, const char* info, const LaneOff& lo, int g) {
    const f32x4 t = lds_f4(info + lo.ci + g * 32);
    ci[4 * g] = t[0]; ci[4 * g + 1] = t[1]; ci[4 * g + 2] = t[2]; ci[4 * g + 3] = t[3];
}

// -DSTRIP_SAFE (EDGL_STRIP_SAFE=1 at build time): every bare MFMA is followed by its full wait states
#ifdef STRIP_SAFE
#define MFMA_PAD "\n\ts_nop 15\n\ts_nop 15"
#else
#define MFMA_PAD ""
#endif
__device__ __forceinline__ void mfma_s0(f32x16& d, const v4i& a, const v4i& b, const f32x16& c) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" MFMA_PAD : "=&v"(d) : "v"(a), "a"(b), "v"(c));
}
__device__ __forceinline__ void mfma_s(f32x16& d, const v4i& a, const v4i& b) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" MFMA_PAD : "+v"(d) : "v"(a), "a"(b));
}
__device__ __forceinline__ void mfma_o(f32x16& d, const v4i& a, const v4i& b) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" MFMA_PAD : "+a"(d) : "v"(a), "v"(b));
}

// One MFMA slot = ONE asm statement: the MFMA and the VALU work on logit e (0..15) of the tile T being exponentiated; no
// instruction depends on a result of the same slot (one wave per SIMD: a dependent pair costs the full VALU latency), and separate
// statements would draw a compiler s_nop between them (an issue slot each).
//   T[e]   <- exp2(T[e])                      T[e] already holds  logit * log2(e) + add  (written one slot earlier)
//   T[e+1] <- T[e+1] * log2(e) + add          (e = 0 also scales itself first)
//   row sum += T[e-1];  after every odd logit the pair before it is packed
// slot_tail() finishes the tile (sum / pack of logits 14, 15).
#define VALU_E0 "v_fma_f32 %[cur], %[cur], %[l2e], %[add]\n\tv_fma_f32 %[nxt], %[nxt], %[l2e], %[add]\n\tv_exp_f32 %[cur], %[cur]"
#define VALU_ODD "v_exp_f32 %[cur], %[cur]\n\tv_fma_f32 %[nxt], %[nxt], %[l2e], %[add]\n\tv_add_f32 %[sum], %[sum], %[p1]"
#define VALU_EVEN VALU_ODD "\n\tv_cvt_pk_bf16_f32 %[pk], %[p2], %[p1]"
#define VALU_E15 "v_exp_f32 %[cur], %[cur]\n\tv_add_f32 %[sum], %[sum], %[p1]"
#define MF_S0 "v_mfma_f32_32x32x16_bf16 %[d], %[a], %[b], %[c]\n\t"
#define MF_S "v_mfma_f32_32x32x16_bf16 %[d], %[a], %[b], %[d]\n\t"
// kind 0: S MFMA with C = ci (D early-clobber VGPR), 1: S MFMA accumulating (D VGPR, B AGPR), 2: O MFMA (D AGPR, B VGPR).
// (KIND, e) in use —
//   C = 128 (two x tiles, a logit in every slot): kind 0 at e = 0, 1 (the two ks = 0 MFMAs); kind 1 at e = 2 .. 15; kind 2 at
//            e = 0 .. 15 (the O half carries the logits of x tile 1);
//   C = 256 (one x tile, a logit in every second slot; the others are bare mfma_s / mfma_o): kind 0 at e = 0; kind 1 at
//            e = 1 .. 7; kind 2 at e = 8 .. 15;
//   C = 512 (all 16 logits in the 32-MFMA S half): kind 0 at e = 0; kind 1 at e = 1 .. 15; no kind 2.
template <int KIND>
__device__ __forceinline__ void slot(f32x16& d, const v4i& a, const v4i& b, const f32x16& c, f32x16& T, int (&pk)[8], float& lsum,
                                     float add, int e) {
    float cur = T[e], nxt = T[e < 15 ? e + 1 : 15];
    int r = 0;
#define SLOT_ASM(MF, VA, DC, BC)                                                                                                  \
    asm volatile(MF VA : [d] DC(d), [cur] "+v"(cur), [nxt] "+v"(nxt), [sum] "+v"(lsum), [pk] "=&v"(r)                          \
                 : [a] "v"(a), [b] BC(b), [l2e] "s"(L2E), [add] "v"(add), [p1] "v"(T[e >= 1 ? e - 1 : 0]), [p2] "v"(T[e >= 2 ? e - 2 : 0]))
#define SLOT_ASM_C(MF, VA, DC, BC)                                                                                                \
    asm volatile(MF VA : [d] DC(d), [cur] "+v"(cur), [nxt] "+v"(nxt), [sum] "+v"(lsum), [pk] "=&v"(r)                          \
                 : [a] "v"(a), [b] BC(b), [c] "v"(c), [l2e] "s"(L2E), [add] "v"(add), [p1] "v"(T[e >= 1 ? e - 1 : 0]),             \
                   [p2] "v"(T[e >= 2 ? e - 2 : 0]))
    if (KIND == 0) {
        if (e == 0) SLOT_ASM_C(MF_S0, VALU_E0, "=&v", "a");
        else SLOT_ASM_C(MF_S0, VALU_ODD, "=&v", "a");
    } else if (KIND == 1) {
        if (e == 15) SLOT_ASM(MF_S, VALU_E15, "+v", "a");
        else if (e & 1) SLOT_ASM(MF_S, VALU_ODD, "+v", "a");
        else SLOT_ASM(MF_S, VALU_EVEN, "+v", "a");
    } else {
        if (e == 0) SLOT_ASM(MF_S, VALU_E0, "+a", "v");
        else if (e == 15) SLOT_ASM(MF_S, VALU_E15, "+a", "v");
        else if (e & 1) SLOT_ASM(MF_S, VALU_ODD, "+a", "v");
        else SLOT_ASM(MF_S, VALU_EVEN, "+a", "v");
    }
#undef SLOT_ASM_C
#undef SLOT_ASM
    T[e] = cur;
    if (e < 15) T[e + 1] = nxt;
    if (e >= 2 && (e & 1) == 0) pk[(e - 2) >> 1] = r;
}
__device__ __forceinline__ void slot_tail(f32x16& T, int (&pk)[8], float& lsum) {
    int r;
    asm volatile("v_add_f32 %0, %0, %2\n\tv_cvt_pk_bf16_f32 %1, %3, %2" : "+v"(lsum), "=&v"(r) : "v"(T[15]), "v"(T[14]));
    pk[7] = r;
}

}  // namespace strip_mma
