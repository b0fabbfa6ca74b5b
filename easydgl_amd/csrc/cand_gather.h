// The row gather of the candidate-list kernels (k_eval_cand.hip: evaluation; k_cand_ce.hip: sampled-softmax
// training): ONE arithmetic rule for the value of (query row, item), shared so that a model is trained on the
// numbers it is evaluated with.
//
//   v(r, c) = rows[r] . table_c[c] + bias_used[c];  item 0 is the used table's zero row with bias -1000 (coding.py:56-57)
//
// The query row stays in registers, spread over a lane group of G = min(64, pieces) lanes (a piece = 16 bytes of the row; G
// rounded up to a power of two, lanes past the row hold zeros; f32 rows longer than 1 KB: two pieces per lane).  cand_value IS
// the rule: per lane the FMAs of its pieces in ascending channel order from +0, a fixed xor butterfly over the lane group
// (offsets 1, 2, .. G / 2: both partners form a + b, so every lane of the group ends with the same bits), then + bias.  It
// depends on rows[r], table_c[c] and the bias only — not on the slot, the list, R or the other candidates.
#pragma once
#include "edgl_common.h"

namespace candg {

constexpr int UNROLL = 4;        // candidate-row loads in flight per wave before the first is consumed

template <typename T, int PPL>
struct RowRegs { float x[PPL][16 / sizeof(T)]; };

// this lane's pieces of row `row`; a piece past the row is clamped into it (unpack reads it as +0)
template <typename T, int G, int PPL>
__device__ __forceinline__ void load_pieces(const T* base, long row, int C, int gl, uint4 (&w)[PPL]) {
    constexpr int VEC = 16 / sizeof(T);
    const int np = C / VEC;
#pragma unroll
    for (int pp = 0; pp < PPL; ++pp) {
        const int piece = gl + pp * 64;
        w[pp] = *reinterpret_cast<const uint4*>(base + row * C + (long)min(piece, np - 1) * VEC);      // (clamped: inside the row)
    }
}
template <typename T>
__device__ __forceinline__ void unpack(const uint4& w, bool keep, float (&f)[16 / sizeof(T)]) {
    constexpr int VEC = 16 / sizeof(T);
    Vec16<T> v;
    *reinterpret_cast<uint4*>(&v) = w;
#pragma unroll
    for (int e = 0; e < VEC; ++e) f[e] = keep ? to_f32(v.v[e]) : 0.0f;
}

// THE value of (query row in `xq`, item c whose pieces are in `w`): see the head of the file.  `b` = bias_used[c].
template <typename T, int G, int PPL>
__device__ __forceinline__ float cand_value(const RowRegs<T, PPL>& xq, const uint4 (&w)[PPL], int c, float b, int C, int gl) {
    constexpr int VEC = 16 / sizeof(T);
    const int np = C / VEC;
    float acc = 0.0f;
#pragma unroll
    for (int pp = 0; pp < PPL; ++pp) {
        float z[VEC];
        unpack<T>(w[pp], c != 0 && gl + pp * 64 < np, z);      // item 0: the used table's zero row
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc = fmaf(xq.x[pp][e], z[e], acc);
    }
#pragma unroll
    for (int o = 1; o < G; o <<= 1) acc += __shfl_xor(acc, o, 64);
    return acc + b;
}

// lane group of a row of `pieces` 16-byte pieces: the next power of two, at most 64
inline int group_of(int pieces) {
    int g = 2;
    while (g < pieces && g < 64) g <<= 1;
    return g;
}

}  // namespace candg
