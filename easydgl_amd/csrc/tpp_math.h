// Formulas of the TPP regulariser that more than one translation unit needs: the kernels of k_tpp.hip and the slot data of a
// sample (batch_prep.h, which also runs inside the encoder's launch: k_encode.hip).
#pragma once
#include "edgl_common.h"

namespace tpp_math {

__device__ __forceinline__ float raw_span(const float* ts_row, int pos, int T) {
    // EasyDGL.py:161-162 on RAW seconds: span[t] = clip(ts[t]-ts[t-1], 0, 100), span[0] := span[1]
    if (T < 2) return 0.f;
    const int t1 = pos == 0 ? 1 : pos;
    return fminf(fmaxf(ts_row[t1] - ts_row[t1 - 1], 0.f), 100.f);
}

// marks of four mark bytes held in one word (temporal.py:330: the bytes are counts); a 16-byte mark row is four such words
__device__ __forceinline__ uint32_t mark_word_count(uint32_t w) {
    return (w & 0xffu) + ((w >> 8) & 0xffu) + ((w >> 16) & 0xffu) + (w >> 24);
}

}  // namespace tpp_math
