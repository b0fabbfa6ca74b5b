// Host entry points of the strip kernels, called from k_score.hip.  Included by k_score.hip AND by the files that define them
// (k_score_strip.hip, k_score_stripw.hip), so that a drifted prototype is a compile error and not a silent overload.
#pragma once

#include "edgl_common.h"

// k_score_strip.hip: one-wave-per-SIMD form of the two product passes (bf16, C = 128)
bool edgl_strip_enabled();
int edgl_strip_rows(const void* rows, const void* table, const float* out_bias, int R, int I, int i0, int i1, const int32_t* nvalid,
                    float* slabs, float* part, int G, int slab16, hipStream_t st);
int edgl_strip_table(const void* rows, const void* table, const float* out_bias, const float* coef, const float* row_lse, int R,
                     int I, int i0, int i1, const int32_t* nvalid, float* slabs, float* bias_slabs, int nchunk, float* acc_table,
                     float* acc_bias, hipStream_t st);
// k_score_stripw.hip: the same passes at C = 256 (32 x vectors per wave, 128 per workgroup) and C = 512 (two workgroups per x block)
bool edgl_stripw_enabled();
bool edgl_stripw_supports(int C);
long edgl_stripw_info_floats(long n);      // floats of scratch a pass needs for its C operands (rows: n = i1 - i0; table: n = R)
int edgl_stripw_rows(const void* rows, const void* table, const float* out_bias, int R, int C, int I, int i0, int i1,
                     const int32_t* nvalid, float* slabs, float* part, int G, float* info_ws, hipStream_t st);
int edgl_stripw_table(const void* rows, const void* table, const float* out_bias, const float* coef, const float* row_lse, int R,
                      int C, int I, int i0, int i1, const int32_t* nvalid, float* slabs, float* bias_slabs, int nchunk, float* info_ws,
                      hipStream_t st);
// k_score_stripw.hip: the one-hot term the ROLE_W pass of either file leaves out, C = 128 / 256 / 512
int edgl_strip_label_scatter(const void* rows, const int64_t* labels, const float* coef, const int32_t* nvalid, int R, int C, int i0,
                             int i1, const float* gscale, float* d_table, float* d_bias, hipStream_t st);
