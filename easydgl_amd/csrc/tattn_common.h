// What the attention kernels of k_tattn.hip (TGAT: narrow and sliced heads) and k_tiattn.hip (TiSASRec: interval buckets) share:
// the parameter block and how the host fills it, the job decode and its launch, and the small tile helpers.
//
// Tile scheme of all of them: one wave per (sample, head, 16-row tile[, slice]); operands are read straight from L2 as
// 4-element row chunks (A/B fragments of the 16x16 MFMA); a tile that has to be contracted along its rows is turned with one
// MFMA against the identity (edgl_common.h transpose_tile) instead of an LDS round trip.
//   fwd   : per query tile, softmax over the key tiles, O^T += V^T . P^T; saves (max, sum) per row and O in f32
//   bwd_q : per query tile, D = dO.O, dS = P*(dP - D), dQ~^T += K~^T . dS^T
//   bwd_k : per key tile, loops the query tiles, dV^T += dO^T . A, dK~^T += Q~^T . dS
// Fully masked query rows (left padding) are uniform over ALL keys in the reference (every score is replaced by the same
// constant, temporal.py:158,166) and the joint LayerNorm that follows reads them, so no tile is skipped.
#pragma once
#include "edgl_common.h"

namespace {

constexpr int TA_CAUSAL = 1;
constexpr int TA_ORDERED = 2;      // interval attention: the LDS bins are filled in a fixed order, without atomics
constexpr float PADV = -4294967296.0f;   // float32(-2**32 + 1): what the reference puts in place of a masked score (temporal.py:158,166)

struct TaP {
    const void *qx, *kx, *v, *resid;
    int ldq, ldk, ldv, ldr;
    const int64_t* ids;
    int B, T, H, Dq, Dv;
    float cscale, rate;
    const uint64_t* rng; uint32_t stream_id;
    void* out; int ldo;
    float *st_m, *st_l, *st_d, *oatt;     // [H*B*T] each, oatt [B,T,H*Dv] f32
    const void* d_out; int ld_do;
    void *d_qx, *d_kx, *d_v; int ld_dq, ld_dk, ld_dv;
    int flags, NT;
};

template <typename T> __device__ __forceinline__ void frag_st(T* dst, const Frag4<T>& f) {
    if constexpr (sizeof(T) == 4) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(&f);
    else *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(&f);
}
// registers of a row-chunk load (lane = row l&15, 4 columns at (l>>4)*4) -> the same tile with rows on (l>>4)*4+r
template <typename T> __device__ __forceinline__ Frag4<T> turn(const Frag4<T>& f, const Frag4<T>& ident) {
    return frag_from_acc<T>(mma16(f, ident, f32x4{0.f, 0.f, 0.f, 0.f}));
}

// One wave = one job (sample, head, 16-row tile, slice).  SLICED: a wide head is cut into nslice slices (k_tattn.hip), the
// slice index runs fastest; a template parameter, so that the unsliced kernels keep their instruction stream to the letter.
struct Job { int b, head, tile, slice; long bp; };
template <bool SLICED = false>
__device__ __forceinline__ bool get_job(const TaP& p, Job& j, int nslice = 1) {
    long job = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    long jobs = (long)p.B * p.H * p.NT;
    if constexpr (SLICED) jobs *= nslice;
    if (job >= jobs) return false;
    j.slice = 0;
    if constexpr (SLICED) { j.slice = (int)(job % nslice); job /= nslice; }
    j.tile = (int)(job % p.NT);
    const long bh = job / p.NT;
    j.head = (int)(bh % p.H);
    j.b = (int)(bh / p.H);
    j.bp = (long)j.head * p.B + j.b;   // head-major b' (temporal.py:139-141)
    return true;
}
// `waves` jobs per block; `extra` are the kernel's arguments behind the TaP
template <typename K, typename... A>
int launch_jobs(K kern, const TaP& p, int nslice, int waves, size_t smem, hipStream_t st, const A&... extra) {
    const long jobs = (long)p.B * p.H * p.NT * nslice;
    hipLaunchKernelGGL(kern, dim3((unsigned)((jobs + waves - 1) / waves)), dim3(64 * waves), smem, st, p, extra...);
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}

// First position of the sequence with ids != 0 (T if none).  Rows before it are fully masked: every score is the same
// replaced constant and the softmax is uniform over ALL keys, so their tiles must be computed.  Every later row has an
// unmasked key, its replaced scores underflow to exactly 0 after the softmax, and key tiles above the diagonal contribute
// exactly nothing — they are skipped (half of the causal work).
__device__ __forceinline__ int first_unpadded(const int64_t* idr, int T, int lane) {
    int f = T;
    for (int k = lane; k < T; k += 64)
        if (idr[k] != 0) f = min(f, k);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) f = min(f, __shfl_xor(f, o, 64));
    return f;
}
// ---- host: the parameter block -----------------------------------------------------------------------------------------
// what the forward saves for the backward: softmax (max, sum), D, and the attention output in f32
struct SavedTa { size_t off_m, off_l, off_d, off_o, bytes; };
inline SavedTa saved_ta(int B, int T, int H, int Dv) {
    const size_t R = ((size_t)B * H * T + 63) & ~(size_t)63;
    SavedTa s;
    s.off_m = 0; s.off_l = R * 4; s.off_d = 2 * R * 4; s.off_o = 3 * R * 4;
    s.bytes = s.off_o + (size_t)B * T * H * Dv * 4;
    return s;
}
inline void bind_saved(TaP& p, void* saved) {
    if (!saved) return;
    const SavedTa s = saved_ta(p.B, p.T, p.H, p.Dv);
    p.st_m = reinterpret_cast<float*>((char*)saved + s.off_m);
    p.st_l = reinterpret_cast<float*>((char*)saved + s.off_l);
    p.st_d = reinterpret_cast<float*>((char*)saved + s.off_d);
    p.oatt = reinterpret_cast<float*>((char*)saved + s.off_o);
}
// the inputs every sweep reads; the forward adds (resid, out), the backward (d_out, d_qx, d_kx, d_v)
inline TaP ta_params(const void* qx, int ldq, const void* kx, int ldk, const void* v, int ldv, const int64_t* ids, int B, int T,
                     int H, int Dq, int Dv, float scale, float drop_rate, const uint64_t* rng_state, uint32_t stream_id,
                     void* saved, int flags) {
    TaP p{};
    p.qx = qx; p.kx = kx; p.v = v; p.ldq = ldq; p.ldk = ldk; p.ldv = ldv;
    p.ids = ids; p.B = B; p.T = T; p.H = H; p.Dq = Dq; p.Dv = Dv; p.cscale = scale; p.rate = drop_rate;
    p.rng = rng_state; p.stream_id = stream_id; p.flags = flags; p.NT = (T + 15) / 16;
    bind_saved(p, saved);
    return p;
}

}  // namespace
