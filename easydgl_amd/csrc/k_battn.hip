// K14: bidirectional attention staged through LDS — BERTAttention.__call__ (sequential.py:111-137, BERT4REC) after its three dense
// layers.  Q | K | V are column blocks of ONE [B,T,3C] projection output (row stride 3C), heads are contiguous dh-wide slices:
//     S = Q K^T / sqrt(dh);  S[q,k] := float32(-2^32+1) where ids[b,k] == 0;  P = softmax over all T keys;  O = drop(P) V
// No causal mask and no residual.  The key mask is one bit per key, shared by every query of the sample, and a masked score is
// REPLACED: as soon as the sample has one real key, every padded key's probability underflows to exactly 0 in every query row
// (padded query rows too).  A 64-key block whose ids are all 0 is then neither staged nor multiplied, in the forward and in both
// sweeps of the backward, and its dK / dV are written as zeros.  A sample without a real key skips nothing: its softmax is uniform
// over all T keys (and dV is the 1/T sum of dO).  The skip is by block CONTENTS, so zeros anywhere in the row are handled.
//
// Work split: a workgroup (4 waves) owns one (sample, head, 64-row block); a wave owns 16 of its rows and keeps their operands
// in registers for the whole walk.  The other side is walked in 64-row blocks that all 256 threads stage into LDS ONCE per
// workgroup with 16-byte loads, double-buffered (the next block's global loads are issued in front of the current block's MFMAs;
// one barrier per block).  A block is staged in the orientation(s) its products need:
//     row image  [64][dh + 16 B]  rows = keys (queries): A operand of S^T = K Q^T, dP^T = V dO^T (S = Q K^T, dP = dO V^T)
//     turned img [dh][64 + 16 B]  rows = channels:       A operand of O^T += V^T P^T, dQ^T += K^T dS^T, dV^T += dO^T A, dK^T += Q^T dS
// so nothing is transposed with an identity MFMA.  The 16-byte row pad makes the 16 rows one fragment read touches fall into
// disjoint banks (row strides of 36 / 20 / 68 dwords at dh = 64 / 32 / 128 in bf16, 68 dwords for every turned f32 image).
// S^T keeps the keys on the accumulator's register axis, so P^T is the B operand of the second product as it stands; in bf16
// two neighbouring 16-key accumulators form ONE operand of v_mfma_f32_16x16x32_bf16 and the turned image is read with the same
// key permutation (keys g4..g4+3 of tile 2p, then of tile 2p+1).  bf16 contracts 32 long wherever the contraction is >= 32
// (16x16x16 for Q K^T at dh = 16); f32 runs on the exact 16x16x4 MFMA.
// LDS: mask (4.25 KB) + stages.  Forward 2 images, query sweep 3 (K rows, V rows, K turned), key sweep 4 (Q / dO rows and turned)
// + the block's row statistics; two stages where they fit in 160 KB, one (load behind the compute) in f32 at dh = 128 backward.
// Backward: D = rowsum(dO o O); query sweep: dS = P o (keep dP / (1-r) - D), dQ = scale dS K; key sweep: dV = (P o keep)^T dO
// / (1-r), dK = scale dS^T Q.  Replaced scores carry no gradient (tf.where).  No f32 atomics: two calls give the same bits.
#include <type_traits>

#include "tattn_common.h"   // PADV, frag_st

namespace {

constexpr int BA_BLK = 64;                   // rows of a staged block = rows a workgroup owns
constexpr int BA_MAXB = 17;                  // T <= 1025
constexpr int BA_MASK_BYTES = BA_MAXB * BA_BLK * 4;
constexpr int BA_LDS = 160 * 1024;

struct BaP {
    const void* qkv; const int64_t* ids;
    int B, T, H, C, NB;
    float cscale, rate;
    const uint64_t* rng; uint32_t stream_id;
    void* out;
    float *st_m, *st_l, *st_d;               // [H*B*T] each, head-major rows
    const void* d_out; void* d_qkv;
};

// ---- geometry of the staged images ---------------------------------------------------------------------------------------
template <typename T, int DH> struct BaGeo {
    static constexpr int VEC = 16 / (int)sizeof(T);
    static constexpr int LDR = DH + VEC, LDT = BA_BLK + VEC;          // row / turned image: 16 bytes of pad per row
    static constexpr int ROW = BA_BLK * LDR, TRN = DH * LDT;          // elements
    static constexpr int CPR = DH / VEC, CHUNKS = BA_BLK * CPR;       // 16-byte chunks per row / per block
    static constexpr int NCH = (CHUNKS + 255) / 256;                  // chunks a thread moves
    // bytes of one stage of: forward (K rows, V turned), query sweep (+ V rows), key sweep (Q, dO rows and turned + m | l | D)
    static constexpr int STAGE_F = (ROW + TRN) * (int)sizeof(T);
    static constexpr int STAGE_Q = (2 * ROW + TRN) * (int)sizeof(T);
    static constexpr int STAGE_K = (2 * ROW + 2 * TRN) * (int)sizeof(T) + 3 * BA_BLK * 4;
    static constexpr int nst(int stage) { return BA_MASK_BYTES + 2 * stage <= BA_LDS ? 2 : 1; }
    static constexpr int smem(int stage) { return BA_MASK_BYTES + nst(stage) * stage; }
};

// the register operand of a product that contracts over the head's channels: 32 long in bf16 where the head has them
template <typename T, int DH> struct BaOp {
    static constexpr bool W32 = sizeof(T) == 2 && DH >= 32;
    static constexpr int KW = W32 ? 8 : 4, STEP = W32 ? 32 : 16, N = DH / STEP;
    using F = typename std::conditional<W32, Vec16<T>, Frag4<T>>::type;
    static __device__ __forceinline__ F ld(const T* row, int i, int lane) {
        const T* s = row + i * STEP + (lane >> 4) * KW;
        if constexpr (W32) return ld16<T>(s); else return frag_ld<T>(s);
    }
    static __device__ __forceinline__ f32x4 mma(const F& a, const F& b, f32x4 c) {
        if constexpr (W32) return mma_kblock(a, b, c); else return mma16(a, b, c);
    }
};

template <typename T, int DH> struct BaTile { Vec16<T> r[BaGeo<T, DH>::NCH]; };

// 64 rows x DH channels at (row0, src) -> registers; rows past the end repeat row T-1 (their scores / probabilities are masked)
template <typename T, int DH>
__device__ __forceinline__ void ba_load(BaTile<T, DH>& t, const T* src, long ld, int row0, int Tn) {
    using G = BaGeo<T, DH>;
#pragma unroll
    for (int i = 0; i < G::NCH; ++i) {
        const int c = threadIdx.x + i * 256;
        if (G::CHUNKS % 256 == 0 || c < G::CHUNKS)
            t.r[i] = ld16<T>(src + (long)min(row0 + c / G::CPR, Tn - 1) * ld + (c % G::CPR) * G::VEC);
    }
}
template <typename T, int DH>
__device__ __forceinline__ void ba_store_rows(T* img, const BaTile<T, DH>& t) {
    using G = BaGeo<T, DH>;
#pragma unroll
    for (int i = 0; i < G::NCH; ++i) {
        const int c = threadIdx.x + i * 256;
        if (G::CHUNKS % 256 == 0 || c < G::CHUNKS) st16<T>(img + (c / G::CPR) * G::LDR + (c % G::CPR) * G::VEC, t.r[i]);
    }
}
template <typename T, int DH>
__device__ __forceinline__ void ba_store_turned(T* img, const BaTile<T, DH>& t) {
    using G = BaGeo<T, DH>;
#pragma unroll
    for (int i = 0; i < G::NCH; ++i) {
        const int c = threadIdx.x + i * 256;
        if (G::CHUNKS % 256 == 0 || c < G::CHUNKS) {
            T* dst = img + (c % G::CPR) * G::VEC * G::LDT + c / G::CPR;
#pragma unroll
            for (int e = 0; e < G::VEC; ++e) dst[e * G::LDT] = t.r[i].v[e];
        }
    }
}

__device__ __forceinline__ Vec16<bf16> ba_join(const Frag4<bf16>& a, const Frag4<bf16>& b) {
    const uint2 ua = __builtin_bit_cast(uint2, a.v), ub = __builtin_bit_cast(uint2, b.v);
    Vec16<bf16> r;
    *reinterpret_cast<uint4*>(&r) = make_uint4(ua.x, ua.y, ub.x, ub.y);
    return r;
}

// one 16-row tile of a row image against the wave's register operand: x[rows g4+r of the image tile][the wave's row l15]
template <typename T, int DH>
__device__ __forceinline__ f32x4 ba_mma_rows(const T* img, int tile, const typename BaOp<T, DH>::F (&f)[BaOp<T, DH>::N], int lane) {
    using O = BaOp<T, DH>;
    const T* row = img + (tile * 16 + (lane & 15)) * BaGeo<T, DH>::LDR;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < O::N; ++i) s = O::mma(O::ld(row, i, lane), f[i], s);
    return s;
}
// acc[ut][r] (channel ut*16+g4+r, the wave's row l15) += sum over the block's 64 rows of turned[channel][row] . y[row][l15],
// y = four accumulator tiles (rows on the register axis) used as the B operand as they stand
template <typename T, int DH>
__device__ __forceinline__ void ba_mma_turned(f32x4 (&acc)[DH / 16], const T* img, const f32x4 (&y)[4], int lane) {
    constexpr int LDT = BaGeo<T, DH>::LDT;
    const int g4 = (lane >> 4) * 4;
    const T* row = img + (lane & 15) * LDT + g4;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            const Vec16<bf16> b = ba_join(frag_from_acc<bf16>(y[2 * pp]), frag_from_acc<bf16>(y[2 * pp + 1]));
#pragma unroll
            for (int ut = 0; ut < DH / 16; ++ut) {
                const T* s = row + ut * 16 * LDT + pp * 32;
                acc[ut] = mma_kblock(ba_join(frag_ld<bf16>(s), frag_ld<bf16>(s + 16)), b, acc[ut]);
            }
        }
    } else {
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const Frag4<float> b = frag_from_acc<float>(y[kt]);
#pragma unroll
            for (int ut = 0; ut < DH / 16; ++ut) acc[ut] = mma16(frag_ld<float>(row + ut * 16 * LDT + kt * 16), b, acc[ut]);
        }
    }
}

// The sample's mask in LDS (0 real, the replacement constant for id 0, -inf past the end) and the bitmap of the key blocks that
// are walked: those with a real key, or all of them in a sample that has none.
__device__ __forceinline__ uint32_t ba_mask(const int64_t* idr, int Tn, int NB, float* madd, uint32_t* s_live) {
    if (threadIdx.x == 0) *s_live = 0u;
    __syncthreads();
    for (int k = threadIdx.x; k < NB * BA_BLK; k += 256) {
        const bool real = k < Tn && idr[k] != 0;
        madd[k] = k >= Tn ? -INFINITY : (real ? 0.f : PADV);
        if (real) atomicOr(s_live, 1u << (k >> 6));
    }
    __syncthreads();
    const uint32_t live = *s_live;
    return live ? live : (1u << NB) - 1u;
}

struct BaJob { int b, head, blk; long bp; };
__device__ __forceinline__ BaJob ba_job(const BaP& p) {
    BaJob j;
    j.blk = blockIdx.x % p.NB;
    const int bh = blockIdx.x / p.NB;
    j.head = bh % p.H; j.b = bh / p.H;
    j.bp = (long)j.head * p.B + j.b;          // head-major b' (sequential.py:112-114)
    return j;
}

// keep bits of keys k0 .. k0+3 (k0 a multiple of 4) of the row whose first element has index dbase: one hash per key pair
__device__ __forceinline__ void ba_keep4(const DropKey& dk, uint32_t dbase, int k0, bool (&keep)[4]) {
    const uint32_t h0 = drop_hash_pair(dk, dbase + k0), h1 = drop_hash_pair(dk, dbase + k0 + 2);
    keep[0] = (h0 & 0xffffu) >= dk.t16; keep[1] = (h0 >> 16) >= dk.t16;
    keep[2] = (h1 & 0xffffu) >= dk.t16; keep[3] = (h1 >> 16) >= dk.t16;
}

// the walk over the blocks of `todo`: stage(j, tile regs) / commit(regs, stage) / compute(j, stage); NST = 2: the next block's
// loads fly over the compute and land in the other stage; NST = 1: they follow it
#define BA_WALK(todo, NST, LOAD, COMMIT, COMPUTE)                                   \
    do {                                                                            \
        uint32_t rem_ = (todo);                                                     \
        int cur_ = 0, j_ = __ffs(rem_) - 1;                                         \
        rem_ &= rem_ - 1;                                                           \
        LOAD(j_);                                                                   \
        COMMIT(0);                                                                  \
        __syncthreads();                                                            \
        while (true) {                                                              \
            const int nxt_ = rem_ ? __ffs(rem_) - 1 : -1;                           \
            rem_ &= rem_ - 1;                                                       \
            if (NST == 2 && nxt_ >= 0) { LOAD(nxt_); }                              \
            COMPUTE(j_, cur_);                                                      \
            if (nxt_ < 0) break;                                                    \
            if (NST == 1) { __syncthreads(); LOAD(nxt_); }                          \
            cur_ = NST == 2 ? cur_ ^ 1 : 0;                                         \
            COMMIT(cur_);                                                           \
            __syncthreads();                                                        \
            j_ = nxt_;                                                              \
        }                                                                           \
    } while (0)

// ---- forward -------------------------------------------------------------------------------------------------------------
template <typename T, int DH>
__global__ __launch_bounds__(256) void ba_fwd_kernel(BaP p) {
    using G = BaGeo<T, DH>; using O = BaOp<T, DH>;
    constexpr int NST = G::nst(G::STAGE_F);
    extern __shared__ __attribute__((aligned(16))) unsigned char ba_smem[];
    __shared__ uint32_t s_live;
    float* madd = reinterpret_cast<float*>(ba_smem);
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15, wave = threadIdx.x >> 6;
    const BaJob j = ba_job(p);
    const uint32_t live = ba_mask(p.ids + (long)j.b * p.T, p.T, p.NB, madd, &s_live);
    const long ld = 3L * p.C;
    const T* base = reinterpret_cast<const T*>(p.qkv) + (long)j.b * p.T * ld + j.head * DH;
    const int q = j.blk * BA_BLK + wave * 16 + l15, qc = min(q, p.T - 1);
    const DropKey dk = make_dropkey(p.rng, p.stream_id, p.rate);
    const uint32_t dbase = (uint32_t)((j.bp * p.T + qc) * p.T);
    typename O::F qf[O::N];
#pragma unroll
    for (int i = 0; i < O::N; ++i) qf[i] = O::ld(base + (long)qc * ld, i, lane);
    float m_run = -INFINITY, l_run = 0.f;
    f32x4 acc[DH / 16];
#pragma unroll
    for (int ut = 0; ut < DH / 16; ++ut) acc[ut] = f32x4{0.f, 0.f, 0.f, 0.f};
    BaTile<T, DH> kr, vr;
    auto stage = [&](int s) { return reinterpret_cast<T*>(ba_smem + BA_MASK_BYTES + s * G::STAGE_F); };
#define BA_LOAD(jb) do { ba_load<T, DH>(kr, base + p.C, ld, (jb) * BA_BLK, p.T); ba_load<T, DH>(vr, base + 2 * p.C, ld, (jb) * BA_BLK, p.T); } while (0)
#define BA_COMMIT(s) do { ba_store_rows<T, DH>(stage(s), kr); ba_store_turned<T, DH>(stage(s) + G::ROW, vr); } while (0)
#define BA_COMPUTE(jb, s) do {                                                                                   \
        const T* ks = stage(s);                                                                                  \
        f32x4 e[4];                                                                                              \
        float tmax = -INFINITY;                                                                                  \
        _Pragma("unroll") for (int kt = 0; kt < 4; ++kt) {                                                       \
            e[kt] = ba_mma_rows<T, DH>(ks, kt, qf, lane);                                                        \
            const f32x4 ma = *reinterpret_cast<const f32x4*>(madd + (jb) * BA_BLK + kt * 16 + g4);               \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                      \
                e[kt][r] = ma[r] == 0.f ? e[kt][r] * p.cscale : ma[r];          /* sequential.py:120-124 */      \
                tmax = fmaxf(tmax, e[kt][r]);                                                                    \
            }                                                                                                    \
        }                                                                                                        \
        tmax = group_max4(tmax);                                                                                 \
        const float m_new = fmaxf(m_run, tmax), corr = __expf(m_run - m_new);                                    \
        float psum = 0.f;                                                                                        \
        _Pragma("unroll") for (int kt = 0; kt < 4; ++kt)                                                         \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) { e[kt][r] = __expf(e[kt][r] - m_new); psum += e[kt][r]; } \
        l_run = l_run * corr + group_sum4(psum);                                                                 \
        m_run = m_new;                                                                                           \
        if (dk.thresh != 0u) {                                                      /* :130 */                   \
            _Pragma("unroll") for (int kt = 0; kt < 4; ++kt) {                                                   \
                bool keep[4];                                                                                    \
                ba_keep4(dk, dbase, (jb) * BA_BLK + kt * 16 + g4, keep);                                         \
                _Pragma("unroll") for (int r = 0; r < 4; ++r) e[kt][r] = keep[r] ? e[kt][r] : 0.f;               \
            }                                                                                                    \
        }                                                                                                        \
        _Pragma("unroll") for (int ut = 0; ut < DH / 16; ++ut)                                                   \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) acc[ut][r] *= corr;                                    \
        ba_mma_turned<T, DH>(acc, ks + G::ROW, e, lane);                            /* :133 */                   \
    } while (0)
    BA_WALK(live, NST, BA_LOAD, BA_COMMIT, BA_COMPUTE);
#undef BA_LOAD
#undef BA_COMMIT
#undef BA_COMPUTE
    if (q >= p.T) return;
    const float inv = dk.scale / l_run;
    if (p.st_m && g4 == 0) { p.st_m[j.bp * p.T + q] = m_run; p.st_l[j.bp * p.T + q] = l_run; }
    T* dst = reinterpret_cast<T*>(p.out) + ((long)j.b * p.T + q) * p.C + j.head * DH;
#pragma unroll
    for (int ut = 0; ut < DH / 16; ++ut) {
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = acc[ut][r] * inv;
        frag_st<T>(dst + ut * 16 + g4, frag_from_acc<T>(o));
    }
}

// ---- backward, query sweep: D, dQ -----------------------------------------------------------------------------------------
template <typename T, int DH>
__global__ __launch_bounds__(256) void ba_bwd_q_kernel(BaP p) {
    using G = BaGeo<T, DH>; using O = BaOp<T, DH>;
    constexpr int NST = G::nst(G::STAGE_Q);
    extern __shared__ __attribute__((aligned(16))) unsigned char ba_smem[];
    __shared__ uint32_t s_live;
    float* madd = reinterpret_cast<float*>(ba_smem);
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15, wave = threadIdx.x >> 6;
    const BaJob j = ba_job(p);
    const uint32_t live = ba_mask(p.ids + (long)j.b * p.T, p.T, p.NB, madd, &s_live);
    const long ld = 3L * p.C;
    const T* base = reinterpret_cast<const T*>(p.qkv) + (long)j.b * p.T * ld + j.head * DH;
    const int q = j.blk * BA_BLK + wave * 16 + l15, qc = min(q, p.T - 1);
    const bool qok = q < p.T;
    const DropKey dk = make_dropkey(p.rng, p.stream_id, p.rate);
    const uint32_t dbase = (uint32_t)((j.bp * p.T + qc) * p.T);
    const long orow = ((long)j.b * p.T + qc) * p.C + j.head * DH;
    typename O::F qf[O::N], gf[O::N];
    float dsum = 0.f;
#pragma unroll
    for (int i = 0; i < O::N; ++i) {
        qf[i] = O::ld(base + (long)qc * ld, i, lane);
        gf[i] = O::ld(reinterpret_cast<const T*>(p.d_out) + orow, i, lane);
        const typename O::F o = O::ld(reinterpret_cast<const T*>(p.out) + orow, i, lane);
#pragma unroll
        for (int e = 0; e < O::KW; ++e) dsum += to_f32(gf[i].v[e]) * to_f32(o.v[e]);
    }
    dsum = group_sum4(dsum);
    if (qok && g4 == 0) p.st_d[j.bp * p.T + q] = dsum;
    const float m = p.st_m[j.bp * p.T + qc], invl = 1.0f / p.st_l[j.bp * p.T + qc];
    f32x4 acc[DH / 16];
#pragma unroll
    for (int ut = 0; ut < DH / 16; ++ut) acc[ut] = f32x4{0.f, 0.f, 0.f, 0.f};
    BaTile<T, DH> kr, vr;
    auto stage = [&](int s) { return reinterpret_cast<T*>(ba_smem + BA_MASK_BYTES + s * G::STAGE_Q); };
#define BA_LOAD(jb) do { ba_load<T, DH>(kr, base + p.C, ld, (jb) * BA_BLK, p.T); ba_load<T, DH>(vr, base + 2 * p.C, ld, (jb) * BA_BLK, p.T); } while (0)
#define BA_COMMIT(s) do { ba_store_rows<T, DH>(stage(s), kr); ba_store_rows<T, DH>(stage(s) + G::ROW, vr); ba_store_turned<T, DH>(stage(s) + 2 * G::ROW, kr); } while (0)
#define BA_COMPUTE(jb, s) do {                                                                                   \
        const T* ks = stage(s);                                                                                  \
        f32x4 ds[4];                                                                                             \
        _Pragma("unroll") for (int kt = 0; kt < 4; ++kt) {                                                       \
            const f32x4 sc = ba_mma_rows<T, DH>(ks, kt, qf, lane), da = ba_mma_rows<T, DH>(ks + G::ROW, kt, gf, lane); \
            const f32x4 ma = *reinterpret_cast<const f32x4*>(madd + (jb) * BA_BLK + kt * 16 + g4);               \
            bool keep[4] = {true, true, true, true};                                                             \
            if (dk.thresh != 0u) ba_keep4(dk, dbase, (jb) * BA_BLK + kt * 16 + g4, keep);                        \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                      \
                const float P = __expf((ma[r] == 0.f ? sc[r] * p.cscale : ma[r]) - m) * invl;                    \
                const float dP = keep[r] ? da[r] * dk.scale : 0.f;                                               \
                /* a replaced score is a constant (tf.where): no gradient, in an all-padding (uniform) row either */ \
                ds[kt][r] = (ma[r] != 0.f || !qok) ? 0.f : P * (dP - dsum) * p.cscale;                           \
            }                                                                                                    \
        }                                                                                                        \
        ba_mma_turned<T, DH>(acc, ks + 2 * G::ROW, ds, lane);                                                    \
    } while (0)
    BA_WALK(live, NST, BA_LOAD, BA_COMMIT, BA_COMPUTE);
#undef BA_LOAD
#undef BA_COMMIT
#undef BA_COMPUTE
    if (!qok) return;
    T* dst = reinterpret_cast<T*>(p.d_qkv) + ((long)j.b * p.T + q) * ld + j.head * DH;
#pragma unroll
    for (int ut = 0; ut < DH / 16; ++ut) frag_st<T>(dst + ut * 16 + g4, frag_from_acc<T>(acc[ut]));
}

// ---- backward, key sweep: dK, dV ------------------------------------------------------------------------------------------
template <typename T, int DH>
__global__ __launch_bounds__(256) void ba_bwd_k_kernel(BaP p) {
    using G = BaGeo<T, DH>; using O = BaOp<T, DH>;
    constexpr int NST = G::nst(G::STAGE_K);
    extern __shared__ __attribute__((aligned(16))) unsigned char ba_smem[];
    __shared__ uint32_t s_live;
    float* madd = reinterpret_cast<float*>(ba_smem);
    const int lane = threadIdx.x & 63, g4 = (lane >> 4) * 4, l15 = lane & 15, wave = threadIdx.x >> 6;
    const BaJob j = ba_job(p);
    const uint32_t live = ba_mask(p.ids + (long)j.b * p.T, p.T, p.NB, madd, &s_live);
    const long ld = 3L * p.C;
    const T* base = reinterpret_cast<const T*>(p.qkv) + (long)j.b * p.T * ld + j.head * DH;
    T* dbase_kv = reinterpret_cast<T*>(p.d_qkv) + (long)j.b * p.T * ld + p.C + j.head * DH;
    if (!((live >> j.blk) & 1u)) {            // a block of padded keys in a sample that has a real key: exact zeros
        for (int c = threadIdx.x; c < G::CHUNKS; c += 256) {
            const int k = j.blk * BA_BLK + c / G::CPR;
            if (k < p.T) {
                st16<T>(dbase_kv + (long)k * ld + (c % G::CPR) * G::VEC, zero16<T>());
                st16<T>(dbase_kv + (long)k * ld + p.C + (c % G::CPR) * G::VEC, zero16<T>());
            }
        }
        return;
    }
    const int k = j.blk * BA_BLK + wave * 16 + l15, kc = min(k, p.T - 1);
    const float ma = madd[k];                 // 0 real, PADV padded, -inf past the end
    const DropKey dk = make_dropkey(p.rng, p.stream_id, p.rate);
    const T* dOb = reinterpret_cast<const T*>(p.d_out) + (long)j.b * p.T * p.C + j.head * DH;
    typename O::F kf[O::N], vf[O::N];
#pragma unroll
    for (int i = 0; i < O::N; ++i) {
        kf[i] = O::ld(base + (long)kc * ld + p.C, i, lane);
        vf[i] = O::ld(base + (long)kc * ld + 2 * p.C, i, lane);
    }
    f32x4 accK[DH / 16], accV[DH / 16];
#pragma unroll
    for (int ut = 0; ut < DH / 16; ++ut) { accK[ut] = f32x4{0.f, 0.f, 0.f, 0.f}; accV[ut] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    BaTile<T, DH> qr, gr;
    float sreg = 0.f;                         // m | l | D of the block's 64 queries: one value per thread of the first three waves
    auto stage = [&](int s) { return reinterpret_cast<T*>(ba_smem + BA_MASK_BYTES + s * G::STAGE_K); };
    auto stats = [&](int s) { return reinterpret_cast<float*>(ba_smem + BA_MASK_BYTES + s * G::STAGE_K + (2 * G::ROW + 2 * G::TRN) * (int)sizeof(T)); };
#define BA_LOAD(jb) do {                                                                                         \
        ba_load<T, DH>(qr, base, ld, (jb) * BA_BLK, p.T); ba_load<T, DH>(gr, dOb, p.C, (jb) * BA_BLK, p.T);       \
        if (wave < 3) sreg = (wave == 0 ? p.st_m : wave == 1 ? p.st_l : p.st_d)[j.bp * p.T + min((jb) * BA_BLK + lane, p.T - 1)]; \
    } while (0)
#define BA_COMMIT(s) do {                                                                                        \
        ba_store_rows<T, DH>(stage(s), qr); ba_store_rows<T, DH>(stage(s) + G::ROW, gr);                         \
        ba_store_turned<T, DH>(stage(s) + 2 * G::ROW, qr); ba_store_turned<T, DH>(stage(s) + 2 * G::ROW + G::TRN, gr); \
        if (wave < 3) stats(s)[wave * BA_BLK + lane] = sreg;                                                     \
    } while (0)
#define BA_COMPUTE(jb, s) do {                                                                                   \
        const T* qs = stage(s);                                                                                  \
        const float* stt = stats(s);                                                                             \
        f32x4 a4[4], ds[4];                                                                                      \
        _Pragma("unroll") for (int qt = 0; qt < 4; ++qt) {                                                       \
            const f32x4 sc = ba_mma_rows<T, DH>(qs, qt, kf, lane), da = ba_mma_rows<T, DH>(qs + G::ROW, qt, vf, lane); \
            const f32x4 mq = *reinterpret_cast<const f32x4*>(stt + qt * 16 + g4);                                \
            const f32x4 lq = *reinterpret_cast<const f32x4*>(stt + BA_BLK + qt * 16 + g4);                       \
            const f32x4 dq = *reinterpret_cast<const f32x4*>(stt + 2 * BA_BLK + qt * 16 + g4);                   \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                      \
                const int qq = (jb) * BA_BLK + qt * 16 + g4 + r;                                                 \
                const float v = ma == 0.f ? sc[r] * p.cscale : ma;                                               \
                const float P = qq < p.T ? __expf(v - mq[r]) / lq[r] : 0.f;                                      \
                bool keep = true;                                                                                \
                if (dk.thresh != 0u) {     /* the forward's pairing: one hash per (k even, k + 1) of a row */    \
                    const uint32_t h = drop_hash_pair(dk, (uint32_t)((j.bp * p.T + qq) * p.T) + (uint32_t)(k & ~1)); \
                    keep = ((k & 1) ? (h >> 16) : (h & 0xffffu)) >= dk.t16;                                      \
                }                                                                                                \
                a4[qt][r] = keep ? P * dk.scale : 0.f;                                                           \
                const float dP = keep ? da[r] * dk.scale : 0.f;                                                  \
                ds[qt][r] = (ma != 0.f || qq >= p.T) ? 0.f : P * (dP - dq[r]) * p.cscale;                        \
            }                                                                                                    \
        }                                                                                                        \
        ba_mma_turned<T, DH>(accV, qs + 2 * G::ROW + G::TRN, a4, lane);                                          \
        ba_mma_turned<T, DH>(accK, qs + 2 * G::ROW, ds, lane);                                                   \
    } while (0)
    BA_WALK((1u << p.NB) - 1u, NST, BA_LOAD, BA_COMMIT, BA_COMPUTE);
#undef BA_LOAD
#undef BA_COMMIT
#undef BA_COMPUTE
    if (k >= p.T) return;
    T* dst = dbase_kv + (long)k * ld;
#pragma unroll
    for (int ut = 0; ut < DH / 16; ++ut) {
        frag_st<T>(dst + ut * 16 + g4, frag_from_acc<T>(accK[ut]));
        frag_st<T>(dst + p.C + ut * 16 + g4, frag_from_acc<T>(accV[ut]));
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
inline size_t ba_rows(int B, int T, int H) { return ((size_t)B * H * T + 63) & ~(size_t)63; }

int ba_check(const char* who, int B, int T, int H, int C, int dtype) {
    const int dh = H > 0 && C > 0 && C % H == 0 ? C / H : 0;
    EDGL_REQUIRE(B > 0 && T >= 1 && T <= 1025, EDGL_ERR_SHAPE, "%s: bad shape B=%d T=%d (1 <= T <= 1025)", who, B, T);
    EDGL_REQUIRE(dh == 16 || dh == 32 || dh == 64 || dh == 128, EDGL_ERR_SHAPE,
                 "%s: C=%d H=%d unsupported (head dim C/H in {16, 32, 64, 128})", who, C, H);
    EDGL_REQUIRE(dtype == EDGL_F32 || dtype == EDGL_BF16, EDGL_ERR_DTYPE, "%s: bad dtype %d", who, dtype);
    EDGL_REQUIRE((double)B * H * T * T < 4294967296.0, EDGL_ERR_SHAPE, "%s: H*B*T*T must be < 2^32", who);
    EDGL_REQUIRE((double)B * H * ((T + BA_BLK - 1) / BA_BLK) < 2147483647.0, EDGL_ERR_SHAPE, "%s: too many workgroups", who);
    return EDGL_OK;
}

// which = 0: forward, 1: query sweep, 2: key sweep
template <typename T, int DH>
int ba_launch_one(const BaP& p, int which, hipStream_t st) {
    using G = BaGeo<T, DH>;
    const dim3 grid((unsigned)((long)p.B * p.H * p.NB)), block(256);
    if (which == 0) {
        EDGL_LDS_LIMIT((ba_fwd_kernel<T, DH>), G::smem(G::STAGE_F), "edgl_battn_fwd");
        hipLaunchKernelGGL((ba_fwd_kernel<T, DH>), grid, block, G::smem(G::STAGE_F), st, p);
    } else if (which == 1) {
        EDGL_LDS_LIMIT((ba_bwd_q_kernel<T, DH>), G::smem(G::STAGE_Q), "edgl_battn_bwd");
        hipLaunchKernelGGL((ba_bwd_q_kernel<T, DH>), grid, block, G::smem(G::STAGE_Q), st, p);
    } else {
        EDGL_LDS_LIMIT((ba_bwd_k_kernel<T, DH>), G::smem(G::STAGE_K), "edgl_battn_bwd");
        hipLaunchKernelGGL((ba_bwd_k_kernel<T, DH>), grid, block, G::smem(G::STAGE_K), st, p);
    }
    EDGL_LAUNCH_CHECK();
    return EDGL_OK;
}
template <typename T>
int ba_launch(const BaP& p, int which, hipStream_t st) {
    switch (p.C / p.H) {
        case 16: return ba_launch_one<T, 16>(p, which, st);
        case 32: return ba_launch_one<T, 32>(p, which, st);
        case 64: return ba_launch_one<T, 64>(p, which, st);
        case 128: return ba_launch_one<T, 128>(p, which, st);
    }
    edgl_set_error("edgl_battn: C=%d H=%d not supported", p.C, p.H);
    return EDGL_ERR_SHAPE;
}

BaP ba_params(const void* qkv, const int64_t* ids, int B, int T, int H, int C, float scale, float drop_rate, const uint64_t* rng_state,
              uint32_t stream_id, void* out, void* saved) {
    BaP p{};
    p.qkv = qkv; p.ids = ids; p.B = B; p.T = T; p.H = H; p.C = C; p.NB = (T + BA_BLK - 1) / BA_BLK;
    p.cscale = scale; p.rate = drop_rate; p.rng = rng_state; p.stream_id = stream_id; p.out = out;
    if (saved) {
        const size_t R = ba_rows(B, T, H);
        p.st_m = reinterpret_cast<float*>(saved); p.st_l = p.st_m + R; p.st_d = p.st_l + R;
    }
    return p;
}

}  // namespace

extern "C" int edgl_battn_supported(int T, int H, int dh, int dtype) {
    return T >= 1 && T <= 1025 && H >= 1 && (dh == 16 || dh == 32 || dh == 64 || dh == 128) && (dtype == EDGL_F32 || dtype == EDGL_BF16);
}

extern "C" long edgl_battn_saved_bytes(int B, int T, int H) {
    if (B <= 0 || T <= 0 || H <= 0) return -1;
    return (long)(3 * ba_rows(B, T, H) * 4);       // softmax max | sum (forward), D = rowsum(dO o O) (query sweep -> key sweep)
}

extern "C" int edgl_battn_fwd(const void* qkv, const int64_t* ids, int B, int T, int H, int C, float scale, float drop_rate,
                              const uint64_t* rng_state, uint32_t stream_id, void* out, void* saved, int dtype, void* stream) {
    EDGL_REQUIRE(qkv && ids && out, EDGL_ERR_NULL, "edgl_battn_fwd: null pointer");
    if (int rc = ba_check("edgl_battn_fwd", B, T, H, C, dtype)) return rc;
    EDGL_REQUIRE(drop_rate == 0.f || rng_state, EDGL_ERR_NULL, "edgl_battn_fwd: dropout without rng_state");
    const BaP p = ba_params(qkv, ids, B, T, H, C, scale, drop_rate, rng_state, stream_id, out, saved);
    return dtype == EDGL_F32 ? ba_launch<float>(p, 0, (hipStream_t)stream) : ba_launch<bf16>(p, 0, (hipStream_t)stream);
}

extern "C" int edgl_battn_bwd(const void* qkv, const int64_t* ids, const void* out, const void* d_out, void* saved, int B, int T,
                              int H, int C, float scale, float drop_rate, const uint64_t* rng_state, uint32_t stream_id,
                              void* d_qkv, int dtype, void* stream) {
    EDGL_REQUIRE(qkv && ids && out && d_out && saved && d_qkv, EDGL_ERR_NULL, "edgl_battn_bwd: null pointer");
    if (int rc = ba_check("edgl_battn_bwd", B, T, H, C, dtype)) return rc;
    EDGL_REQUIRE(drop_rate == 0.f || rng_state, EDGL_ERR_NULL, "edgl_battn_bwd: dropout without rng_state");
    BaP p = ba_params(qkv, ids, B, T, H, C, scale, drop_rate, rng_state, stream_id, const_cast<void*>(out), saved);
    p.d_out = d_out; p.d_qkv = d_qkv;
    for (int which = 1; which <= 2; ++which)      // the key sweep reads the D the query sweep left
        if (int rc = dtype == EDGL_F32 ? ba_launch<float>(p, which, (hipStream_t)stream) : ba_launch<bf16>(p, which, (hipStream_t)stream))
            return rc;
    return EDGL_OK;
}
