// Intent-aware aggregation of DCCF (reference models/general_cf/dccf.py:77-80) on the stacked table X = [users; items]:
//   Y_r = softmax(X_r C) C^T,  C = C_u for rows [0, n_split), C_i for rows [n_split, N),  C [d, K] row-major
// forward and backward in one launch each for both row ranges, without anything of size N x K in global memory: the backward
// recomputes the probabilities from X, C and one saved float per row (the log-sum-exp of the row's logits).
//
// Layout.  A workgroup of 4 waves belongs to ONE row range and keeps that range's C in LDS for its lifetime (row stride
// 32 KB + 1 floats: rows are read along k by the first product and down i by the second, both free of bank conflicts; the
// columns K .. 32 KB - 1 are zero).  A wave owns tiles of 32 rows of its range -- tiles are counted per range, so none holds rows
// of both.  All products are exact-fp32 MFMAs (32x32x2) formed TRANSPOSED, Z^T = C^T X^T: the accumulator then has the tile's ROW
// on the lane (row = lane & 31) and the logits k = 32 kb + (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) in its registers, so
//   * the softmax of a row is a sum inside a lane plus ONE exchange with lane ^ 32;
//   * P^T is already the B operand of the next product Y^T = C P^T (the sum over k may run in any order: a step takes k from the
//     low half and k + 4 from the high half), no movement between lanes, no LDS.
// Only dC = X^T dZ + dY^T P sums over rows, i.e. over lanes: dZ^T and P^T go through a 32 x 33 LDS tile per wave, one block of 32
// logits at a time.  dC has no atomics: a wave keeps its sum in registers over all its tiles, the 4 waves add up in a fixed order in
// LDS, the workgroup writes its [d, K] slab to the workspace and a second kernel adds the slabs in a fixed order.
#include "common.h"

namespace {

typedef float in_f32x4 __attribute__((ext_vector_type(4)));
typedef float in_f32x16 __attribute__((ext_vector_type(16)));

constexpr int IN_WAVES = 4;
constexpr int IN_FWD_CAP = 1024;       // workgroups per row range at most (each loads C once)
constexpr int IN_BWD_CAP = 256;        // ... in the backward: one [d, K] slab of the workspace each
constexpr int IN_TSTRIDE = 33;         // row stride of the per-wave transposition tile

__device__ __forceinline__ void in_wave_sync() {          // LDS traffic between the lanes of ONE wave
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// row blocks of dC a backward workgroup accumulates (16 accumulator registers per 32 x 32 block, at most 128 in all)
template <int D, int KB> struct InCfg {
    static constexpr int DB = D / 32;
    static constexpr int DC = (DB * KB <= 8) ? DB : ((8 / KB) > 0 ? 8 / KB : 1);
    static constexpr int CHUNKS = DB / DC;
    static constexpr int KS = KB * 32 + 1;
    static constexpr int C_FLOATS = D * KS;
    static constexpr int RED_FLOATS = DC * KB * 16 * 64;
    static constexpr int BWD_MAIN = C_FLOATS > RED_FLOATS ? C_FLOATS : RED_FLOATS;
    static constexpr size_t FWD_LDS = (size_t)C_FLOATS * 4;
    static constexpr size_t BWD_LDS = (size_t)(BWD_MAIN + IN_WAVES * 32 * IN_TSTRIDE) * 4;
};

struct InRange {
    const float *C;
    int lo, hi, g, G;                  // rows [lo, hi), this workgroup's index among the G of the range
};

__device__ __forceinline__ InRange in_range(const float *C_u, const float *C_i, int N, int n_split, int G_u) {
    InRange r;
    if ((int)blockIdx.x < G_u) {
        r.C = C_u; r.lo = 0; r.hi = n_split; r.g = blockIdx.x; r.G = G_u;
    } else {
        r.C = C_i; r.lo = n_split; r.hi = N; r.g = blockIdx.x - G_u; r.G = gridDim.x - G_u;
    }
    return r;
}

template <int D, int KB>
__device__ __forceinline__ void in_load_c(float *lds, const float *__restrict__ C, int K) {
    constexpr int KS = KB * 32 + 1;
    for (int e = threadIdx.x; e < D * KS; e += IN_WAVES * 64) {
        const int i = e / KS, k = e - i * KS;
        lds[e] = (k < K) ? C[(size_t)i * K + k] : 0.f;
    }
    __syncthreads();
}

// this lane's half of row `row` of a [*, D] table: columns [half D / 2, (half + 1) D / 2); zeros for a row past the range
template <int D>
__device__ __forceinline__ void in_load_half_row(const float *__restrict__ T, long long row, bool valid, int half, float (&v)[D / 2]) {
    const in_f32x4 *p = reinterpret_cast<const in_f32x4 *>(T + (size_t)row * D + half * (D / 2));
#pragma unroll
    for (int j = 0; j < D / 8; ++j) {
        in_f32x4 q = {0.f, 0.f, 0.f, 0.f};
        if (valid) q = p[j];
        v[4 * j] = q.x; v[4 * j + 1] = q.y; v[4 * j + 2] = q.z; v[4 * j + 3] = q.w;
    }
}

// acc[kb] = (C^T V^T) block kb: acc[kb][reg] = <V_row, C[:, k(kb, reg, half)]>
template <int D, int KB>
__device__ __forceinline__ void in_logits(const float *lds, const float (&v)[D / 2], int l32, int half, in_f32x16 (&acc)[KB]) {
    constexpr int KS = KB * 32 + 1;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[kb][r] = 0.f;
#pragma unroll
        for (int s = 0; s < D / 2; ++s)
            acc[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[(half * (D / 2) + s) * KS + kb * 32 + l32], v[s], acc[kb], 0, 0, 0);
    }
}

// out[row, :] = sum_k W[row, k] C[:, k] for the accumulator-layout weights W, stored as float4s
template <int D, int KB>
__device__ __forceinline__ void in_project_store(const float *lds, const in_f32x16 (&w)[KB], int l32, int half, float *__restrict__ out,
                                                 long long row, bool valid) {
    constexpr int KS = KB * 32 + 1;
#pragma unroll
    for (int ib = 0; ib < D / 32; ++ib) {
        in_f32x16 y;
#pragma unroll
        for (int r = 0; r < 16; ++r) y[r] = 0.f;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                y = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[(ib * 32 + l32) * KS + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half], w[kb][r], y, 0,
                                                         0, 0);
        if (valid) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                in_f32x4 o = {y[4 * q], y[4 * q + 1], y[4 * q + 2], y[4 * q + 3]};
                *reinterpret_cast<in_f32x4 *>(out + (size_t)row * D + ib * 32 + 8 * q + 4 * half) = o;
            }
        }
    }
}

template <int D, int KB>
__global__ __launch_bounds__(256, D * KB <= 128 ? 2 : 1) void intent_fwd_kernel(const float *__restrict__ X, int N, int n_split, const float *__restrict__ C_u,
                                                         const float *__restrict__ C_i, int K, int G_u, float *__restrict__ Y,
                                                         float *__restrict__ lse) {
    extern __shared__ float in_lds[];
    const InRange rg = in_range(C_u, C_i, N, n_split, G_u);
    in_load_c<D, KB>(in_lds, rg.C, K);
    const int lane = threadIdx.x & 63, l32 = lane & 31, half = lane >> 5, wave = wave_in_block();
    const int tiles = (rg.hi - rg.lo + 31) / 32;
    for (int t = rg.g * IN_WAVES + wave; t < tiles; t += rg.G * IN_WAVES) {
        const long long row = (long long)rg.lo + (long long)t * 32 + l32;
        const bool valid = row < rg.hi;
        float xb[D / 2];
        in_load_half_row<D>(X, row, valid, half, xb);
        in_f32x16 z[KB];
        in_logits<D, KB>(in_lds, xb, l32, half, z);
        float m = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (k >= K) z[kb][r] = -INFINITY;                        // a padded logit: exp = 0, not exp(0)
                m = fmaxf(m, z[kb][r]);
            }
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float s = 0.f;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                z[kb][r] = expf(z[kb][r] - m);
                s += z[kb][r];
            }
        s += __shfl_xor(s, 32, 64);
        const float inv = 1.f / s;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) z[kb][r] *= inv;
        if (lse && valid && half == 0) lse[row] = m + logf(s);
        in_project_store<D, KB>(in_lds, z, l32, half, Y, row, valid);
    }
}

template <int D, int KB>
__global__ __launch_bounds__(256) void intent_bwd_kernel(const float *__restrict__ X, const float *__restrict__ dY,
                                                         const float *__restrict__ lse, int N, int n_split,
                                                         const float *__restrict__ C_u, const float *__restrict__ C_i, int K, int G_u,
                                                         float *__restrict__ dX, float *__restrict__ ws) {
    using Cfg = InCfg<D, KB>;
    constexpr int DC = Cfg::DC, KS = Cfg::KS, KP = KB * 32;
    extern __shared__ float in_lds[];
    const InRange rg = in_range(C_u, C_i, N, n_split, G_u);
    in_load_c<D, KB>(in_lds, rg.C, K);
    const int lane = threadIdx.x & 63, l32 = lane & 31, half = lane >> 5, wave = wave_in_block();
    const int chunk = blockIdx.y;                              // which DC row blocks of dC this workgroup sums; chunk 0 also writes dX
    float *tile = in_lds + Cfg::BWD_MAIN + wave * (32 * IN_TSTRIDE);
    in_f32x16 dc[DC][KB];
#pragma unroll
    for (int a = 0; a < DC; ++a)
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) dc[a][kb][r] = 0.f;
    const int tiles = (rg.hi - rg.lo + 31) / 32;
    for (int t = rg.g * IN_WAVES + wave; t < tiles; t += rg.G * IN_WAVES) {
        const long long row0 = (long long)rg.lo + (long long)t * 32, row = row0 + l32;
        const bool valid = row < rg.hi;
        in_f32x16 p[KB], dz[KB];
        {
            float xb[D / 2];
            in_load_half_row<D>(X, row, valid, half, xb);
            in_logits<D, KB>(in_lds, xb, l32, half, p);
        }
        {
            float gb[D / 2];
            in_load_half_row<D>(dY, row, valid, half, gb);
            in_logits<D, KB>(in_lds, gb, l32, half, dz);       // dP
        }
        const float l = valid ? lse[row] : 0.f;
        float dot = 0.f;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                p[kb][r] = (valid && k < K) ? expf(p[kb][r] - l) : 0.f;
                dot = fmaf(p[kb][r], dz[kb][r], dot);
            }
        dot += __shfl_xor(dot, 32, 64);
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) dz[kb][r] = p[kb][r] * (dz[kb][r] - dot);
        if (chunk == 0) in_project_store<D, KB>(in_lds, dz, l32, half, dX, row, valid);
        // dC[i, k] += sum over the tile's rows of X[row, i] dZ[row, k] + dY[row, i] P[row, k]; A operand straight from global memory
        // (lane = column i: coalesced, the tile was read a moment ago), B operand from the transposition tile
        float xa[DC][16], ga[DC][16];
#pragma unroll
        for (int a = 0; a < DC; ++a)
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const long long rr = row0 + 2 * s + half;
                const size_t at = (size_t)rr * D + (chunk * DC + a) * 32 + l32;
                const bool ok = rr < rg.hi;
                xa[a][s] = ok ? X[at] : 0.f;
                ga[a][s] = ok ? dY[at] : 0.f;
            }
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                in_wave_sync();                                 // (the previous block's readers are done)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    tile[l32 * IN_TSTRIDE + (r & 3) + 8 * (r >> 2) + 4 * half] = pass == 0 ? dz[kb][r] : p[kb][r];
                in_wave_sync();
#pragma unroll
                for (int a = 0; a < DC; ++a)
#pragma unroll
                    for (int s = 0; s < 16; ++s)
                        dc[a][kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(pass == 0 ? xa[a][s] : ga[a][s],
                                                                         tile[(2 * s + half) * IN_TSTRIDE + l32], dc[a][kb], 0, 0, 0);
            }
        }
    }
    // the 4 waves' sums, added in the order of the waves, then the workgroup's slab
    float *red = in_lds;
    for (int w = 0; w < IN_WAVES; ++w) {
        __syncthreads();                                       // (first round: every wave is done with C)
        if (wave == w) {
#pragma unroll
            for (int a = 0; a < DC; ++a)
#pragma unroll
                for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int at = ((a * KB + kb) * 16 + r) * 64 + lane;
                        red[at] = (w == 0) ? dc[a][kb][r] : red[at] + dc[a][kb][r];
                    }
        }
    }
    __syncthreads();
    float *slab = ws + (size_t)blockIdx.x * (D * KP);
    for (int e = threadIdx.x; e < DC * KB * 16 * 64; e += IN_WAVES * 64) {
        const int ln = e & 63, r = (e >> 6) & 15, blk = e >> 10, kb = blk % KB, a = blk / KB;
        const int i = (chunk * DC + a) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5), k = kb * 32 + (ln & 31);
        slab[i * KP + k] = red[e];
    }
}

// dC[i, k] = sum over the range's slabs in index order (four interleaved partial sums, combined in a fixed order)
__global__ __launch_bounds__(256) void intent_reduce_kernel(const float *__restrict__ ws, int G_u, int G_i, int d, int K, int KP,
                                                            float *__restrict__ dC_u, float *__restrict__ dC_i) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= d * K) return;
    const int which = blockIdx.y;
    float *out = which == 0 ? dC_u : dC_i;
    if (!out) return;
    const int g0 = which == 0 ? 0 : G_u, G = which == 0 ? G_u : G_i;
    const int i = e / K, k = e - i * K;
    const float *src = ws + (size_t)g0 * d * KP + (size_t)i * KP + k;
    const size_t step = (size_t)d * KP;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int g = 0;
    for (; g + 4 <= G; g += 4) {
        s0 += src[(size_t)g * step];
        s1 += src[(size_t)(g + 1) * step];
        s2 += src[(size_t)(g + 2) * step];
        s3 += src[(size_t)(g + 3) * step];
    }
    for (; g < G; ++g) s0 += src[(size_t)g * step];
    out[e] = (s0 + s1) + (s2 + s3);
}

inline int in_kb(int K) { return K <= 32 ? 1 : (K <= 64 ? 2 : (K <= 128 ? 4 : 8)); }

inline int in_groups(long long rows, int cap) {
    const long long g = (rows + 32 * IN_WAVES - 1) / (32 * IN_WAVES);
    return (int)(g < cap ? g : cap);
}

inline bool in_args_ok(int64_t N, int64_t n_split, int d, int K, const void *C_u, const void *C_i) {
    if (N < 0 || N > 0x7fffffff || n_split < 0 || n_split > N || (d != 32 && d != 64 && d != 128) || K < 1 || K > 256) return false;
    if (n_split > 0 && !C_u) return false;
    if (n_split < N && !C_i) return false;
    return true;
}

#define SSLREC_INTENT_DISPATCH(d, kb, CALL)                                                           \
    switch ((d) * 16 + (kb)) {                                                                        \
    case 32 * 16 + 1: CALL(32, 1); break;                                                             \
    case 32 * 16 + 2: CALL(32, 2); break;                                                             \
    case 32 * 16 + 4: CALL(32, 4); break;                                                             \
    case 32 * 16 + 8: CALL(32, 8); break;                                                             \
    case 64 * 16 + 1: CALL(64, 1); break;                                                             \
    case 64 * 16 + 2: CALL(64, 2); break;                                                             \
    case 64 * 16 + 4: CALL(64, 4); break;                                                             \
    case 64 * 16 + 8: CALL(64, 8); break;                                                             \
    case 128 * 16 + 1: CALL(128, 1); break;                                                           \
    case 128 * 16 + 2: CALL(128, 2); break;                                                           \
    case 128 * 16 + 4: CALL(128, 4); break;                                                           \
    default: CALL(128, 8); break;                                                                     \
    }

}      // namespace

extern "C" {

size_t sslrec_intent_ws_bytes(int32_t N, int32_t n_split, int32_t d, int32_t K) {
    if (N < 0 || n_split < 0 || n_split > N || (d != 32 && d != 64 && d != 128) || K < 1 || K > 256) return 0;
    const size_t G = (size_t)in_groups(n_split, IN_BWD_CAP) + (size_t)in_groups((long long)N - n_split, IN_BWD_CAP);
    return G * (size_t)d * (size_t)(in_kb(K) * 32) * sizeof(float);
}

int sslrec_intent_fwd_f32(const float *X, int32_t N, int32_t n_split, int32_t d, const float *C_u, const float *C_i, int32_t K, float *Y,
                          float *lse, void *stream) {
    if (!in_args_ok(N, n_split, d, K, C_u, C_i) || !X || !Y) return SSLREC_E_BADARG;
    if (N == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int G_u = in_groups(n_split, IN_FWD_CAP), G_i = in_groups((long long)N - n_split, IN_FWD_CAP);
#define CALL(D, KB)                                                                                                                       \
    {                                                                                                                                     \
        const size_t lds = InCfg<D, KB>::FWD_LDS;                                                                                         \
        if (lds > 65536) {                                                                                                                \
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(intent_fwd_kernel<D, KB>),                                  \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                                     \
            if (e != hipSuccess) return (int)e;                                                                                           \
        }                                                                                                                                 \
        hipLaunchKernelGGL((intent_fwd_kernel<D, KB>), dim3((unsigned)(G_u + G_i)), dim3(IN_WAVES * 64), lds, st, X, (int)N, (int)n_split, \
                           C_u, C_i, (int)K, G_u, Y, lse);                                                                                \
    }
    SSLREC_INTENT_DISPATCH(d, in_kb(K), CALL)
#undef CALL
    SSLREC_LAUNCH_CHECK();
    return 0;
}

int sslrec_intent_bwd_f32(const float *X, const float *dY, const float *lse, int32_t N, int32_t n_split, int32_t d, const float *C_u,
                          const float *C_i, int32_t K, float *dX, float *dC_u, float *dC_i, void *ws, void *stream) {
    if (!in_args_ok(N, n_split, d, K, C_u, C_i) || !X || !dY || !lse || !dX) return SSLREC_E_BADARG;
    if ((n_split > 0 && !dC_u) || (n_split < N && !dC_i) || (N > 0 && !ws)) return SSLREC_E_BADARG;
    if (N == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int G_u = in_groups(n_split, IN_BWD_CAP), G_i = in_groups((long long)N - n_split, IN_BWD_CAP);
    const int kb = in_kb(K);
    {
#define CALL(D, KB)                                                                                                                       \
    {                                                                                                                                     \
        const size_t lds = InCfg<D, KB>::BWD_LDS;                                                                                         \
        if (lds > 65536) {                                                                                                                \
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(intent_bwd_kernel<D, KB>),                                  \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                                     \
            if (e != hipSuccess) return (int)e;                                                                                           \
        }                                                                                                                                 \
        hipLaunchKernelGGL((intent_bwd_kernel<D, KB>), dim3((unsigned)(G_u + G_i), (unsigned)InCfg<D, KB>::CHUNKS), dim3(IN_WAVES * 64),  \
                           lds, st, X, dY, lse, (int)N, (int)n_split, C_u, C_i, (int)K, G_u, dX, (float *)ws);                            \
    }
        SSLREC_INTENT_DISPATCH(d, kb, CALL)
#undef CALL
    }
    if (dC_u || dC_i)          // (an empty range: its gradient, if asked for, is zero)
        hipLaunchKernelGGL(intent_reduce_kernel, dim3((unsigned)((d * K + 255) / 256), 2), dim3(256), 0, st, (const float *)ws, G_u, G_i,
                           (int)d, (int)K, kb * 32, dC_u, dC_i);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

}      // extern "C"
