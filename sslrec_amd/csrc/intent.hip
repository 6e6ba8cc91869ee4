// Intent-aware aggregation of DCCF (reference models/general_cf/dccf.py:77-80) on the stacked table X = [users; items]:
//   Y_r = softmax(X_r C) C^T,  C = C_u for rows [0, n_split), C_i for rows [n_split, N),  C [d, K] row-major
// forward and backward in one launch each for both row ranges, without anything of size N x K in global memory: the backward
// recomputes the probabilities from X, C and one saved float per row (the log-sum-exp of the row's logits).
//
// Layout and the tile helpers: rowtile.h.  The accumulator of the transposed product has the tile's ROW on the lane and the logits in
// its registers, so the softmax of a row is a sum inside a lane plus ONE exchange with lane ^ 32, and P^T is already the B operand of
// Y^T = C P^T.  Only dC = X^T dZ + dY^T P sums over rows: dZ^T and P^T go through the wave's transposition tile, and the workgroups'
// slabs are added in a fixed order by a second kernel -- no atomics.
#include "common.h"
#include "rowtile.h"

namespace {

constexpr int IN_FWD_CAP = 1024;       // workgroups per row range at most (each loads C once)
constexpr int IN_BWD_CAP = 256;        // ... in the backward: one [d, K] slab of the workspace each

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
    in_slab_store<D, KB>(in_lds, dc, chunk, ws + (size_t)blockIdx.x * (D * KP));
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
