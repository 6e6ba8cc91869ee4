// Self-gating units of MHCN (reference models/social/mhcn.py:34-52): Y_c = X (.) sigmoid(X W_c^T + b_c) for C <= 4 gates that share one
// table X [N, d], forward and backward, on the exact-fp32 MFMA through rowtile.h.
//
// The [d, d] matrices are handed in TRANSPOSED, Wt_c = W_c^T (row i = input feature, column k = output feature), stacked [C, d, d]; a
// workgroup keeps them in LDS with rowtile.h's padded row stride.  d = 32 / 64: all C matrices at once (4 x 64 x 65 floats = 66.5 KB),
// a tile's rows are read once and give all C outputs; d = 128: one matrix is 66 KB, the gates are taken in turn inside the launch.
// A wave owns tiles of 32 rows; in_logits leaves the tile's ROW on the lane and the logits of the columns
// k = 32 kb + (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) in its registers, i.e. four runs of 4 consecutive columns per block: X, dY and
// Y are read and written there as float4s.
//
// Backward recomputes the logits: nothing of size [N, d] is kept by the forward.  With T_c = dY_c (.) X (.) s_c (1 - s_c), s_c the gate,
//   dX    = sum_c (dY_c (.) s_c + T_c W_c)      in_project_block on the same LDS matrix; gates in turn, a lane adds to its own stores
//   dW_c  = T_c^T X                             in_rowsum_block into per-wave accumulators, the workgroup's slab, a fixed-order finish
//   db_c  = column sums of T_c                  column sums of the transposed blocks in the wave's tile, waves in order, the same finish
// No atomics; tiles are dealt to waves by index, so two calls give the same bits.
#include "common.h"
#include "rowtile.h"

namespace {

constexpr int SG_FWD_CAP = 1024;
constexpr int SG_BWD_CAP = 256;
constexpr int SG_MAX_GATES = 4;

struct SgPtrs {
    float *p[SG_MAX_GATES];
};
struct SgConstPtrs {
    const float *p[SG_MAX_GATES];
};

__device__ __forceinline__ float sg_sigmoid(const float z) {
    const float e = expf(-fabsf(z));
    return z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// the accumulator-layout float4 `q` of block `kb` of row `row`: columns kb 32 + 8 q + 4 half .. + 3
template <int D>
__device__ __forceinline__ in_f32x4 sg_load4(const float *__restrict__ T, long long row, bool valid, int kb, int q, int half) {
    in_f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (valid) v = *reinterpret_cast<const in_f32x4 *>(T + (size_t)row * D + kb * 32 + 8 * q + 4 * half);
    return v;
}

template <int D, int CG>
__global__ __launch_bounds__(256) void sg_fwd_kernel(const float *__restrict__ X, const int N, const float *__restrict__ Wt,
                                                     const float *__restrict__ B, const int C, const SgPtrs Y) {
    constexpr int KB = D / 32, CF = InCfg<D, KB>::C_FLOATS;
    extern __shared__ float sg_lds[];
    const int lane = threadIdx.x & 63, l32 = lane & 31, half = lane >> 5, wave = wave_in_block();
    const int tiles = (N + 31) / 32;
    for (int c0 = 0; c0 < C; c0 += CG) {
        if (c0) __syncthreads();                                       // (every wave is done with the previous matrices)
        const int cn = (C - c0) < CG ? (C - c0) : CG;
        for (int m = 0; m < cn; ++m) in_load_c<D, KB>(sg_lds + m * CF, Wt + (size_t)(c0 + m) * D * D, D);
        for (int t = blockIdx.x * IN_WAVES + wave; t < tiles; t += gridDim.x * IN_WAVES) {
            const long long row = (long long)t * 32 + l32;
            const bool valid = row < N;
            float xb[D / 2];
            in_load_half_row<D>(X, row, valid, half, xb);
            for (int m = 0; m < cn; ++m) {
                in_f32x16 z[KB];
                in_logits<D, KB>(sg_lds + m * CF, xb, l32, half, z);
                const float *bias = B + (size_t)(c0 + m) * D;
                float *y = Y.p[c0 + m];
#pragma unroll
                for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const in_f32x4 x4 = sg_load4<D>(X, row, valid, kb, q, half);
                        const in_f32x4 b4 = *reinterpret_cast<const in_f32x4 *>(bias + kb * 32 + 8 * q + 4 * half);
                        in_f32x4 o;
#pragma unroll
                        for (int j = 0; j < 4; ++j) o[j] = x4[j] * sg_sigmoid(z[kb][4 * q + j] + b4[j]);
                        if (valid) *reinterpret_cast<in_f32x4 *>(y + (size_t)row * D + kb * 32 + 8 * q + 4 * half) = o;
                    }
            }
        }
    }
}

// grid (G, CHUNKS): workgroup (g, chunk) sums the rows [chunk DC 32, (chunk + 1) DC 32) of every dW_c^T over its tiles; chunk 0 also
// writes dX and the db partials.  ws: slabs [C][G][D, D], then db partials [C][G][D].
template <int D>
__global__ __launch_bounds__(256) void sg_bwd_kernel(const float *__restrict__ X, const int N, const float *__restrict__ Wt,
                                                     const float *__restrict__ B, const int C, const SgConstPtrs dY, float *__restrict__ dX,
                                                     float *__restrict__ ws) {
    constexpr int KB = D / 32;
    using Cfg = InCfg<D, KB>;
    constexpr int DC = Cfg::DC;
    extern __shared__ float sg_lds[];
    const int lane = threadIdx.x & 63, l32 = lane & 31, half = lane >> 5, wave = wave_in_block();
    const int chunk = blockIdx.y, G = gridDim.x;
    float *tile_all = sg_lds + Cfg::BWD_MAIN;
    float *tile = tile_all + wave * (32 * IN_TSTRIDE);
    const int tiles = (N + 31) / 32;
    float *db_part = ws + (size_t)C * G * D * D;
    for (int c = 0; c < C; ++c) {
        if (c) __syncthreads();                                        // (the previous gate's slab and db reads are done)
        in_load_c<D, KB>(sg_lds, Wt + (size_t)c * D * D, D);
        const float *bias = B + (size_t)c * D;
        const float *g_y = dY.p[c];
        in_f32x16 dc[DC][KB];
        float tb[KB];                                                  // column l32 of block kb of T_c, summed over this half's rows
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            tb[kb] = 0.f;
#pragma unroll
            for (int a = 0; a < DC; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) dc[a][kb][r] = 0.f;
        }
        for (int t = blockIdx.x * IN_WAVES + wave; t < tiles; t += G * IN_WAVES) {
            const long long row0 = (long long)t * 32, row = row0 + l32;
            const bool valid = row < N;
            in_f32x16 tt[KB];                                          // T_c in the accumulator layout
            {
                float xb[D / 2];
                in_load_half_row<D>(X, row, valid, half, xb);
                in_logits<D, KB>(sg_lds, xb, l32, half, tt);
            }
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const in_f32x4 x4 = sg_load4<D>(X, row, valid, kb, q, half);
                    const in_f32x4 g4 = sg_load4<D>(g_y, row, valid, kb, q, half);
                    const in_f32x4 b4 = *reinterpret_cast<const in_f32x4 *>(bias + kb * 32 + 8 * q + 4 * half);
                    in_f32x4 u4;                                       // dY_c (.) s_c, the gate's direct share of dX
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float s = sg_sigmoid(tt[kb][4 * q + j] + b4[j]);
                        u4[j] = g4[j] * s;
                        tt[kb][4 * q + j] = (g4[j] * x4[j]) * (s * (1.f - s));
                    }
                    if (chunk == 0 && valid) {                         // (kept out of the registers: T_c W_c is added below)
                        in_f32x4 *dst = reinterpret_cast<in_f32x4 *>(dX + (size_t)row * D + kb * 32 + 8 * q + 4 * half);
                        if (c) {                                       // this lane's own store of the previous gate
                            const in_f32x4 o = *dst;
#pragma unroll
                            for (int j = 0; j < 4; ++j) u4[j] += o[j];
                        }
                        *dst = u4;
                    }
                }
            if (chunk == 0) {
#pragma unroll
                for (int ib = 0; ib < KB; ++ib) {
                    const in_f32x16 y = in_project_block<D, KB>(sg_lds, tt, ib, l32, half);
                    if (valid) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            in_f32x4 *dst = reinterpret_cast<in_f32x4 *>(dX + (size_t)row * D + ib * 32 + 8 * q + 4 * half);
                            in_f32x4 o = *dst;                         // this lane's own store above
#pragma unroll
                            for (int j = 0; j < 4; ++j) o[j] += y[4 * q + j];
                            *dst = o;
                        }
                    }
                }
            }
            // dW_c^T[i, k] += sum over the tile's rows of X[row, i] T[row, k]: A operand from global memory (lane = column i), B operand
            // from the wave's transposition tile
            float xa[DC][16];
#pragma unroll
            for (int a = 0; a < DC; ++a)
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const long long rr = row0 + 2 * s + half;
                    xa[a][s] = rr < N ? X[(size_t)rr * D + (chunk * DC + a) * 32 + l32] : 0.f;
                }
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                in_rowsum_block<DC, KB>(tile, tt[kb], xa, l32, half, dc, kb);
                if (chunk == 0) {                                      // db: the transposed block is still in the tile, rows ascending
#pragma unroll
                    for (int s = 0; s < 16; ++s) tb[kb] += tile[(2 * s + half) * IN_TSTRIDE + l32];
                }
            }
        }
        // db: the two halves (even and odd rows of the tiles), then the waves in order
        __syncthreads();                                               // (every wave is done with its transposition tile and the matrix)
        if (chunk == 0) {
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                const float v = tb[kb] + __shfl_xor(tb[kb], 32, 64);
                if (half == 0) tile_all[wave * D + kb * 32 + l32] = v;
            }
        }
        __syncthreads();
        if (chunk == 0 && (int)threadIdx.x < D)
            db_part[((size_t)c * G + blockIdx.x) * D + threadIdx.x] =
                ((tile_all[threadIdx.x] + tile_all[D + threadIdx.x]) + tile_all[2 * D + threadIdx.x]) + tile_all[3 * D + threadIdx.x];
        in_slab_store<D, KB>(sg_lds, dc, chunk, ws + ((size_t)c * G + blockIdx.x) * (D * D));
    }
}

// dW_c[k, i] = sum over the G slabs of slab[i, k] and db_c[k] = sum of the G partials: 4 interleaved sets in ascending order, then
// (s0 + s1) + (s2 + s3)
__global__ __launch_bounds__(256) void sg_finish_kernel(const float *__restrict__ ws, const int C, const int G, const int d, float *__restrict__ dW,
                                                        float *__restrict__ dB) {
    const int n_w = C * d * d, n_b = C * d;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_w + n_b) return;
    const float *src;
    size_t step;
    float *dst;
    if (e < n_w) {
        const int c = e / (d * d), rem = e - c * d * d, k = rem / d, i = rem - k * d;          // dW_c[k][i]
        src = ws + (size_t)c * G * d * d + (size_t)i * d + k;
        step = (size_t)d * d;
        dst = dW + e;
    } else {
        const int f = e - n_w, c = f / d, k = f - c * d;
        src = ws + (size_t)C * G * d * d + (size_t)c * G * d + k;
        step = (size_t)d;
        dst = dB + f;
    }
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int g = 0;
    for (; g + 4 <= G; g += 4) {
        s0 += src[(size_t)g * step];
        s1 += src[(size_t)(g + 1) * step];
        s2 += src[(size_t)(g + 2) * step];
        s3 += src[(size_t)(g + 3) * step];
    }
    for (; g < G; ++g) s0 += src[(size_t)g * step];
    *dst = (s0 + s1) + (s2 + s3);
}

inline bool sg_shape_ok(int64_t N, int64_t d, int64_t C) {
    return N >= 1 && N < 0x7fffffffLL - 64 && (d == 32 || d == 64 || d == 128) && C >= 1 && C <= SG_MAX_GATES;
}

template <int D, typename K>
int sg_set_lds(K kernel, size_t lds) {
    if (lds > 65536) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

template <int D, int CG>
int sg_fwd(const float *X, int N, const float *Wt, const float *B, int C, const SgPtrs &Y, hipStream_t st) {
    const int cg = C < CG ? C : CG;
    const size_t lds = (size_t)cg * InCfg<D, D / 32>::C_FLOATS * sizeof(float);
    const int rc = sg_set_lds<D>(sg_fwd_kernel<D, CG>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL((sg_fwd_kernel<D, CG>), dim3((unsigned)in_groups(N, SG_FWD_CAP)), dim3(IN_WAVES * 64), lds, st, X, N, Wt, B, C, Y);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

template <int D>
int sg_bwd(const float *X, int N, const float *Wt, const float *B, int C, const SgConstPtrs &dY, float *dX, float *dW, float *dB, float *ws,
           hipStream_t st) {
    using Cfg = InCfg<D, D / 32>;
    const size_t lds = Cfg::BWD_LDS;
    const int rc = sg_set_lds<D>(sg_bwd_kernel<D>, lds);
    if (rc) return rc;
    const int G = in_groups(N, SG_BWD_CAP);
    hipLaunchKernelGGL((sg_bwd_kernel<D>), dim3((unsigned)G, (unsigned)Cfg::CHUNKS), dim3(IN_WAVES * 64), lds, st, X, N, Wt, B, C, dY, dX, ws);
    hipLaunchKernelGGL(sg_finish_kernel, dim3((unsigned)((C * D * D + C * D + 255) / 256)), dim3(256), 0, st, (const float *)ws, C, G, D, dW, dB);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

}      // namespace

extern "C" {

size_t sslrec_mhcn_gate_ws_bytes(int32_t N, int32_t d, int32_t C) {
    if (!sg_shape_ok(N, d, C)) return 0;
    return (size_t)C * in_groups(N, SG_BWD_CAP) * ((size_t)d * d + d) * sizeof(float);
}

int sslrec_mhcn_gate_fwd_f32(const float *X, int32_t N, int32_t d, const float *Wt, const float *B, int32_t C, float *Y0, float *Y1, float *Y2,
                             float *Y3, void *stream) {
    if (!X || !Wt || !B || !sg_shape_ok(N, d, C)) return SSLREC_E_BADARG;
    SgPtrs Y = {{Y0, Y1, Y2, Y3}};
    uintptr_t bits = (uintptr_t)X | (uintptr_t)B;
    for (int c = 0; c < C; ++c) {
        if (!Y.p[c]) return SSLREC_E_BADARG;
        bits |= (uintptr_t)Y.p[c];
    }
    if (bits & 15) return SSLREC_E_BADARG;                             // rows and biases are read and written as float4
    hipStream_t st = (hipStream_t)stream;
    switch (d) {
    case 32: return sg_fwd<32, 4>(X, N, Wt, B, C, Y, st);
    case 64: return sg_fwd<64, 4>(X, N, Wt, B, C, Y, st);
    default: return sg_fwd<128, 1>(X, N, Wt, B, C, Y, st);
    }
}

int sslrec_mhcn_gate_bwd_f32(const float *X, int32_t N, int32_t d, const float *Wt, const float *B, int32_t C, const float *dY0, const float *dY1,
                             const float *dY2, const float *dY3, float *dX, float *dW, float *dB, void *ws, void *stream) {
    if (!X || !Wt || !B || !dX || !dW || !dB || !ws || !sg_shape_ok(N, d, C)) return SSLREC_E_BADARG;
    SgConstPtrs dY = {{dY0, dY1, dY2, dY3}};
    uintptr_t bits = (uintptr_t)X | (uintptr_t)B | (uintptr_t)dX;
    for (int c = 0; c < C; ++c) {
        if (!dY.p[c]) return SSLREC_E_BADARG;
        bits |= (uintptr_t)dY.p[c];
    }
    if (bits & 15) return SSLREC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    switch (d) {
    case 32: return sg_bwd<32>(X, N, Wt, B, C, dY, dX, dW, dB, (float *)ws, st);
    case 64: return sg_bwd<64>(X, N, Wt, B, C, dY, dX, dW, dB, (float *)ws, st);
    default: return sg_bwd<128>(X, N, Wt, B, C, dY, dX, dW, dB, (float *)ws, st);
    }
}

}      // extern "C"
