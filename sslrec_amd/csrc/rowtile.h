// Row-tile machinery shared by the kernels that multiply the stacked table [users; items] with one small [d, K] matrix per row range
// (intent.hip: DCCF's intent aggregation; hyper.hip: HCCF's hypergraph layer).
//
// Layout.  A workgroup of 4 waves belongs to ONE row range and keeps that range's matrices in LDS for its lifetime (row stride
// 32 KB + 1 floats: rows are read along k by the first product and down i by the second, both free of bank conflicts; the
// columns K .. 32 KB - 1 are zero).  A wave owns tiles of 32 rows of its range -- tiles are counted per range, so none holds rows
// of both.  All products are exact-fp32 MFMAs (32x32x2) formed TRANSPOSED, Z^T = C^T X^T: the accumulator then has the tile's ROW
// on the lane (row = lane & 31) and the columns k = 32 kb + (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) in its registers, so
//   * anything per row (a softmax, a mask) is arithmetic inside a lane plus at most ONE exchange with lane ^ 32;
//   * the accumulator is already the B operand of the next product Y^T = C P^T (the sum over k may run in any order: a step takes k
//     from the low half and k + 4 from the high half), no movement between lanes, no LDS.
// Only a [d, K]-sized sum over rows, i.e. over lanes, moves data: the accumulator goes through a 32 x 33 LDS tile per wave, one
// block of 32 columns at a time.  Such a sum has no atomics: a wave keeps it in registers over all its tiles, the 4 waves add up in
// a fixed order in LDS, the workgroup writes its [d, K] slab to the workspace and a second kernel adds the slabs in a fixed order.
#pragma once
#include "common.h"

namespace {

typedef float in_f32x4 __attribute__((ext_vector_type(4)));
typedef float in_f32x16 __attribute__((ext_vector_type(16)));

constexpr int IN_WAVES = 4;
constexpr int IN_TSTRIDE = 33;         // row stride of the per-wave transposition tile

__device__ __forceinline__ void in_wave_sync() {          // LDS traffic between the lanes of ONE wave
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// row blocks of a [d, K] sum over rows a workgroup accumulates (16 accumulator registers per 32 x 32 block, at most 128 in all)
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

// acc[kb] (+)= (C^T V^T) block kb: acc[kb][reg] = <V_row, C[:, k(kb, reg, half)]>; ZERO = false adds to what acc holds
template <int D, int KB, bool ZERO = true>
__device__ __forceinline__ void in_logits(const float *lds, const float (&v)[D / 2], int l32, int half, in_f32x16 (&acc)[KB]) {
    constexpr int KS = KB * 32 + 1;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
        if constexpr (ZERO) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[kb][r] = 0.f;
        }
#pragma unroll
        for (int s = 0; s < D / 2; ++s)
            acc[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[(half * (D / 2) + s) * KS + kb * 32 + l32], v[s], acc[kb], 0, 0, 0);
    }
}

// block ib of sum_k W[row, k] C[:, k] for the accumulator-layout weights W: y[4 q + j] = column ib 32 + 8 q + 4 half + j of the row
template <int D, int KB>
__device__ __forceinline__ in_f32x16 in_project_block(const float *lds, const in_f32x16 (&w)[KB], int ib, int l32, int half) {
    constexpr int KS = KB * 32 + 1;
    in_f32x16 y;
#pragma unroll
    for (int r = 0; r < 16; ++r) y[r] = 0.f;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            y = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[(ib * 32 + l32) * KS + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half], w[kb][r], y, 0, 0,
                                                     0);
    return y;
}

// out[row, :] = sum_k W[row, k] C[:, k], stored as float4s
template <int D, int KB>
__device__ __forceinline__ void in_project_store(const float *lds, const in_f32x16 (&w)[KB], int l32, int half, float *__restrict__ out,
                                                 long long row, bool valid) {
#pragma unroll
    for (int ib = 0; ib < D / 32; ++ib) {
        const in_f32x16 y = in_project_block<D, KB>(lds, w, ib, l32, half);
        if (valid) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                in_f32x4 o = {y[4 * q], y[4 * q + 1], y[4 * q + 2], y[4 * q + 3]};
                *reinterpret_cast<in_f32x4 *>(out + (size_t)row * D + ib * 32 + 8 * q + 4 * half) = o;
            }
        }
    }
}

// dc[a][kb] += T_a^T S for the tile's 32 rows: T_a = ta (column (chunk DC + a) 32 + lane of rows 2 s + half, read by the caller), S = the
// accumulator-layout block s_kb, which crosses the lanes through the wave's transposition tile
template <int DC, int KB>
__device__ __forceinline__ void in_rowsum_block(float *tile, const in_f32x16 &s_kb, const float (&ta)[DC][16], int l32, int half,
                                                in_f32x16 (&dc)[DC][KB], int kb) {
    in_wave_sync();                                 // (the previous block's readers are done)
#pragma unroll
    for (int r = 0; r < 16; ++r) tile[l32 * IN_TSTRIDE + (r & 3) + 8 * (r >> 2) + 4 * half] = s_kb[r];
    in_wave_sync();
#pragma unroll
    for (int a = 0; a < DC; ++a)
#pragma unroll
        for (int s = 0; s < 16; ++s)
            dc[a][kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(ta[a][s], tile[(2 * s + half) * IN_TSTRIDE + l32], dc[a][kb], 0, 0, 0);
}

// the 4 waves' sums, added in the order of the waves in `red` (LDS, InCfg::RED_FLOATS floats that every wave is done with), then the
// workgroup's rows [chunk DC 32, (chunk + 1) DC 32) of its [D, KB 32] slab
template <int D, int KB>
__device__ __forceinline__ void in_slab_store(float *red, const in_f32x16 (&dc)[InCfg<D, KB>::DC][KB], int chunk, float *__restrict__ slab) {
    constexpr int DC = InCfg<D, KB>::DC, KP = KB * 32;
    const int lane = threadIdx.x & 63, wave = wave_in_block();
    for (int w = 0; w < IN_WAVES; ++w) {
        __syncthreads();                                       // (first round: every wave is done with the matrices)
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
    for (int e = threadIdx.x; e < DC * KB * 16 * 64; e += IN_WAVES * 64) {
        const int ln = e & 63, r = (e >> 6) & 15, blk = e >> 10, kb = blk % KB, a = blk / KB;
        const int i = (chunk * DC + a) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5), k = kb * 32 + (ln & 31);
        slab[i * KP + k] = red[e];
    }
}

inline int in_kb(int K) { return K <= 32 ? 1 : (K <= 64 ? 2 : (K <= 128 ? 4 : 8)); }

inline int in_groups(long long rows, int cap) {
    const long long g = (rows + 32 * IN_WAVES - 1) / (32 * IN_WAVES);
    return (int)(g < cap ? g : cap);
}

}      // namespace
