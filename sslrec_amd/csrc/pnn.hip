// Position features of GFormer's PNNLayer (reference models/general_cf/gformer.py:202-218) without its [N, A, d] and [N, A, 2d] tensors.
// The layer applies Linear(2d, d) to every one of the N * A rows [w[a, n] * E[a], self[n, a]] and averages over A; the Linear commutes
// with the mean, so the layer is Linear([s, u]) with two [N, d] halves,
//     s[n] = (1 / A) sum_a w[n, a] * X[anchor[a]],          w = 1 / (hop + 1), 0 for an unreached node (hop < 0)
//     u[n] = (1 / A) sum_{a < A} X[(n A + a) mod N].
// The second line is what the reference's `embeds.repeat(A, 1).reshape(-1, A, d)` computes: element [n, a] of that tensor is row
// (n A + a) mod N of X, not row n.  This file writes Z = [s, u] [N, 2d]; the Linear stays the caller's (one [N, 2d] x [2d, d]
// product whose weight gradients autograd already gives).
//
// Forward.  pnn_s_kernel: one row per LANE with its d sums in registers, the A anchor rows in LDS, read by every lane at the same
// address (broadcast), a ascending; the hop is decoded in the kernel with an IEEE division, which equals float32(1.0 / (h + 1)) of the
// reference's float64 array for every h in 0 .. 32766 (tests/test_gformer_host.py).  pnn_u_kernel: a lane group of d / 4 lanes per row
// adds its A cyclically consecutive rows, a ascending.
// Backward from gZ = [gs, gu].  Row m is covered by exactly A pairs (n, a), n A + a = m + j N for j = 0 .. A - 1, so
//     dX[m] = (1 / A) sum_{j < A} gu[floor((m + j N) / A)]                                             (pnn_dx_kernel: a gather)
//     dE[a] = (1 / A) sum_n w[n, a] gs[n]    (pnn_de_partial_kernel: slab partials in row order; pnn_de_finish_kernel: the slabs in a
//                                             fixed order; pnn_de_apply_kernel: dX[anchor[a]] += dE[a], one writer per word)
// No float atomics, nothing of size N x A x d or N x A floats: two runs give the same bits.
#include "common.h"

namespace {

constexpr int PNN_MAX_A = 256;
constexpr int PNN_MAX_LDS = 128 * 1024;
constexpr int PNN_ST = 128;                   // threads (= rows) of a pnn_s_kernel workgroup
constexpr int PNN_TILE = 64;                  // rows per slab are a multiple of this
constexpr int PNN_MAX_SLABS = 256;

inline bool pnn_shape_ok(int64_t N, int64_t A, int64_t d) {
    return N >= 1 && N < 0x7fffffffLL && (d == 32 || d == 64 || d == 128) && A >= 1 && A <= PNN_MAX_A && A * d * 4 <= PNN_MAX_LDS;
}

struct PnnGeom {
    int rows_per_slab, S;
};

inline PnnGeom pnn_geom(int N) {
    PnnGeom g;
    const int n_tiles = (N + PNN_TILE - 1) / PNN_TILE;
    const int s0 = n_tiles < PNN_MAX_SLABS ? n_tiles : PNN_MAX_SLABS;
    const int tiles_per_slab = (n_tiles + s0 - 1) / s0;
    g.S = (n_tiles + tiles_per_slab - 1) / tiles_per_slab;
    g.rows_per_slab = tiles_per_slab * PNN_TILE;
    return g;
}

__device__ __forceinline__ float hop_weight(const int h) { return h < 0 ? 0.f : 1.0f / (float)(h + 1); }

template <int D>
__global__ __launch_bounds__(PNN_ST) void pnn_s_kernel(const float *__restrict__ X, const int32_t *__restrict__ anchors,
                                                       const int16_t *__restrict__ hops, const int N, const int A, float *__restrict__ Z) {
    extern __shared__ float4 pnn_e4[];                           // A * D floats: the anchor rows
    const int n4 = A * (D / 4);
    for (int e = threadIdx.x; e < n4; e += PNN_ST) {
        int id = anchors[e / (D / 4)];
        if ((unsigned)id >= (unsigned)N) id = 0;                 // (ids are validated by the caller; never read outside the table)
        pnn_e4[e] = reinterpret_cast<const float4 *>(X + (size_t)id * D)[e % (D / 4)];
    }
    __syncthreads();
    const int r = blockIdx.x * PNN_ST + threadIdx.x;
    if (r >= N) return;
    float acc[D];
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] = 0.f;
    const int16_t *hp = hops + (size_t)r * A;
    for (int a = 0; a < A; ++a) {
        const float w = hop_weight((int)hp[a]);
        const float4 *e = pnn_e4 + a * (D / 4);
#pragma unroll
        for (int q = 0; q < D / 4; ++q) {
            const float4 m = e[q];
            acc[4 * q] = fmaf(w, m.x, acc[4 * q]);
            acc[4 * q + 1] = fmaf(w, m.y, acc[4 * q + 1]);
            acc[4 * q + 2] = fmaf(w, m.z, acc[4 * q + 2]);
            acc[4 * q + 3] = fmaf(w, m.w, acc[4 * q + 3]);
        }
    }
    const float fa = (float)A;
    float4 *dst = reinterpret_cast<float4 *>(Z + (size_t)r * 2 * D);
#pragma unroll
    for (int q = 0; q < D / 4; ++q) dst[q] = make_float4(acc[4 * q] / fa, acc[4 * q + 1] / fa, acc[4 * q + 2] / fa, acc[4 * q + 3] / fa);
}

template <int D>
__global__ __launch_bounds__(256) void pnn_u_kernel(const float4 *__restrict__ X, const int N, const int A, float4 *__restrict__ Z) {
    constexpr int L = D / 4;
    const int lig = threadIdx.x % L;
    const long long rr = (long long)blockIdx.x * (256 / L) + threadIdx.x / L;
    if (rr >= N) return;
    int m = (int)((rr * A) % N);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int a = 0; a < A; ++a) {
        const float4 v = X[(size_t)m * L + lig];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        if (++m == N) m = 0;
    }
    const float fa = (float)A;
    Z[(size_t)rr * 2 * L + L + lig] = make_float4(acc.x / fa, acc.y / fa, acc.z / fa, acc.w / fa);
}

// dX[m] = (1 / A) sum_j gu[(m + j N) / A]; the quotient is stepped: q += N / A, rem += N % A with a carry
template <int D>
__global__ __launch_bounds__(256) void pnn_dx_kernel(const float4 *__restrict__ gZ, const int N, const int A, float4 *__restrict__ dX) {
    constexpr int L = D / 4;
    const int lig = threadIdx.x % L;
    const long long rr = (long long)blockIdx.x * (256 / L) + threadIdx.x / L;
    if (rr >= N) return;
    const int m = (int)rr;
    const int dq = N / A, dr = N % A;
    int q = m / A, rem = m % A;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int j = 0; j < A; ++j) {
        const float4 v = gZ[(size_t)q * 2 * L + L + lig];        // q <= (A N - 1) / A < N
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        q += dq;
        rem += dr;
        if (rem >= A) { rem -= A; ++q; }
    }
    const float fa = (float)A;
    dX[(size_t)m * L + lig] = make_float4(acc.x / fa, acc.y / fa, acc.z / fa, acc.w / fa);
}

// workgroup (slab, chunk): 256 / L anchors, a lane group of L lanes each, the slab's rows in ascending order
template <int D>
__global__ __launch_bounds__(256) void pnn_de_partial_kernel(const float4 *__restrict__ gZ, const int16_t *__restrict__ hops, const int N, const int A,
                                                             const int rows_per_slab, float4 *__restrict__ part) {
    constexpr int L = D / 4;
    const int lig = threadIdx.x % L;
    const int a = blockIdx.y * (256 / L) + threadIdx.x / L;
    if (a >= A) return;                                          // (whole lane groups leave; the kernel has no barrier)
    const int slab = blockIdx.x;
    const long long r0 = (long long)slab * rows_per_slab;
    const long long r1 = r0 + rows_per_slab < N ? r0 + rows_per_slab : N;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (long long r = r0; r < r1; ++r) {
        const float w = hop_weight((int)hops[(size_t)r * A + a]);
        const float4 g = gZ[(size_t)r * 2 * L + lig];
        acc.x = fmaf(w, g.x, acc.x); acc.y = fmaf(w, g.y, acc.y); acc.z = fmaf(w, g.z, acc.z); acc.w = fmaf(w, g.w, acc.w);
    }
    part[((size_t)slab * A + a) * L + lig] = acc;
}

// 64 elements of dE per workgroup; thread (g, j) adds slabs g, g + 4, ... of element j, then ((s0 + s1) + s2) + s3
__global__ __launch_bounds__(256) void pnn_de_finish_kernel(const float *__restrict__ part, const int S, const int A, const int d,
                                                            float *__restrict__ dE) {
    __shared__ float fs[4][64];
    const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int n_elem = A * d;
    const int e = blockIdx.x * 64 + j;
    float s = 0.f;
    if (e < n_elem)
        for (int sl = g; sl < S; sl += 4) s += part[(size_t)sl * n_elem + e];
    fs[g][j] = s;
    __syncthreads();
    if (g == 0 && e < n_elem) dE[e] = (((fs[0][j] + fs[1][j]) + fs[2][j]) + fs[3][j]) / (float)A;
}

// dX[anchors[a]] += dE[a].  Anchors are distinct in the model; a caller's repeated id is still exact and ordered: the FIRST occurrence
// adds the rows of all its repeats in ascending a, the repeats leave -- one writer per word either way.
__global__ __launch_bounds__(256) void pnn_de_apply_kernel(const float *__restrict__ dE, const int A, const int d, const int32_t *__restrict__ anchors,
                                                           const int N, float *__restrict__ dX) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= A * d) return;
    const int a = e / d, c = e % d;
    const int id = anchors[a];
    if ((unsigned)id >= (unsigned)N) return;
    for (int a2 = 0; a2 < a; ++a2)
        if (anchors[a2] == id) return;
    float s = dE[e];
    for (int a2 = a + 1; a2 < A; ++a2)
        if (anchors[a2] == id) s += dE[(size_t)a2 * d + c];
    dX[(size_t)id * d + c] += s;
}

inline unsigned pnn_blocks(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

template <int D>
int pnn_fwd(const float *X, int N, const int32_t *anchors, int A, const int16_t *hops, float *Z, hipStream_t st) {
    const size_t lds = (size_t)A * D * sizeof(float);
    if (lds > 65536) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(pnn_s_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((pnn_s_kernel<D>), dim3(pnn_blocks(N, PNN_ST)), dim3(PNN_ST), lds, st, X, anchors, hops, N, A, Z);
    hipLaunchKernelGGL((pnn_u_kernel<D>), dim3(pnn_blocks(N, 256 / (D / 4))), dim3(256), 0, st, (const float4 *)X, N, A, (float4 *)Z);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

template <int D>
int pnn_bwd(const float *gZ, int N, const int32_t *anchors, int A, const int16_t *hops, float *dX, float *part, hipStream_t st) {
    const PnnGeom g = pnn_geom(N);
    constexpr int AC = 256 / (D / 4);
    hipLaunchKernelGGL((pnn_dx_kernel<D>), dim3(pnn_blocks(N, 256 / (D / 4))), dim3(256), 0, st, (const float4 *)gZ, N, A, (float4 *)dX);
    hipLaunchKernelGGL((pnn_de_partial_kernel<D>), dim3((unsigned)g.S, (unsigned)((A + AC - 1) / AC)), dim3(256), 0, st, (const float4 *)gZ, hops, N, A,
                       g.rows_per_slab, (float4 *)part);
    float *dE = part + (size_t)g.S * A * D;
    hipLaunchKernelGGL(pnn_de_finish_kernel, dim3(pnn_blocks((long long)A * D, 64)), dim3(256), 0, st, (const float *)part, g.S, A, D, dE);
    hipLaunchKernelGGL(pnn_de_apply_kernel, dim3(pnn_blocks((long long)A * D, 256)), dim3(256), 0, st, (const float *)dE, A, D, anchors, N, dX);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

}      // namespace

extern "C" {

size_t sslrec_pnn_bwd_ws_bytes(int32_t N, int32_t A, int32_t d) {
    if (!pnn_shape_ok(N, A, d)) return 0;
    return ((size_t)pnn_geom(N).S + 1) * A * d * sizeof(float) + 32;      // slab partials, then dE
}

int sslrec_pnn_fwd_f32(const float *X, int32_t N, int32_t d, const int32_t *anchors, int32_t A, const int16_t *hops, float *Z, void *stream) {
    if (!X || !anchors || !hops || !Z || !pnn_shape_ok(N, A, d)) return SSLREC_E_BADARG;
    if (((uintptr_t)X | (uintptr_t)Z) & 15) return SSLREC_E_BADARG;         // rows are read and written as float4
    hipStream_t st = (hipStream_t)stream;
    switch (d) {
    case 32: return pnn_fwd<32>(X, N, anchors, A, hops, Z, st);
    case 64: return pnn_fwd<64>(X, N, anchors, A, hops, Z, st);
    default: return pnn_fwd<128>(X, N, anchors, A, hops, Z, st);
    }
}

int sslrec_pnn_bwd_f32(const float *gZ, int32_t N, int32_t d, const int32_t *anchors, int32_t A, const int16_t *hops, float *dX, void *ws,
                       void *stream) {
    if (!gZ || !anchors || !hops || !dX || !ws || !pnn_shape_ok(N, A, d)) return SSLREC_E_BADARG;
    if (((uintptr_t)gZ | (uintptr_t)dX) & 15) return SSLREC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    float *part = (float *)(((uintptr_t)ws + 15) & ~(uintptr_t)15);
    switch (d) {
    case 32: return pnn_bwd<32>(gZ, N, anchors, A, hops, dX, part, st);
    case 64: return pnn_bwd<64>(gZ, N, anchors, A, hops, dX, part, st);
    default: return pnn_bwd<128>(gZ, N, anchors, A, hops, dX, part, st);
    }
}

}      // extern "C"
