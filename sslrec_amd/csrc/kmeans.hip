// Lloyd's k-means of NCL's KMeansClustering.forward (reference models/aug_utils.py:147-157) on an embedding table X [N, d]:
//   dists = (X.view(-1, 1, d) - C.view(1, -1, d)).square().sum(-1);  _, idx = t.min(dists, dim=1)
//   newC = zeros.index_add_(0, idx, X);  cnt = zeros.index_add_(0, idx, ones);  C = newC / (cnt + 1e-6)
// repeated max_iter times, without the [N, K, d] tensor and without float atomics: equal inputs give equal bits.
//
// One iteration is three ordinary launches; the loop is on the host (sslrec_kmeans_f32).
//   1. km_assign_kernel   one row per LANE (the row in d registers), the K centroids in LDS, read by every lane at the same address
//                         (broadcast).  d^2 = sum_c (x_c - m_c)^2 in fp32 on the VALU, c ascending -- the DIFFERENCE form: after the first
//                         iteration rows and centroids are both ~1e-2 and the Gram form |x|^2 - 2 <x, m> + |m|^2 would cancel (au.hip
//                         made the same choice).  The smallest distance wins and among equal distances the LOWEST index (k ascending,
//                         strict <): what t.min returns on the CPU.  Writes idx[r] and, per workgroup, how many of its rows changed
//                         against the previous idx (an integer; `first`: every row counts).
//   2. km_partial_kernel  the rows are cut into S slabs of whole 64-row tiles, S a function of N alone.  Workgroup (slab, chunk) keeps
//                         the sums of KM_ACC_FLOATS / d clusters in LDS and walks its tiles in row order; wave w alone owns the clusters
//                         with (k - k0) % 4 == w and adds their rows in ascending row order.  Slab partials [S][K][d], counts [S][K].
//   3. km_finish_kernel   per element the S slab partials: four interleaved partial sums in slab order, then ((s0 + s1) + s2) + s3;
//                         the counts as integers; C = sum / (float(cnt) + 1e-6f); an empty cluster is 0 / 1e-6 = 0 exactly.  Workgroup 0
//                         also adds the workgroups' changed-row counts into chg[slot].
// Every sum's order depends on (N, K, d) and idx only.
//
// Early exit.  An iteration that changed no row has idx_j == idx_{j-1}; C_j is a function of (idx_j, X) alone, so C_j == C_{j-1} bit for
// bit, iteration j + 1 sees the input of iteration j, and every later iteration is the identity: stopping returns what max_iter
// iterations return.  The host reads the `poll` counters of a period with one copy and stops at the end of the first period that
// holds a zero.  Iteration 0 counts every row (N >= 1), so it never reports zero.
#include <cmath>
#include "common.h"

namespace {

constexpr int KM_AT = 128;                   // threads (= rows) of an assignment workgroup
constexpr int KM_MAX_CENT_FLOATS = 16384;    // K d <= 64 KiB of LDS
constexpr int KM_TILE = 64;                  // rows of an update tile
constexpr int KM_ACC_FLOATS = 4096;          // cluster sums a partial workgroup keeps: 4096 / d clusters per chunk
constexpr int KM_MAX_SLABS = 256;
constexpr int KM_MAX_POLL = 64;

inline bool km_shape_ok(int64_t K, int64_t d) { return (d == 32 || d == 64 || d == 128) && K >= 1 && K * d <= KM_MAX_CENT_FLOATS; }

struct KmGeom {
    int n_ablocks;                           // assignment workgroups
    int n_tiles, tiles_per_slab, S;          // update slabs
    int n_chunks;                            // cluster chunks of the partial kernel
};

inline KmGeom km_geom(int N, int K, int d) {
    KmGeom g;
    g.n_ablocks = (N + KM_AT - 1) / KM_AT;
    g.n_tiles = (N + KM_TILE - 1) / KM_TILE;
    const int s0 = g.n_tiles < KM_MAX_SLABS ? g.n_tiles : KM_MAX_SLABS;
    g.tiles_per_slab = (g.n_tiles + s0 - 1) / s0;
    g.S = (g.n_tiles + g.tiles_per_slab - 1) / g.tiles_per_slab;
    const int kch = KM_ACC_FLOATS / d;
    g.n_chunks = (K + kch - 1) / kch;
    return g;
}

struct KmWs {
    float *part;                             // [S][K][d]
    int *cpart;                              // [S][K]
    int *chg_part;                           // [n_ablocks]
    int *chg;                                // [KM_MAX_POLL]
    size_t bytes;
};

inline KmWs km_ws(void *ws, int N, int K, int d) {
    const KmGeom g = km_geom(N, K, d);
    char *p = (char *)(((uintptr_t)ws + 15) & ~(uintptr_t)15);
    char *p0 = p;
    KmWs w;
    auto al = [](size_t n) { return (n + 15) & ~(size_t)15; };
    w.part = (float *)p; p += al((size_t)g.S * K * d * 4);
    w.cpart = (int *)p; p += al((size_t)g.S * K * 4);
    w.chg_part = (int *)p; p += al((size_t)g.n_ablocks * 4);
    w.chg = (int *)p; p += al((size_t)KM_MAX_POLL * 4);
    w.bytes = (size_t)(p - p0) + 16;
    return w;
}

template <int D>
__global__ __launch_bounds__(KM_AT) void km_assign_kernel(const float *__restrict__ X, const float *__restrict__ cent, int N, int K, int first,
                                                          int *__restrict__ idx, int *__restrict__ chg_part) {
    extern __shared__ float4 km_cent4[];                         // K * D floats
    const int n4 = K * (D / 4);
    for (int e = threadIdx.x; e < n4; e += KM_AT) km_cent4[e] = reinterpret_cast<const float4 *>(cent)[e];
    __syncthreads();
    const int r = blockIdx.x * KM_AT + threadIdx.x;
    const bool valid = r < N;
    float x[D];
    {
        const float4 *p = reinterpret_cast<const float4 *>(X + (size_t)(valid ? r : 0) * D);
#pragma unroll
        for (int q = 0; q < D / 4; ++q) {
            const float4 v = p[q];
            x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
        }
    }
    float best = INFINITY;
    int bk = 0;
    for (int k = 0; k < K; ++k) {
        const float4 *c = km_cent4 + k * (D / 4);
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < D / 4; ++q) {
            const float4 m = c[q];
            const float a0 = x[4 * q] - m.x, a1 = x[4 * q + 1] - m.y, a2 = x[4 * q + 2] - m.z, a3 = x[4 * q + 3] - m.w;
            s = fmaf(a0, a0, s); s = fmaf(a1, a1, s); s = fmaf(a2, a2, s); s = fmaf(a3, a3, s);
        }
        if (s < best) { best = s; bk = k; }                      // strict: the lowest index among equal distances
    }
    bool changed = false;
    if (valid) {
        changed = first || idx[r] != bk;
        idx[r] = bk;
    }
    const int n_changed = __popcll(__ballot(changed));
    __syncthreads();                                             // everybody is done with the centroids: their LDS carries the counts
    int *red = reinterpret_cast<int *>(km_cent4);                // (K * D >= 32 floats)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n_changed;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < KM_AT / 64; ++w) total += red[w];
        chg_part[blockIdx.x] = total;
    }
}

template <int D>
__global__ __launch_bounds__(256) void km_partial_kernel(const float *__restrict__ X, const int *__restrict__ idx, int N, int K, int n_tiles,
                                                         int tiles_per_slab, float *__restrict__ part, int *__restrict__ cpart) {
    constexpr int KCH = KM_ACC_FLOATS / D;
    __shared__ float4 tile4[KM_TILE * D / 4];
    __shared__ float acc[KM_ACC_FLOATS];
    __shared__ int cacc[KCH];
    const float *tile = reinterpret_cast<const float *>(tile4);
    const int lane = threadIdx.x & 63, wave = wave_in_block();
    const int slab = blockIdx.x, k0 = blockIdx.y * KCH;
    const int kn = min(KCH, K - k0);
    for (int e = threadIdx.x; e < kn * D; e += 256) acc[e] = 0.f;
    for (int e = threadIdx.x; e < kn; e += 256) cacc[e] = 0;
    const int t0 = slab * tiles_per_slab, t1 = min(t0 + tiles_per_slab, n_tiles);
    for (int t = t0; t < t1; ++t) {
        const int row0 = t * KM_TILE;
        const int nr = min(KM_TILE, N - row0);
        __syncthreads();                                         // the previous tile's readers are done (first round: acc is zero)
        {
            const float4 *src = reinterpret_cast<const float4 *>(X + (size_t)row0 * D);
            for (int e4 = threadIdx.x; e4 < nr * (D / 4); e4 += 256) tile4[e4] = src[e4];
        }
        const int myk = lane < nr ? idx[row0 + lane] - k0 : -1;  // lane r of every wave: the cluster of tile row r
        __syncthreads();
        unsigned long long m = __ballot(myk >= 0 && myk < kn && (myk & 3) == wave);
        while (m) {                                              // this wave's rows of the tile, ascending
            const int r = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int k = __shfl(myk, r, 64);
#pragma unroll
            for (int c = lane; c < D; c += 64) acc[k * D + c] += tile[r * D + c];
            if (lane == 0) cacc[k] += 1;
        }
    }
    __syncthreads();
    float *dst = part + ((size_t)slab * K + k0) * D;
    for (int e = threadIdx.x; e < kn * D; e += 256) dst[e] = acc[e];
    for (int e = threadIdx.x; e < kn; e += 256) cpart[(size_t)slab * K + k0 + e] = cacc[e];
}

// 64 elements of C per workgroup; thread (g, j) adds slabs g, g + 4, ... of element j
__global__ __launch_bounds__(256) void km_finish_kernel(const float *__restrict__ part, const int *__restrict__ cpart, int S, int K, int d,
                                                        float *__restrict__ cent, float *__restrict__ counts, const int *__restrict__ chg_part,
                                                        int n_ablocks, int *__restrict__ chg_slot) {
    __shared__ float fs[4][64];
    __shared__ int is[4][64];
    __shared__ int red[256];
    const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int n_elem = K * d;
    const int e = blockIdx.x * 64 + j;
    float s = 0.f;
    int c = 0;
    if (e < n_elem) {
        const int k = e / d;
        for (int sl = g; sl < S; sl += 4) {
            s += part[(size_t)sl * n_elem + e];
            c += cpart[(size_t)sl * K + k];
        }
    }
    fs[g][j] = s;
    is[g][j] = c;
    __syncthreads();
    if (g == 0 && e < n_elem) {
        const float tot = ((fs[0][j] + fs[1][j]) + fs[2][j]) + fs[3][j];
        const int cnt = is[0][j] + is[1][j] + is[2][j] + is[3][j];
        cent[e] = tot / ((float)cnt + 1e-6f);
        if (e % d == 0) counts[e / d] = (float)cnt;
    }
    if (blockIdx.x == 0) {
        int v = 0;
        for (int i = threadIdx.x; i < n_ablocks; i += 256) v += chg_part[i];
        red[threadIdx.x] = v;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) chg_slot[0] = red[0];
    }
}

template <int D>
int km_iteration(const float *X, int N, int K, float *cent, int *idx, float *counts, const KmWs &w, const KmGeom &g, int first, int slot,
                 hipStream_t st) {
    hipLaunchKernelGGL((km_assign_kernel<D>), dim3(g.n_ablocks), dim3(KM_AT), (size_t)K * D * sizeof(float), st, X, (const float *)cent, N, K,
                       first, idx, w.chg_part);
    hipLaunchKernelGGL((km_partial_kernel<D>), dim3(g.S, g.n_chunks), dim3(256), 0, st, X, (const int *)idx, N, K, g.n_tiles, g.tiles_per_slab,
                       w.part, w.cpart);
    hipLaunchKernelGGL(km_finish_kernel, dim3((K * D + 63) / 64), dim3(256), 0, st, (const float *)w.part, (const int *)w.cpart, g.S, K, D,
                       cent, counts, (const int *)w.chg_part, g.n_ablocks, w.chg + slot);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

}      // namespace

extern "C" {

size_t sslrec_kmeans_ws_bytes(int32_t N, int32_t K, int32_t d) {
    if (N < 1 || !km_shape_ok(K, d)) return 0;
    return km_ws(nullptr, N, K, d).bytes;
}

int sslrec_kmeans_f32(const float *X, int32_t N, int32_t d, int32_t K, float *cent, int32_t *idx, float *counts, int32_t max_iter,
                      int32_t early_exit, int32_t poll, int32_t *iters_run, void *ws, void *stream) {
    if (!X || !cent || !idx || !counts || !iters_run || !ws || N < 1 || !km_shape_ok(K, d) || max_iter < 1 || poll < 1 || poll > KM_MAX_POLL)
        return SSLREC_E_BADARG;
    if (((uintptr_t)X | (uintptr_t)cent) & 15) return SSLREC_E_BADARG;      // rows and centroids are read as float4
    hipStream_t st = (hipStream_t)stream;
    const KmGeom g = km_geom(N, K, d);
    const KmWs w = km_ws(ws, N, K, d);
    int host_chg[KM_MAX_POLL];
    int it = 0;
    while (it < max_iter) {
        const int n = (max_iter - it) < poll ? (max_iter - it) : poll;
        for (int i = 0; i < n; ++i, ++it) {
            int rc;
            switch (d) {
            case 32: rc = km_iteration<32>(X, N, K, cent, idx, counts, w, g, it == 0, i, st); break;
            case 64: rc = km_iteration<64>(X, N, K, cent, idx, counts, w, g, it == 0, i, st); break;
            default: rc = km_iteration<128>(X, N, K, cent, idx, counts, w, g, it == 0, i, st); break;
            }
            if (rc) return rc;
        }
        if (!early_exit || it >= max_iter) continue;
        hipError_t e = hipMemcpyAsync(host_chg, w.chg, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return (int)e;
        bool settled = false;
        for (int i = 0; i < n; ++i) settled = settled || host_chg[i] == 0;
        if (settled) break;
    }
    *iters_run = it;
    return 0;
}

}      // extern "C"
