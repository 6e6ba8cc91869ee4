// Hop counts from A anchor nodes to every node of GFormer's adjacency (reference models/general_cf/gformer.py:146-180: a networkx graph of
// all entries, one Python BFS per anchor, a Python double loop that fills a [A, N] float64 array with 1 / (dist + 1)) as ONE
// level-synchronous breadth-first search from all anchors at once: integers only, so the result is exact.
//
// Every node holds W = ceil(A / 64) 64-bit "reached" words; bit a of node n is set once anchor a has reached n.  A level is an ordinary
// launch over the CSR rows of the pattern in PULL form: a row ORs the previous level's words of its neighbours, new = acc & ~own, the
// level number goes to hops[n, a] for every bit of `new`, and the NEXT buffer gets own | new.  The two buffers ping-pong, so no kernel
// reads what it writes, and OR does not depend on an order: two runs give the same bits.  The pattern must be symmetric (the
// reference's nx.Graph makes it so); it is not checked.
//
// Layout.  A TEAM of BFS_L lanes owns a row and takes its entries interleaved; the partial words are OR-ed with shuffles.  A row whose
// own words are already full copies them and does not walk its entries.  A row of more than SSLREC_EDGE_LONG_ROW entries gets a whole
// workgroup from the long-row list (gt.hip's scheme): wave shuffles, then LDS.
//
// Exit.  Every level counts the rows that gained a bit (an integer atomic per wave) into its own slot.  The host launches `poll` levels,
// reads their slots with one copy and stops at the first period that holds a zero: a level that changed nothing leaves reached(l + 1)
// == reached(l), every later level is the identity and writes no hop, so the result does not depend on `poll`.  After 32766 levels
// without such a level the call reports that it did not converge; int16 never saturates.
#include "common.h"

namespace {

constexpr int BFS_MAX_A = 256;
constexpr int BFS_MAX_POLL = 64;
constexpr int BFS_MAX_LEVEL = 32766;
constexpr int BFS_L = 8;                      // lanes of a row team

inline bool bfs_shape_ok(int64_t N, int64_t A) { return N >= 1 && N < 0x7fffffffLL && A >= 1 && A <= BFS_MAX_A; }

struct BfsWs {
    unsigned long long *buf[2];              // [N][W] each
    int *chg;                                // [BFS_MAX_POLL]
    size_t bytes;
};

inline BfsWs bfs_ws(void *ws, int N, int A) {
    const size_t W = (size_t)(A + 63) / 64;
    char *p = (char *)(((uintptr_t)ws + 15) & ~(uintptr_t)15);
    char *p0 = p;
    auto al = [](size_t n) { return (n + 15) & ~(size_t)15; };
    BfsWs w;
    w.buf[0] = (unsigned long long *)p; p += al((size_t)N * W * 8);
    w.buf[1] = (unsigned long long *)p; p += al((size_t)N * W * 8);
    w.chg = (int *)p; p += al((size_t)BFS_MAX_POLL * 4);
    w.bytes = (size_t)(p - p0) + 16;
    return w;
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(const unsigned long long v, const int o) {
    const int lo = __shfl_xor((int)(unsigned)(v & 0xffffffffull), o, 64), hi = __shfl_xor((int)(unsigned)(v >> 32), o, 64);
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo;
}

__global__ __launch_bounds__(256) void bfs_init_kernel(unsigned long long *__restrict__ reach, const size_t n_words, int16_t *__restrict__ hops,
                                                       const size_t n_hops) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += stride) reach[i] = 0ull;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_hops; i += stride) hops[i] = (int16_t)-1;
}

// anchors start at hop 0 (distinct anchors are distinct nodes; the OR keeps a caller's duplicate harmless)
__global__ __launch_bounds__(256) void bfs_seed_kernel(const int32_t *__restrict__ anchors, const int A, const int N, const int W,
                                                       unsigned long long *__restrict__ reach, int16_t *__restrict__ hops) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= A) return;
    const int n = anchors[a];
    if (n < 0 || n >= N) return;
    atomicOr(&reach[(size_t)n * W + (a >> 6)], 1ull << (a & 63));
    hops[(size_t)n * A + a] = (int16_t)0;
}

template <int W, bool LONG>
__global__ __launch_bounds__(256) void bfs_level_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int n,
                                                        const int32_t *__restrict__ long_rows, const int A, const int level,
                                                        const unsigned long long *__restrict__ prev, unsigned long long *__restrict__ next,
                                                        int16_t *__restrict__ hops, int *__restrict__ chg_slot) {
    constexpr int L = LONG ? 256 : BFS_L;
    __shared__ unsigned long long red[LONG ? 4 * W : 1];
    const int t = threadIdx.x % L;
    bool active;
    int r = 0, k = 0, k1 = 0;
    if constexpr (LONG) {
        r = long_rows[blockIdx.x];
        active = r >= 0 && r < n;                                // (uniform over the workgroup)
        if (active) { k = rowptr[r]; k1 = rowptr[r + 1]; }
    } else {
        const long long rr = (long long)blockIdx.x * (256 / L) + threadIdx.x / L;
        active = rr < n;                                         // (whole teams: L divides 64)
        if (active) {
            r = (int)rr;
            k = rowptr[r];
            k1 = rowptr[r + 1];
            if (long_rows && k1 - k > SSLREC_EDGE_LONG_ROW) active = false;      // the workgroup-per-row launch has it
        }
    }
    unsigned long long own[W], acc[W];
    bool full = true;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        own[w] = active ? prev[(size_t)r * W + w] : 0ull;
        acc[w] = 0ull;
        const int bits = A - 64 * w;
        const unsigned long long all = bits >= 64 ? ~0ull : ((1ull << bits) - 1ull);
        full = full && own[w] == all;
    }
    if (active && !full) {
        for (int kk = k + t; kk < k1; kk += L) {
            const int c = col[kk];
            if ((unsigned)c < (unsigned)n) {
#pragma unroll
                for (int w = 0; w < W; ++w) acc[w] |= prev[(size_t)c * W + w];
            }
        }
    }
    // OR over the team; every lane of the wave takes part (nobody has left)
    constexpr int TOP = LONG ? 32 : BFS_L / 2;
#pragma unroll
    for (int o = TOP; o > 0; o >>= 1) {
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] |= shfl_xor_u64(acc[w], o);
    }
    if constexpr (LONG) {
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int w = 0; w < W; ++w) red[(threadIdx.x >> 6) * W + w] = acc[w];
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] = red[w] | red[W + w] | red[2 * W + w] | red[3 * W + w];
    }
    bool gained = false;
    if (active && t == 0) {
#pragma unroll
        for (int w = 0; w < W; ++w) {
            unsigned long long nw = acc[w] & ~own[w];
            next[(size_t)r * W + w] = own[w] | nw;
            gained = gained || nw != 0ull;
            while (nw) {
                const int b = __ffsll((long long)nw) - 1;
                nw &= nw - 1ull;
                const int a = 64 * w + b;
                if (a < A) hops[(size_t)r * A + a] = (int16_t)level;
            }
        }
    }
    const unsigned long long m = __ballot(gained);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(chg_slot, (int)__popcll(m));
}

inline unsigned bfs_blocks(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

template <int W>
int bfs_level(const int32_t *rowptr, const int32_t *col, int n, const int32_t *long_rows, int n_long, int A, int level,
              const unsigned long long *prev, unsigned long long *next, int16_t *hops, int *slot, hipStream_t st) {
    hipLaunchKernelGGL((bfs_level_kernel<W, false>), dim3(bfs_blocks(n, 256 / BFS_L)), dim3(256), 0, st, rowptr, col, n, long_rows, A, level, prev,
                       next, hops, slot);
    if (n_long > 0)
        hipLaunchKernelGGL((bfs_level_kernel<W, true>), dim3((unsigned)n_long), dim3(256), 0, st, rowptr, col, n, long_rows, A, level, prev, next,
                           hops, slot);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

}      // namespace

extern "C" {

size_t sslrec_anchor_hops_ws_bytes(int32_t N, int32_t A) {
    if (!bfs_shape_ok(N, A)) return 0;
    return bfs_ws(nullptr, N, A).bytes;
}

int sslrec_anchor_hops(const int32_t *rowptr, const int32_t *col, int32_t n, const int32_t *long_rows, int32_t n_long, const int32_t *anchors,
                       int32_t A, int16_t *hops, int32_t poll, int32_t *levels, int32_t *converged, void *ws, void *stream) {
    if (!rowptr || !col || !anchors || !hops || !levels || !converged || !ws || !bfs_shape_ok(n, A) || n_long < 0 || (n_long > 0 && !long_rows) ||
        poll < 1 || poll > BFS_MAX_POLL)
        return SSLREC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (n_long == 0) long_rows = nullptr;
    const BfsWs w = bfs_ws(ws, n, A);
    const int W = (A + 63) / 64;
    const size_t n_words = (size_t)n * W, n_hops = (size_t)n * A;
    const size_t most = n_hops > n_words ? n_hops : n_words;
    unsigned init_blocks = bfs_blocks((long long)most, 256);
    if (init_blocks > 4096u) init_blocks = 4096u;
    hipLaunchKernelGGL(bfs_init_kernel, dim3(init_blocks), dim3(256), 0, st, w.buf[0], n_words, hops, n_hops);
    hipLaunchKernelGGL(bfs_seed_kernel, dim3(bfs_blocks(A, 256)), dim3(256), 0, st, anchors, (int)A, (int)n, W, w.buf[0], hops);
    SSLREC_LAUNCH_CHECK();
    int host_chg[BFS_MAX_POLL];
    int level = 0, cur = 0;
    *converged = 0;
    *levels = 0;
    while (level < BFS_MAX_LEVEL) {
        const int base = level;
        const int nl = (BFS_MAX_LEVEL - level) < poll ? (BFS_MAX_LEVEL - level) : poll;
        hipError_t e = hipMemsetAsync(w.chg, 0, (size_t)nl * sizeof(int), st);
        if (e != hipSuccess) return (int)e;
        for (int i = 0; i < nl; ++i) {
            ++level;
            int rc;
            switch (W) {
            case 1: rc = bfs_level<1>(rowptr, col, n, long_rows, n_long, A, level, w.buf[cur], w.buf[cur ^ 1], hops, w.chg + i, st); break;
            case 2: rc = bfs_level<2>(rowptr, col, n, long_rows, n_long, A, level, w.buf[cur], w.buf[cur ^ 1], hops, w.chg + i, st); break;
            case 3: rc = bfs_level<3>(rowptr, col, n, long_rows, n_long, A, level, w.buf[cur], w.buf[cur ^ 1], hops, w.chg + i, st); break;
            default: rc = bfs_level<4>(rowptr, col, n, long_rows, n_long, A, level, w.buf[cur], w.buf[cur ^ 1], hops, w.chg + i, st); break;
            }
            if (rc) return rc;
            cur ^= 1;
        }
        e = hipMemcpyAsync(host_chg, w.chg, (size_t)nl * sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return (int)e;
        for (int i = 0; i < nl && !*converged; ++i) {
            if (host_chg[i] == 0) {
                *converged = 1;
                *levels = base + i;                              // levels that changed something
            }
        }
        if (*converged) break;
    }
    if (!*converged) *levels = level;
    return 0;
}

}      // extern "C"
