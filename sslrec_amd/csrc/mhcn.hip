// Row-wise kernels of MHCN (reference models/social/mhcn.py): the channel attention with the normalised layer sums (:54-64, :80-113),
// the normalised sum of one table (:95-97) and the hierarchical mutual-information loss (:120-143), forward and backward.
//
// Geometry, the same in every kernel.  A row of d = 32 / 64 / 128 floats belongs to a LANE GROUP of L = d / 4 lanes (8 / 16 / 32: groups
// never straddle a wavefront), one float4 per lane; a sum over the row is L / 2 ... 1 exchanges with lane ^ o, a fixed tree.  A
// workgroup of 256 threads takes 256 / L rows per pass and owns a CONTIGUOUS range of rows (mh_geom: at most MH_MAX_BLOCKS workgroups,
// a function of N and d alone), which it walks in ascending order.
// Sums over rows (dv of the attention, the column mean of the loss and its gradient, the loss itself) have no atomics: a thread adds its
// rows in ascending order, the workgroup's lane groups are added in ascending order in LDS, the workgroup writes one partial, and a
// finishing kernel adds the partials of 4 interleaved sets in ascending order and then ((s0 + s1) + s2) + s3.  Two runs give the same bits.
//
// The loss uses log sigma(x) = min(x, 0) - log1p(exp(-|x|)), finite for every finite x (the reference's sigmoid().log() is -inf below
// about -104), and is accumulated in double.  Its backward keeps [N, 3] coefficients sigma(-x) of the forward; scatters through a
// permutation are gathers through its inverse, which the caller hands in.  No [N, d] shuffled copy exists in either direction.
// Index arrays are int32; an index outside its range reads row / column 0 (an undefined RESULT, never memory outside the tables).
#include "common.h"

namespace {

constexpr int MH_THREADS = 256;
constexpr int MH_MAX_BLOCKS = 512;
constexpr float MH_EPS = 1e-12f;              // F.normalize's clamp of the norm

inline bool mh_shape_ok(int64_t N, int64_t d) { return N >= 1 && N < 0x7fffffffLL && (d == 32 || d == 64 || d == 128); }

struct MhGeom {
    int G, rows_per_block;
};

inline MhGeom mh_geom(int N, int d) {
    const int rpb = MH_THREADS / (d / 4);
    const long long passes = ((long long)N + rpb - 1) / rpb;
    const long long g0 = passes < MH_MAX_BLOCKS ? passes : MH_MAX_BLOCKS;
    const long long ppb = (passes + g0 - 1) / g0;
    MhGeom g;
    g.G = (int)((passes + ppb - 1) / ppb);
    g.rows_per_block = (int)(ppb * rpb);
    return g;
}

__device__ __forceinline__ float4 f4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }
__device__ __forceinline__ float4 axpy4(const float s, const float4 a, const float4 y) {
    return make_float4(fmaf(s, a.x, y.x), fmaf(s, a.y, y.y), fmaf(s, a.z, y.z), fmaf(s, a.w, y.w));
}
__device__ __forceinline__ float4 scale4(const float s, const float4 a) { return make_float4(s * a.x, s * a.y, s * a.z, s * a.w); }
__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

template <int L>
__device__ __forceinline__ float grp_sum(float v) {
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int mh_index(const int32_t *__restrict__ p, const long long at, const int n) {
    const int i = p[at];
    return ((unsigned)i < (unsigned)n) ? i : 0;
}

// columns col[4 lig .. 4 lig + 3] of row `row` of a [*, D] table
template <int D>
__device__ __forceinline__ float4 mh_gather_cols(const float *__restrict__ T, const long long row, const int4 c) {
    const float *p = T + (size_t)row * D;
    return make_float4(p[c.x], p[c.y], p[c.z], p[c.w]);
}

template <int D>
__device__ __forceinline__ int4 mh_cols(const int32_t *__restrict__ col, const int lig) {
    int4 c;
    c.x = mh_index(col, 4 * lig, D);
    c.y = mh_index(col, 4 * lig + 1, D);
    c.z = mh_index(col, 4 * lig + 2, D);
    c.w = mh_index(col, 4 * lig + 3, D);
    return c;
}

// the workgroup's column sum: `acc` of every thread (its rows in ascending order) -> part[block][D], lane groups in ascending order
template <int D>
__device__ __forceinline__ void mh_block_colsum(const float4 acc, float4 *__restrict__ part) {
    constexpr int L = D / 4, RPB = MH_THREADS / L;
    __shared__ float4 s[MH_THREADS];
    s[threadIdx.x] = acc;
    __syncthreads();
    if ((int)threadIdx.x < L) {
        float4 t = s[threadIdx.x];
#pragma unroll 4
        for (int g = 1; g < RPB; ++g) t = add4(t, s[g * L + threadIdx.x]);
        part[(size_t)blockIdx.x * L + threadIdx.x] = t;
    }
}

// out[e] = (((s0 + s1) + s2) + s3) / div [+ nothing]; s_g = partials g, g + 4, ... of element e in ascending order.  64 elements per workgroup.
__global__ __launch_bounds__(256) void mh_colsum_finish_kernel(const float *__restrict__ part, const int S, const int n_elem, const float div,
                                                               float *__restrict__ out) {
    __shared__ float fs[4][64];
    const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + j;
    float s = 0.f;
    if (e < n_elem)
        for (int sl = g; sl < S; sl += 4) s += part[(size_t)sl * n_elem + e];
    fs[g][j] = s;
    __syncthreads();
    if (g == 0 && e < n_elem) out[e] = (((fs[0][j] + fs[1][j]) + fs[2][j]) + fs[3][j]) / div;
}

// ---- channel attention -------------------------------------------------------------------------------------------------------------
struct MhTables4 {
    const float4 *p[4];
};
struct MhOut4 {
    float4 *p[4];
};

// x / max(|x|, eps) added to a
template <int L>
__device__ __forceinline__ float4 mh_norm_add(const float4 a, const float4 e) {
    const float den = fmaxf(sqrtf(grp_sum<L>(dot4(e, e))), MH_EPS);
    return make_float4(a.x + e.x / den, a.y + e.y / den, a.z + e.z / den, a.w + e.w / den);
}

// gradient of x / max(|x|, eps) in x for the upstream row `go`: (go - y <go, y>) / n with y = x / n where n >= eps, go / eps below
template <int L>
__device__ __forceinline__ float4 mh_norm_bwd(const float4 e, const float4 go) {
    const float n = sqrtf(grp_sum<L>(dot4(e, e)));
    const float ge = grp_sum<L>(dot4(go, e));
    if (n >= MH_EPS) {
        const float k = ge / (n * n);
        return make_float4((go.x - k * e.x) / n, (go.y - k * e.y) / n, (go.z - k * e.z) / n, (go.w - k * e.w) / n);
    }
    return make_float4(go.x / MH_EPS, go.y / MH_EPS, go.z / MH_EPS, go.w / MH_EPS);
}

template <int D, bool SUMS>
__global__ __launch_bounds__(MH_THREADS) void mh_mix_fwd_kernel(const MhTables4 e_in, const float4 *__restrict__ v, const int N,
                                                                const int rows_per_block, const MhTables4 a_in, float4 *__restrict__ mixed,
                                                                float *__restrict__ scores, const MhOut4 o_out) {
    constexpr int L = D / 4, RPB = MH_THREADS / L;
    const int lig = threadIdx.x % L, grp = threadIdx.x / L;
    const float4 vv = v[lig];
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = r0 + rows_per_block < N ? r0 + rows_per_block : N;
    for (long long base = r0; base < r1; base += RPB) {
        const long long r = base + grp;
        const bool valid = r < r1;
        float4 e[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = valid ? e_in.p[k][(size_t)r * L + lig] : f4_zero();
        const float w0 = grp_sum<L>(dot4(e[0], vv)), w1 = grp_sum<L>(dot4(e[1], vv)), w2 = grp_sum<L>(dot4(e[2], vv));
        const float m = fmaxf(w0, fmaxf(w1, w2));
        const float p0 = expf(w0 - m), p1 = expf(w1 - m), p2 = expf(w2 - m);
        const float ps = (p0 + p1) + p2;
        const float s0 = p0 / ps, s1 = p1 / ps, s2 = p2 / ps;
        float4 mx = scale4(0.5f, e[3]);
        mx = axpy4(s2, e[2], mx);
        mx = axpy4(s1, e[1], mx);
        mx = axpy4(s0, e[0], mx);
        if (valid) {
            mixed[(size_t)r * L + lig] = mx;
            if (lig == 0) {
                scores[(size_t)r * 3] = s0;
                scores[(size_t)r * 3 + 1] = s1;
                scores[(size_t)r * 3 + 2] = s2;
            }
        }
        if constexpr (SUMS) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 a = valid ? a_in.p[k][(size_t)r * L + lig] : f4_zero();
                const float4 o = mh_norm_add<L>(a, e[k]);
                if (valid) o_out.p[k][(size_t)r * L + lig] = o;
            }
        }
    }
}

template <int D, bool SUMS>
__global__ __launch_bounds__(MH_THREADS) void mh_mix_bwd_kernel(const MhTables4 e_in, const float4 *__restrict__ v, const float *__restrict__ scores,
                                                                const int N, const int rows_per_block, const float4 *__restrict__ g_mixed,
                                                                const MhTables4 go_in, const MhOut4 d_out, float4 *__restrict__ part) {
    constexpr int L = D / 4, RPB = MH_THREADS / L;
    const int lig = threadIdx.x % L, grp = threadIdx.x / L;
    const float4 vv = v[lig];
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = r0 + rows_per_block < N ? r0 + rows_per_block : N;
    float4 dv = f4_zero();
    for (long long base = r0; base < r1; base += RPB) {
        const long long r = base + grp;
        const bool valid = r < r1;
        float4 e[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = valid ? e_in.p[k][(size_t)r * L + lig] : f4_zero();
        const float4 g = valid ? g_mixed[(size_t)r * L + lig] : f4_zero();
        float s[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = valid ? scores[(size_t)r * 3 + c] : 0.f;
        float ds[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) ds[c] = grp_sum<L>(dot4(g, e[c]));
        const float t = fmaf(s[2], ds[2], fmaf(s[1], ds[1], s[0] * ds[0]));
        float4 de[4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float dw = s[c] * (ds[c] - t);
            de[c] = axpy4(dw, vv, scale4(s[c], g));
            dv = axpy4(dw, e[c], dv);
        }
        de[3] = scale4(0.5f, g);
        if constexpr (SUMS) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 go = valid ? go_in.p[k][(size_t)r * L + lig] : f4_zero();
                de[k] = add4(de[k], mh_norm_bwd<L>(e[k], go));
            }
        }
        if (valid) {
#pragma unroll
            for (int k = 0; k < 4; ++k) d_out.p[k][(size_t)r * L + lig] = de[k];
        }
    }
    mh_block_colsum<D>(dv, part);
}

template <int D>
__global__ __launch_bounds__(MH_THREADS) void mh_normadd_fwd_kernel(const float4 *__restrict__ acc, const float4 *__restrict__ x, const int N,
                                                                    float4 *__restrict__ out) {
    constexpr int L = D / 4, RPB = MH_THREADS / L;
    const int lig = threadIdx.x % L;
    const long long r = (long long)blockIdx.x * RPB + threadIdx.x / L;
    const bool valid = r < N;
    const float4 e = valid ? x[(size_t)r * L + lig] : f4_zero();
    const float4 a = valid ? acc[(size_t)r * L + lig] : f4_zero();
    const float4 o = mh_norm_add<L>(a, e);
    if (valid) out[(size_t)r * L + lig] = o;
}

template <int D>
__global__ __launch_bounds__(MH_THREADS) void mh_normadd_bwd_kernel(const float4 *__restrict__ x, const float4 *__restrict__ g, const int N,
                                                                    float4 *__restrict__ dx) {
    constexpr int L = D / 4, RPB = MH_THREADS / L;
    const int lig = threadIdx.x % L;
    const long long r = (long long)blockIdx.x * RPB + threadIdx.x / L;
    const bool valid = r < N;
    const float4 e = valid ? x[(size_t)r * L + lig] : f4_zero();
    const float4 go = valid ? g[(size_t)r * L + lig] : f4_zero();
    const float4 d = mh_norm_bwd<L>(e, go);
    if (valid) dx[(size_t)r * L + lig] = d;
}

// ---- hierarchical self-supervision -------------------------------------------------------------------------------------------------
struct MhPerms {
    const int32_t *row_u, *col_1, *row_1, *col_2, *row_2;
};

template <int D>
__global__ __launch_bounds__(MH_THREADS) void mh_colsum_partial_kernel(const float4 *__restrict__ X, const int N, const int rows_per_block,
                                                                       float4 *__restrict__ part) {
    constexpr int L = D / 4, RPB = MH_THREADS / L;
    const int lig = threadIdx.x % L, grp = threadIdx.x / L;
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = r0 + rows_per_block < N ? r0 + rows_per_block : N;
    float4 acc = f4_zero();
    for (long long r = r0 + grp; r < r1; r += RPB) acc = add4(acc, X[(size_t)r * L + lig]);
    mh_block_colsum<D>(acc, part);
}

__device__ __forceinline__ float mh_log_sigmoid(const float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }
// sigma(-x), the derivative of log sigma(x)
__device__ __forceinline__ float mh_sigmoid_neg(const float x) {
    const float t = expf(-fabsf(x));
    return x >= 0.f ? t / (1.f + t) : 1.f / (1.f + t);
}

template <int D>
__global__ __launch_bounds__(MH_THREADS) void mh_ssl_fwd_kernel(const float *__restrict__ em, const float *__restrict__ edge, const MhPerms pm,
                                                                const float4 *__restrict__ graph, const int N, const int rows_per_block,
                                                                float *__restrict__ coef, double *__restrict__ lpart) {
    constexpr int L = D / 4, RPB = MH_THREADS / L;
    __shared__ double ls[RPB];
    const int lig = threadIdx.x % L, grp = threadIdx.x / L;
    const float4 *em4 = reinterpret_cast<const float4 *>(em), *ed4 = reinterpret_cast<const float4 *>(edge);
    const float4 gr = graph[lig];
    const int4 c1 = mh_cols<D>(pm.col_1, lig), c2 = mh_cols<D>(pm.col_2, lig);
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = r0 + rows_per_block < N ? r0 + rows_per_block : N;
    double loss = 0.0;
    for (long long base = r0; base < r1; base += RPB) {
        const long long r = base + grp;
        const bool valid = r < r1;
        float4 u = f4_zero(), e = f4_zero(), us = f4_zero(), e1 = f4_zero(), e2 = f4_zero();
        if (valid) {
            u = em4[(size_t)r * L + lig];
            e = ed4[(size_t)r * L + lig];
            us = em4[(size_t)mh_index(pm.row_u, r, N) * L + lig];
            e1 = mh_gather_cols<D>(edge, mh_index(pm.row_1, r, N), c1);
            e2 = mh_gather_cols<D>(edge, mh_index(pm.row_2, r, N), c2);
        }
        const float pos = grp_sum<L>(dot4(u, e)), neg1 = grp_sum<L>(dot4(us, e)), neg2 = grp_sum<L>(dot4(e1, u));
        const float gpos = grp_sum<L>(dot4(e, gr)), gneg = grp_sum<L>(dot4(e2, gr));
        const float x1 = pos - neg1, x2 = neg1 - neg2, x3 = gpos - gneg;
        if (valid && lig == 0) {
            loss -= ((double)mh_log_sigmoid(x1) + (double)mh_log_sigmoid(x2)) + (double)mh_log_sigmoid(x3);
            coef[(size_t)r * 3] = mh_sigmoid_neg(x1);
            coef[(size_t)r * 3 + 1] = mh_sigmoid_neg(x2);
            coef[(size_t)r * 3 + 2] = mh_sigmoid_neg(x3);
        }
    }
    if (lig == 0) ls[grp] = loss;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = ls[0];
        for (int g = 1; g < RPB; ++g) t += ls[g];
        lpart[blockIdx.x] = t;
    }
}

// the workgroups' partial losses in ascending order, 64 interleaved sets, then the sets in ascending order
__global__ __launch_bounds__(64) void mh_loss_finish_kernel(const double *__restrict__ lpart, const int S, float *__restrict__ out) {
    __shared__ double s[64];
    double t = 0.0;
    for (int i = threadIdx.x; i < S; i += 64) t += lpart[i];
    s[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = s[0];
        for (int i = 1; i < 64; ++i) a += s[i];
        out[0] = (float)a;
    }
}

// d_em, and d_edge without the term of the column mean; part = the workgroup's share of the mean's gradient (before / N)
template <int D>
__global__ __launch_bounds__(MH_THREADS) void mh_ssl_bwd_kernel(const float *__restrict__ em, const float *__restrict__ edge, const MhPerms pm,
                                                                const MhPerms inv, const float *__restrict__ coef, const float *__restrict__ graph,
                                                                const float *__restrict__ gloss, const int N, const int rows_per_block,
                                                                float4 *__restrict__ d_em, float4 *__restrict__ d_edge, float4 *__restrict__ part) {
    constexpr int L = D / 4, RPB = MH_THREADS / L;
    const int lig = threadIdx.x % L, grp = threadIdx.x / L;
    const float4 *em4 = reinterpret_cast<const float4 *>(em), *ed4 = reinterpret_cast<const float4 *>(edge);
    const float g = gloss[0];
    const float4 gr = reinterpret_cast<const float4 *>(graph)[lig];
    const int4 c1 = mh_cols<D>(pm.col_1, lig), c2 = mh_cols<D>(pm.col_2, lig);
    const int4 ic1 = mh_cols<D>(inv.col_1, lig), ic2 = mh_cols<D>(inv.col_2, lig);
    const float4 gr_ic2 = make_float4(graph[ic2.x], graph[ic2.y], graph[ic2.z], graph[ic2.w]);
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = r0 + rows_per_block < N ? r0 + rows_per_block : N;
    float4 dg = f4_zero();
    for (long long r = r0 + grp; r < r1; r += RPB) {
        const float k1 = coef[(size_t)r * 3], k2 = coef[(size_t)r * 3 + 1], k3 = coef[(size_t)r * 3 + 2];
        const float dpos = -g * k1, dneg1 = g * (k1 - k2), dneg2 = g * k2, dgpos = -g * k3, dgneg = g * k3;
        const float4 u = em4[(size_t)r * L + lig], e = ed4[(size_t)r * L + lig];
        const int ju = mh_index(inv.row_u, r, N), j1 = mh_index(inv.row_1, r, N), j2 = mh_index(inv.row_2, r, N);
        const float dneg1_ju = g * (coef[(size_t)ju * 3] - coef[(size_t)ju * 3 + 1]);
        const float dneg2_j1 = g * coef[(size_t)j1 * 3 + 1];
        const float dgneg_j2 = g * coef[(size_t)j2 * 3 + 2];
        // d em[r]: pos and neg2 of row r, neg1 of the row whose shuffled partner r is
        float4 du = scale4(dpos, e);
        du = axpy4(dneg2, mh_gather_cols<D>(edge, mh_index(pm.row_1, r, N), c1), du);
        du = axpy4(dneg1_ju, ed4[(size_t)ju * L + lig], du);
        d_em[(size_t)r * L + lig] = du;
        // d edge[r]: pos, neg1 and the global positive of row r; neg2 / the global negative of the rows that read row r through (row, col)
        float4 de = scale4(dpos, u);
        de = axpy4(dneg1, em4[(size_t)mh_index(pm.row_u, r, N) * L + lig], de);
        de = axpy4(dgpos, gr, de);
        de = axpy4(dneg2_j1, mh_gather_cols<D>(em, j1, ic1), de);
        de = axpy4(dgneg_j2, gr_ic2, de);
        d_edge[(size_t)r * L + lig] = de;
        // d graph: the global positive and negative of row r
        dg = axpy4(dgpos, e, dg);
        dg = axpy4(dgneg, mh_gather_cols<D>(edge, mh_index(pm.row_2, r, N), c2), dg);
    }
    mh_block_colsum<D>(dg, part);
}

template <int D>
__global__ __launch_bounds__(MH_THREADS) void mh_add_row_kernel(float4 *__restrict__ X, const float4 *__restrict__ row, const int N) {
    constexpr int L = D / 4, RPB = MH_THREADS / L;
    const long long r = (long long)blockIdx.x * RPB + threadIdx.x / L;
    if (r >= N) return;
    const int lig = threadIdx.x % L;
    X[(size_t)r * L + lig] = add4(X[(size_t)r * L + lig], row[lig]);
}

inline unsigned mh_blocks(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }
inline bool mh_aligned(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline float *mh_ws(void *ws) { return (float *)(((uintptr_t)ws + 15) & ~(uintptr_t)15); }

template <int D>
int mh_mix_fwd(const MhTables4 &e, const float *v, int N, const MhTables4 &a, bool sums, float *mixed, float *scores, const MhOut4 &o, hipStream_t st) {
    const MhGeom g = mh_geom(N, D);
    if (sums)
        hipLaunchKernelGGL((mh_mix_fwd_kernel<D, true>), dim3(g.G), dim3(MH_THREADS), 0, st, e, (const float4 *)v, N, g.rows_per_block, a, (float4 *)mixed,
                           scores, o);
    else
        hipLaunchKernelGGL((mh_mix_fwd_kernel<D, false>), dim3(g.G), dim3(MH_THREADS), 0, st, e, (const float4 *)v, N, g.rows_per_block, a,
                           (float4 *)mixed, scores, o);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

template <int D>
int mh_mix_bwd(const MhTables4 &e, const float *v, const float *scores, int N, const float *g_mixed, const MhTables4 &go, bool sums, const MhOut4 &d,
               float *dv, float *part, hipStream_t st) {
    const MhGeom g = mh_geom(N, D);
    if (sums)
        hipLaunchKernelGGL((mh_mix_bwd_kernel<D, true>), dim3(g.G), dim3(MH_THREADS), 0, st, e, (const float4 *)v, scores, N, g.rows_per_block,
                           (const float4 *)g_mixed, go, d, (float4 *)part);
    else
        hipLaunchKernelGGL((mh_mix_bwd_kernel<D, false>), dim3(g.G), dim3(MH_THREADS), 0, st, e, (const float4 *)v, scores, N, g.rows_per_block,
                           (const float4 *)g_mixed, go, d, (float4 *)part);
    hipLaunchKernelGGL(mh_colsum_finish_kernel, dim3(mh_blocks(D, 64)), dim3(256), 0, st, (const float *)part, g.G, D, 1.0f, dv);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

template <int D>
int mh_ssl_fwd(const float *em, const float *edge, const MhPerms &pm, int N, float *coef, float *graph, float *loss, float *ws, hipStream_t st) {
    const MhGeom g = mh_geom(N, D);
    float *part = ws;                                                   // [G, D]
    double *lpart = reinterpret_cast<double *>(ws + (size_t)g.G * D);   // [G] (the offset is a multiple of 16 bytes)
    hipLaunchKernelGGL((mh_colsum_partial_kernel<D>), dim3(g.G), dim3(MH_THREADS), 0, st, (const float4 *)edge, N, g.rows_per_block, (float4 *)part);
    hipLaunchKernelGGL(mh_colsum_finish_kernel, dim3(mh_blocks(D, 64)), dim3(256), 0, st, (const float *)part, g.G, D, (float)N, graph);
    hipLaunchKernelGGL((mh_ssl_fwd_kernel<D>), dim3(g.G), dim3(MH_THREADS), 0, st, em, edge, pm, (const float4 *)graph, N, g.rows_per_block, coef, lpart);
    hipLaunchKernelGGL(mh_loss_finish_kernel, dim3(1), dim3(64), 0, st, (const double *)lpart, g.G, loss);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

template <int D>
int mh_ssl_bwd(const float *em, const float *edge, const MhPerms &pm, const MhPerms &inv, const float *coef, const float *graph, const float *gloss,
               int N, float *d_em, float *d_edge, float *ws, hipStream_t st) {
    const MhGeom g = mh_geom(N, D);
    float *part = ws, *dgraph = ws + (size_t)g.G * D;
    hipLaunchKernelGGL((mh_ssl_bwd_kernel<D>), dim3(g.G), dim3(MH_THREADS), 0, st, em, edge, pm, inv, coef, graph, gloss, N, g.rows_per_block,
                       (float4 *)d_em, (float4 *)d_edge, (float4 *)part);
    hipLaunchKernelGGL(mh_colsum_finish_kernel, dim3(mh_blocks(D, 64)), dim3(256), 0, st, (const float *)part, g.G, D, (float)N, dgraph);
    hipLaunchKernelGGL((mh_add_row_kernel<D>), dim3(mh_blocks(N, MH_THREADS / (D / 4))), dim3(MH_THREADS), 0, st, (float4 *)d_edge, (const float4 *)dgraph, N);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

}      // namespace

#define MH_DISPATCH(d, call)             \
    switch (d) {                         \
    case 32: return call(32);            \
    case 64: return call(64);            \
    default: return call(128);           \
    }

extern "C" {

size_t sslrec_mhcn_ws_bytes(int32_t N, int32_t d) {
    if (!mh_shape_ok(N, d)) return 0;
    // [G, d] column partials, then G doubles (forward) or d floats (backward), plus the alignment slack
    return ((size_t)mh_geom(N, d).G * (d + 2) + d) * sizeof(float) + 32;
}

int sslrec_mhcn_mix_fwd_f32(const float *c1, const float *c2, const float *c3, const float *simp, const float *v, int32_t N, int32_t d,
                            const float *a1, const float *a2, const float *a3, const float *a4, float *mixed, float *scores, float *o1, float *o2,
                            float *o3, float *o4, void *stream) {
    if (!c1 || !c2 || !c3 || !simp || !v || !mixed || !scores || !mh_shape_ok(N, d)) return SSLREC_E_BADARG;
    const bool sums = a1 != nullptr;
    if (sums && (!a2 || !a3 || !a4 || !o1 || !o2 || !o3 || !o4)) return SSLREC_E_BADARG;
    if (!mh_aligned(c1) || !mh_aligned(c2) || !mh_aligned(c3) || !mh_aligned(simp) || !mh_aligned(v) || !mh_aligned(mixed)) return SSLREC_E_BADARG;
    if (sums && !(mh_aligned(a1) && mh_aligned(a2) && mh_aligned(a3) && mh_aligned(a4) && mh_aligned(o1) && mh_aligned(o2) && mh_aligned(o3) &&
                  mh_aligned(o4)))
        return SSLREC_E_BADARG;
    MhTables4 e, a;
    MhOut4 o;
    e.p[0] = (const float4 *)c1; e.p[1] = (const float4 *)c2; e.p[2] = (const float4 *)c3; e.p[3] = (const float4 *)simp;
    a.p[0] = (const float4 *)a1; a.p[1] = (const float4 *)a2; a.p[2] = (const float4 *)a3; a.p[3] = (const float4 *)a4;
    o.p[0] = (float4 *)o1; o.p[1] = (float4 *)o2; o.p[2] = (float4 *)o3; o.p[3] = (float4 *)o4;
    hipStream_t st = (hipStream_t)stream;
#define MH_CALL(D) mh_mix_fwd<D>(e, v, N, a, sums, mixed, scores, o, st)
    MH_DISPATCH(d, MH_CALL)
#undef MH_CALL
}

int sslrec_mhcn_mix_bwd_f32(const float *c1, const float *c2, const float *c3, const float *simp, const float *v, const float *scores, int32_t N,
                            int32_t d, const float *g_mixed, const float *go1, const float *go2, const float *go3, const float *go4, float *d1,
                            float *d2, float *d3, float *dsimp, float *dv, void *ws, void *stream) {
    if (!c1 || !c2 || !c3 || !simp || !v || !scores || !g_mixed || !d1 || !d2 || !d3 || !dsimp || !dv || !ws || !mh_shape_ok(N, d)) return SSLREC_E_BADARG;
    const bool sums = go1 != nullptr;
    if (sums && (!go2 || !go3 || !go4)) return SSLREC_E_BADARG;
    if (!mh_aligned(c1) || !mh_aligned(c2) || !mh_aligned(c3) || !mh_aligned(simp) || !mh_aligned(v) || !mh_aligned(g_mixed) || !mh_aligned(d1) ||
        !mh_aligned(d2) || !mh_aligned(d3) || !mh_aligned(dsimp))
        return SSLREC_E_BADARG;
    if (sums && !(mh_aligned(go1) && mh_aligned(go2) && mh_aligned(go3) && mh_aligned(go4))) return SSLREC_E_BADARG;
    MhTables4 e, go;
    MhOut4 o;
    e.p[0] = (const float4 *)c1; e.p[1] = (const float4 *)c2; e.p[2] = (const float4 *)c3; e.p[3] = (const float4 *)simp;
    go.p[0] = (const float4 *)go1; go.p[1] = (const float4 *)go2; go.p[2] = (const float4 *)go3; go.p[3] = (const float4 *)go4;
    o.p[0] = (float4 *)d1; o.p[1] = (float4 *)d2; o.p[2] = (float4 *)d3; o.p[3] = (float4 *)dsimp;
    hipStream_t st = (hipStream_t)stream;
    float *part = mh_ws(ws);
#define MH_CALL(D) mh_mix_bwd<D>(e, v, scores, N, g_mixed, go, sums, o, dv, part, st)
    MH_DISPATCH(d, MH_CALL)
#undef MH_CALL
}

int sslrec_mhcn_normadd_fwd_f32(const float *acc, const float *x, int32_t N, int32_t d, float *out, void *stream) {
    if (!acc || !x || !out || !mh_shape_ok(N, d) || !mh_aligned(acc) || !mh_aligned(x) || !mh_aligned(out)) return SSLREC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = mh_blocks(N, MH_THREADS / (d / 4));
    switch (d) {
    case 32: hipLaunchKernelGGL((mh_normadd_fwd_kernel<32>), dim3(blocks), dim3(MH_THREADS), 0, st, (const float4 *)acc, (const float4 *)x, N, (float4 *)out); break;
    case 64: hipLaunchKernelGGL((mh_normadd_fwd_kernel<64>), dim3(blocks), dim3(MH_THREADS), 0, st, (const float4 *)acc, (const float4 *)x, N, (float4 *)out); break;
    default: hipLaunchKernelGGL((mh_normadd_fwd_kernel<128>), dim3(blocks), dim3(MH_THREADS), 0, st, (const float4 *)acc, (const float4 *)x, N, (float4 *)out); break;
    }
    SSLREC_LAUNCH_CHECK();
    return 0;
}

int sslrec_mhcn_normadd_bwd_f32(const float *x, const float *g, int32_t N, int32_t d, float *dx, void *stream) {
    if (!x || !g || !dx || !mh_shape_ok(N, d) || !mh_aligned(x) || !mh_aligned(g) || !mh_aligned(dx)) return SSLREC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = mh_blocks(N, MH_THREADS / (d / 4));
    switch (d) {
    case 32: hipLaunchKernelGGL((mh_normadd_bwd_kernel<32>), dim3(blocks), dim3(MH_THREADS), 0, st, (const float4 *)x, (const float4 *)g, N, (float4 *)dx); break;
    case 64: hipLaunchKernelGGL((mh_normadd_bwd_kernel<64>), dim3(blocks), dim3(MH_THREADS), 0, st, (const float4 *)x, (const float4 *)g, N, (float4 *)dx); break;
    default: hipLaunchKernelGGL((mh_normadd_bwd_kernel<128>), dim3(blocks), dim3(MH_THREADS), 0, st, (const float4 *)x, (const float4 *)g, N, (float4 *)dx); break;
    }
    SSLREC_LAUNCH_CHECK();
    return 0;
}

int sslrec_mhcn_ssl_fwd_f32(const float *em, const float *edge, const int32_t *row_u, const int32_t *col_1, const int32_t *row_1,
                            const int32_t *col_2, const int32_t *row_2, int32_t N, int32_t d, float *coef, float *graph, float *loss, void *ws,
                            void *stream) {
    if (!em || !edge || !row_u || !col_1 || !row_1 || !col_2 || !row_2 || !coef || !graph || !loss || !ws || !mh_shape_ok(N, d)) return SSLREC_E_BADARG;
    if (!mh_aligned(em) || !mh_aligned(edge) || !mh_aligned(graph)) return SSLREC_E_BADARG;
    MhPerms pm = {row_u, col_1, row_1, col_2, row_2};
    hipStream_t st = (hipStream_t)stream;
    float *w = mh_ws(ws);
#define MH_CALL(D) mh_ssl_fwd<D>(em, edge, pm, N, coef, graph, loss, w, st)
    MH_DISPATCH(d, MH_CALL)
#undef MH_CALL
}

int sslrec_mhcn_ssl_bwd_f32(const float *em, const float *edge, const int32_t *row_u, const int32_t *col_1, const int32_t *row_1,
                            const int32_t *col_2, const int32_t *row_2, const int32_t *inv_row_u, const int32_t *inv_col_1,
                            const int32_t *inv_row_1, const int32_t *inv_col_2, const int32_t *inv_row_2, const float *coef, const float *graph,
                            const float *gloss, int32_t N, int32_t d, float *d_em, float *d_edge, void *ws, void *stream) {
    if (!em || !edge || !row_u || !col_1 || !row_1 || !col_2 || !row_2 || !inv_row_u || !inv_col_1 || !inv_row_1 || !inv_col_2 || !inv_row_2 || !coef ||
        !graph || !gloss || !d_em || !d_edge || !ws || !mh_shape_ok(N, d))
        return SSLREC_E_BADARG;
    if (!mh_aligned(em) || !mh_aligned(edge) || !mh_aligned(graph) || !mh_aligned(d_em) || !mh_aligned(d_edge)) return SSLREC_E_BADARG;
    MhPerms pm = {row_u, col_1, row_1, col_2, row_2};
    MhPerms inv = {inv_row_u, inv_col_1, inv_row_1, inv_col_2, inv_row_2};
    hipStream_t st = (hipStream_t)stream;
    float *w = mh_ws(ws);
#define MH_CALL(D) mh_ssl_bwd<D>(em, edge, pm, inv, coef, graph, gloss, N, d_em, d_edge, w, st)
    MH_DISPATCH(d, MH_CALL)
#undef MH_CALL
}

}      // extern "C"
