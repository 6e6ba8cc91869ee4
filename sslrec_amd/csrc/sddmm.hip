// Learned edge weights (AdaptiveMask, reference models/aug_utils.py:52-80 as DCCF calls it, models/general_cf/dccf.py:82-90):
//   * SDDMM: one dot product <A[row(e)], B[col(e)]> per entry of a sparse pattern, nothing of size nnz x d ever stored;
//   * the row normalization of the entry values, w = alpha / row sum of alpha, forward and backward;
//   * the inverse row norms of a table (F.normalize's) and the finish of the cosine's backward.
// The two valued SpMMs of the backward run on the tuned SpMM kernels (spmm.hip / spmm_swept.hip) through a re-valued view.
//
// Layout of every kernel: a LANE GROUP of L lanes owns one row of d = 4 L floats (one float4 per lane) or one row of the
// CSR; sums over a lane group are DPP permutes inside a 16-lane DPP row, ds_bpermute beyond it.  No atomics: every output
// word has exactly one writer, every sum a fixed order, so two runs give the same bits.
#include "common.h"
#include "lanegroup.h"      // dpp_add, group_sum, dot4

namespace {

// ---- SDDMM ---------------------------------------------------------------------------------------------------------------
// Work is split by ENTRIES (a hub row is spread over many waves): a wave takes G * U consecutive CSR positions, G = 64 / L lane
// groups times U entries in flight per group, so U random tail-row gathers of 4 d bytes overlap per lane; consecutive positions
// share the head row, which stays in L1.  The first lane of a group stores to the caller's entry id perm[k].
constexpr int SDDMM_U = 4;

template <int D>
__global__ __launch_bounds__(256) void sddmm_kernel(const int32_t *__restrict__ row_of_entry, const int32_t *__restrict__ col,
                                                    const int32_t *__restrict__ perm, const int nnz, const float4 *A, const float4 *B,
                                                    const float *__restrict__ ra, const float *__restrict__ cb, float *__restrict__ out) {
    constexpr int L = D / 4, G = 64 / L, U = SDDMM_U;
    const int lane = threadIdx.x & 63, lig = lane % L, g = lane / L;
    const long long k0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * (G * U) + g;
    if (k0 - g >= nnz) return;                               // (wave-uniform)
    int r[U], c[U];
    long long k[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        k[u] = k0 + u * G;
        const int kk = (int)(k[u] < nnz ? k[u] : nnz - 1);   // the tail of the last wave re-reads the last entry and does not store
        r[u] = row_of_entry[kk];
        c[u] = col[kk];
    }
    float4 a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        a[u] = A[(size_t)r[u] * L + lig];
        b[u] = B[(size_t)c[u] * L + lig];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        float s = group_sum<L>(dot4(a[u], b[u]));
        if (lig == 0 && k[u] < nnz) {
            if (ra) s *= ra[r[u]];
            if (cb) s *= cb[c[u]];
            out[perm[k[u]]] = s;
        }
    }
}

// ---- per-row work on [nnz] arrays ---------------------------------------------------------------------------------------------
// TEAM = 16: a DPP row of 16 lanes per CSR row (16 rows per workgroup of 256); TEAM = 256: a whole workgroup per row of the
// long-row list (rows of more than SSLREC_EDGE_LONG_ROW entries), so a hub row is cut into 256 interleaved chunks.
template <int TEAM>
__device__ __forceinline__ float team_sum(float v, float *lds) {
    v = group_sum<16>(v);
    if constexpr (TEAM == 256) {
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        __syncthreads();                                     // (the previous sum's readers are done with lds)
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
        __syncthreads();
        v = ((lds[0] + lds[1]) + lds[2]) + lds[3];
    }
    return v;
}

// the row this thread's team works on: false = none (past the end, or a long row the 256-lane launch handles)
template <int TEAM>
__device__ __forceinline__ bool team_row(const int32_t *rowptr, const int n_rows, const int32_t *long_rows, int &r, int &k0, int &k1,
                                         int &lane) {
    if constexpr (TEAM == 16) {
        r = (int)(((long long)blockIdx.x * 256 + threadIdx.x) >> 4);
        lane = threadIdx.x & 15;
        if (r >= n_rows) return false;
        k0 = rowptr[r];
        k1 = rowptr[r + 1];
        return !(long_rows && k1 - k0 > SSLREC_EDGE_LONG_ROW);
    } else {
        r = long_rows[blockIdx.x];
        lane = threadIdx.x;
        k0 = rowptr[r];
        k1 = rowptr[r + 1];
        return true;
    }
}

template <int TEAM>
__global__ __launch_bounds__(256) void rownorm_fwd_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ perm,
                                                          const int n_rows, const int32_t *__restrict__ long_rows,
                                                          const float *__restrict__ c, float *__restrict__ w, float *__restrict__ inv_s) {
    __shared__ float lds[4];
    int r, k0, k1, lane;
    if (!team_row<TEAM>(rowptr, n_rows, long_rows, r, k0, k1, lane)) return;
    float s = 0.f;
    for (int k = k0 + lane; k < k1; k += TEAM) s += (c[perm[k]] + 1.f) * 0.5f;
    s = team_sum<TEAM>(s, lds);
    float inv = 1.f / s;
    if (!(fabsf(inv) <= 3.402823466e38f)) inv = 0.f;         // .pow(-1).nan_to_num(0, 0, 0): an empty row has s = 0
    for (int k = k0 + lane; k < k1; k += TEAM) {
        const int e = perm[k];
        w[e] = (c[e] + 1.f) * 0.5f * inv;
    }
    if (lane == 0) inv_s[r] = inv;
}

template <int TEAM>
__global__ __launch_bounds__(256) void rownorm_bwd_head_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ perm,
                                                               const int n_rows, const int32_t *__restrict__ long_rows,
                                                               const float *__restrict__ dw, const float *__restrict__ w,
                                                               const float *__restrict__ inv_s, const float *__restrict__ c,
                                                               float *__restrict__ dc, float *__restrict__ p_head) {
    __shared__ float lds[4];
    int r, k0, k1, lane;
    if (!team_row<TEAM>(rowptr, n_rows, long_rows, r, k0, k1, lane)) return;
    float t = 0.f;
    for (int k = k0 + lane; k < k1; k += TEAM) {
        const int e = perm[k];
        t = fmaf(w[e], dw[e], t);
    }
    t = team_sum<TEAM>(t, lds);
    const float half_inv = 0.5f * inv_s[r];
    float p = 0.f;
    for (int k = k0 + lane; k < k1; k += TEAM) {
        const int e = perm[k];
        const float g = half_inv * (dw[e] - t);
        dc[e] = g;
        p = fmaf(g, c[e], p);
    }
    p = team_sum<TEAM>(p, lds);
    if (lane == 0) p_head[r] = p;
}

template <int TEAM>
__global__ __launch_bounds__(256) void rownorm_bwd_tail_kernel(const int32_t *__restrict__ rowptr_t, const int32_t *__restrict__ perm_t,
                                                               const int n_cols, const int32_t *__restrict__ long_rows_t,
                                                               const float *__restrict__ dc, const float *__restrict__ c,
                                                               float *__restrict__ p_tail) {
    __shared__ float lds[4];
    int r, k0, k1, lane;
    if (!team_row<TEAM>(rowptr_t, n_cols, long_rows_t, r, k0, k1, lane)) return;
    float p = 0.f;
    for (int k = k0 + lane; k < k1; k += TEAM) {
        const int e = perm_t[k];
        p = fmaf(dc[e], c[e], p);
    }
    p = team_sum<TEAM>(p, lds);
    if (lane == 0) p_tail[r] = p;
}

// ---- per-row work on [n_rows, d] tables: a lane group of d / 4 lanes per row -----------------------------------------------
constexpr float NORM_EPS = 1e-12f;                           // F.normalize's eps

template <int D>
__global__ __launch_bounds__(256) void row_invnorm_kernel(const float4 *__restrict__ S, const int n_rows, float *__restrict__ n,
                                                          float4 *__restrict__ normalized) {
    constexpr int L = D / 4;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int r = (int)(t / L), lig = (int)(t % L);
    if (r >= n_rows) return;                                 // (whole lane groups leave: L divides 256)
    const float4 x = S[(size_t)r * L + lig];
    const float ss = group_sum<L>(dot4(x, x));
    const float inv = 1.f / fmaxf(sqrtf(ss), NORM_EPS);
    if (lig == 0) n[r] = inv;
    if (normalized) normalized[(size_t)r * L + lig] = make_float4(x.x * inv, x.y * inv, x.z * inv, x.w * inv);
}

// dS = n (.) (G - (p_a + p_b) (.) n (.) S); rows whose norm is below eps were scaled by the CONSTANT 1 / eps: no projection term
template <int D>
__global__ __launch_bounds__(256) void cosine_finish_kernel(const float4 *__restrict__ S, const float *__restrict__ n, const float4 *G,
                                                            const float *__restrict__ p_a, const float *__restrict__ p_b, const int n_rows,
                                                            float4 *dS) {
    constexpr int L = D / 4;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int r = (int)(t / L);
    if (r >= n_rows) return;
    const float inv = n[r];
    float p = p_a[r];
    if (p_b) p += p_b[r];
    const float q = (inv < 1.f / NORM_EPS) ? p * inv : 0.f;
    const float4 x = S[t], g = G[t];
    dS[t] = make_float4(inv * fmaf(-q, x.x, g.x), inv * fmaf(-q, x.y, g.y), inv * fmaf(-q, x.z, g.z), inv * fmaf(-q, x.w, g.w));
}

inline bool dim_ok(int d) { return d == 8 || d == 16 || d == 32 || d == 64 || d == 128 || d == 256; }

inline unsigned blocks_for(long long threads) { return (unsigned)((threads + 255) / 256); }

#define SSLREC_BY_DIM(d, CALL)                                                                   \
    switch (d) {                                                                                 \
    case 8: CALL(8); break;                                                                      \
    case 16: CALL(16); break;                                                                    \
    case 32: CALL(32); break;                                                                    \
    case 64: CALL(64); break;                                                                    \
    case 128: CALL(128); break;                                                                  \
    default: CALL(256); break;                                                                   \
    }

}      // namespace

extern "C" {

int sslrec_sddmm_f32(const int32_t *row_of_entry, const int32_t *col, const int32_t *perm, int32_t n_rows, int32_t n_cols, int32_t nnz,
                     const float *A, const float *B, int32_t d, const float *ra, const float *cb, float *out, void *stream) {
    if (!row_of_entry || !col || !perm || !A || !B || !out || n_rows < 0 || n_cols < 0 || nnz < 0 || !dim_ok(d)) return SSLREC_E_BADARG;
    if (nnz == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
#define CALL(D)                                                                                                                \
    {                                                                                                                          \
        constexpr int per_block = 4 * (64 / (D / 4)) * SDDMM_U;                                                                \
        hipLaunchKernelGGL(sddmm_kernel<D>, dim3((unsigned)(((long long)nnz + per_block - 1) / per_block)), dim3(256), 0, st,  \
                           row_of_entry, col, perm, (int)nnz, (const float4 *)A, (const float4 *)B, ra, cb, out);              \
    }
    SSLREC_BY_DIM(d, CALL)
#undef CALL
    SSLREC_LAUNCH_CHECK();
    return 0;
}

int sslrec_edge_rownorm_fwd_f32(const int32_t *rowptr, const int32_t *perm, int32_t n_rows, const int32_t *long_rows, int32_t n_long,
                                const float *c, float *w, float *inv_s, void *stream) {
    if (!rowptr || !perm || !c || !w || !inv_s || n_rows < 0 || n_long < 0 || (n_long > 0 && !long_rows)) return SSLREC_E_BADARG;
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (n_long == 0) long_rows = nullptr;
    hipLaunchKernelGGL(rownorm_fwd_kernel<16>, dim3(blocks_for((long long)n_rows * 16)), dim3(256), 0, st, rowptr, perm, (int)n_rows,
                       long_rows, c, w, inv_s);
    if (n_long > 0)
        hipLaunchKernelGGL(rownorm_fwd_kernel<256>, dim3((unsigned)n_long), dim3(256), 0, st, rowptr, perm, (int)n_rows, long_rows, c, w,
                           inv_s);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

int sslrec_edge_rownorm_bwd_f32(const int32_t *rowptr, const int32_t *perm, int32_t n_rows, const int32_t *long_rows, int32_t n_long,
                                const int32_t *rowptr_t, const int32_t *perm_t, int32_t n_cols, const int32_t *long_rows_t,
                                int32_t n_long_t, const float *dw, const float *w, const float *inv_s, const float *c, float *dc,
                                float *p_head, float *p_tail, void *stream) {
    if (!rowptr || !perm || !rowptr_t || !perm_t || !dw || !w || !inv_s || !c || !dc || !p_head || !p_tail || n_rows < 0 || n_cols < 0 ||
        n_long < 0 || n_long_t < 0 || (n_long > 0 && !long_rows) || (n_long_t > 0 && !long_rows_t))
        return SSLREC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (n_long == 0) long_rows = nullptr;
    if (n_long_t == 0) long_rows_t = nullptr;
    if (n_rows > 0)
        hipLaunchKernelGGL(rownorm_bwd_head_kernel<16>, dim3(blocks_for((long long)n_rows * 16)), dim3(256), 0, st, rowptr, perm,
                           (int)n_rows, long_rows, dw, w, inv_s, c, dc, p_head);
    if (n_long > 0)
        hipLaunchKernelGGL(rownorm_bwd_head_kernel<256>, dim3((unsigned)n_long), dim3(256), 0, st, rowptr, perm, (int)n_rows, long_rows,
                           dw, w, inv_s, c, dc, p_head);
    if (n_cols > 0)
        hipLaunchKernelGGL(rownorm_bwd_tail_kernel<16>, dim3(blocks_for((long long)n_cols * 16)), dim3(256), 0, st, rowptr_t, perm_t,
                           (int)n_cols, long_rows_t, dc, c, p_tail);
    if (n_long_t > 0)
        hipLaunchKernelGGL(rownorm_bwd_tail_kernel<256>, dim3((unsigned)n_long_t), dim3(256), 0, st, rowptr_t, perm_t, (int)n_cols,
                           long_rows_t, dc, c, p_tail);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

int sslrec_row_invnorm_f32(const float *S, int32_t n_rows, int32_t d, float *n, float *normalized, void *stream) {
    if (!S || !n || n_rows < 0 || !dim_ok(d)) return SSLREC_E_BADARG;
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
#define CALL(D)                                                                                                                         \
    hipLaunchKernelGGL(row_invnorm_kernel<D>, dim3(blocks_for((long long)n_rows * (D / 4))), dim3(256), 0, st, (const float4 *)S, (int)n_rows, \
                       n, (float4 *)normalized);
    SSLREC_BY_DIM(d, CALL)
#undef CALL
    SSLREC_LAUNCH_CHECK();
    return 0;
}

int sslrec_cosine_finish_f32(const float *S, const float *n, const float *G, const float *p_a, const float *p_b, int32_t n_rows,
                             int32_t d, float *dS, void *stream) {
    if (!S || !n || !G || !p_a || !dS || n_rows < 0 || !dim_ok(d)) return SSLREC_E_BADARG;
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
#define CALL(D)                                                                                                                            \
    hipLaunchKernelGGL(cosine_finish_kernel<D>, dim3(blocks_for((long long)n_rows * (D / 4))), dim3(256), 0, st, (const float4 *)S, n,     \
                       (const float4 *)G, p_a, p_b, (int)n_rows, (float4 *)dS);
    SSLREC_BY_DIM(d, CALL)
#undef CALL
    SSLREC_LAUNCH_CHECK();
    return 0;
}

}      // extern "C"
