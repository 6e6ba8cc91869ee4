// Graph-transformer layer of AutoCF / GFormer (reference models/general_cf/autocf.py:109-129, gformer.py:221-255) on NODE tables:
// with the projections hoisted from entries to nodes, (X[rows]) W = (X W)[rows], the layer is an edge attention over a sparse
// N x N pattern,
//     s_eh = clamp(<Q[r_e, h, :], K[c_e, h, :]>, -10, 10),  w_eh = exp(s_eh),  Z_ih = sum over row i of w_eh,
//     Y[i, h, :] = sum over row i of w_eh / (Z_ih + 1e-8) * V[c_e, h, :].
// Nothing of size E x d or E x H is written, forward or backward: every pass recomputes the scores from the node tables.
//
// Layout, as in sddmm.hip: a LANE GROUP of L = d / 4 lanes owns one row of the pattern and holds its own table rows as one float4
// per lane; a head is HL = dh / 4 adjacent lanes and group_sum<HL> gives the head's dot product to all of them.  The group walks
// the row's entries in CSR order, U of them in flight, and keeps sum w V and Z in registers: one pass, no max subtraction (the
// clamp bounds w by e^10).  A row of more than SSLREC_EDGE_LONG_ROW entries gets a whole workgroup from the long-row list: its
// 256 / L lane groups take interleaved entries and their partial sums are added through LDS in the order of the groups.
// No atomics, one writer per output word, every sum in a fixed order: two runs give the same bits.
//
// Backward from dY: da_eh = <dY[r_e, h], V[c_e, h]>, t_ih = sum over row i of a da = <dY[i, h], Y[i, h]> (a kernel over rows, no pass
// over entries), ds_eh = a_eh (da_eh - t) [-10 < raw score < 10].  dQ is a pass over rows; dK and dV are ONE pass over the
// transposed pattern that recomputes a and ds per entry from Q[r], K[c], Z[r], t[r], dY[r], V[c].
#include "common.h"
#include "lanegroup.h"

namespace {

constexpr float GT_CLAMP = 10.f;
constexpr float GT_EPS = 1e-8f;

__device__ __forceinline__ float4 fma4(const float s, const float4 a, const float4 acc) {
    return make_float4(fmaf(s, a.x, acc.x), fmaf(s, a.y, acc.y), fmaf(s, a.z, acc.z), fmaf(s, a.w, acc.w));
}

__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// the row this thread's lane group works on, its first entry k and the end k1; false = none (past the end, or a long row that the
// workgroup-per-row launch handles).  LONG: the workgroup's 256 / L groups take entries g, g + 256 / L, ...
template <int L, bool LONG>
__device__ __forceinline__ bool gt_row(const int32_t *ptr, const int n, const int32_t *long_rows, int &r, int &k, int &k1) {
    constexpr int NG = 256 / L;
    const int g = threadIdx.x / L;
    if constexpr (LONG) {
        r = long_rows[blockIdx.x];
        k = ptr[r] + g;
        k1 = ptr[r + 1];
        return true;
    } else {
        const long long rr = (long long)blockIdx.x * NG + g;
        if (rr >= n) return false;                             // (whole lane groups leave: L divides 256)
        r = (int)rr;
        k = ptr[r];
        k1 = ptr[r + 1];
        return !(long_rows && k1 - k > SSLREC_EDGE_LONG_ROW);
    }
}

// LONG rows: the partial sums of the workgroup's lane groups, added in the order of the groups; every thread gets the total
template <int L>
__device__ __forceinline__ float4 gt_combine4(const float4 v, float4 *lds) {
    constexpr int NG = 256 / L;
    const int lig = threadIdx.x % L;
    __syncthreads();                                           // (the previous sum's readers are done with lds)
    lds[threadIdx.x] = v;
    __syncthreads();
    float4 s = lds[lig];
#pragma unroll 4
    for (int j = 1; j < NG; ++j) s = add4(s, lds[j * L + lig]);
    return s;
}

template <int L>
__device__ __forceinline__ float gt_combine1(const float v, float *lds) {
    constexpr int NG = 256 / L;
    const int lig = threadIdx.x % L;
    __syncthreads();
    lds[threadIdx.x] = v;
    __syncthreads();
    float s = lds[lig];
#pragma unroll 4
    for (int j = 1; j < NG; ++j) s += lds[j * L + lig];
    return s;
}

// ---- forward: Y and Z, one pass over the rows ------------------------------------------------------------------------------
template <int D, int DH, bool LONG>
__global__ __launch_bounds__(256) void gt_fwd_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int n,
                                                     const int32_t *__restrict__ long_rows, const float4 *__restrict__ Q,
                                                     const float4 *__restrict__ K, const float4 *__restrict__ V, float4 *__restrict__ Y,
                                                     float *__restrict__ Z) {
    constexpr int L = D / 4, HL = DH / 4, H = D / DH, STEP = LONG ? 256 / L : 1, U = 4;
    __shared__ float4 lds4[LONG ? 256 : 1];
    __shared__ float lds1[LONG ? 256 : 1];
    int r, k, k1;
    if (!gt_row<L, LONG>(rowptr, n, long_rows, r, k, k1)) return;
    const int lig = threadIdx.x % L;
    const float4 q = Q[(size_t)r * L + lig];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float z = 0.f;
    auto eat = [&](const float4 kv, const float4 vv) {
        const float s = group_sum<HL>(dot4(q, kv));
        const float w = expf(fminf(fmaxf(s, -GT_CLAMP), GT_CLAMP));
        z += w;
        acc = fma4(w, vv, acc);
    };
    for (; k + (U - 1) * STEP < k1; k += U * STEP) {
        int c[U];
        float4 kv[U], vv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) c[u] = col[k + u * STEP];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            kv[u] = K[(size_t)c[u] * L + lig];
            vv[u] = V[(size_t)c[u] * L + lig];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) eat(kv[u], vv[u]);
    }
    for (; k < k1; k += STEP) {
        const int c = col[k];
        eat(K[(size_t)c * L + lig], V[(size_t)c * L + lig]);
    }
    if constexpr (LONG) {
        acc = gt_combine4<L>(acc, lds4);
        z = gt_combine1<L>(z, lds1);
        if (threadIdx.x >= L) return;                          // the first lane group writes
    }
    const float den = z + GT_EPS;                              // a row without entries: 0 / 1e-8 = exact zeros
    Y[(size_t)r * L + lig] = make_float4(acc.x / den, acc.y / den, acc.z / den, acc.w / den);
    if (lig % HL == 0) Z[(size_t)r * H + lig / HL] = z;
}

// ---- t[i, h] = <dY[i, h, :], Y[i, h, :]> ---------------------------------------------------------------------------------------
template <int D, int DH>
__global__ __launch_bounds__(256) void gt_t_kernel(const float4 *__restrict__ dY, const float4 *__restrict__ Y, const int n,
                                                   float *__restrict__ T) {
    constexpr int L = D / 4, HL = DH / 4, H = D / DH;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long r = i / L;
    const int lig = (int)(i % L);
    if (r >= n) return;                                        // (whole lane groups leave)
    const float t = group_sum<HL>(dot4(dY[i], Y[i]));
    if (lig % HL == 0) T[(size_t)r * H + lig / HL] = t;
}

// ---- dQ: a pass over the rows --------------------------------------------------------------------------------------------------
template <int D, int DH, bool LONG>
__global__ __launch_bounds__(256) void gt_dq_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int n,
                                                    const int32_t *__restrict__ long_rows, const float4 *__restrict__ Q,
                                                    const float4 *__restrict__ K, const float4 *__restrict__ V,
                                                    const float4 *__restrict__ dY, const float *__restrict__ Z,
                                                    const float *__restrict__ T, float4 *__restrict__ dQ) {
    constexpr int L = D / 4, HL = DH / 4, H = D / DH, STEP = LONG ? 256 / L : 1, U = 2;
    __shared__ float4 lds4[LONG ? 256 : 1];
    int r, k, k1;
    if (!gt_row<L, LONG>(rowptr, n, long_rows, r, k, k1)) return;
    const int lig = threadIdx.x % L;
    const float4 q = Q[(size_t)r * L + lig], dy = dY[(size_t)r * L + lig];
    const float den = Z[(size_t)r * H + lig / HL] + GT_EPS, t = T[(size_t)r * H + lig / HL];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    auto eat = [&](const float4 kv, const float4 vv) {
        const float s = group_sum<HL>(dot4(q, kv));
        const float da = group_sum<HL>(dot4(dy, vv));
        const float a = expf(fminf(fmaxf(s, -GT_CLAMP), GT_CLAMP)) / den;
        const float ds = (s > -GT_CLAMP && s < GT_CLAMP) ? a * (da - t) : 0.f;
        acc = fma4(ds, kv, acc);
    };
    for (; k + (U - 1) * STEP < k1; k += U * STEP) {
        int c[U];
        float4 kv[U], vv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) c[u] = col[k + u * STEP];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            kv[u] = K[(size_t)c[u] * L + lig];
            vv[u] = V[(size_t)c[u] * L + lig];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) eat(kv[u], vv[u]);
    }
    for (; k < k1; k += STEP) {
        const int c = col[k];
        eat(K[(size_t)c * L + lig], V[(size_t)c * L + lig]);
    }
    if constexpr (LONG) {
        acc = gt_combine4<L>(acc, lds4);
        if (threadIdx.x >= L) return;
    }
    dQ[(size_t)r * L + lig] = acc;
}

// ---- dK and dV: a pass over the TRANSPOSED pattern (colptr / row), a lane group per column ------------------------------------
template <int D, int DH, bool LONG>
__global__ __launch_bounds__(256) void gt_dkv_kernel(const int32_t *__restrict__ colptr, const int32_t *__restrict__ row, const int n,
                                                     const int32_t *__restrict__ long_cols, const float4 *__restrict__ Q,
                                                     const float4 *__restrict__ K, const float4 *__restrict__ V,
                                                     const float4 *__restrict__ dY, const float *__restrict__ Z,
                                                     const float *__restrict__ T, float4 *__restrict__ dK, float4 *__restrict__ dV) {
    constexpr int L = D / 4, HL = DH / 4, H = D / DH, STEP = LONG ? 256 / L : 1, U = 2;
    __shared__ float4 lds4[LONG ? 256 : 1];
    int c, k, k1;
    if (!gt_row<L, LONG>(colptr, n, long_cols, c, k, k1)) return;
    const int lig = threadIdx.x % L, h = lig / HL;
    const float4 kv = K[(size_t)c * L + lig], vv = V[(size_t)c * L + lig];
    float4 acc_k = make_float4(0.f, 0.f, 0.f, 0.f), acc_v = acc_k;
    auto eat = [&](const float4 q, const float4 dy, const float z, const float t) {
        const float s = group_sum<HL>(dot4(q, kv));
        const float da = group_sum<HL>(dot4(dy, vv));
        const float a = expf(fminf(fmaxf(s, -GT_CLAMP), GT_CLAMP)) / (z + GT_EPS);
        const float ds = (s > -GT_CLAMP && s < GT_CLAMP) ? a * (da - t) : 0.f;
        acc_k = fma4(ds, q, acc_k);
        acc_v = fma4(a, dy, acc_v);
    };
    for (; k + (U - 1) * STEP < k1; k += U * STEP) {
        int r[U];
        float4 q[U], dy[U];
        float z[U], t[U];
#pragma unroll
        for (int u = 0; u < U; ++u) r[u] = row[k + u * STEP];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            q[u] = Q[(size_t)r[u] * L + lig];
            dy[u] = dY[(size_t)r[u] * L + lig];
            z[u] = Z[(size_t)r[u] * H + h];
            t[u] = T[(size_t)r[u] * H + h];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) eat(q[u], dy[u], z[u], t[u]);
    }
    for (; k < k1; k += STEP) {
        const int r = row[k];
        eat(Q[(size_t)r * L + lig], dY[(size_t)r * L + lig], Z[(size_t)r * H + h], T[(size_t)r * H + h]);
    }
    if constexpr (LONG) {
        acc_k = gt_combine4<L>(acc_k, lds4);
        acc_v = gt_combine4<L>(acc_v, lds4);
        if (threadIdx.x >= L) return;
    }
    if (dK) dK[(size_t)c * L + lig] = acc_k;
    if (dV) dV[(size_t)c * L + lig] = acc_v;
}

// ---- per-entry attention summed over the heads (GFormer's LocalGraph, gformer.py:351-352: att_edge = t.sum(atten, dim=-1)) ---------
// Two passes over the rows with the forward's walk.  WRITE = false: Z[r, h]; WRITE = true: out[k] = sum_h w_kh / (Z[r, h] + 1e-8) for every
// CSR position k of the row.  The heads' values sit on the first lane of each head; group_sum<L> adds them in a fixed order.
template <int D, int DH, bool LONG, bool WRITE>
__global__ __launch_bounds__(256) void gt_scores_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int n,
                                                        const int32_t *__restrict__ long_rows, const float4 *__restrict__ Q,
                                                        const float4 *__restrict__ K, float *__restrict__ Z, float *__restrict__ out) {
    constexpr int L = D / 4, HL = DH / 4, H = D / DH, STEP = LONG ? 256 / L : 1;
    __shared__ float lds1[LONG ? 256 : 1];
    int r, k, k1;
    if (!gt_row<L, LONG>(rowptr, n, long_rows, r, k, k1)) return;
    const int lig = threadIdx.x % L;
    const float4 q = Q[(size_t)r * L + lig];
    if constexpr (WRITE) {
        const float den = Z[(size_t)r * H + lig / HL] + GT_EPS;
        for (; k < k1; k += STEP) {
            const int c = col[k];
            const float s = group_sum<HL>(dot4(q, K[(size_t)c * L + lig]));
            const float a = expf(fminf(fmaxf(s, -GT_CLAMP), GT_CLAMP)) / den;
            const float tot = group_sum<L>(lig % HL == 0 ? a : 0.f);
            if (lig == 0) out[k] = tot;
        }
    } else {
        float z = 0.f;
        for (; k < k1; k += STEP) {
            const int c = col[k];
            const float s = group_sum<HL>(dot4(q, K[(size_t)c * L + lig]));
            z += expf(fminf(fmaxf(s, -GT_CLAMP), GT_CLAMP));
        }
        if constexpr (LONG) {
            z = gt_combine1<L>(z, lds1);
            if (threadIdx.x >= L) return;
        }
        if (lig % HL == 0) Z[(size_t)r * H + lig / HL] = z;
    }
}

inline bool gt_shape_ok(int d, int heads) {
    if (d != 32 && d != 64 && d != 128) return false;
    if (heads < 1 || d % heads != 0) return false;
    const int dh = d / heads;
    return dh >= 4 && (dh & (dh - 1)) == 0;
}

inline unsigned gt_blocks(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

#define GT_BY_SHAPE(d, dh, CALL)                                                                 \
    switch ((d) * 1000 + (dh)) {                                                                 \
    case 32004: CALL(32, 4); break;                                                              \
    case 32008: CALL(32, 8); break;                                                              \
    case 32016: CALL(32, 16); break;                                                             \
    case 32032: CALL(32, 32); break;                                                             \
    case 64004: CALL(64, 4); break;                                                              \
    case 64008: CALL(64, 8); break;                                                              \
    case 64016: CALL(64, 16); break;                                                             \
    case 64032: CALL(64, 32); break;                                                             \
    case 64064: CALL(64, 64); break;                                                             \
    case 128004: CALL(128, 4); break;                                                            \
    case 128008: CALL(128, 8); break;                                                            \
    case 128016: CALL(128, 16); break;                                                           \
    case 128032: CALL(128, 32); break;                                                           \
    case 128064: CALL(128, 64); break;                                                           \
    case 128128: CALL(128, 128); break;                                                          \
    default: return SSLREC_E_BADARG;                                                             \
    }

}      // namespace

extern "C" {

int sslrec_gt_fwd_f32(const int32_t *rowptr, const int32_t *col, int32_t n, const int32_t *long_rows, int32_t n_long, const float *Q,
                      const float *K, const float *V, int32_t d, int32_t heads, float *Y, float *Z, void *stream) {
    if (!rowptr || !col || !Q || !K || !V || !Y || !Z || n < 0 || n_long < 0 || (n_long > 0 && !long_rows) || !gt_shape_ok(d, heads))
        return SSLREC_E_BADARG;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (n_long == 0) long_rows = nullptr;
#define CALL(D, DH)                                                                                                                       \
    {                                                                                                                                     \
        hipLaunchKernelGGL((gt_fwd_kernel<D, DH, false>), dim3(gt_blocks(n, 256 / (D / 4))), dim3(256), 0, st, rowptr, col, (int)n,       \
                           long_rows, (const float4 *)Q, (const float4 *)K, (const float4 *)V, (float4 *)Y, Z);                           \
        if (n_long > 0)                                                                                                                   \
            hipLaunchKernelGGL((gt_fwd_kernel<D, DH, true>), dim3((unsigned)n_long), dim3(256), 0, st, rowptr, col, (int)n, long_rows,    \
                               (const float4 *)Q, (const float4 *)K, (const float4 *)V, (float4 *)Y, Z);                                  \
    }
    GT_BY_SHAPE(d, d / heads, CALL)
#undef CALL
    SSLREC_LAUNCH_CHECK();
    return 0;
}

size_t sslrec_gt_scores_ws_bytes(int32_t n, int32_t d, int32_t heads) {
    if (n < 1 || !gt_shape_ok(d, heads)) return 0;
    return (size_t)n * heads * sizeof(float);
}

int sslrec_gt_scores_f32(const int32_t *rowptr, const int32_t *col, int32_t n, const int32_t *long_rows, int32_t n_long, const float *Q,
                         const float *K, int32_t d, int32_t heads, float *out, float *z_ws, void *stream) {
    if (!rowptr || !col || !Q || !K || !out || !z_ws || n < 0 || n_long < 0 || (n_long > 0 && !long_rows) || !gt_shape_ok(d, heads))
        return SSLREC_E_BADARG;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (n_long == 0) long_rows = nullptr;
#define CALL(D, DH)                                                                                                                       \
    {                                                                                                                                     \
        hipLaunchKernelGGL((gt_scores_kernel<D, DH, false, false>), dim3(gt_blocks(n, 256 / (D / 4))), dim3(256), 0, st, rowptr, col,     \
                           (int)n, long_rows, (const float4 *)Q, (const float4 *)K, z_ws, out);                                           \
        if (n_long > 0)                                                                                                                   \
            hipLaunchKernelGGL((gt_scores_kernel<D, DH, true, false>), dim3((unsigned)n_long), dim3(256), 0, st, rowptr, col, (int)n,     \
                               long_rows, (const float4 *)Q, (const float4 *)K, z_ws, out);                                               \
        hipLaunchKernelGGL((gt_scores_kernel<D, DH, false, true>), dim3(gt_blocks(n, 256 / (D / 4))), dim3(256), 0, st, rowptr, col,      \
                           (int)n, long_rows, (const float4 *)Q, (const float4 *)K, z_ws, out);                                           \
        if (n_long > 0)                                                                                                                   \
            hipLaunchKernelGGL((gt_scores_kernel<D, DH, true, true>), dim3((unsigned)n_long), dim3(256), 0, st, rowptr, col, (int)n,      \
                               long_rows, (const float4 *)Q, (const float4 *)K, z_ws, out);                                               \
    }
    GT_BY_SHAPE(d, d / heads, CALL)
#undef CALL
    SSLREC_LAUNCH_CHECK();
    return 0;
}

int sslrec_gt_bwd_f32(const int32_t *rowptr, const int32_t *col, const int32_t *long_rows, int32_t n_long, const int32_t *colptr,
                      const int32_t *row, const int32_t *long_cols, int32_t n_long_cols, int32_t n, const float *Q, const float *K,
                      const float *V, const float *Y, const float *Z, const float *dY, int32_t d, int32_t heads, float *dQ, float *dK,
                      float *dV, float *t_ws, void *stream) {
    if (!rowptr || !col || !colptr || !row || !Q || !K || !V || !Y || !Z || !dY || !t_ws || n < 0 || n_long < 0 || n_long_cols < 0 ||
        (n_long > 0 && !long_rows) || (n_long_cols > 0 && !long_cols) || !gt_shape_ok(d, heads))
        return SSLREC_E_BADARG;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (n_long == 0) long_rows = nullptr;
    if (n_long_cols == 0) long_cols = nullptr;
#define CALL(D, DH)                                                                                                                       \
    {                                                                                                                                     \
        hipLaunchKernelGGL((gt_t_kernel<D, DH>), dim3(gt_blocks((long long)n * (D / 4), 256)), dim3(256), 0, st, (const float4 *)dY,      \
                           (const float4 *)Y, (int)n, t_ws);                                                                              \
        if (dQ) {                                                                                                                         \
            hipLaunchKernelGGL((gt_dq_kernel<D, DH, false>), dim3(gt_blocks(n, 256 / (D / 4))), dim3(256), 0, st, rowptr, col, (int)n,    \
                               long_rows, (const float4 *)Q, (const float4 *)K, (const float4 *)V, (const float4 *)dY, Z,                 \
                               (const float *)t_ws, (float4 *)dQ);                                                                        \
            if (n_long > 0)                                                                                                               \
                hipLaunchKernelGGL((gt_dq_kernel<D, DH, true>), dim3((unsigned)n_long), dim3(256), 0, st, rowptr, col, (int)n,            \
                                   long_rows, (const float4 *)Q, (const float4 *)K, (const float4 *)V, (const float4 *)dY, Z,             \
                                   (const float *)t_ws, (float4 *)dQ);                                                                    \
        }                                                                                                                                 \
        if (dK || dV) {                                                                                                                   \
            hipLaunchKernelGGL((gt_dkv_kernel<D, DH, false>), dim3(gt_blocks(n, 256 / (D / 4))), dim3(256), 0, st, colptr, row, (int)n,   \
                               long_cols, (const float4 *)Q, (const float4 *)K, (const float4 *)V, (const float4 *)dY, Z,                 \
                               (const float *)t_ws, (float4 *)dK, (float4 *)dV);                                                          \
            if (n_long_cols > 0)                                                                                                          \
                hipLaunchKernelGGL((gt_dkv_kernel<D, DH, true>), dim3((unsigned)n_long_cols), dim3(256), 0, st, colptr, row, (int)n,      \
                                   long_cols, (const float4 *)Q, (const float4 *)K, (const float4 *)V, (const float4 *)dY, Z,             \
                                   (const float *)t_ws, (float4 *)dK, (float4 *)dV);                                                      \
        }                                                                                                                                 \
    }
    GT_BY_SHAPE(d, d / heads, CALL)
#undef CALL
    SSLREC_LAUNCH_CHECK();
    return 0;
}

}      // extern "C"
