// DenoiseNet's edge gate and symmetric normalisation of AdaGCL, forward and backward (reference models/general_cf/adagcl.py:274-338,
// :358-401 and l0_norm :340-347), on [nnz] and [N] vectors only.  get_attention's Linear + ReLU on the gathered rows is the gather
// of the transformed NODE table and its final Linear(2 d, 1) splits into two dots, so log_alpha[e] = p[row(e)] + q[col(e)] + bias
// with two [N] vectors that dense torch computes (and carries the gradients of).
//
// Layout, as the row normalizations of sddmm.hip: a TEAM of 16 lanes (one DPP row) owns one row of the CSR, a whole workgroup one
// row of the long-row list; sums over a column run over the TRANSPOSED plan's rows.  No float atomics: every output word has one
// writer and every sum a fixed order, so two runs give the same bits.
#include "common.h"
#include "lanegroup.h"      // group_sum

namespace {

template <int TEAM>
__device__ __forceinline__ float gate_team_sum(float v, float *lds) {
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
__device__ __forceinline__ bool gate_team_row(const int32_t *rowptr, const int n_rows, const int32_t *long_rows, int &r, int &k0, int &k1,
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

struct GateArgs {
    float gamma, zeta, beta, l0_shift, eps;      // l0_shift = beta * log(-gamma / zeta)
};

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// the gate's input: (noise + log_alpha) / beta in training, log_alpha itself without a noise vector
__device__ __forceinline__ float gate_input(const float la, const float *noise, const int e, const float beta) {
    return noise ? (noise[e] + la) / beta : la;
}

// m[e], s[n] = eps + row sum, dinv[n] = clamp(s^-0.5, 0, 10), l0_row[n] = row sum of sigmoid(log_alpha - l0_shift)
template <int TEAM>
__global__ __launch_bounds__(256) void gate_fwd_rows_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                            const int32_t *__restrict__ perm, const int n_rows,
                                                            const int32_t *__restrict__ long_rows, const float *__restrict__ p,
                                                            const float *__restrict__ q, const float *__restrict__ bias,
                                                            const float *__restrict__ noise, const GateArgs a, float *__restrict__ m,
                                                            float *__restrict__ s_out, float *__restrict__ dinv, float *__restrict__ l0_row) {
    __shared__ float lds[4];
    int r, k0, k1, lane;
    if (!gate_team_row<TEAM>(rowptr, n_rows, long_rows, r, k0, k1, lane)) return;
    const float pb = p[r] + bias[0];
    float s = 0.f, l0 = 0.f;
    for (int k = k0 + lane; k < k1; k += TEAM) {
        const int e = perm[k];
        const float la = pb + q[col[k]];
        const float sg = sigmoid_f(gate_input(la, noise, e, a.beta));
        const float mm = fminf(fmaxf(sg * (a.zeta - a.gamma) + a.gamma, 0.f), 1.f);
        m[e] = mm;
        s += mm;
        l0 += sigmoid_f(la - a.l0_shift);
    }
    s = gate_team_sum<TEAM>(s, lds) + a.eps;
    l0 = gate_team_sum<TEAM>(l0, lds);
    if (lane == 0) {
        s_out[r] = s;
        dinv[r] = fminf(fmaxf(1.f / sqrtf(s), 0.f), 10.f);      // (s = 0: inf -> 10)
        l0_row[r] = l0;
    }
}

// vals[e] = m[e] dinv[row] dinv[col]: the reference takes ROW sums for both ends
__global__ __launch_bounds__(256) void gate_fwd_vals_kernel(const int32_t *__restrict__ row_of_entry, const int32_t *__restrict__ col,
                                                            const int32_t *__restrict__ perm, const int nnz, const float *__restrict__ m,
                                                            const float *__restrict__ dinv, float *__restrict__ vals) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= nnz) return;
    const int e = perm[k];
    vals[e] = (m[e] * dinv[row_of_entry[k]]) * dinv[col[k]];
}

// out[0] = scale * sum of v[0 .. n) in a fixed order (one workgroup: thread t adds the elements t, t + 256, ..., then a tree)
__global__ __launch_bounds__(256) void gate_reduce_kernel(const float *__restrict__ v, const int n, const float scale, float *__restrict__ out) {
    __shared__ float part[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += v[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = part[0] * scale;
}

// t[e] = dvals[e] m[e], a_row[n] = sum over the row of t[e] dinv[col(e)]
template <int TEAM>
__global__ __launch_bounds__(256) void gate_bwd_rowdot_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                              const int32_t *__restrict__ perm, const int n_rows,
                                                              const int32_t *__restrict__ long_rows, const float *__restrict__ dvals,
                                                              const float *__restrict__ m, const float *__restrict__ dinv,
                                                              float *__restrict__ a_row) {
    __shared__ float lds[4];
    int r, k0, k1, lane;
    if (!gate_team_row<TEAM>(rowptr, n_rows, long_rows, r, k0, k1, lane)) return;
    float s = 0.f;
    for (int k = k0 + lane; k < k1; k += TEAM) {
        const int e = perm[k];
        s = fmaf(dvals[e] * m[e], dinv[col[k]], s);
    }
    s = gate_team_sum<TEAM>(s, lds);
    if (lane == 0) a_row[r] = s;
}

// over the TRANSPOSED plan (its rows are the columns, its `col` the rows): ddinv[n] = a_row[n] + sum over column n of t[e] dinv[row(e)],
// ds[n] = ddinv d clamp(s^-0.5, 0, 10) / ds: -0.5 s^-1.5, and 0 where the clamp at 10 is active
template <int TEAM>
__global__ __launch_bounds__(256) void gate_bwd_coldot_kernel(const int32_t *__restrict__ rowptr_t, const int32_t *__restrict__ col_t,
                                                              const int32_t *__restrict__ perm_t, const int n_cols,
                                                              const int32_t *__restrict__ long_rows_t, const float *__restrict__ dvals,
                                                              const float *__restrict__ m, const float *__restrict__ dinv,
                                                              const float *__restrict__ s_in, const float *__restrict__ a_row,
                                                              float *__restrict__ ds) {
    __shared__ float lds[4];
    int r, k0, k1, lane;
    if (!gate_team_row<TEAM>(rowptr_t, n_cols, long_rows_t, r, k0, k1, lane)) return;
    float s = 0.f;
    for (int k = k0 + lane; k < k1; k += TEAM) {
        const int e = perm_t[k];
        s = fmaf(dvals[e] * m[e], dinv[col_t[k]], s);
    }
    s = gate_team_sum<TEAM>(s, lds);
    if (lane == 0) {
        const float sn = s_in[r], raw = 1.f / sqrtf(sn);
        ds[r] = (raw > 10.f) ? 0.f : -0.5f * (a_row[r] + s) * raw / sn;
    }
}

// dm = dvals dinv_r dinv_c + ds[row], 0 where the [0, 1] clamp is active; back through the sigmoid and 1 / beta, plus the l0 term:
// dla[e] and dp[n] = its row sum
template <int TEAM>
__global__ __launch_bounds__(256) void gate_bwd_rows_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                            const int32_t *__restrict__ perm, const int n_rows,
                                                            const int32_t *__restrict__ long_rows, const float *__restrict__ p,
                                                            const float *__restrict__ q, const float *__restrict__ bias,
                                                            const float *__restrict__ noise, const GateArgs a, const float *__restrict__ dvals,
                                                            const float *__restrict__ dl0, const float inv_nnz, const float *__restrict__ dinv,
                                                            const float *__restrict__ ds, float *__restrict__ dla, float *__restrict__ dp) {
    __shared__ float lds[4];
    int r, k0, k1, lane;
    if (!gate_team_row<TEAM>(rowptr, n_rows, long_rows, r, k0, k1, lane)) return;
    const float pb = p[r] + bias[0], dr = dinv[r], dsr = ds[r], gl0 = dl0[0] * inv_nnz;
    float acc = 0.f;
    for (int k = k0 + lane; k < k1; k += TEAM) {
        const int e = perm[k];
        const int c = col[k];
        const float la = pb + q[c];
        const float sg = sigmoid_f(gate_input(la, noise, e, a.beta));
        const float st = sg * (a.zeta - a.gamma) + a.gamma;
        float dm = fmaf(dvals[e] * dr, dinv[c], dsr);
        if (st < 0.f || st > 1.f) dm = 0.f;
        float g = dm * (a.zeta - a.gamma) * (sg * (1.f - sg));
        if (noise) g /= a.beta;
        const float s0 = sigmoid_f(la - a.l0_shift);
        g = fmaf(gl0, s0 * (1.f - s0), g);
        dla[e] = g;
        acc += g;
    }
    acc = gate_team_sum<TEAM>(acc, lds);
    if (lane == 0) dp[r] = acc;
}

// dq[n] = sum over column n of dla[e] (the transposed plan's row n)
template <int TEAM>
__global__ __launch_bounds__(256) void gate_bwd_cols_kernel(const int32_t *__restrict__ rowptr_t, const int32_t *__restrict__ perm_t,
                                                            const int n_cols, const int32_t *__restrict__ long_rows_t,
                                                            const float *__restrict__ dla, float *__restrict__ dq) {
    __shared__ float lds[4];
    int r, k0, k1, lane;
    if (!gate_team_row<TEAM>(rowptr_t, n_cols, long_rows_t, r, k0, k1, lane)) return;
    float acc = 0.f;
    for (int k = k0 + lane; k < k1; k += TEAM) acc += dla[perm_t[k]];
    acc = gate_team_sum<TEAM>(acc, lds);
    if (lane == 0) dq[r] = acc;
}

inline unsigned gate_blocks(long long threads) { return (unsigned)((threads + 255) / 256); }

inline bool gate_args_ok(float gamma, float zeta, float beta) { return gamma < 0.f && zeta > 0.f && beta > 0.f; }

inline GateArgs gate_args(float gamma, float zeta, float beta, float eps) {
    GateArgs a;
    a.gamma = gamma; a.zeta = zeta; a.beta = beta; a.eps = eps;
    a.l0_shift = beta * logf(-gamma / zeta);
    return a;
}

}      // namespace

extern "C" {

int sslrec_edge_gate_fwd_f32(const int32_t *rowptr, const int32_t *col, const int32_t *perm, const int32_t *row_of_entry, int32_t n, int32_t nnz,
                             const int32_t *long_rows, int32_t n_long, const float *p, const float *q, const float *bias, const float *noise,
                             float gamma, float zeta, float beta, float eps, float *m, float *s, float *dinv, float *vals, float *l0,
                             float *l0_row, void *stream) {
    if (!rowptr || !col || !perm || !row_of_entry || !p || !q || !bias || !m || !s || !dinv || !vals || !l0 || !l0_row || n <= 0 || nnz <= 0 ||
        n_long < 0 || (n_long > 0 && !long_rows) || !gate_args_ok(gamma, zeta, beta) || !(eps >= 0.f))
        return SSLREC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (n_long == 0) long_rows = nullptr;
    const GateArgs a = gate_args(gamma, zeta, beta, eps);
    hipLaunchKernelGGL(gate_fwd_rows_kernel<16>, dim3(gate_blocks((long long)n * 16)), dim3(256), 0, st, rowptr, col, perm, (int)n, long_rows, p,
                       q, bias, noise, a, m, s, dinv, l0_row);
    if (n_long > 0)
        hipLaunchKernelGGL(gate_fwd_rows_kernel<256>, dim3((unsigned)n_long), dim3(256), 0, st, rowptr, col, perm, (int)n, long_rows, p, q, bias,
                           noise, a, m, s, dinv, l0_row);
    hipLaunchKernelGGL(gate_fwd_vals_kernel, dim3(gate_blocks(nnz)), dim3(256), 0, st, row_of_entry, col, perm, (int)nnz, m, dinv, vals);
    hipLaunchKernelGGL(gate_reduce_kernel, dim3(1), dim3(256), 0, st, l0_row, (int)n, 1.f / (float)nnz, l0);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

int sslrec_edge_gate_bwd_f32(const int32_t *rowptr, const int32_t *col, const int32_t *perm, const int32_t *long_rows, int32_t n_long,
                             const int32_t *rowptr_t, const int32_t *col_t, const int32_t *perm_t, const int32_t *long_rows_t, int32_t n_long_t,
                             int32_t n, int32_t nnz, const float *p, const float *q, const float *bias, const float *noise, float gamma,
                             float zeta, float beta, float eps, const float *m, const float *s, const float *dinv, const float *dvals,
                             const float *dl0, float *dp, float *dq, float *dbias, float *dla_ws, float *n_ws, void *stream) {
    if (!rowptr || !col || !perm || !rowptr_t || !col_t || !perm_t || !p || !q || !bias || !m || !s || !dinv || !dvals || !dl0 || !dp || !dq ||
        !dbias || !dla_ws || !n_ws || n <= 0 || nnz <= 0 || n_long < 0 || n_long_t < 0 || (n_long > 0 && !long_rows) ||
        (n_long_t > 0 && !long_rows_t) || !gate_args_ok(gamma, zeta, beta) || !(eps >= 0.f))
        return SSLREC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (n_long == 0) long_rows = nullptr;
    if (n_long_t == 0) long_rows_t = nullptr;
    const GateArgs a = gate_args(gamma, zeta, beta, eps);
    float *a_row = n_ws, *ds = n_ws + n;                       // n_ws: 2 n floats
    const dim3 rows16(gate_blocks((long long)n * 16)), tb(256);
    hipLaunchKernelGGL(gate_bwd_rowdot_kernel<16>, rows16, tb, 0, st, rowptr, col, perm, (int)n, long_rows, dvals, m, dinv, a_row);
    if (n_long > 0)
        hipLaunchKernelGGL(gate_bwd_rowdot_kernel<256>, dim3((unsigned)n_long), tb, 0, st, rowptr, col, perm, (int)n, long_rows, dvals, m, dinv,
                           a_row);
    hipLaunchKernelGGL(gate_bwd_coldot_kernel<16>, rows16, tb, 0, st, rowptr_t, col_t, perm_t, (int)n, long_rows_t, dvals, m, dinv, s, a_row, ds);
    if (n_long_t > 0)
        hipLaunchKernelGGL(gate_bwd_coldot_kernel<256>, dim3((unsigned)n_long_t), tb, 0, st, rowptr_t, col_t, perm_t, (int)n, long_rows_t, dvals,
                           m, dinv, s, a_row, ds);
    const float inv_nnz = 1.f / (float)nnz;
    hipLaunchKernelGGL(gate_bwd_rows_kernel<16>, rows16, tb, 0, st, rowptr, col, perm, (int)n, long_rows, p, q, bias, noise, a, dvals, dl0, inv_nnz,
                       dinv, ds, dla_ws, dp);
    if (n_long > 0)
        hipLaunchKernelGGL(gate_bwd_rows_kernel<256>, dim3((unsigned)n_long), tb, 0, st, rowptr, col, perm, (int)n, long_rows, p, q, bias, noise, a,
                           dvals, dl0, inv_nnz, dinv, ds, dla_ws, dp);
    hipLaunchKernelGGL(gate_bwd_cols_kernel<16>, rows16, tb, 0, st, rowptr_t, perm_t, (int)n, long_rows_t, dla_ws, dq);
    if (n_long_t > 0)
        hipLaunchKernelGGL(gate_bwd_cols_kernel<256>, dim3((unsigned)n_long_t), tb, 0, st, rowptr_t, perm_t, (int)n, long_rows_t, dla_ws, dq);
    hipLaunchKernelGGL(gate_reduce_kernel, dim3(1), dim3(256), 0, st, dp, (int)n, 1.f, dbias);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

}      // extern "C"
