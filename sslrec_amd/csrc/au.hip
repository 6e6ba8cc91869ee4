// Alignment + uniformity loss of DirectAU (reference models/loss_utils.py:75-86, call site models/general_cf/directau.py:42-47) on the
// stacked table T [N, d] = [users; items]:
//   x^_b = normalize(scale T[anc_b]),  y^_b = normalize(scale T[n_user + pos_b])            normalize(v) = v / max(|v|, 1e-12)
//   align   = mean_b |x^_b - y^_b|^2
//   uni(z)  = log( sum_{i != j} exp(-2 |z_i - z_j|^2) / (B (B - 1)) )
//   uniform = gamma (uni(x^) + uni(y^)) / 2,   loss = align + uniform
// forward and backward without anything of size B x B or B (B - 1) / 2 in global memory, without float atomics: two runs give the same
// bits.  A pair is left out when its two batch POSITIONS are equal, never by value: two positions that hold the same table row are a
// pair like any other (term exp(0) = 1).
//
// Both passes use the DIFFERENCE form on the VALU, not the Gram form on the matrix cores.  d^2 = sum_k (z_ik - z_jk)^2 has no
// cancellation where the Gram form n_i + n_j - 2 <z_i, z_j> loses every digit for the near-equal rows a batch is full of (a user
// occurs several times), and the backward's sum_j e_ij (z_i - z_j) is formed term by term instead of as z_i r_i - sum_j e_ij z_j,
// whose two halves are each ~B times the result.  The price is 3 d (forward) / 5 d (backward) lane operations per pair, a third of
// them fp64 (below), instead of d / 32 MFMA cycles: 0.19 ms forward, 0.48 ms forward + backward at B = 4096, d = 32.
//
// Layout.  A workgroup of 4 waves owns 64 rows i of one side, one per LANE: z_i lives in d registers, the row sum r_i (forward) or
// the d sums of e_ij (z_i - z_j) (backward) in the lane's accumulators -- nothing crosses lanes in the sweep.  The B columns j are
// cut into 4 S parts of `cp` columns: workgroup (rowtile, split) takes parts 4 split .. 4 split + 3, one per wave.  A wave stages
// 2048 / d rows z_j at a time in its own LDS tile (a contiguous piece of Z: coalesced float4 loads) and every lane reads the same z_j
// from it (LDS broadcast, no bank conflict).  The 4 waves' sums are added in wave order in LDS, the workgroup's sums go to slab
// `split` of the workspace, and the finishing kernels add the S slabs in index order.  S = au_splits(B) depends on B alone.
//
//   forward   1. au_prep_kernel     gather, scale, normalise -> Z [2 B, d], |v| [2 B], |x^_b - y^_b|^2 [B]
//             2. au_sweep_kernel<0> row sums of e_ij per split
//             3. au_fwd_finish      S_x, S_y, align -> out[0..4] = loss, align, uniform, S_x, S_y
//   backward  1. au_sweep_kernel<1> sum_j e_ij (z_i - z_j) per split (e_ij recomputed); also clears the scatter table
//             2. au_bwd_finish      (-8 / S) gamma / 2 g_uniform * sum  +  2 g_align (x^ - y^) / B, back through the normalisation and
//                                   `scale`, staged as rows G [2 B, d] and registered for the deterministic scatter
//             3. det_reduce_kernel  dT[row] += the rows of G that share the destination, in ascending batch position (det_scatter.h)
// The backward reads Z, |v| (workspace) and S_x, S_y (out) as the forward left them.
#include <cmath>
#include "common.h"
#include "det_scatter.h"

namespace {

constexpr int AU_WAVES = 4;
constexpr int AU_TILE_FLOATS = 2048;                         // a wave's column tile: 2048 / d rows of Z
constexpr int AU_LDS_FLOATS = 64 * 129 + 3;                  // >= 4 tiles, >= the 64 x (d + 1) reduction tile at d = 128
constexpr int AU_MAX_SPLIT = 8;
constexpr int AU_MAX_B = DET_MAX / 2;                        // 2 B contributions must fit the scatter table
constexpr float AU_EPS = 1e-12f;

__device__ __forceinline__ void au_wave_sync() {             // LDS traffic between the lanes of ONE wave
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ double au_wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

inline bool au_dim_ok(int d) { return d == 32 || d == 64 || d == 128; }

// column splits: enough workgroups (row tiles x splits x 2 sides) for the 256 CUs, a function of B alone
inline int au_splits(int B) {
    const int tiles = (B + 63) / 64;
    int s = 256 / (2 * tiles);
    return s < 1 ? 1 : (s > AU_MAX_SPLIT ? AU_MAX_SPLIT : s);
}

struct AuWs {
    float *Z, *nrm, *gpart, *G;
    double *apart, *rpart;                                   // the forward's scalars are summed in double (see au_prep_kernel)
    void *det;
    size_t floats;                                           // before the scatter table
};

inline size_t au_al(size_t n) { return (n + 3) & ~(size_t)3; }

inline AuWs au_ws(void *ws, int B, int d) {
    const size_t S = (size_t)au_splits(B), B2 = 2 * (size_t)B;
    AuWs w;
    float *p = (float *)(((uintptr_t)ws + 15) & ~(uintptr_t)15);
    float *p0 = p;
    w.Z = p; p += au_al(B2 * d);
    w.nrm = p; p += au_al(B2);
    w.apart = (double *)p; p += au_al(2 * (size_t)B);
    w.rpart = (double *)p; p += au_al(2 * S * B2);
    w.gpart = p; p += au_al(S * B2 * d);
    w.G = p; p += au_al(B2 * d);
    w.det = p;
    w.floats = (size_t)(p - p0);
    return w;
}

// one wave per batch position b: both gathered rows, scaled and normalised, and |x^_b - y^_b|^2.  An index outside its table part
// contributes a zero row and is marked (norm -1): it gets no gradient instead of a fault.
// Precision of the forward's scalars.  align ~ 2 and uniform ~ -gamma 3.5 nearly cancel in the loss at small gamma (0.2 at gamma =
// 0.5), so a loss correct to fp32 rounding needs both terms well below it: the norms, the alignment terms and (au_sweep_kernel) the
// squared distances and the row sums are accumulated in double -- a few operations per row here, one conversion and one fp64 FMA per
// element in the sweep -- and only the stored Z and the exponentials are fp32.  The backward needs no such care (no cancellation).
template <int D>
__global__ __launch_bounds__(256) void au_prep_kernel(const float *__restrict__ T, long long N, long long n_user,
                                                      const int64_t *__restrict__ ancs, const int64_t *__restrict__ poss, int B, float scale,
                                                      float *__restrict__ Z, float *__restrict__ nrm, double *__restrict__ apart) {
    constexpr int Q = (D + 63) / 64;
    const int lane = threadIdx.x & 63;
    for (int b = blockIdx.x * AU_WAVES + wave_in_block(); b < B; b += gridDim.x * AU_WAVES) {
        double z[2][Q];
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const long long idx = side == 0 ? (long long)ancs[b] : (long long)poss[b];
            const long long lim = side == 0 ? n_user : N - n_user;
            const bool ok = idx >= 0 && idx < lim;
            const float *src = T + (size_t)((side == 0 ? 0 : n_user) + (ok ? idx : 0)) * D;
            double ss = 0.0;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int k = lane + 64 * q;
                const float v = (ok && k < D) ? scale * src[k] : 0.f;
                z[side][q] = (double)v;
                ss += (double)v * (double)v;
            }
            const double n = sqrt(au_wave_sum_d(ss));
            const double den = fmax(n, (double)AU_EPS);
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int k = lane + 64 * q;
                z[side][q] = z[side][q] / den;
                if (k < D) Z[((size_t)side * B + b) * D + k] = (float)z[side][q];
            }
            if (lane == 0) nrm[(size_t)side * B + b] = ok ? (float)n : -1.f;
        }
        double a = 0.0;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const double df = z[0][q] - z[1][q];
            a += df * df;
        }
        a = au_wave_sum_d(a);
        if (lane == 0) apart[b] = a;
    }
}

// BWD = false: part[side][split][i] = sum over the workgroup's columns j != i of e_ij
// BWD = true:  part[side][split][i][:] = sum over the same columns of e_ij (z_i - z_j)          e_ij = exp(-2 |z_i - z_j|^2)
template <int D, bool BWD>
__global__ __launch_bounds__(256) void au_sweep_kernel(const float *__restrict__ Z, int B, int S, int cp, int terms, void *__restrict__ part,
                                                       DetTable tab) {
    __shared__ float4 lds4[(AU_LDS_FLOATS + 3) / 4];
    float *lds = reinterpret_cast<float *>(lds4);
    if constexpr (BWD) {
        const int n_threads = gridDim.x * gridDim.y * gridDim.z * 256;
        const int tid = ((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        det_clear_from(tab, tid, n_threads);
    }
    const int side = blockIdx.z;
    if (!(terms & (2 << side))) return;                          // (the whole workgroup: this side has no uniformity term)
    const int lane = threadIdx.x & 63, wave = wave_in_block();
    const int i = blockIdx.x * 64 + lane;
    const bool valid = i < B;
    const float *Zs = Z + (size_t)side * B * D;
    float zi[D];
    {
        const float4 *p = reinterpret_cast<const float4 *>(Zs + (size_t)(valid ? i : 0) * D);
#pragma unroll
        for (int q = 0; q < D / 4; ++q) {
            const float4 v = p[q];
            zi[4 * q] = v.x; zi[4 * q + 1] = v.y; zi[4 * q + 2] = v.z; zi[4 * q + 3] = v.w;
        }
    }
    constexpr int TC = AU_TILE_FLOATS / D;
    const int part_id = blockIdx.y * AU_WAVES + wave;
    const int jbeg = min(part_id * cp, B), jend = min(jbeg + cp, B);
    float *tile = lds + wave * AU_TILE_FLOATS;
    double r = 0.0;
    float acc[BWD ? D : 1];
#pragma unroll
    for (int k = 0; k < (BWD ? D : 1); ++k) acc[k] = 0.f;
    for (int j0 = jbeg; j0 < jend; j0 += TC) {
        const int nc = min(TC, jend - j0);
        au_wave_sync();                                          // (the previous tile's readers are done)
        {
            const float4 *src = reinterpret_cast<const float4 *>(Zs + (size_t)j0 * D);
            float4 *dst = reinterpret_cast<float4 *>(tile);
#pragma unroll
            for (int q = 0; q < AU_TILE_FLOATS / 256; ++q) {
                const int e4 = q * 64 + lane;
                if (e4 * 4 < nc * D) dst[e4] = src[e4];
            }
        }
        au_wave_sync();
        for (int jj = 0; jj < nc; ++jj) {
            const float4 *t = reinterpret_cast<const float4 *>(tile + jj * D);
            // the squared distance in double (see au_prep_kernel).  The backward needs it too: an fp32 sum of d squares is off by up to
            // ~sqrt(d) 2^-24 relative, times 2 d^2 ~ 4 in the exponent: 1e-6 in e_ij, which at B = 2 is the gradient's own error
            double d2 = 0.0;
#pragma unroll
            for (int q = 0; q < D / 4; ++q) {
                const float4 c = t[q];
                const double a0 = (double)(zi[4 * q] - c.x), a1 = (double)(zi[4 * q + 1] - c.y);
                const double a2 = (double)(zi[4 * q + 2] - c.z), a3 = (double)(zi[4 * q + 3] - c.w);
                d2 = fma(a0, a0, d2); d2 = fma(a1, a1, d2); d2 = fma(a2, a2, d2); d2 = fma(a3, a3, d2);
            }
            const double x = -2.0 * d2;                          // exp(hi + lo) = exp(hi) (1 + lo), |lo| <= 2^-24 |hi|
            const float hi = (float)x, lo = (float)(x - (double)hi);
            float e = expf(hi);
            e = fmaf(e, lo, e);
            e = (j0 + jj == i) ? 0.f : e;                        // the pair of a position with itself, by index
            if constexpr (BWD) {
#pragma unroll
                for (int q = 0; q < D / 4; ++q) {
                    const float4 c = t[q];
                    acc[4 * q] = fmaf(e, zi[4 * q] - c.x, acc[4 * q]);
                    acc[4 * q + 1] = fmaf(e, zi[4 * q + 1] - c.y, acc[4 * q + 1]);
                    acc[4 * q + 2] = fmaf(e, zi[4 * q + 2] - c.z, acc[4 * q + 2]);
                    acc[4 * q + 3] = fmaf(e, zi[4 * q + 3] - c.w, acc[4 * q + 3]);
                }
            } else {
                r += (double)e;
            }
        }
    }
    // the 4 waves' sums in wave order, then this workgroup's rows of slab `split`
    const size_t slab = (size_t)side * S + blockIdx.y;
    if constexpr (BWD) {
        constexpr int RS = D + 1;
        for (int w = 0; w < AU_WAVES; ++w) {
            __syncthreads();                                     // (first round: every wave is done with its tile)
            if (wave == w) {
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const int at = lane * RS + k;
                    lds[at] = (w == 0) ? acc[k] : lds[at] + acc[k];
                }
            }
        }
        __syncthreads();
        const int row0 = blockIdx.x * 64;
        const int n_rows = min(64, B - row0);
        float *dst = static_cast<float *>(part) + (slab * B + row0) * D;
        for (int e = threadIdx.x; e < n_rows * D; e += 256) dst[e] = lds[(e / D) * RS + (e % D)];
    } else {
        double *ldsd = reinterpret_cast<double *>(lds4);
        __syncthreads();
        ldsd[wave * 64 + lane] = r;
        __syncthreads();
        if (wave == 0 && valid)
            static_cast<double *>(part)[slab * B + i] = ((ldsd[lane] + ldsd[64 + lane]) + ldsd[128 + lane]) + ldsd[192 + lane];
    }
}

// one workgroup: S_side = sum_i sum_split rpart, align = sum_b apart / B; a thread adds its rows in index order, the 256 threads'
// sums are added as a fixed tree
__global__ __launch_bounds__(256) void au_fwd_finish_kernel(const double *__restrict__ rpart, const double *__restrict__ apart, int B, int S,
                                                            int terms, float gamma, float *__restrict__ out) {
    __shared__ double red[3][256];
    const int tid = threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < B; i += 256) {
        if (terms & 1) s[0] += apart[i];
#pragma unroll
        for (int side = 0; side < 2; ++side)
            if (terms & (2 << side)) {
                double v = 0.0;
                for (int sp = 0; sp < S; ++sp) v += rpart[((size_t)side * S + sp) * B + i];
                s[1 + side] += v;
            }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) red[q][tid] = s[q];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int q = 0; q < 3; ++q) red[q][tid] += red[q][tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double pairs = (double)B * (double)(B - 1);
        const double align = (terms & 1) ? red[0][0] / (double)B : 0.0;
        const double ux = (terms & 2) ? log(red[1][0] / pairs) : 0.0;
        const double uy = (terms & 4) ? log(red[2][0] / pairs) : 0.0;
        const double uniform = (double)gamma * (ux + uy) * 0.5;
        out[0] = (float)(align + uniform);                       // (rounded once: the two terms nearly cancel at small gamma)
        out[1] = (float)align;
        out[2] = (float)uniform;
        out[3] = (float)red[1][0];
        out[4] = (float)red[2][0];
    }
}

// one wave per gathered row e (e < B: x^_e, else y^_{e - B}): the row's gradient, back through the normalisation and `scale`, staged
// in G and registered for the scatter
template <int D>
__global__ __launch_bounds__(256) void au_bwd_finish_kernel(const float *__restrict__ Z, const float *__restrict__ nrm,
                                                            const float *__restrict__ gpart, int B, int S, int terms, float scale, float gamma,
                                                            const float *__restrict__ out, const float *__restrict__ g_align,
                                                            const float *__restrict__ g_uniform, long long n_user,
                                                            const int64_t *__restrict__ ancs, const int64_t *__restrict__ poss,
                                                            float *__restrict__ dT, float *__restrict__ G, DetTable tab) {
    constexpr int Q = (D + 63) / 64;
    const int lane = threadIdx.x & 63;
    const float ga = (terms & 1) ? g_align[0] * 2.f / (float)B : 0.f;
    const float gu = g_uniform[0] * gamma * 0.5f;
    for (int e = blockIdx.x * AU_WAVES + wave_in_block(); e < 2 * B; e += gridDim.x * AU_WAVES) {
        const int side = e < B ? 0 : 1, b = e - side * B;
        const bool uni = (terms & (2 << side)) != 0;
        // d uni / d z_i = sum_j d e_ij / d z_i / (S / 2) with S the sum over the FULL square (every pair twice): -8 / S
        const float cu = uni ? gu * (-8.f / out[3 + side]) : 0.f;
        const float n = nrm[e];
        float z[Q], g[Q];
        double dot = 0.0;                                        // <z, g> z is of g's size: the projection cancels, keep it exact
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int k = lane + 64 * q;
            z[q] = g[q] = 0.f;
            if (k < D) {
                z[q] = Z[(size_t)e * D + k];
                float sum = 0.f;
                if (uni)
                    for (int sp = 0; sp < S; ++sp) sum += gpart[(((size_t)side * S + sp) * B + b) * D + k];
                const float other = Z[((size_t)(1 - side) * B + b) * D + k];
                g[q] = cu * sum + ga * (z[q] - other);          // d align / d x^ = 2 (x^ - y^) / B, d align / d y^ = 2 (y^ - x^) / B
                dot += (double)z[q] * (double)g[q];
            }
        }
        dot = au_wave_sum_d(dot);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int k = lane + 64 * q;
            if (k < D) {
                float gv = (n > AU_EPS) ? (float)(((double)g[q] - (double)z[q] * dot) / (double)n) : g[q] / AU_EPS;
                if (n < 0.f) gv = 0.f;
                G[(size_t)e * D + k] = gv * scale;
            }
        }
        if (lane == 0) {
            if (n < 0.f) tab.slot_of[e] = -1;                    // an index outside its table part: nowhere to add
            else det_insert(tab, dT + (size_t)((side == 0 ? 0 : n_user) + (side == 0 ? ancs[b] : poss[b])) * D, e);
        }
    }
}

inline bool au_args_ok(int64_t N, int64_t n_user, int d, int64_t B, float scale, float gamma, int terms) {
    if (!au_dim_ok(d) || B < 2 || B > AU_MAX_B || N < 0 || N > 0x7fffffff || n_user < 0 || n_user > N) return false;
    if (!std::isfinite(scale) || !std::isfinite(gamma) || terms < 1 || terms > 7) return false;
    return true;
}

inline int au_grid_rows(int rows) {
    const int g = (rows + AU_WAVES - 1) / AU_WAVES;
    return g > 2048 ? 2048 : g;
}

}      // namespace

extern "C" {

size_t sslrec_au_ws_bytes(int32_t B, int32_t d) {
    if (!au_dim_ok(d) || B < 2 || B > AU_MAX_B) return 0;
    return au_ws(nullptr, B, d).floats * sizeof(float) + det_ws_bytes(2 * B) + 32;
}

int sslrec_au_fwd_f32(const float *T, int32_t N, int32_t n_user, int32_t d, const int64_t *ancs, const int64_t *poss, int32_t B, float scale,
                      float gamma, int32_t terms, float *out, void *ws, void *stream) {
    if (!au_args_ok(N, n_user, d, B, scale, gamma, terms) || !T || !ancs || !poss || !out || !ws) return SSLREC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const AuWs w = au_ws(ws, B, d);
    const int S = au_splits(B), cp = (B + AU_WAVES * S - 1) / (AU_WAVES * S);
    const dim3 sweep((unsigned)((B + 63) / 64), (unsigned)S, 2);
#define CALL(D)                                                                                                                            \
    {                                                                                                                                      \
        hipLaunchKernelGGL((au_prep_kernel<D>), dim3(au_grid_rows(B)), dim3(256), 0, st, T, (long long)N, (long long)n_user, ancs, poss,   \
                           (int)B, scale, w.Z, w.nrm, w.apart);                                                                            \
        if (terms & 6)                                                                                                                     \
            hipLaunchKernelGGL((au_sweep_kernel<D, false>), sweep, dim3(256), 0, st, (const float *)w.Z, (int)B, S, cp, (int)terms,        \
                               w.rpart, DetTable{});                                                                                       \
    }
    switch (d) {
    case 32: CALL(32); break;
    case 64: CALL(64); break;
    default: CALL(128); break;
    }
#undef CALL
    hipLaunchKernelGGL(au_fwd_finish_kernel, dim3(1), dim3(256), 0, st, (const double *)w.rpart, (const double *)w.apart, (int)B, S, (int)terms,
                       gamma, out);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

int sslrec_au_bwd_f32(int32_t N, int32_t n_user, int32_t d, const int64_t *ancs, const int64_t *poss, int32_t B, float scale, float gamma,
                      int32_t terms, const float *out, const float *g_align, const float *g_uniform, float *dT, void *ws, void *stream) {
    if (!au_args_ok(N, n_user, d, B, scale, gamma, terms) || !ancs || !poss || !out || !g_align || !g_uniform || !dT || !ws)
        return SSLREC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const AuWs w = au_ws(ws, B, d);
    const DetTable tab = det_table(w.det);
    const int S = au_splits(B), cp = (B + AU_WAVES * S - 1) / (AU_WAVES * S);
    const dim3 sweep((unsigned)((B + 63) / 64), (unsigned)S, 2);
#define CALL(D)                                                                                                                            \
    {                                                                                                                                      \
        hipLaunchKernelGGL((au_sweep_kernel<D, true>), sweep, dim3(256), 0, st, (const float *)w.Z, (int)B, S, cp, (int)terms, w.gpart,    \
                           tab);                                                                                                           \
        hipLaunchKernelGGL((au_bwd_finish_kernel<D>), dim3(au_grid_rows(2 * B)), dim3(256), 0, st, (const float *)w.Z,                     \
                           (const float *)w.nrm, (const float *)w.gpart, (int)B, S, (int)terms, scale, gamma, out, g_align, g_uniform,     \
                           (long long)n_user, ancs, poss, dT, w.G, tab);                                                                   \
    }
    switch (d) {
    case 32: CALL(32); break;
    case 64: CALL(64); break;
    default: CALL(128); break;
    }
#undef CALL
    SSLREC_LAUNCH_CHECK();
    return det_reduce(tab, 2 * B, w.G, d, st);
}

}      // extern "C"
