// VGAE edge decoder of AdaGCL over ALL entries of a sparse pattern (reference models/general_cf/adagcl.py:221-237, vgae_generate):
//   logit[e] = w2 . relu(W1 relu(x[row(e)] (.) x[col(e)]) + b1) + b2,    keep[e] = logit[e] >= 0,
// and the values of the generated view, vals[e] * keep[e] / (kept / nnz).  Forward only: the reference calls it under no_grad.
//
// Layout (rowtile.h): an ENTRY is a row of the transposed 32x32x2 fp32 MFMA tile.  A wave takes 32 consecutive CSR positions; lane
// (l32, half) gathers its half of the two table rows of entry l32, multiplies them and applies the first ReLU in registers.  W1^T
// stays in LDS for the workgroup's lifetime, and the hidden units k = 32 kb + (reg & 3) + 8 (reg >> 2) + 4 half of an entry land in
// the registers of its lane: bias, ReLU and the dot with w2 are arithmetic inside a lane plus ONE exchange with lane ^ 32.  Nothing
// of size nnz x d is written.  The kept count is an integer: per-workgroup counts, summed by the finishing launch.
#include "rowtile.h"

namespace {

constexpr int EM_CAP = SSLREC_EDGE_MLP_SLOTS;      // workgroups of the decoder launch = entries of the count workspace

template <int D>
__global__ __launch_bounds__(256, D <= 64 ? 2 : 1) void edge_mlp_kernel(const int32_t *__restrict__ row_of_entry, const int32_t *__restrict__ col,
                                                                         const int32_t *__restrict__ perm, const int nnz,
                                                                         const float *__restrict__ X, const float *__restrict__ W1,
                                                                         const float *__restrict__ b1, const float *__restrict__ w2,
                                                                         const float *__restrict__ b2, float *__restrict__ logit,
                                                                         uint8_t *__restrict__ keep, int32_t *__restrict__ counts) {
    constexpr int KB = D / 32, KS = KB * 32 + 1;
    extern __shared__ float em_lds[];
    __shared__ int em_count[IN_WAVES];
    // W1 is [out, in] row-major (nn.Linear); the tile wants C[i, k] = W1[k, i] at em_lds[i * KS + k]
    for (int e = threadIdx.x; e < D * D; e += IN_WAVES * 64) {
        const int k = e / D, i = e - k * D;
        em_lds[i * KS + k] = W1[e];
    }
    for (int i = threadIdx.x; i < D; i += IN_WAVES * 64) em_lds[i * KS + D] = 0.f;      // (the pad column, never read by the products)
    constexpr bool IN_REGS = D <= 64;                           // b1 and w2 of this lane's hidden units: registers, at d = 128 LDS
    float *em_b1 = em_lds + D * KS, *em_w2 = em_b1 + D;
    if constexpr (!IN_REGS)
        for (int i = threadIdx.x; i < D; i += IN_WAVES * 64) {
            em_b1[i] = b1[i];
            em_w2[i] = w2[i];
        }
    __syncthreads();
    const int lane = threadIdx.x & 63, l32 = lane & 31, half = lane >> 5, wave = wave_in_block();
    const float bias2 = b2[0];
    float hb[IN_REGS ? KB : 1][16], hw[IN_REGS ? KB : 1][16];
    if constexpr (IN_REGS) {
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                hb[kb][r] = b1[k];
                hw[kb][r] = w2[k];
            }
    }
    const int tiles = (int)(((long long)nnz + 31) / 32);
    int kept = 0;
    for (int t = blockIdx.x * IN_WAVES + wave; t < tiles; t += gridDim.x * IN_WAVES) {
        const long long k = (long long)t * 32 + l32;
        const bool valid = k < nnz;
        int r = 0, c = 0;
        if (valid) {
            r = row_of_entry[k];
            c = col[k];
        }
        float v[D / 2];
        {
            const in_f32x4 *pr = reinterpret_cast<const in_f32x4 *>(X + (size_t)r * D + half * (D / 2));
            const in_f32x4 *pc = reinterpret_cast<const in_f32x4 *>(X + (size_t)c * D + half * (D / 2));
#pragma unroll
            for (int j = 0; j < D / 8; ++j) {
                in_f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
                if (valid) {
                    a = pr[j];
                    b = pc[j];
                }
                v[4 * j] = fmaxf(a.x * b.x, 0.f); v[4 * j + 1] = fmaxf(a.y * b.y, 0.f);
                v[4 * j + 2] = fmaxf(a.z * b.z, 0.f); v[4 * j + 3] = fmaxf(a.w * b.w, 0.f);
            }
        }
        in_f32x16 acc[KB];
        in_logits<D, KB>(em_lds, v, l32, half, acc);
        float part = 0.f;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if constexpr (IN_REGS) {
                    part = fmaf(fmaxf(acc[kb][q] + hb[kb][q], 0.f), hw[kb][q], part);
                } else {
                    const int k = kb * 32 + (q & 3) + 8 * (q >> 2) + 4 * half;
                    part = fmaf(fmaxf(acc[kb][q] + em_b1[k], 0.f), em_w2[k], part);
                }
            }
        const float lg = (part + __shfl_xor(part, 32, 64)) + bias2;
        const bool kp = lg >= 0.f;
        if (valid && half == 0) {
            const int e = perm[k];
            logit[e] = lg;
            keep[e] = kp ? 1 : 0;
        }
        kept += __popcll(__ballot(valid && half == 0 && kp));
    }
    if (lane == 0) em_count[wave] = kept;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = ((em_count[0] + em_count[1]) + em_count[2]) + em_count[3];
}

// kept = sum of the counts (every workgroup adds them up for itself: at most EM_CAP integers); out[e] = vals[e] * keep[e] / (kept / nnz)
// with the reference's arithmetic (:234: the quotient is a Python float, the division an fp32 one).  kept == 0: every value is 0.
__global__ __launch_bounds__(256) void edge_keep_finish_kernel(const float *__restrict__ vals, const uint8_t *__restrict__ keep,
                                                               const int32_t *__restrict__ counts, const int n_counts, const int nnz,
                                                               float *__restrict__ out, int32_t *__restrict__ kept_out) {
    __shared__ int part[256];
    int s = 0;
    for (int i = threadIdx.x; i < n_counts; i += 256) s += counts[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    const int kept = part[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) kept_out[0] = kept;
    const float share = (float)((double)kept / (double)nnz);
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (long long)gridDim.x * 256)
        out[e] = (kept > 0 && keep[e]) ? vals[e] / share : 0.f;
}

// keep flags and one count per workgroup from given logits (the composed path of an embedding size without a decoder kernel)
__global__ __launch_bounds__(256) void edge_keep_flags_kernel(const float *__restrict__ logit, const int nnz, uint8_t *__restrict__ keep,
                                                              int32_t *__restrict__ counts) {
    __shared__ int part[4];
    int kept = 0;
    for (long long e0 = (long long)blockIdx.x * 256; e0 < nnz; e0 += (long long)gridDim.x * 256) {
        const long long e = e0 + threadIdx.x;
        const bool kp = e < nnz && logit[e] >= 0.f;
        if (e < nnz) keep[e] = kp ? 1 : 0;
        kept += __popcll(__ballot(kp));
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = kept;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

inline int em_groups(long long nnz) {
    const long long g = (nnz + 32 * IN_WAVES - 1) / (32 * IN_WAVES);
    return (int)(g < EM_CAP ? (g > 0 ? g : 1) : EM_CAP);
}

}      // namespace

extern "C" {

int sslrec_edge_mlp_fwd_f32(const int32_t *row_of_entry, const int32_t *col, const int32_t *perm, int32_t n_rows, int32_t n_cols, int32_t nnz,
                            const float *X, int32_t d, const float *W1, const float *b1, const float *w2, const float *b2, float *logit,
                            uint8_t *keep, int32_t *counts, int32_t *n_counts, void *stream) {
    if (!row_of_entry || !col || !perm || !X || !W1 || !b1 || !w2 || !b2 || !logit || !keep || !counts || !n_counts || n_rows < 0 ||
        n_cols < 0 || nnz < 0 || (d != 32 && d != 64 && d != 128))
        return SSLREC_E_BADARG;
    *n_counts = 0;
    if (nnz == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int G = em_groups(nnz);
    *n_counts = G;
#define CALL(D)                                                                                                                            \
    {                                                                                                                                      \
        const size_t lds = ((size_t)D * (D + 1) + 2 * D) * 4;                                                                              \
        if (lds > 65536) {                                                                                                                 \
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(edge_mlp_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                               (int)lds);                                                                                  \
            if (e != hipSuccess) return (int)e;                                                                                            \
        }                                                                                                                                  \
        hipLaunchKernelGGL(edge_mlp_kernel<D>, dim3((unsigned)G), dim3(IN_WAVES * 64), lds, st, row_of_entry, col, perm, (int)nnz, X, W1, b1, \
                           w2, b2, logit, keep, counts);                                                                                   \
    }
    if (d == 32) CALL(32) else if (d == 64) CALL(64) else CALL(128)
#undef CALL
    SSLREC_LAUNCH_CHECK();
    return 0;
}

int sslrec_edge_keep_flags(const float *logit, int32_t nnz, uint8_t *keep, int32_t *counts, int32_t *n_counts, void *stream) {
    if (!logit || !keep || !counts || !n_counts || nnz < 0) return SSLREC_E_BADARG;
    *n_counts = 0;
    if (nnz == 0) return 0;
    const long long g = ((long long)nnz + 255) / 256;
    const int G = (int)(g < EM_CAP ? g : EM_CAP);
    *n_counts = G;
    hipLaunchKernelGGL(edge_keep_flags_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, logit, (int)nnz, keep, counts);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

int sslrec_edge_keep_finish_f32(const float *vals, const uint8_t *keep, const int32_t *counts, int32_t n_counts, int32_t nnz, float *out,
                                int32_t *kept, void *stream) {
    if (!vals || !keep || !counts || !out || !kept || nnz <= 0 || n_counts < 1 || n_counts > EM_CAP) return SSLREC_E_BADARG;
    const long long g = ((long long)nnz + 255) / 256;
    hipLaunchKernelGGL(edge_keep_finish_kernel, dim3((unsigned)(g < 2048 ? g : 2048)), dim3(256), 0, (hipStream_t)stream, vals, keep, counts,
                       (int)n_counts, (int)nnz, out, kept);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

}      // extern "C"
