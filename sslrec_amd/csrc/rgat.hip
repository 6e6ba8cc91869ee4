// Kernels of KGCL's relation-aware graph attention (reference models/kg/kgcl.py, RGAT.agg :60-72): per edge (h, t, r) a logit, a LeakyReLU,
// a softmax over the edges of one head and the attention-weighted sum of the tail rows, forward and backward.
//
// fc is a Linear(2 d, d), so fc(cat(x[h], x[t])) = P[h] + Q[t] with the NODE tables P = X Wh^T + b and Q = X Wt^T that the caller forms with
// one dense GEMM; the per-edge matvec is gone.  With the kept edges e = (h, t, r):
//     l_e  = <P[h] + Q[t], R[r]>            s_e = l_e > 0 ? l_e : slope l_e
//     a_e  = exp(s_e - M_h) / z_h           M_h = max over the head's kept edges, z_h the sum of the exponentials
//     Y[h] = sum a_e X[t]                   (0 for a head without a kept edge)
// and from G = dY:  delta_h = <G[h], Y[h]>,  ds_e = a_e (<G[h], X[t]> - delta_h),  dl_e = ds_e (s_e > 0 ? 1 : slope),
//     dP[h] = sum dl_e R[r]   (walk by head, which also writes a_e and dl_e by edge id)
//     dX[t] = sum a_e G[h]    dQ[t] = sum dl_e R[r]   (one walk by tail)
//     dR[r] = sum dl_e (P[h] + Q[t])                  (walk by relation)
// Between forward and backward only [E]- and [N]-sized vectors live (s by edge id, M, z) beside Y; no [E, d] tensor exists.
//
// Lists and geometry are those of kgin.hip: graph.RelGraph's three orders as ptr / ia / ib / eid, the keep mask read through eid; a lane
// group of L = d / 4 lanes (one float4 per lane) takes one work item, a destination of at most RG_CHUNK slots or one RG_CHUNK-slot chunk of
// a longer one.  Slots are added in list order.  The forward keeps a running maximum (online softmax); a chunk leaves (m_c, z_c, acc_c)
// and the finishing launch merges a long head's chunks in chunk order, M = max m_c, z = sum z_c e^(m_c - M), acc = sum acc_c e^(m_c - M).
// The backward's chunk sums are added in chunk order.  No float atomics: two calls give the same bits.  R sits in LDS when it fits
// RG_LDS_BYTES.  Index arrays are int32 and validated by the host class that builds them; the kernels do not re-check them.
#include "lanegroup.h"

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_CHUNK = 512;                 // slots per work item (graph.REL_CHUNK, SSLREC_KGIN_CHUNK)
constexpr int RG_FLIGHT = 4;                  // slots a lane group loads before it adds them (in list order)
constexpr int RG_MAX_BLOCKS = 2048;           // workgroups stride over the work items
constexpr int RG_LDS_BYTES = 48 * 1024;       // R is staged in LDS up to this size

inline bool rg_dim_ok(int64_t d) { return d == 32 || d == 64 || d == 128; }
inline bool rg_aligned(const void *p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ float4 z4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 axpy4(const float s, const float4 a, const float4 y) {
    return make_float4(fmaf(s, a.x, y.x), fmaf(s, a.y, y.y), fmaf(s, a.z, y.z), fmaf(s, a.w, y.w));
}
__device__ __forceinline__ float4 scale4(const float s, const float4 a) { return make_float4(s * a.x, s * a.y, s * a.z, s * a.w); }
__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

struct RgList {
    const int32_t *ptr, *ia, *ib, *eid;       // [n_dest + 1], [E], [E], [E]
    const int32_t *chunk_dest, *chunk_begin;  // [n_chunks]
    int n_dest, n_chunks;
};

struct RgLong {
    const int32_t *dest, *ptr;
    int n;
};

// the slots [s0, s1) of work item `item`; false for a long destination's own item (its chunks are items of their own)
__device__ __forceinline__ bool rg_item(const RgList &ls, const long long item, int &dest, int &s0, int &s1) {
    if (item < ls.n_dest) {
        dest = (int)item;
        s0 = ls.ptr[dest];
        s1 = ls.ptr[dest + 1];
        return s1 - s0 <= RG_CHUNK;
    }
    const int c = (int)(item - ls.n_dest);
    dest = ls.chunk_dest[c];
    s0 = ls.chunk_begin[c];
    const int end = ls.ptr[dest + 1];
    s1 = s0 + RG_CHUNK < end ? s0 + RG_CHUNK : end;
    return true;
}

template <int L>
__device__ __forceinline__ void rg_stage(float4 *__restrict__ lds, const float4 *__restrict__ R, const int n_rel) {
    for (int i = threadIdx.x; i < n_rel * L; i += RG_THREADS) lds[i] = R[i];
    __syncthreads();
}

// ---- forward: the list ordered by head, ia = tail, ib = relation ------------------------------------------------------------------------
template <int D, bool RLDS>
__global__ __launch_bounds__(RG_THREADS) void rg_fwd_kernel(const RgList ls, const float4 *__restrict__ X, const float4 *__restrict__ P,
                                                            const float4 *__restrict__ Q, const float4 *__restrict__ R, const int n_rel,
                                                            const float slope, const uint8_t *__restrict__ keep, float *__restrict__ S,
                                                            float *__restrict__ M, float *__restrict__ Z, float4 *__restrict__ Y,
                                                            float4 *__restrict__ part, float *__restrict__ part_mz) {
    constexpr int L = D / 4, RPB = RG_THREADS / L;
    extern __shared__ float4 rg_rs[];
    if constexpr (RLDS) rg_stage<L>(rg_rs, R, n_rel);
    const int lig = threadIdx.x % L, grp = threadIdx.x / L;
    const long long items = (long long)ls.n_dest + ls.n_chunks;
    for (long long item = (long long)blockIdx.x * RPB + grp; item < items; item += (long long)gridDim.x * RPB) {
        int dest, s0, s1;
        if (!rg_item(ls, item, dest, s0, s1)) continue;
        const float4 ph = P[(size_t)dest * L + lig];
        float m = -INFINITY, z = 0.f;
        float4 acc = z4();
        for (int s = s0; s < s1; s += RG_FLIGHT) {
            bool k[RG_FLIGHT];
            int rt[RG_FLIGHT], rr[RG_FLIGHT], id[RG_FLIGHT];
#pragma unroll
            for (int j = 0; j < RG_FLIGHT; ++j) {
                const bool in = s + j < s1;
                id[j] = in ? ls.eid[s + j] : 0;
                rt[j] = in ? ls.ia[s + j] : 0;
                rr[j] = in ? ls.ib[s + j] : 0;
            }
#pragma unroll
            for (int j = 0; j < RG_FLIGHT; ++j) k[j] = s + j < s1 && (keep == nullptr || keep[id[j]] != 0);
            float4 q[RG_FLIGHT], x[RG_FLIGHT], r[RG_FLIGHT];
#pragma unroll
            for (int j = 0; j < RG_FLIGHT; ++j) {
                q[j] = k[j] ? Q[(size_t)rt[j] * L + lig] : z4();
                x[j] = k[j] ? X[(size_t)rt[j] * L + lig] : z4();
                if constexpr (RLDS)
                    r[j] = rg_rs[rr[j] * L + lig];
                else
                    r[j] = k[j] ? R[(size_t)rr[j] * L + lig] : z4();
            }
            float lg[RG_FLIGHT];
#pragma unroll
            for (int j = 0; j < RG_FLIGHT; ++j) lg[j] = group_sum<L>(dot4(add4(ph, q[j]), r[j]));      // (k is the same in the whole group)
#pragma unroll
            for (int j = 0; j < RG_FLIGHT; ++j) {       // slots in list order
                if (k[j]) {
                    const float sj = lg[j] > 0.f ? lg[j] : slope * lg[j];
                    if (lig == 0) S[id[j]] = sj;
                    if (sj > m) {                        // a new maximum: what was summed so far shrinks by e^(m - sj) (0 the first time)
                        const float c = expf(m - sj);
                        z *= c;
                        acc = scale4(c, acc);
                        m = sj;
                    }
                    const float e = expf(sj - m);
                    z += e;
                    acc = axpy4(e, x[j], acc);
                }
            }
        }
        if (item < ls.n_dest) {
            const bool any = z > 0.f;
            Y[(size_t)dest * L + lig] = any ? scale4(1.f / z, acc) : z4();
            if (lig == 0) {
                M[dest] = any ? m : 0.f;
                Z[dest] = z;
            }
        } else {
            const size_t c = (size_t)(item - ls.n_dest);
            part[c * L + lig] = acc;
            if (lig == 0) {
                part_mz[2 * c] = m;
                part_mz[2 * c + 1] = z;
            }
        }
    }
}

// one lane group per long head: its chunks' (m, z, acc) in chunk order
template <int D>
__global__ __launch_bounds__(RG_THREADS) void rg_fwd_finish_kernel(const RgLong lg, const float4 *__restrict__ part,
                                                                   const float *__restrict__ part_mz, float *__restrict__ M,
                                                                   float *__restrict__ Z, float4 *__restrict__ Y) {
    constexpr int L = D / 4, RPB = RG_THREADS / L;
    const int lig = threadIdx.x % L;
    const long long j = (long long)blockIdx.x * RPB + threadIdx.x / L;
    if (j >= lg.n) return;
    const int c0 = lg.ptr[j], c1 = lg.ptr[j + 1], dest = lg.dest[j];
    float m = -INFINITY;
    for (int c = c0; c < c1; ++c)
        if (part_mz[2 * c + 1] > 0.f) m = fmaxf(m, part_mz[2 * c]);
    float z = 0.f;
    float4 acc = z4();
    for (int c = c0; c < c1; ++c) {
        const float zc = part_mz[2 * c + 1];
        if (zc > 0.f) {                                  // (a chunk without a kept edge carries m_c = -inf)
            const float w = expf(part_mz[2 * c] - m);
            z = fmaf(zc, w, z);
            acc = axpy4(w, part[(size_t)c * L + lig], acc);
        }
    }
    const bool any = z > 0.f;
    Y[(size_t)dest * L + lig] = any ? scale4(1.f / z, acc) : z4();
    if (lig == 0) {
        M[dest] = any ? m : 0.f;
        Z[dest] = z;
    }
}

// ---- backward, walk by head: a_e and dl_e by edge id, dP[h] = sum dl_e R[r] -------------------------------------------------------------
template <int D, bool RLDS>
__global__ __launch_bounds__(RG_THREADS) void rg_bwd_head_kernel(const RgList ls, const float4 *__restrict__ X, const float4 *__restrict__ R,
                                                                 const int n_rel, const float slope, const uint8_t *__restrict__ keep,
                                                                 const float4 *__restrict__ G, const float4 *__restrict__ Y,
                                                                 const float *__restrict__ S, const float *__restrict__ M,
                                                                 const float *__restrict__ Z, float *__restrict__ alpha, float *__restrict__ dl,
                                                                 float4 *__restrict__ dP, float4 *__restrict__ part) {
    constexpr int L = D / 4, RPB = RG_THREADS / L;
    extern __shared__ float4 rg_rs[];
    if constexpr (RLDS) rg_stage<L>(rg_rs, R, n_rel);
    const int lig = threadIdx.x % L, grp = threadIdx.x / L;
    const long long items = (long long)ls.n_dest + ls.n_chunks;
    for (long long item = (long long)blockIdx.x * RPB + grp; item < items; item += (long long)gridDim.x * RPB) {
        int dest, s0, s1;
        if (!rg_item(ls, item, dest, s0, s1)) continue;
        const float4 g = G[(size_t)dest * L + lig];
        const float delta = group_sum<L>(dot4(g, Y[(size_t)dest * L + lig]));
        const float mh = M[dest], zh = Z[dest];
        const float inv = zh > 0.f ? 1.f / zh : 0.f;
        float4 acc = z4();
        for (int s = s0; s < s1; s += RG_FLIGHT) {
            bool k[RG_FLIGHT];
            int rt[RG_FLIGHT], rr[RG_FLIGHT], id[RG_FLIGHT];
#pragma unroll
            for (int j = 0; j < RG_FLIGHT; ++j) {
                const bool in = s + j < s1;
                id[j] = in ? ls.eid[s + j] : 0;
                rt[j] = in ? ls.ia[s + j] : 0;
                rr[j] = in ? ls.ib[s + j] : 0;
            }
#pragma unroll
            for (int j = 0; j < RG_FLIGHT; ++j) k[j] = s + j < s1 && (keep == nullptr || keep[id[j]] != 0);
            float4 x[RG_FLIGHT], r[RG_FLIGHT];
            float sv[RG_FLIGHT];
#pragma unroll
            for (int j = 0; j < RG_FLIGHT; ++j) {
                x[j] = k[j] ? X[(size_t)rt[j] * L + lig] : z4();
                sv[j] = k[j] ? S[id[j]] : 0.f;
                if constexpr (RLDS)
                    r[j] = rg_rs[rr[j] * L + lig];
                else
                    r[j] = k[j] ? R[(size_t)rr[j] * L + lig] : z4();
            }
            float gx[RG_FLIGHT];
#pragma unroll
            for (int j = 0; j < RG_FLIGHT; ++j) gx[j] = group_sum<L>(dot4(g, x[j]));
#pragma unroll
            for (int j = 0; j < RG_FLIGHT; ++j) {
                if (k[j]) {
                    const float a = expf(sv[j] - mh) * inv;
                    const float d_l = a * (gx[j] - delta) * (sv[j] > 0.f ? 1.f : slope);
                    if (lig == 0) {
                        alpha[id[j]] = a;
                        dl[id[j]] = d_l;
                    }
                    acc = axpy4(d_l, r[j], acc);
                }
            }
        }
        if (item < ls.n_dest)
            dP[(size_t)dest * L + lig] = acc;
        else
            part[(size_t)(item - ls.n_dest) * L + lig] = acc;
    }
}

// ---- backward, walks by tail and by relation --------------------------------------------------------------------------------------------
// TAIL: ia = head, ib = relation; out1[t] = sum a_e A[head] (A = G), out2[t] = sum dl_e B[rel] (B = R); partials [chunk][2][d]
// !TAIL: ia = head, ib = tail;    out1[r] = sum dl_e (A[head] + B[tail]) (A = P, B = Q);                  partials [chunk][d]
template <int D, bool TAIL, bool BLDS>
__global__ __launch_bounds__(RG_THREADS) void rg_bwd_walk_kernel(const RgList ls, const float4 *__restrict__ A, const float4 *__restrict__ B,
                                                                 const int n_b_rows, const uint8_t *__restrict__ keep,
                                                                 const float *__restrict__ alpha, const float *__restrict__ dl,
                                                                 float4 *__restrict__ out1, float4 *__restrict__ out2, float4 *__restrict__ part) {
    constexpr int L = D / 4, RPB = RG_THREADS / L, W = TAIL ? 2 : 1, FL = 2 * RG_FLIGHT;
    extern __shared__ float4 rg_rs[];
    if constexpr (BLDS) rg_stage<L>(rg_rs, B, n_b_rows);
    const int lig = threadIdx.x % L, grp = threadIdx.x / L;
    const long long items = (long long)ls.n_dest + ls.n_chunks;
    for (long long item = (long long)blockIdx.x * RPB + grp; item < items; item += (long long)gridDim.x * RPB) {
        int dest, s0, s1;
        if (!rg_item(ls, item, dest, s0, s1)) continue;
        float4 acc1 = z4(), acc2 = z4();
        for (int s = s0; s < s1; s += FL) {
            bool k[FL];
            int ra[FL], rb[FL], id[FL];
#pragma unroll
            for (int j = 0; j < FL; ++j) {
                const bool in = s + j < s1;
                id[j] = in ? ls.eid[s + j] : 0;
                ra[j] = in ? ls.ia[s + j] : 0;
                rb[j] = in ? ls.ib[s + j] : 0;
            }
#pragma unroll
            for (int j = 0; j < FL; ++j) k[j] = s + j < s1 && (keep == nullptr || keep[id[j]] != 0);
            float4 a[FL], b[FL];
            float wa[FL], wd[FL];
#pragma unroll
            for (int j = 0; j < FL; ++j) {
                a[j] = k[j] ? A[(size_t)ra[j] * L + lig] : z4();
                if constexpr (BLDS)
                    b[j] = rg_rs[rb[j] * L + lig];
                else
                    b[j] = k[j] ? B[(size_t)rb[j] * L + lig] : z4();
                wd[j] = k[j] ? dl[id[j]] : 0.f;
                if constexpr (TAIL) wa[j] = k[j] ? alpha[id[j]] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < FL; ++j) {               // slots in list order
                if (k[j]) {
                    if constexpr (TAIL) {
                        acc1 = axpy4(wa[j], a[j], acc1);
                        acc2 = axpy4(wd[j], b[j], acc2);
                    } else {
                        acc1 = axpy4(wd[j], add4(a[j], b[j]), acc1);
                    }
                }
            }
        }
        if (item < ls.n_dest) {
            out1[(size_t)dest * L + lig] = acc1;
            if constexpr (TAIL) out2[(size_t)dest * L + lig] = acc2;
        } else {
            const size_t c = (size_t)(item - ls.n_dest);
            part[(c * W) * L + lig] = acc1;
            if constexpr (TAIL) part[(c * W + 1) * L + lig] = acc2;
        }
    }
}

// one lane group per long destination: its W partial rows per chunk, in chunk order
template <int D, int W>
__global__ __launch_bounds__(RG_THREADS) void rg_sum_finish_kernel(const RgLong lg, const float4 *__restrict__ part, float4 *__restrict__ out1,
                                                                   float4 *__restrict__ out2) {
    constexpr int L = D / 4, RPB = RG_THREADS / L;
    const int lig = threadIdx.x % L;
    const long long j = (long long)blockIdx.x * RPB + threadIdx.x / L;
    if (j >= lg.n) return;
    const int c0 = lg.ptr[j], c1 = lg.ptr[j + 1], dest = lg.dest[j];
    float4 acc1 = z4(), acc2 = z4();
    for (int c = c0; c < c1; ++c) {
        acc1 = add4(acc1, part[((size_t)c * W) * L + lig]);
        if constexpr (W == 2) acc2 = add4(acc2, part[((size_t)c * W + 1) * L + lig]);
    }
    out1[(size_t)dest * L + lig] = acc1;
    if constexpr (W == 2) out2[(size_t)dest * L + lig] = acc2;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
template <int D>
inline unsigned rg_blocks(long long items) {
    constexpr int RPB = RG_THREADS / (D / 4);
    const long long b = (items + RPB - 1) / RPB;
    return (unsigned)(b > RG_MAX_BLOCKS ? RG_MAX_BLOCKS : b);
}

template <int D>
inline unsigned rg_finish_blocks(int n_long) {
    constexpr int RPB = RG_THREADS / (D / 4);
    return (unsigned)((n_long + RPB - 1) / RPB);
}

template <int D>
int rg_fwd(const RgList &ls, const RgLong &lg, const float *X, const float *P, const float *Q, const float *R, int n_rel, bool lds, float slope,
           const uint8_t *keep, float *S, float *M, float *Z, float *Y, float *part, float *part_mz, hipStream_t st) {
    const long long items = (long long)ls.n_dest + ls.n_chunks;
    if (items > 0) {
        if (lds)
            hipLaunchKernelGGL((rg_fwd_kernel<D, true>), dim3(rg_blocks<D>(items)), dim3(RG_THREADS), (size_t)n_rel * D * sizeof(float), st, ls,
                               (const float4 *)X, (const float4 *)P, (const float4 *)Q, (const float4 *)R, n_rel, slope, keep, S, M, Z, (float4 *)Y,
                               (float4 *)part, part_mz);
        else
            hipLaunchKernelGGL((rg_fwd_kernel<D, false>), dim3(rg_blocks<D>(items)), dim3(RG_THREADS), 0, st, ls, (const float4 *)X,
                               (const float4 *)P, (const float4 *)Q, (const float4 *)R, n_rel, slope, keep, S, M, Z, (float4 *)Y, (float4 *)part,
                               part_mz);
    }
    if (lg.n > 0)
        hipLaunchKernelGGL((rg_fwd_finish_kernel<D>), dim3(rg_finish_blocks<D>(lg.n)), dim3(RG_THREADS), 0, st, lg, (const float4 *)part,
                           (const float *)part_mz, M, Z, (float4 *)Y);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

template <int D>
int rg_bwd_head(const RgList &ls, const RgLong &lg, const float *X, const float *R, int n_rel, bool lds, float slope, const uint8_t *keep,
                const float *G, const float *Y, const float *S, const float *M, const float *Z, float *alpha, float *dl, float *dP, float *part,
                hipStream_t st) {
    const long long items = (long long)ls.n_dest + ls.n_chunks;
    if (items > 0) {
        if (lds)
            hipLaunchKernelGGL((rg_bwd_head_kernel<D, true>), dim3(rg_blocks<D>(items)), dim3(RG_THREADS), (size_t)n_rel * D * sizeof(float), st, ls,
                               (const float4 *)X, (const float4 *)R, n_rel, slope, keep, (const float4 *)G, (const float4 *)Y, S, M, Z, alpha, dl,
                               (float4 *)dP, (float4 *)part);
        else
            hipLaunchKernelGGL((rg_bwd_head_kernel<D, false>), dim3(rg_blocks<D>(items)), dim3(RG_THREADS), 0, st, ls, (const float4 *)X,
                               (const float4 *)R, n_rel, slope, keep, (const float4 *)G, (const float4 *)Y, S, M, Z, alpha, dl, (float4 *)dP,
                               (float4 *)part);
    }
    if (lg.n > 0)
        hipLaunchKernelGGL((rg_sum_finish_kernel<D, 1>), dim3(rg_finish_blocks<D>(lg.n)), dim3(RG_THREADS), 0, st, lg, (const float4 *)part,
                           (float4 *)dP, (float4 *)nullptr);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

template <int D, bool TAIL>
int rg_bwd_walk(const RgList &ls, const RgLong &lg, const float *A, const float *B, int n_b_rows, bool lds, const uint8_t *keep, const float *alpha,
                const float *dl, float *out1, float *out2, float *part, hipStream_t st) {
    const long long items = (long long)ls.n_dest + ls.n_chunks;
    if (items > 0) {
        if (TAIL && lds)
            hipLaunchKernelGGL((rg_bwd_walk_kernel<D, TAIL, true>), dim3(rg_blocks<D>(items)), dim3(RG_THREADS), (size_t)n_b_rows * D * sizeof(float),
                               st, ls, (const float4 *)A, (const float4 *)B, n_b_rows, keep, alpha, dl, (float4 *)out1, (float4 *)out2,
                               (float4 *)part);
        else
            hipLaunchKernelGGL((rg_bwd_walk_kernel<D, TAIL, false>), dim3(rg_blocks<D>(items)), dim3(RG_THREADS), 0, st, ls, (const float4 *)A,
                               (const float4 *)B, n_b_rows, keep, alpha, dl, (float4 *)out1, (float4 *)out2, (float4 *)part);
    }
    if (lg.n > 0)
        hipLaunchKernelGGL((rg_sum_finish_kernel<D, TAIL ? 2 : 1>), dim3(rg_finish_blocks<D>(lg.n)), dim3(RG_THREADS), 0, st, lg,
                           (const float4 *)part, (float4 *)out1, (float4 *)out2);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

// the checks every entry shares; `part` is needed exactly when the list has chunks
inline bool rg_list_ok(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                       const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest, const int32_t *long_ptr,
                       int32_t n_long, const void *part, int32_t d) {
    if (!ptr || n_dest < 1 || n_slots < 0 || n_slots >= 0x7fffffffLL || n_chunks < 0 || n_long < 0 || !rg_dim_ok(d)) return false;
    if (n_slots > 0 && (!ia || !ib || !eid)) return false;
    if ((n_chunks > 0) != (n_long > 0)) return false;
    if (n_chunks > 0 && (!chunk_dest || !chunk_begin || !long_dest || !long_ptr || !part || !rg_aligned(part))) return false;
    return true;
}

inline bool rg_lds(int32_t n_rows, int32_t d) { return (size_t)n_rows * d * sizeof(float) <= (size_t)RG_LDS_BYTES; }

#define RG_SWITCH(d, CALL32, CALL64, CALL128) \
    switch (d) {                              \
    case 32: return CALL32;                   \
    case 64: return CALL64;                   \
    default: return CALL128;                  \
    }

}      // namespace

extern "C" {

int sslrec_rgat_fwd_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                        const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest, const int32_t *long_ptr,
                        int32_t n_long, const float *X, const float *P, const float *Q, const float *R, int32_t n_rel, int32_t d, float slope,
                        const uint8_t *keep, float *S, float *M, float *Z, float *Y, float *part, float *part_mz, void *stream) {
    if (!rg_list_ok(ptr, ia, ib, eid, n_dest, n_slots, chunk_dest, chunk_begin, n_chunks, long_dest, long_ptr, n_long, part, d))
        return SSLREC_E_BADARG;
    if (!X || !P || !Q || !R || !M || !Z || !Y || n_rel < 1 || !(slope >= 0.f) || (n_slots > 0 && !S) || (n_chunks > 0 && !part_mz))
        return SSLREC_E_BADARG;
    if (!rg_aligned(X) || !rg_aligned(P) || !rg_aligned(Q) || !rg_aligned(R) || !rg_aligned(Y)) return SSLREC_E_BADARG;
    const RgList ls = {ptr, ia, ib, eid, chunk_dest, chunk_begin, n_dest, n_chunks};
    const RgLong lg = {long_dest, long_ptr, n_long};
    const bool lds = rg_lds(n_rel, d);
    hipStream_t st = (hipStream_t)stream;
#define RG_CALL(D) rg_fwd<D>(ls, lg, X, P, Q, R, n_rel, lds, slope, keep, S, M, Z, Y, part, part_mz, st)
    RG_SWITCH(d, RG_CALL(32), RG_CALL(64), RG_CALL(128))
#undef RG_CALL
}

int sslrec_rgat_bwd_head_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                             const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest,
                             const int32_t *long_ptr, int32_t n_long, const float *X, const float *R, int32_t n_rel, int32_t d, float slope,
                             const uint8_t *keep, const float *G, const float *Y, const float *S, const float *M, const float *Z, float *alpha,
                             float *dl, float *dP, float *part, void *stream) {
    if (!rg_list_ok(ptr, ia, ib, eid, n_dest, n_slots, chunk_dest, chunk_begin, n_chunks, long_dest, long_ptr, n_long, part, d))
        return SSLREC_E_BADARG;
    if (!X || !R || !G || !Y || !M || !Z || !dP || n_rel < 1 || !(slope >= 0.f) || (n_slots > 0 && (!S || !alpha || !dl))) return SSLREC_E_BADARG;
    if (!rg_aligned(X) || !rg_aligned(R) || !rg_aligned(G) || !rg_aligned(Y) || !rg_aligned(dP)) return SSLREC_E_BADARG;
    const RgList ls = {ptr, ia, ib, eid, chunk_dest, chunk_begin, n_dest, n_chunks};
    const RgLong lg = {long_dest, long_ptr, n_long};
    const bool lds = rg_lds(n_rel, d);
    hipStream_t st = (hipStream_t)stream;
#define RG_CALL(D) rg_bwd_head<D>(ls, lg, X, R, n_rel, lds, slope, keep, G, Y, S, M, Z, alpha, dl, dP, part, st)
    RG_SWITCH(d, RG_CALL(32), RG_CALL(64), RG_CALL(128))
#undef RG_CALL
}

int sslrec_rgat_bwd_tail_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                             const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest,
                             const int32_t *long_ptr, int32_t n_long, const float *G, const float *R, int32_t n_rel, int32_t d, const uint8_t *keep,
                             const float *alpha, const float *dl, float *dX, float *dQ, float *part, void *stream) {
    if (!rg_list_ok(ptr, ia, ib, eid, n_dest, n_slots, chunk_dest, chunk_begin, n_chunks, long_dest, long_ptr, n_long, part, d))
        return SSLREC_E_BADARG;
    if (!G || !R || !dX || !dQ || n_rel < 1 || (n_slots > 0 && (!alpha || !dl))) return SSLREC_E_BADARG;
    if (!rg_aligned(G) || !rg_aligned(R) || !rg_aligned(dX) || !rg_aligned(dQ)) return SSLREC_E_BADARG;
    const RgList ls = {ptr, ia, ib, eid, chunk_dest, chunk_begin, n_dest, n_chunks};
    const RgLong lg = {long_dest, long_ptr, n_long};
    const bool lds = rg_lds(n_rel, d);
    hipStream_t st = (hipStream_t)stream;
#define RG_CALL(D) rg_bwd_walk<D, true>(ls, lg, G, R, n_rel, lds, keep, alpha, dl, dX, dQ, part, st)
    RG_SWITCH(d, RG_CALL(32), RG_CALL(64), RG_CALL(128))
#undef RG_CALL
}

int sslrec_rgat_bwd_rel_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                            const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest,
                            const int32_t *long_ptr, int32_t n_long, const float *P, const float *Q, int32_t d, const uint8_t *keep, const float *dl,
                            float *dR, float *part, void *stream) {
    if (!rg_list_ok(ptr, ia, ib, eid, n_dest, n_slots, chunk_dest, chunk_begin, n_chunks, long_dest, long_ptr, n_long, part, d))
        return SSLREC_E_BADARG;
    if (!P || !Q || !dR || (n_slots > 0 && !dl)) return SSLREC_E_BADARG;
    if (!rg_aligned(P) || !rg_aligned(Q) || !rg_aligned(dR)) return SSLREC_E_BADARG;
    const RgList ls = {ptr, ia, ib, eid, chunk_dest, chunk_begin, n_dest, n_chunks};
    const RgLong lg = {long_dest, long_ptr, n_long};
    hipStream_t st = (hipStream_t)stream;
#define RG_CALL(D) rg_bwd_walk<D, false>(ls, lg, P, Q, 0, false, keep, (const float *)nullptr, dl, dR, (float *)nullptr, part, st)
    RG_SWITCH(d, RG_CALL(32), RG_CALL(64), RG_CALL(128))
#undef RG_CALL
}

}      // extern "C"
