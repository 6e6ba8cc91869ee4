// Kernels of KGIN (reference models/kg/kgin.py): the relational aggregation over the typed edges of a knowledge graph (:33-36), forward
// and backward, and the row-wise factor modulation of the user side (:38-46).
//
// Relational walk.  The edges are given in some ORDER (by head, by tail or by relation: graph.RelGraph builds the three once) as a CSR-like
// list: ptr [n_dest + 1] and, per slot, a row of table A (ia), a row of table B (ib) and the id of the edge in the caller's numbering
// (eid), through which the optional keep mask is read, so a new mask rebuilds nothing.  One kernel serves three sums:
//     forward   Y[h]  = mean over kept slots of   X[tail] (.) W[rel]               (A = X, B = W, the list ordered by head)
//     backward  dX[t] = sum  over kept slots of   G[head] (.) W[rel] / max(c_head, 1)   (A = G, B = W, ordered by tail)
//               dW[r] = sum  over kept slots of   G[head] (.) X[tail] / max(c_head, 1)  (A = G, B = X, ordered by relation)
// with c_h the INTEGER number of kept edges of head h, written by the forward and read by both backward sums.  No [E, d] tensor exists.
//
// Geometry.  A row of d = 32 / 64 / 128 floats belongs to a lane group of L = d / 4 lanes, one float4 per lane; a workgroup of 256 threads
// holds 256 / L groups, each of which takes one WORK ITEM at a time: a destination of at most KG_CHUNK slots, or one KG_CHUNK-slot chunk
// of a longer destination (an attribute entity with tens of thousands of inbound edges, a relation with all its edges: the normal case).
// A group adds its slots in list order.  A chunk's sum goes to part[chunk]; a finishing launch adds every long destination's partials in
// chunk order.  No float atomics anywhere: two calls give the same bits.  B sits in LDS when it is W and fits KG_LDS_BYTES.
//
// Factor modulation.  Row-wise with the mhcn.hip geometry (contiguous row ranges, at most KG_MAX_ROW_BLOCKS workgroups); the backward
// recomputes the softmax and sums dlatent and dD [F, d] from per-workgroup slabs that a finishing launch adds in a fixed order.
// Index arrays are int32 and are validated by the host class that builds them; the kernels do not re-check them.
#include "common.h"

namespace {

constexpr int KG_THREADS = 256;
constexpr int KG_CHUNK = 512;                 // slots per work item (SSLREC_KGIN_CHUNK of the header)
constexpr int KG_FLIGHT = 8;                  // slots a lane group loads before it adds them (in list order)
constexpr int KG_MAX_BLOCKS = 2048;           // walk: workgroups stride over the work items
constexpr int KG_MAX_ROW_BLOCKS = 512;        // factor modulation: workgroups own contiguous row ranges
constexpr int KG_LDS_BYTES = 48 * 1024;       // W is staged in LDS up to this size
constexpr int KG_FMAX = 8;                    // latent factors

inline bool kg_dim_ok(int64_t d) { return d == 32 || d == 64 || d == 128; }
inline bool kg_aligned(const void *p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ float4 f4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }
__device__ __forceinline__ float4 axpy4(const float s, const float4 a, const float4 y) {
    return make_float4(fmaf(s, a.x, y.x), fmaf(s, a.y, y.y), fmaf(s, a.z, y.z), fmaf(s, a.w, y.w));
}
__device__ __forceinline__ float4 fma4(const float4 a, const float4 b, const float4 y) {
    return make_float4(fmaf(a.x, b.x, y.x), fmaf(a.y, b.y, y.y), fmaf(a.z, b.z, y.z), fmaf(a.w, b.w, y.w));
}
__device__ __forceinline__ float4 mul4(const float4 a, const float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 scale4(const float s, const float4 a) { return make_float4(s * a.x, s * a.y, s * a.z, s * a.w); }
__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

template <int L>
__device__ __forceinline__ float grp_sum(float v) {
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- the relational walk -----------------------------------------------------------------------------------------------------------
struct KgList {
    const int32_t *ptr, *ia, *ib, *eid;       // [n_dest + 1], [E], [E], [E]
    const int32_t *chunk_dest, *chunk_begin;  // [n_chunks]: the chunks of the destinations of more than KG_CHUNK slots
    int n_dest, n_chunks;
};

// FWD: the mean, cnt is written.  !FWD: every term is scaled by 1 / max(cnt[ia], 1), cnt is read.
template <int D, bool FWD, bool BLDS>
__global__ __launch_bounds__(KG_THREADS) void kg_walk_kernel(const KgList ls, const float4 *__restrict__ A, const float4 *__restrict__ B,
                                                             const int n_b_rows, const uint8_t *__restrict__ keep, int32_t *__restrict__ cnt,
                                                             float4 *__restrict__ out, float4 *__restrict__ part, int32_t *__restrict__ part_cnt) {
    constexpr int L = D / 4, RPB = KG_THREADS / L;
    extern __shared__ float4 kg_bs[];
    if constexpr (BLDS) {
        for (int i = threadIdx.x; i < n_b_rows * L; i += KG_THREADS) kg_bs[i] = B[i];
        __syncthreads();
    }
    const int lig = threadIdx.x % L, grp = threadIdx.x / L;
    const long long items = (long long)ls.n_dest + ls.n_chunks;
    for (long long item = (long long)blockIdx.x * RPB + grp; item < items; item += (long long)gridDim.x * RPB) {
        const bool chunk = item >= ls.n_dest;
        int dest, s0, s1;
        if (!chunk) {
            dest = (int)item;
            s0 = ls.ptr[dest];
            s1 = ls.ptr[dest + 1];
            if (s1 - s0 > KG_CHUNK) continue;          // its chunks are work items of their own
        } else {
            const int c = (int)(item - ls.n_dest);
            dest = ls.chunk_dest[c];
            s0 = ls.chunk_begin[c];
            const int end = ls.ptr[dest + 1];
            s1 = s0 + KG_CHUNK < end ? s0 + KG_CHUNK : end;
        }
        float4 acc = f4_zero();
        int n = 0;
        for (int s = s0; s < s1; s += KG_FLIGHT) {
            // the slot's three indices are loaded side by side (all are valid rows), so a table row waits on two loads, not three
            bool k[KG_FLIGHT];
            int ra[KG_FLIGHT], rb[KG_FLIGHT], id[KG_FLIGHT];
#pragma unroll
            for (int j = 0; j < KG_FLIGHT; ++j) {
                const bool in = s + j < s1;
                id[j] = (in && keep != nullptr) ? ls.eid[s + j] : 0;
                ra[j] = in ? ls.ia[s + j] : 0;
                rb[j] = in ? ls.ib[s + j] : 0;
            }
#pragma unroll
            for (int j = 0; j < KG_FLIGHT; ++j) k[j] = s + j < s1 && (keep == nullptr || keep[id[j]] != 0);
            float4 a[KG_FLIGHT], b[KG_FLIGHT];
            float sc[KG_FLIGHT];
#pragma unroll
            for (int j = 0; j < KG_FLIGHT; ++j) {
                a[j] = k[j] ? A[(size_t)ra[j] * L + lig] : f4_zero();
                if constexpr (BLDS)
                    b[j] = kg_bs[rb[j] * L + lig];
                else
                    b[j] = k[j] ? B[(size_t)rb[j] * L + lig] : f4_zero();
                if constexpr (!FWD) {
                    const int c = k[j] ? cnt[ra[j]] : 1;
                    sc[j] = 1.f / (float)(c > 1 ? c : 1);
                }
            }
#pragma unroll
            for (int j = 0; j < KG_FLIGHT; ++j) {       // slots in list order
                if (k[j]) {
                    if constexpr (FWD)
                        acc = fma4(a[j], b[j], acc);
                    else
                        acc = fma4(scale4(sc[j], a[j]), b[j], acc);
                    ++n;
                }
            }
        }
        if (!chunk) {
            if constexpr (FWD) {
                out[(size_t)dest * L + lig] = scale4(1.f / (float)(n > 1 ? n : 1), acc);
                if (lig == 0) cnt[dest] = n;
            } else {
                out[(size_t)dest * L + lig] = acc;
            }
        } else {
            const size_t c = (size_t)(item - ls.n_dest);
            part[c * L + lig] = acc;
            if (FWD && lig == 0) part_cnt[c] = n;
        }
    }
}

// one lane group per long destination: its partials in chunk order
template <int D, bool FWD>
__global__ __launch_bounds__(KG_THREADS) void kg_walk_finish_kernel(const int32_t *__restrict__ long_dest, const int32_t *__restrict__ long_ptr,
                                                                    const int n_long, const float4 *__restrict__ part,
                                                                    const int32_t *__restrict__ part_cnt, int32_t *__restrict__ cnt,
                                                                    float4 *__restrict__ out) {
    constexpr int L = D / 4, RPB = KG_THREADS / L;
    const int lig = threadIdx.x % L;
    const long long j = (long long)blockIdx.x * RPB + threadIdx.x / L;
    if (j >= n_long) return;
    const int c0 = long_ptr[j], c1 = long_ptr[j + 1], dest = long_dest[j];
    float4 acc = f4_zero();
    int n = 0;
    for (int c = c0; c < c1; ++c) {
        acc = add4(acc, part[(size_t)c * L + lig]);
        if constexpr (FWD) n += part_cnt[c];
    }
    if constexpr (FWD) {
        out[(size_t)dest * L + lig] = scale4(1.f / (float)(n > 1 ? n : 1), acc);
        if (lig == 0) cnt[dest] = n;
    } else {
        out[(size_t)dest * L + lig] = acc;
    }
}

struct KgLong {
    const int32_t *dest, *ptr;
    int n;
};

template <int D, bool FWD>
int kg_walk(const KgList &ls, const KgLong &lg, const float *A, const float *B, int n_b_rows, bool b_lds, const uint8_t *keep, int32_t *cnt,
            float *out, float *part, int32_t *part_cnt, hipStream_t st) {
    constexpr int L = D / 4, RPB = KG_THREADS / L;
    const long long items = (long long)ls.n_dest + ls.n_chunks;
    if (items > 0) {
        long long blocks = (items + RPB - 1) / RPB;
        if (blocks > KG_MAX_BLOCKS) blocks = KG_MAX_BLOCKS;
        if (b_lds)
            hipLaunchKernelGGL((kg_walk_kernel<D, FWD, true>), dim3((unsigned)blocks), dim3(KG_THREADS), (size_t)n_b_rows * D * sizeof(float), st, ls,
                               (const float4 *)A, (const float4 *)B, n_b_rows, keep, cnt, (float4 *)out, (float4 *)part, part_cnt);
        else
            hipLaunchKernelGGL((kg_walk_kernel<D, FWD, false>), dim3((unsigned)blocks), dim3(KG_THREADS), 0, st, ls, (const float4 *)A,
                               (const float4 *)B, n_b_rows, keep, cnt, (float4 *)out, (float4 *)part, part_cnt);
    }
    if (lg.n > 0)
        hipLaunchKernelGGL((kg_walk_finish_kernel<D, FWD>), dim3((unsigned)((lg.n + RPB - 1) / RPB)), dim3(KG_THREADS), 0, st, lg.dest, lg.ptr, lg.n,
                           (const float4 *)part, (const int32_t *)part_cnt, cnt, (float4 *)out);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

// ---- factor modulation -------------------------------------------------------------------------------------------------------------
struct KgGeom {
    int G, rows_per_block;
};

inline KgGeom kg_geom(int N, int d) {
    const int rpb = KG_THREADS / (d / 4);
    const long long passes = ((long long)N + rpb - 1) / rpb;
    const long long g0 = passes < KG_MAX_ROW_BLOCKS ? passes : KG_MAX_ROW_BLOCKS;
    const long long ppb = (passes + g0 - 1) / g0;
    KgGeom g;
    g.G = (int)((passes + ppb - 1) / ppb);
    g.rows_per_block = (int)(ppb * rpb);
    return g;
}

// p = softmax_f <u, latent_f> of the group's row and m = sum_f p_f D_f; factors f >= F carry p_f = 0
template <int L>
__device__ __forceinline__ float4 kg_factor_mix(const float4 uu, const float4 *__restrict__ sl, const float4 *__restrict__ sd, const int F,
                                                const int lig, float (&p)[KG_FMAX]) {
    float lg[KG_FMAX];
    float mx = -INFINITY;
#pragma unroll
    for (int f = 0; f < KG_FMAX; ++f) {
        if (f < F) {
            lg[f] = grp_sum<L>(dot4(uu, sl[f * L + lig]));
            mx = fmaxf(mx, lg[f]);
        }
    }
    float ps = 0.f;
#pragma unroll
    for (int f = 0; f < KG_FMAX; ++f) {
        p[f] = f < F ? expf(lg[f] - mx) : 0.f;
        ps += p[f];
    }
    float4 m = f4_zero();
#pragma unroll
    for (int f = 0; f < KG_FMAX; ++f) {
        if (f < F) {
            p[f] = p[f] / ps;
            m = axpy4(p[f], sd[f * L + lig], m);
        }
    }
    return m;
}

template <int D>
__global__ __launch_bounds__(KG_THREADS) void kg_fm_fwd_kernel(const float4 *__restrict__ agg, const float4 *__restrict__ u,
                                                               const float4 *__restrict__ latent, const float4 *__restrict__ Dm, const int U,
                                                               const int F, const int rows_per_block, float4 *__restrict__ out) {
    constexpr int L = D / 4, RPB = KG_THREADS / L;
    __shared__ float4 sl[KG_FMAX * L], sd[KG_FMAX * L];
    for (int i = threadIdx.x; i < F * L; i += KG_THREADS) {
        sl[i] = latent[i];
        sd[i] = Dm[i];
    }
    __syncthreads();
    const int lig = threadIdx.x % L, grp = threadIdx.x / L;
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = r0 + rows_per_block < U ? r0 + rows_per_block : U;
    for (long long base = r0; base < r1; base += RPB) {
        const long long r = base + grp;
        const bool valid = r < r1;
        const float4 uu = valid ? u[(size_t)r * L + lig] : f4_zero();
        const float4 a = valid ? agg[(size_t)r * L + lig] : f4_zero();
        float p[KG_FMAX];
        const float4 m = kg_factor_mix<L>(uu, sl, sd, F, lig, p);
        if (valid) out[(size_t)r * L + lig] = fma4(a, m, a);
    }
}

// the workgroup's sum of one [d] row per thread -> dst[L] (lane groups in ascending order); `s` is reused: barrier before and after
template <int D>
__device__ __forceinline__ void kg_block_colsum(const float4 acc, float4 *__restrict__ s, float4 *__restrict__ dst) {
    constexpr int L = D / 4, RPB = KG_THREADS / L;
    __syncthreads();
    s[threadIdx.x] = acc;
    __syncthreads();
    if ((int)threadIdx.x < L) {
        float4 t = s[threadIdx.x];
#pragma unroll 4
        for (int g = 1; g < RPB; ++g) t = add4(t, s[g * L + threadIdx.x]);
        dst[threadIdx.x] = t;
    }
}

template <int D>
__global__ __launch_bounds__(KG_THREADS) void kg_fm_bwd_kernel(const float4 *__restrict__ agg, const float4 *__restrict__ u,
                                                               const float4 *__restrict__ latent, const float4 *__restrict__ Dm,
                                                               const float4 *__restrict__ gout, const int U, const int F, const int rows_per_block,
                                                               float4 *__restrict__ d_agg, float4 *__restrict__ d_u, float4 *__restrict__ part) {
    constexpr int L = D / 4, RPB = KG_THREADS / L;
    __shared__ float4 sl[KG_FMAX * L], sd[KG_FMAX * L];
    __shared__ float4 red[KG_THREADS];
    for (int i = threadIdx.x; i < F * L; i += KG_THREADS) {
        sl[i] = latent[i];
        sd[i] = Dm[i];
    }
    __syncthreads();
    const int lig = threadIdx.x % L, grp = threadIdx.x / L;
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = r0 + rows_per_block < U ? r0 + rows_per_block : U;
    float4 acc_l[KG_FMAX], acc_d[KG_FMAX];
#pragma unroll
    for (int f = 0; f < KG_FMAX; ++f) acc_l[f] = acc_d[f] = f4_zero();
    for (long long base = r0; base < r1; base += RPB) {
        const long long r = base + grp;
        const bool valid = r < r1;
        const float4 uu = valid ? u[(size_t)r * L + lig] : f4_zero();
        const float4 a = valid ? agg[(size_t)r * L + lig] : f4_zero();
        const float4 g = valid ? gout[(size_t)r * L + lig] : f4_zero();
        float p[KG_FMAX];
        const float4 m = kg_factor_mix<L>(uu, sl, sd, F, lig, p);
        const float4 dm = mul4(g, a);
        float dp[KG_FMAX];
        float t = 0.f;
#pragma unroll
        for (int f = 0; f < KG_FMAX; ++f) {
            dp[f] = 0.f;
            if (f < F) {
                dp[f] = grp_sum<L>(dot4(dm, sd[f * L + lig]));
                t = fmaf(p[f], dp[f], t);
            }
        }
        float4 du = f4_zero();
#pragma unroll
        for (int f = 0; f < KG_FMAX; ++f) {
            if (f < F) {
                const float dl = p[f] * (dp[f] - t);
                du = axpy4(dl, sl[f * L + lig], du);
                acc_l[f] = axpy4(dl, uu, acc_l[f]);
                acc_d[f] = axpy4(p[f], dm, acc_d[f]);
            }
        }
        if (valid) {
            d_agg[(size_t)r * L + lig] = fma4(g, m, g);
            d_u[(size_t)r * L + lig] = du;
        }
    }
    // part[block][2 F][D]: dlatent rows, then dD rows
    float4 *mine = part + (size_t)blockIdx.x * 2 * F * L;
#pragma unroll
    for (int f = 0; f < KG_FMAX; ++f) {
        if (f < F) {
            kg_block_colsum<D>(acc_l[f], red, mine + (size_t)f * L);
            kg_block_colsum<D>(acc_d[f], red, mine + (size_t)(F + f) * L);
        }
    }
}

// out[e] = ((s0 + s1) + s2) + s3; s_g = partials g, g + 4, ... of element e in ascending order.  64 elements per workgroup.
__global__ __launch_bounds__(256) void kg_colsum_finish_kernel(const float *__restrict__ part, const int S, const int n_elem, float *__restrict__ out) {
    __shared__ float fs[4][64];
    const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + j;
    float s = 0.f;
    if (e < n_elem)
        for (int sl = g; sl < S; sl += 4) s += part[(size_t)sl * n_elem + e];
    fs[g][j] = s;
    __syncthreads();
    if (g == 0 && e < n_elem) out[e] = ((fs[0][j] + fs[1][j]) + fs[2][j]) + fs[3][j];
}

inline float *kg_ws(void *ws) { return (float *)(((uintptr_t)ws + 15) & ~(uintptr_t)15); }

template <int D>
int kg_fm_fwd(const float *agg, const float *u, const float *latent, const float *Dm, int U, int F, float *out, hipStream_t st) {
    const KgGeom g = kg_geom(U, D);
    hipLaunchKernelGGL((kg_fm_fwd_kernel<D>), dim3(g.G), dim3(KG_THREADS), 0, st, (const float4 *)agg, (const float4 *)u, (const float4 *)latent,
                       (const float4 *)Dm, U, F, g.rows_per_block, (float4 *)out);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

template <int D>
int kg_fm_bwd(const float *agg, const float *u, const float *latent, const float *Dm, const float *gout, int U, int F, float *d_agg, float *d_u,
              float *d_lat_and_d, float *part, hipStream_t st) {
    const KgGeom g = kg_geom(U, D);
    hipLaunchKernelGGL((kg_fm_bwd_kernel<D>), dim3(g.G), dim3(KG_THREADS), 0, st, (const float4 *)agg, (const float4 *)u, (const float4 *)latent,
                       (const float4 *)Dm, (const float4 *)gout, U, F, g.rows_per_block, (float4 *)d_agg, (float4 *)d_u, (float4 *)part);
    const int n_elem = 2 * F * D;
    hipLaunchKernelGGL(kg_colsum_finish_kernel, dim3((unsigned)((n_elem + 63) / 64)), dim3(256), 0, st, (const float *)part, g.G, n_elem, d_lat_and_d);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

int kg_rel(bool fwd, const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
           const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest, const int32_t *long_ptr, int32_t n_long,
           const float *A, const float *B, int32_t n_b_rows, int32_t b_in_lds, int32_t d, const uint8_t *keep, int32_t *cnt, float *out, float *part,
           int32_t *part_cnt, void *stream) {
    if (!ptr || !A || !B || !cnt || !out || n_dest < 0 || n_slots < 0 || n_slots >= 0x7fffffffLL || n_chunks < 0 || n_long < 0 || n_b_rows < 1 ||
        !kg_dim_ok(d))
        return SSLREC_E_BADARG;
    if (n_slots > 0 && (!ia || !ib || !eid)) return SSLREC_E_BADARG;
    if ((n_chunks > 0) != (n_long > 0)) return SSLREC_E_BADARG;
    if (n_chunks > 0 && (!chunk_dest || !chunk_begin || !long_dest || !long_ptr || !part || (fwd && !part_cnt))) return SSLREC_E_BADARG;
    if (!kg_aligned(A) || !kg_aligned(B) || !kg_aligned(out) || (part && !kg_aligned(part))) return SSLREC_E_BADARG;
    const bool lds = b_in_lds != 0 && (size_t)n_b_rows * d * sizeof(float) <= (size_t)KG_LDS_BYTES;
    const KgList ls = {ptr, ia, ib, eid, chunk_dest, chunk_begin, n_dest, n_chunks};
    const KgLong lg = {long_dest, long_ptr, n_long};
    hipStream_t st = (hipStream_t)stream;
#define KG_CALL(D) (fwd ? kg_walk<D, true>(ls, lg, A, B, n_b_rows, lds, keep, cnt, out, part, part_cnt, st) \
                        : kg_walk<D, false>(ls, lg, A, B, n_b_rows, lds, keep, cnt, out, part, part_cnt, st))
    switch (d) {
    case 32: return KG_CALL(32);
    case 64: return KG_CALL(64);
    default: return KG_CALL(128);
    }
#undef KG_CALL
}

}      // namespace

extern "C" {

int sslrec_kgin_rel_fwd_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                            const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest,
                            const int32_t *long_ptr, int32_t n_long, const float *X, const float *W, int32_t R, int32_t d, const uint8_t *keep,
                            int32_t *cnt, float *Y, float *part, int32_t *part_cnt, void *stream) {
    return kg_rel(true, ptr, ia, ib, eid, n_dest, n_slots, chunk_dest, chunk_begin, n_chunks, long_dest, long_ptr, n_long, X, W, R, 1, d, keep, cnt, Y,
                  part, part_cnt, stream);
}

int sslrec_kgin_rel_bwd_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                            const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest,
                            const int32_t *long_ptr, int32_t n_long, const float *G, const float *B, int32_t n_b_rows, int32_t b_in_lds, int32_t d,
                            const uint8_t *keep, const int32_t *cnt, float *out, float *part, void *stream) {
    return kg_rel(false, ptr, ia, ib, eid, n_dest, n_slots, chunk_dest, chunk_begin, n_chunks, long_dest, long_ptr, n_long, G, B, n_b_rows, b_in_lds, d,
                  keep, const_cast<int32_t *>(cnt), out, part, nullptr, stream);
}

size_t sslrec_kgin_fm_ws_bytes(int32_t U, int32_t d, int32_t F) {
    if (U < 1 || !kg_dim_ok(d) || F < 1 || F > KG_FMAX) return 0;
    return (size_t)kg_geom(U, d).G * 2 * F * d * sizeof(float) + 32;
}

int sslrec_kgin_fm_fwd_f32(const float *agg, const float *u, const float *latent, const float *Dm, int32_t U, int32_t d, int32_t F, float *out,
                           void *stream) {
    if (!agg || !u || !latent || !Dm || !out || U < 1 || !kg_dim_ok(d) || F < 1 || F > KG_FMAX) return SSLREC_E_BADARG;
    if (!kg_aligned(agg) || !kg_aligned(u) || !kg_aligned(latent) || !kg_aligned(Dm) || !kg_aligned(out)) return SSLREC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    switch (d) {
    case 32: return kg_fm_fwd<32>(agg, u, latent, Dm, U, F, out, st);
    case 64: return kg_fm_fwd<64>(agg, u, latent, Dm, U, F, out, st);
    default: return kg_fm_fwd<128>(agg, u, latent, Dm, U, F, out, st);
    }
}

int sslrec_kgin_fm_bwd_f32(const float *agg, const float *u, const float *latent, const float *Dm, const float *gout, int32_t U, int32_t d, int32_t F,
                           float *d_agg, float *d_u, float *d_latent_and_d, void *ws, void *stream) {
    if (!agg || !u || !latent || !Dm || !gout || !d_agg || !d_u || !d_latent_and_d || !ws || U < 1 || !kg_dim_ok(d) || F < 1 || F > KG_FMAX)
        return SSLREC_E_BADARG;
    if (!kg_aligned(agg) || !kg_aligned(u) || !kg_aligned(latent) || !kg_aligned(Dm) || !kg_aligned(gout) || !kg_aligned(d_agg) || !kg_aligned(d_u))
        return SSLREC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    float *part = kg_ws(ws);
    switch (d) {
    case 32: return kg_fm_bwd<32>(agg, u, latent, Dm, gout, U, F, d_agg, d_u, d_latent_and_d, part, st);
    case 64: return kg_fm_bwd<64>(agg, u, latent, Dm, gout, U, F, d_agg, d_u, d_latent_and_d, part, st);
    default: return kg_fm_bwd<128>(agg, u, latent, Dm, gout, U, F, d_agg, d_u, d_latent_and_d, part, st);
    }
}

}      // extern "C"
