// Kernels of KGRec's two-head relational attention (reference models/kg/kgrec.py, AttnHGCN.shared_layer_agg :63-88 and norm_attn_computer
// :165-188): a scaled dot-product attention over typed edges whose key and value are modulated by the relation row, forward and backward,
// and the forward-only rationale scores.
//
// query = X[h] W_Q and key = X[t] W_Q are rows of the NODE table T = X W_Q that the caller forms with one dense GEMM; the per-edge matvec is
// gone.  Attention head a in {0, 1} owns the columns C_a = [a d/2, (a + 1) d/2), c = 1 / sqrt(d / 2).  With the kept edges e = (h, t, r):
//     l_ea  = c sum_{j in C_a} T[h]_j T[t]_j R[r]_j
//     al_ea = exp(l_ea - M_ha) / z_ha           M_ha = max over the head entity's kept edges, z_ha the sum of the exponentials
//     Y[h]_j = sum_e al_ea(j) X[t]_j R[r]_j     (0 for an entity without a kept edge)
// and from G = dY:  delta_ha = sum_{C_a} G[h]_j Y[h]_j,  dl_ea = al_ea (sum_{C_a} G[h]_j X[t]_j R[r]_j - delta_ha),
//     dT[h]_j += c dl_ea T[t]_j R[r]_j                  (walk by head, which also writes al and dl by edge id as [E, 2])
//     dT[t]_j += c dl_ea T[h]_j R[r]_j    dX[t]_j += al_ea G[h]_j R[r]_j                        (one walk by tail)
//     dR[r]_j += c dl_ea T[h]_j T[t]_j + al_ea G[h]_j X[t]_j                                    (walk by relation)
// Between forward and backward only [E, 2]- and [N, 2]-sized vectors live (l by edge id, M, z) beside Y; no [E, d] tensor exists.
//
// Lists and geometry are those of kgin.hip / rgat.hip: graph.RelGraph's three orders as ptr / ia / ib / eid, the keep mask read through eid;
// a lane group of L = d / 4 lanes (one float4 per lane) takes one work item, a destination of at most MH_CHUNK slots or one MH_CHUNK-slot
// chunk of a longer one.  The two attention heads are the two aligned halves of the lane group, so a per-head sum is group_sum<L / 2>
// (4, 8 or 16 lanes: inside one DPP row) and every lane carries the running (m, z) of ITS head.  Slots are added in list order.  A chunk
// leaves (m_c, z_c, acc_c) per attention head and the finishing launch merges a long destination's chunks in chunk order, per head.  The
// backward's chunk sums are added in chunk order.  No float atomics: two calls give the same bits.  R sits in LDS when it fits MH_LDS_BYTES.
// Index arrays are int32 and validated by the host class that builds them; the kernels do not re-check them.
#include "lanegroup.h"

namespace {

constexpr int MH_THREADS = 256;
constexpr int MH_CHUNK = 512;                 // slots per work item (graph.REL_CHUNK, SSLREC_KGIN_CHUNK)
constexpr int MH_FLIGHT = 4;                  // slots a lane group loads before it adds them (in list order)
constexpr int MH_MAX_BLOCKS = 2048;           // workgroups stride over the work items
constexpr int MH_LDS_BYTES = 48 * 1024;       // R is staged in LDS up to this size

inline bool mh_dim_ok(int64_t d) { return d == 32 || d == 64 || d == 128; }
inline bool mh_aligned(const void *p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ float4 z4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 axpy4(const float s, const float4 a, const float4 y) {
    return make_float4(fmaf(s, a.x, y.x), fmaf(s, a.y, y.y), fmaf(s, a.z, y.z), fmaf(s, a.w, y.w));
}
__device__ __forceinline__ float4 scale4(const float s, const float4 a) { return make_float4(s * a.x, s * a.y, s * a.z, s * a.w); }
__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 mul4(const float4 a, const float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }

struct MhList {
    const int32_t *ptr, *ia, *ib, *eid;       // [n_dest + 1], [E], [E], [E]
    const int32_t *chunk_dest, *chunk_begin;  // [n_chunks]
    int n_dest, n_chunks;
};

struct MhLong {
    const int32_t *dest, *ptr;
    int n;
};

// the slots [s0, s1) of work item `item`; false for a long destination's own item (its chunks are items of their own)
__device__ __forceinline__ bool mh_item(const MhList &ls, const long long item, int &dest, int &s0, int &s1) {
    if (item < ls.n_dest) {
        dest = (int)item;
        s0 = ls.ptr[dest];
        s1 = ls.ptr[dest + 1];
        return s1 - s0 <= MH_CHUNK;
    }
    const int c = (int)(item - ls.n_dest);
    dest = ls.chunk_dest[c];
    s0 = ls.chunk_begin[c];
    const int end = ls.ptr[dest + 1];
    s1 = s0 + MH_CHUNK < end ? s0 + MH_CHUNK : end;
    return true;
}

template <int L>
__device__ __forceinline__ void mh_stage(float4 *__restrict__ lds, const float4 *__restrict__ R, const int n_rel) {
    for (int i = threadIdx.x; i < n_rel * L; i += MH_THREADS) lds[i] = R[i];
    __syncthreads();
}

// ---- forward: the list ordered by head, ia = tail, ib = relation ------------------------------------------------------------------------
// Lg [E, 2] by edge id; M, Z [n_dest, 2]; part [n_chunks, d]; part_mz [n_chunks, 2 heads, (m, z)]
template <int D, bool RLDS>
__global__ __launch_bounds__(MH_THREADS) void mh_fwd_kernel(const MhList ls, const float4 *__restrict__ X, const float4 *__restrict__ T,
                                                            const float4 *__restrict__ R, const int n_rel, const float c,
                                                            const uint8_t *__restrict__ keep, float *__restrict__ Lg, float *__restrict__ M,
                                                            float *__restrict__ Z, float4 *__restrict__ Y, float4 *__restrict__ part,
                                                            float *__restrict__ part_mz) {
    constexpr int L = D / 4, H = L / 2, RPB = MH_THREADS / L;
    extern __shared__ float4 mh_rs[];
    if constexpr (RLDS) mh_stage<L>(mh_rs, R, n_rel);
    const int lig = threadIdx.x % L, grp = threadIdx.x / L;
    const int a = lig / H;                                // this lane's attention head
    const bool lead = lig % H == 0;
    const long long items = (long long)ls.n_dest + ls.n_chunks;
    for (long long item = (long long)blockIdx.x * RPB + grp; item < items; item += (long long)gridDim.x * RPB) {
        int dest, s0, s1;
        if (!mh_item(ls, item, dest, s0, s1)) continue;
        const float4 th = T[(size_t)dest * L + lig];
        float m = -INFINITY, z = 0.f;
        float4 acc = z4();
        for (int s = s0; s < s1; s += MH_FLIGHT) {
            bool k[MH_FLIGHT];
            int rt[MH_FLIGHT], rr[MH_FLIGHT], id[MH_FLIGHT];
#pragma unroll
            for (int j = 0; j < MH_FLIGHT; ++j) {
                const bool in = s + j < s1;
                id[j] = in ? ls.eid[s + j] : 0;
                rt[j] = in ? ls.ia[s + j] : 0;
                rr[j] = in ? ls.ib[s + j] : 0;
            }
#pragma unroll
            for (int j = 0; j < MH_FLIGHT; ++j) k[j] = s + j < s1 && (keep == nullptr || keep[id[j]] != 0);
            float4 tt[MH_FLIGHT], v[MH_FLIGHT];
#pragma unroll
            for (int j = 0; j < MH_FLIGHT; ++j) {
                float4 r;
                if constexpr (RLDS)
                    r = mh_rs[rr[j] * L + lig];
                else
                    r = k[j] ? R[(size_t)rr[j] * L + lig] : z4();
                tt[j] = mul4(k[j] ? T[(size_t)rt[j] * L + lig] : z4(), r);           // the key, T[t] * R[r]
                v[j] = mul4(k[j] ? X[(size_t)rt[j] * L + lig] : z4(), r);            // the value, X[t] * R[r]
            }
            float lg[MH_FLIGHT];
#pragma unroll
            for (int j = 0; j < MH_FLIGHT; ++j) lg[j] = c * group_sum<H>(dot4(th, tt[j]));      // (k is the same in the whole group)
#pragma unroll
            for (int j = 0; j < MH_FLIGHT; ++j) {       // slots in list order
                if (k[j]) {
                    const float lj = lg[j];
                    if (lead) Lg[2 * (size_t)id[j] + a] = lj;
                    if (lj > m) {                        // a new maximum: what was summed so far shrinks by e^(m - lj) (0 the first time)
                        const float w = expf(m - lj);
                        z *= w;
                        acc = scale4(w, acc);
                        m = lj;
                    }
                    const float e = expf(lj - m);
                    z += e;
                    acc = axpy4(e, v[j], acc);
                }
            }
        }
        if (item < ls.n_dest) {
            const bool any = z > 0.f;
            Y[(size_t)dest * L + lig] = any ? scale4(1.f / z, acc) : z4();
            if (lead) {
                M[2 * (size_t)dest + a] = any ? m : 0.f;
                Z[2 * (size_t)dest + a] = z;
            }
        } else {
            const size_t ch = (size_t)(item - ls.n_dest);
            part[ch * L + lig] = acc;
            if (lead) {
                part_mz[(2 * ch + a) * 2] = m;
                part_mz[(2 * ch + a) * 2 + 1] = z;
            }
        }
    }
}

// one lane group per long head entity: its chunks' (m, z, acc) in chunk order, per attention head
template <int D>
__global__ __launch_bounds__(MH_THREADS) void mh_fwd_finish_kernel(const MhLong lg, const float4 *__restrict__ part,
                                                                   const float *__restrict__ part_mz, float *__restrict__ M,
                                                                   float *__restrict__ Z, float4 *__restrict__ Y) {
    constexpr int L = D / 4, H = L / 2, RPB = MH_THREADS / L;
    const int lig = threadIdx.x % L, a = lig / H;
    const long long j = (long long)blockIdx.x * RPB + threadIdx.x / L;
    if (j >= lg.n) return;
    const int c0 = lg.ptr[j], c1 = lg.ptr[j + 1], dest = lg.dest[j];
    float m = -INFINITY;
    for (int ch = c0; ch < c1; ++ch)
        if (part_mz[(2 * (size_t)ch + a) * 2 + 1] > 0.f) m = fmaxf(m, part_mz[(2 * (size_t)ch + a) * 2]);
    float z = 0.f;
    float4 acc = z4();
    for (int ch = c0; ch < c1; ++ch) {
        const float zc = part_mz[(2 * (size_t)ch + a) * 2 + 1];
        if (zc > 0.f) {                                  // (a chunk without a kept edge carries m_c = -inf)
            const float w = expf(part_mz[(2 * (size_t)ch + a) * 2] - m);
            z = fmaf(zc, w, z);
            acc = axpy4(w, part[(size_t)ch * L + lig], acc);
        }
    }
    const bool any = z > 0.f;
    Y[(size_t)dest * L + lig] = any ? scale4(1.f / z, acc) : z4();
    if (lig % H == 0) {
        M[2 * (size_t)dest + a] = any ? m : 0.f;
        Z[2 * (size_t)dest + a] = z;
    }
}

// ---- backward, walk by head: al_ea and dl_ea by edge id, dT[h] = c sum dl_ea T[t] R[r] --------------------------------------------------
template <int D, bool RLDS>
__global__ __launch_bounds__(MH_THREADS) void mh_bwd_head_kernel(const MhList ls, const float4 *__restrict__ X, const float4 *__restrict__ T,
                                                                 const float4 *__restrict__ R, const int n_rel, const float c,
                                                                 const uint8_t *__restrict__ keep, const float4 *__restrict__ G,
                                                                 const float4 *__restrict__ Y, const float *__restrict__ Lg,
                                                                 const float *__restrict__ M, const float *__restrict__ Z,
                                                                 float *__restrict__ alpha, float *__restrict__ dl, float4 *__restrict__ dT,
                                                                 float4 *__restrict__ part) {
    constexpr int L = D / 4, H = L / 2, RPB = MH_THREADS / L;
    extern __shared__ float4 mh_rs[];
    if constexpr (RLDS) mh_stage<L>(mh_rs, R, n_rel);
    const int lig = threadIdx.x % L, grp = threadIdx.x / L;
    const int a = lig / H;
    const bool lead = lig % H == 0;
    const long long items = (long long)ls.n_dest + ls.n_chunks;
    for (long long item = (long long)blockIdx.x * RPB + grp; item < items; item += (long long)gridDim.x * RPB) {
        int dest, s0, s1;
        if (!mh_item(ls, item, dest, s0, s1)) continue;
        const float4 g = G[(size_t)dest * L + lig];
        const float delta = group_sum<H>(dot4(g, Y[(size_t)dest * L + lig]));
        const float mh = M[2 * (size_t)dest + a], zh = Z[2 * (size_t)dest + a];
        const float inv = zh > 0.f ? 1.f / zh : 0.f;
        float4 acc = z4();
        for (int s = s0; s < s1; s += MH_FLIGHT) {
            bool k[MH_FLIGHT];
            int rt[MH_FLIGHT], rr[MH_FLIGHT], id[MH_FLIGHT];
#pragma unroll
            for (int j = 0; j < MH_FLIGHT; ++j) {
                const bool in = s + j < s1;
                id[j] = in ? ls.eid[s + j] : 0;
                rt[j] = in ? ls.ia[s + j] : 0;
                rr[j] = in ? ls.ib[s + j] : 0;
            }
#pragma unroll
            for (int j = 0; j < MH_FLIGHT; ++j) k[j] = s + j < s1 && (keep == nullptr || keep[id[j]] != 0);
            float4 tt[MH_FLIGHT], v[MH_FLIGHT];
            float lv[MH_FLIGHT];
#pragma unroll
            for (int j = 0; j < MH_FLIGHT; ++j) {
                float4 r;
                if constexpr (RLDS)
                    r = mh_rs[rr[j] * L + lig];
                else
                    r = k[j] ? R[(size_t)rr[j] * L + lig] : z4();
                tt[j] = mul4(k[j] ? T[(size_t)rt[j] * L + lig] : z4(), r);
                v[j] = mul4(k[j] ? X[(size_t)rt[j] * L + lig] : z4(), r);
                lv[j] = k[j] ? Lg[2 * (size_t)id[j] + a] : 0.f;
            }
            float gv[MH_FLIGHT];
#pragma unroll
            for (int j = 0; j < MH_FLIGHT; ++j) gv[j] = group_sum<H>(dot4(g, v[j]));
#pragma unroll
            for (int j = 0; j < MH_FLIGHT; ++j) {
                if (k[j]) {
                    const float al = expf(lv[j] - mh) * inv;
                    const float d_l = al * (gv[j] - delta);
                    if (lead) {
                        alpha[2 * (size_t)id[j] + a] = al;
                        dl[2 * (size_t)id[j] + a] = d_l;
                    }
                    acc = axpy4(c * d_l, tt[j], acc);
                }
            }
        }
        if (item < ls.n_dest)
            dT[(size_t)dest * L + lig] = acc;
        else
            part[(size_t)(item - ls.n_dest) * L + lig] = acc;
    }
}

// ---- backward, walks by tail and by relation --------------------------------------------------------------------------------------------
// TAIL: ia = head, ib = relation; out1[t] = sum al_e G[head] R[rel] (dX), out2[t] = c sum dl_e T[head] R[rel] (dT); partials [chunk][2][d]
// !TAIL: ia = head, ib = tail;    out1[r] = sum (c dl_e T[head] T[tail] + al_e G[head] X[tail]) (dR);             partials [chunk][d]
template <int D, bool TAIL, bool RLDS>
__global__ __launch_bounds__(MH_THREADS) void mh_bwd_walk_kernel(const MhList ls, const float4 *__restrict__ G, const float4 *__restrict__ X,
                                                                 const float4 *__restrict__ T, const float4 *__restrict__ R, const int n_rel,
                                                                 const float c, const uint8_t *__restrict__ keep,
                                                                 const float *__restrict__ alpha, const float *__restrict__ dl,
                                                                 float4 *__restrict__ out1, float4 *__restrict__ out2, float4 *__restrict__ part) {
    constexpr int L = D / 4, H = L / 2, RPB = MH_THREADS / L, W = TAIL ? 2 : 1;
    extern __shared__ float4 mh_rs[];
    if constexpr (RLDS) mh_stage<L>(mh_rs, R, n_rel);
    const int lig = threadIdx.x % L, grp = threadIdx.x / L;
    const int a = lig / H;
    const long long items = (long long)ls.n_dest + ls.n_chunks;
    for (long long item = (long long)blockIdx.x * RPB + grp; item < items; item += (long long)gridDim.x * RPB) {
        int dest, s0, s1;
        if (!mh_item(ls, item, dest, s0, s1)) continue;
        float4 acc1 = z4(), acc2 = z4();
        for (int s = s0; s < s1; s += MH_FLIGHT) {
            bool k[MH_FLIGHT];
            int ra[MH_FLIGHT], rb[MH_FLIGHT], id[MH_FLIGHT];
#pragma unroll
            for (int j = 0; j < MH_FLIGHT; ++j) {
                const bool in = s + j < s1;
                id[j] = in ? ls.eid[s + j] : 0;
                ra[j] = in ? ls.ia[s + j] : 0;
                rb[j] = in ? ls.ib[s + j] : 0;
            }
#pragma unroll
            for (int j = 0; j < MH_FLIGHT; ++j) k[j] = s + j < s1 && (keep == nullptr || keep[id[j]] != 0);
            float4 p1[MH_FLIGHT], p2[MH_FLIGHT];
            float wa[MH_FLIGHT], wd[MH_FLIGHT];
#pragma unroll
            for (int j = 0; j < MH_FLIGHT; ++j) {
                const float4 gh = k[j] ? G[(size_t)ra[j] * L + lig] : z4();
                const float4 th = k[j] ? T[(size_t)ra[j] * L + lig] : z4();
                if constexpr (TAIL) {
                    float4 r;
                    if constexpr (RLDS)
                        r = mh_rs[rb[j] * L + lig];
                    else
                        r = k[j] ? R[(size_t)rb[j] * L + lig] : z4();
                    p1[j] = mul4(gh, r);
                    p2[j] = mul4(th, r);
                } else {
                    p1[j] = mul4(gh, k[j] ? X[(size_t)rb[j] * L + lig] : z4());
                    p2[j] = mul4(th, k[j] ? T[(size_t)rb[j] * L + lig] : z4());
                }
                wa[j] = k[j] ? alpha[2 * (size_t)id[j] + a] : 0.f;
                wd[j] = k[j] ? c * dl[2 * (size_t)id[j] + a] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < MH_FLIGHT; ++j) {        // slots in list order
                if (k[j]) {
                    if constexpr (TAIL) {
                        acc1 = axpy4(wa[j], p1[j], acc1);
                        acc2 = axpy4(wd[j], p2[j], acc2);
                    } else {
                        acc1 = axpy4(wa[j], p1[j], axpy4(wd[j], p2[j], acc1));
                    }
                }
            }
        }
        if (item < ls.n_dest) {
            out1[(size_t)dest * L + lig] = acc1;
            if constexpr (TAIL) out2[(size_t)dest * L + lig] = acc2;
        } else {
            const size_t ch = (size_t)(item - ls.n_dest);
            part[(ch * W) * L + lig] = acc1;
            if constexpr (TAIL) part[(ch * W + 1) * L + lig] = acc2;
        }
    }
}

// one lane group per long destination: its W partial rows per chunk, in chunk order
template <int D, int W>
__global__ __launch_bounds__(MH_THREADS) void mh_sum_finish_kernel(const MhLong lg, const float4 *__restrict__ part, float4 *__restrict__ out1,
                                                                   float4 *__restrict__ out2) {
    constexpr int L = D / 4, RPB = MH_THREADS / L;
    const int lig = threadIdx.x % L;
    const long long j = (long long)blockIdx.x * RPB + threadIdx.x / L;
    if (j >= lg.n) return;
    const int c0 = lg.ptr[j], c1 = lg.ptr[j + 1], dest = lg.dest[j];
    float4 acc1 = z4(), acc2 = z4();
    for (int ch = c0; ch < c1; ++ch) {
        acc1 = add4(acc1, part[((size_t)ch * W) * L + lig]);
        if constexpr (W == 2) acc2 = add4(acc2, part[((size_t)ch * W + 1) * L + lig]);
    }
    out1[(size_t)dest * L + lig] = acc1;
    if constexpr (W == 2) out2[(size_t)dest * L + lig] = acc2;
}

// ---- rationale scores (norm_attn_computer): the mean of the two heads' logits, a softmax per head entity, times its kept degree ---------
// the scores of the kept slots [s0, s1) of one head entity from (m, z, cnt): the lanes of the group take the slots in turn.  Their mean
// needs no second sum: sum_e score_e = (cnt / z) sum_e exp(l_e - m) = (cnt / z) z, which mh_score_mean evaluates in this form, so the
// mean does not depend on where the slots that are not kept lie.
template <int L>
__device__ __forceinline__ void mh_write_scores(const MhList &ls, const int s0, const int s1, const int lig, const uint8_t *__restrict__ keep,
                                                const float *logit, const float m, const float z, const int cnt, float *__restrict__ score) {
    const float f = (float)cnt / z;
    for (int s = s0 + lig; s < s1; s += L) {
        const int id = ls.eid[s];
        if (keep == nullptr || keep[id] != 0) score[id] = expf(logit[id] - m) * f;
    }
}

__device__ __forceinline__ float mh_score_mean(const float z, const int cnt) { return cnt > 0 ? z * ((float)cnt / z) / (float)cnt : 0.f; }

// logit, score [E] by edge id (kept edges only: the caller zeroes them); mean_head [n_dest]; part_mz [n_chunks, 2]; part_cnt [n_chunks]
template <int D, bool RLDS>
__global__ __launch_bounds__(MH_THREADS) void mh_score_kernel(const MhList ls, const float4 *__restrict__ T, const float4 *__restrict__ R,
                                                              const int n_rel, const float c_half, const uint8_t *__restrict__ keep,
                                                              float *logit, float *__restrict__ score, float *__restrict__ mean_head,
                                                              float *__restrict__ part_mz, int32_t *__restrict__ part_cnt) {
    constexpr int L = D / 4, RPB = MH_THREADS / L;
    extern __shared__ float4 mh_rs[];
    if constexpr (RLDS) mh_stage<L>(mh_rs, R, n_rel);
    const int lig = threadIdx.x % L, grp = threadIdx.x / L;
    const long long items = (long long)ls.n_dest + ls.n_chunks;
    for (long long item = (long long)blockIdx.x * RPB + grp; item < items; item += (long long)gridDim.x * RPB) {
        int dest, s0, s1;
        if (!mh_item(ls, item, dest, s0, s1)) continue;
        const float4 th = T[(size_t)dest * L + lig];
        float m = -INFINITY, z = 0.f;
        int cnt = 0;
        for (int s = s0; s < s1; s += MH_FLIGHT) {
            bool k[MH_FLIGHT];
            int rt[MH_FLIGHT], rr[MH_FLIGHT], id[MH_FLIGHT];
#pragma unroll
            for (int j = 0; j < MH_FLIGHT; ++j) {
                const bool in = s + j < s1;
                id[j] = in ? ls.eid[s + j] : 0;
                rt[j] = in ? ls.ia[s + j] : 0;
                rr[j] = in ? ls.ib[s + j] : 0;
            }
#pragma unroll
            for (int j = 0; j < MH_FLIGHT; ++j) k[j] = s + j < s1 && (keep == nullptr || keep[id[j]] != 0);
            float lg[MH_FLIGHT];
#pragma unroll
            for (int j = 0; j < MH_FLIGHT; ++j) {
                float4 r;
                if constexpr (RLDS)
                    r = mh_rs[rr[j] * L + lig];
                else
                    r = k[j] ? R[(size_t)rr[j] * L + lig] : z4();
                const float4 tt = mul4(k[j] ? T[(size_t)rt[j] * L + lig] : z4(), r);
                lg[j] = c_half * group_sum<L>(dot4(th, tt));            // (l_0 + l_1) / 2: the sum over both halves times c / 2
            }
#pragma unroll
            for (int j = 0; j < MH_FLIGHT; ++j) {
                if (k[j]) {
                    const float lj = lg[j];
                    if (lig == 0) logit[id[j]] = lj;
                    if (lj > m) {
                        z *= expf(m - lj);
                        m = lj;
                    }
                    z += expf(lj - m);
                    ++cnt;
                }
            }
        }
        if (item < ls.n_dest) {
            if (cnt > 0) {
                __threadfence_block();                   // lane 0's logits of this walk are read by the other lanes of the group
                mh_write_scores<L>(ls, s0, s1, lig, keep, logit, m, z, cnt, score);
            }
            if (lig == 0) mean_head[dest] = mh_score_mean(z, cnt);
        } else if (lig == 0) {
            const size_t ch = (size_t)(item - ls.n_dest);
            part_mz[2 * ch] = m;
            part_mz[2 * ch + 1] = z;
            part_cnt[ch] = cnt;
        }
    }
}

// one lane group per long head entity: (m, z, cnt) of its chunks in chunk order, then the scores of all its slots
template <int D>
__global__ __launch_bounds__(MH_THREADS) void mh_score_finish_kernel(const MhList ls, const MhLong lg, const uint8_t *__restrict__ keep,
                                                                     const float *__restrict__ part_mz, const int32_t *__restrict__ part_cnt,
                                                                     const float *logit, float *__restrict__ score,
                                                                     float *__restrict__ mean_head) {
    constexpr int L = D / 4, RPB = MH_THREADS / L;
    const int lig = threadIdx.x % L;
    const long long j = (long long)blockIdx.x * RPB + threadIdx.x / L;
    if (j >= lg.n) return;
    const int c0 = lg.ptr[j], c1 = lg.ptr[j + 1], dest = lg.dest[j];
    float m = -INFINITY;
    for (int ch = c0; ch < c1; ++ch)
        if (part_cnt[ch] > 0) m = fmaxf(m, part_mz[2 * (size_t)ch]);
    float z = 0.f;
    int cnt = 0;
    for (int ch = c0; ch < c1; ++ch) {
        if (part_cnt[ch] > 0) {
            z = fmaf(part_mz[2 * (size_t)ch + 1], expf(part_mz[2 * (size_t)ch] - m), z);
            cnt += part_cnt[ch];
        }
    }
    if (cnt > 0) mh_write_scores<L>(ls, ls.ptr[dest], ls.ptr[dest + 1], lig, keep, logit, m, z, cnt, score);
    if (lig == 0) mean_head[dest] = mh_score_mean(z, cnt);
}

// the mean of the scores over the kept slots of each destination of a list (by tail): one thread per work item, slots in list order
__global__ __launch_bounds__(MH_THREADS) void mh_mean_kernel(const MhList ls, const uint8_t *__restrict__ keep, const float *__restrict__ score,
                                                             float *__restrict__ mean, float *__restrict__ part_sum,
                                                             int32_t *__restrict__ part_cnt) {
    const long long items = (long long)ls.n_dest + ls.n_chunks;
    for (long long item = (long long)blockIdx.x * MH_THREADS + threadIdx.x; item < items; item += (long long)gridDim.x * MH_THREADS) {
        int dest, s0, s1;
        if (!mh_item(ls, item, dest, s0, s1)) continue;
        float sum = 0.f;
        int cnt = 0;
        for (int s = s0; s < s1; ++s) {
            const int id = ls.eid[s];
            if (keep == nullptr || keep[id] != 0) {
                sum += score[id];
                ++cnt;
            }
        }
        if (item < ls.n_dest) {
            mean[dest] = cnt > 0 ? sum / (float)cnt : 0.f;
        } else {
            part_sum[item - ls.n_dest] = sum;
            part_cnt[item - ls.n_dest] = cnt;
        }
    }
}

__global__ __launch_bounds__(MH_THREADS) void mh_mean_finish_kernel(const MhLong lg, const float *__restrict__ part_sum,
                                                                    const int32_t *__restrict__ part_cnt, float *__restrict__ mean) {
    const long long j = (long long)blockIdx.x * MH_THREADS + threadIdx.x;
    if (j >= lg.n) return;
    float sum = 0.f;
    int cnt = 0;
    for (int ch = lg.ptr[j]; ch < lg.ptr[j + 1]; ++ch) {
        sum += part_sum[ch];
        cnt += part_cnt[ch];
    }
    mean[lg.dest[j]] = cnt > 0 ? sum / (float)cnt : 0.f;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
template <int D>
inline unsigned mh_blocks(long long items) {
    constexpr int RPB = MH_THREADS / (D / 4);
    const long long b = (items + RPB - 1) / RPB;
    return (unsigned)(b > MH_MAX_BLOCKS ? MH_MAX_BLOCKS : b);
}

template <int D>
inline unsigned mh_finish_blocks(int n_long) {
    constexpr int RPB = MH_THREADS / (D / 4);
    return (unsigned)((n_long + RPB - 1) / RPB);
}

inline float mh_scale(int d) { return 1.0f / sqrtf((float)(d / 2)); }

template <int D>
int mh_fwd(const MhList &ls, const MhLong &lg, const float *X, const float *T, const float *R, int n_rel, bool lds, const uint8_t *keep, float *Lg,
           float *M, float *Z, float *Y, float *part, float *part_mz, hipStream_t st) {
    const long long items = (long long)ls.n_dest + ls.n_chunks;
    const float c = mh_scale(D);
    if (items > 0) {
        if (lds)
            hipLaunchKernelGGL((mh_fwd_kernel<D, true>), dim3(mh_blocks<D>(items)), dim3(MH_THREADS), (size_t)n_rel * D * sizeof(float), st, ls,
                               (const float4 *)X, (const float4 *)T, (const float4 *)R, n_rel, c, keep, Lg, M, Z, (float4 *)Y, (float4 *)part,
                               part_mz);
        else
            hipLaunchKernelGGL((mh_fwd_kernel<D, false>), dim3(mh_blocks<D>(items)), dim3(MH_THREADS), 0, st, ls, (const float4 *)X,
                               (const float4 *)T, (const float4 *)R, n_rel, c, keep, Lg, M, Z, (float4 *)Y, (float4 *)part, part_mz);
    }
    if (lg.n > 0)
        hipLaunchKernelGGL((mh_fwd_finish_kernel<D>), dim3(mh_finish_blocks<D>(lg.n)), dim3(MH_THREADS), 0, st, lg, (const float4 *)part,
                           (const float *)part_mz, M, Z, (float4 *)Y);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

template <int D>
int mh_bwd_head(const MhList &ls, const MhLong &lg, const float *X, const float *T, const float *R, int n_rel, bool lds, const uint8_t *keep,
                const float *G, const float *Y, const float *Lg, const float *M, const float *Z, float *alpha, float *dl, float *dT, float *part,
                hipStream_t st) {
    const long long items = (long long)ls.n_dest + ls.n_chunks;
    const float c = mh_scale(D);
    if (items > 0) {
        if (lds)
            hipLaunchKernelGGL((mh_bwd_head_kernel<D, true>), dim3(mh_blocks<D>(items)), dim3(MH_THREADS), (size_t)n_rel * D * sizeof(float), st, ls,
                               (const float4 *)X, (const float4 *)T, (const float4 *)R, n_rel, c, keep, (const float4 *)G, (const float4 *)Y, Lg, M,
                               Z, alpha, dl, (float4 *)dT, (float4 *)part);
        else
            hipLaunchKernelGGL((mh_bwd_head_kernel<D, false>), dim3(mh_blocks<D>(items)), dim3(MH_THREADS), 0, st, ls, (const float4 *)X,
                               (const float4 *)T, (const float4 *)R, n_rel, c, keep, (const float4 *)G, (const float4 *)Y, Lg, M, Z, alpha, dl,
                               (float4 *)dT, (float4 *)part);
    }
    if (lg.n > 0)
        hipLaunchKernelGGL((mh_sum_finish_kernel<D, 1>), dim3(mh_finish_blocks<D>(lg.n)), dim3(MH_THREADS), 0, st, lg, (const float4 *)part,
                           (float4 *)dT, (float4 *)nullptr);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

template <int D, bool TAIL>
int mh_bwd_walk(const MhList &ls, const MhLong &lg, const float *G, const float *X, const float *T, const float *R, int n_rel, bool lds,
                const uint8_t *keep, const float *alpha, const float *dl, float *out1, float *out2, float *part, hipStream_t st) {
    const long long items = (long long)ls.n_dest + ls.n_chunks;
    const float c = mh_scale(D);
    if (items > 0) {
        if (TAIL && lds)
            hipLaunchKernelGGL((mh_bwd_walk_kernel<D, TAIL, true>), dim3(mh_blocks<D>(items)), dim3(MH_THREADS), (size_t)n_rel * D * sizeof(float),
                               st, ls, (const float4 *)G, (const float4 *)X, (const float4 *)T, (const float4 *)R, n_rel, c, keep, alpha, dl,
                               (float4 *)out1, (float4 *)out2, (float4 *)part);
        else
            hipLaunchKernelGGL((mh_bwd_walk_kernel<D, TAIL, false>), dim3(mh_blocks<D>(items)), dim3(MH_THREADS), 0, st, ls, (const float4 *)G,
                               (const float4 *)X, (const float4 *)T, (const float4 *)R, n_rel, c, keep, alpha, dl, (float4 *)out1, (float4 *)out2,
                               (float4 *)part);
    }
    if (lg.n > 0)
        hipLaunchKernelGGL((mh_sum_finish_kernel<D, TAIL ? 2 : 1>), dim3(mh_finish_blocks<D>(lg.n)), dim3(MH_THREADS), 0, st, lg,
                           (const float4 *)part, (float4 *)out1, (float4 *)out2);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

template <int D>
int mh_score(const MhList &ls, const MhLong &lg, const float *T, const float *R, int n_rel, bool lds, const uint8_t *keep, float *logit, float *score,
             float *mean_head, float *part_mz, int32_t *part_cnt, hipStream_t st) {
    const long long items = (long long)ls.n_dest + ls.n_chunks;
    const float c_half = 0.5f * mh_scale(D);
    if (items > 0) {
        if (lds)
            hipLaunchKernelGGL((mh_score_kernel<D, true>), dim3(mh_blocks<D>(items)), dim3(MH_THREADS), (size_t)n_rel * D * sizeof(float), st, ls,
                               (const float4 *)T, (const float4 *)R, n_rel, c_half, keep, logit, score, mean_head, part_mz, part_cnt);
        else
            hipLaunchKernelGGL((mh_score_kernel<D, false>), dim3(mh_blocks<D>(items)), dim3(MH_THREADS), 0, st, ls, (const float4 *)T,
                               (const float4 *)R, n_rel, c_half, keep, logit, score, mean_head, part_mz, part_cnt);
    }
    if (lg.n > 0)
        hipLaunchKernelGGL((mh_score_finish_kernel<D>), dim3(mh_finish_blocks<D>(lg.n)), dim3(MH_THREADS), 0, st, ls, lg, keep,
                           (const float *)part_mz, (const int32_t *)part_cnt, (const float *)logit, score, mean_head);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

// the checks every entry shares; `part` is needed exactly when the list has chunks
inline bool mh_list_ok(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                       const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest, const int32_t *long_ptr,
                       int32_t n_long, const void *part, int32_t d) {
    if (!ptr || n_dest < 1 || n_slots < 0 || n_slots >= 0x3fffffffLL || n_chunks < 0 || n_long < 0 || !mh_dim_ok(d)) return false;
    if (n_slots > 0 && (!ia || !ib || !eid)) return false;
    if ((n_chunks > 0) != (n_long > 0)) return false;
    if (n_chunks > 0 && (!chunk_dest || !chunk_begin || !long_dest || !long_ptr || !part || !mh_aligned(part))) return false;
    return true;
}

inline bool mh_lds(int32_t n_rows, int32_t d) { return (size_t)n_rows * d * sizeof(float) <= (size_t)MH_LDS_BYTES; }

#define MH_SWITCH(d, CALL32, CALL64, CALL128) \
    switch (d) {                              \
    case 32: return CALL32;                   \
    case 64: return CALL64;                   \
    default: return CALL128;                  \
    }

}      // namespace

extern "C" {

int sslrec_rmha_fwd_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                        const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest, const int32_t *long_ptr,
                        int32_t n_long, const float *X, const float *T, const float *R, int32_t n_rel, int32_t d, const uint8_t *keep, float *Lg,
                        float *M, float *Z, float *Y, float *part, float *part_mz, void *stream) {
    if (!mh_list_ok(ptr, ia, ib, eid, n_dest, n_slots, chunk_dest, chunk_begin, n_chunks, long_dest, long_ptr, n_long, part, d))
        return SSLREC_E_BADARG;
    if (!X || !T || !R || !M || !Z || !Y || n_rel < 1 || (n_slots > 0 && !Lg) || (n_chunks > 0 && !part_mz)) return SSLREC_E_BADARG;
    if (!mh_aligned(X) || !mh_aligned(T) || !mh_aligned(R) || !mh_aligned(Y)) return SSLREC_E_BADARG;
    const MhList ls = {ptr, ia, ib, eid, chunk_dest, chunk_begin, n_dest, n_chunks};
    const MhLong lg = {long_dest, long_ptr, n_long};
    const bool lds = mh_lds(n_rel, d);
    hipStream_t st = (hipStream_t)stream;
#define MH_CALL(D) mh_fwd<D>(ls, lg, X, T, R, n_rel, lds, keep, Lg, M, Z, Y, part, part_mz, st)
    MH_SWITCH(d, MH_CALL(32), MH_CALL(64), MH_CALL(128))
#undef MH_CALL
}

int sslrec_rmha_bwd_head_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                             const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest,
                             const int32_t *long_ptr, int32_t n_long, const float *X, const float *T, const float *R, int32_t n_rel, int32_t d,
                             const uint8_t *keep, const float *G, const float *Y, const float *Lg, const float *M, const float *Z, float *alpha,
                             float *dl, float *dT, float *part, void *stream) {
    if (!mh_list_ok(ptr, ia, ib, eid, n_dest, n_slots, chunk_dest, chunk_begin, n_chunks, long_dest, long_ptr, n_long, part, d))
        return SSLREC_E_BADARG;
    if (!X || !T || !R || !G || !Y || !M || !Z || !dT || n_rel < 1 || (n_slots > 0 && (!Lg || !alpha || !dl))) return SSLREC_E_BADARG;
    if (!mh_aligned(X) || !mh_aligned(T) || !mh_aligned(R) || !mh_aligned(G) || !mh_aligned(Y) || !mh_aligned(dT)) return SSLREC_E_BADARG;
    const MhList ls = {ptr, ia, ib, eid, chunk_dest, chunk_begin, n_dest, n_chunks};
    const MhLong lg = {long_dest, long_ptr, n_long};
    const bool lds = mh_lds(n_rel, d);
    hipStream_t st = (hipStream_t)stream;
#define MH_CALL(D) mh_bwd_head<D>(ls, lg, X, T, R, n_rel, lds, keep, G, Y, Lg, M, Z, alpha, dl, dT, part, st)
    MH_SWITCH(d, MH_CALL(32), MH_CALL(64), MH_CALL(128))
#undef MH_CALL
}

int sslrec_rmha_bwd_tail_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                             const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest,
                             const int32_t *long_ptr, int32_t n_long, const float *G, const float *T, const float *R, int32_t n_rel, int32_t d,
                             const uint8_t *keep, const float *alpha, const float *dl, float *dX, float *dT, float *part, void *stream) {
    if (!mh_list_ok(ptr, ia, ib, eid, n_dest, n_slots, chunk_dest, chunk_begin, n_chunks, long_dest, long_ptr, n_long, part, d))
        return SSLREC_E_BADARG;
    if (!G || !T || !R || !dX || !dT || n_rel < 1 || (n_slots > 0 && (!alpha || !dl))) return SSLREC_E_BADARG;
    if (!mh_aligned(G) || !mh_aligned(T) || !mh_aligned(R) || !mh_aligned(dX) || !mh_aligned(dT)) return SSLREC_E_BADARG;
    const MhList ls = {ptr, ia, ib, eid, chunk_dest, chunk_begin, n_dest, n_chunks};
    const MhLong lg = {long_dest, long_ptr, n_long};
    const bool lds = mh_lds(n_rel, d);
    hipStream_t st = (hipStream_t)stream;
#define MH_CALL(D) mh_bwd_walk<D, true>(ls, lg, G, (const float *)nullptr, T, R, n_rel, lds, keep, alpha, dl, dX, dT, part, st)
    MH_SWITCH(d, MH_CALL(32), MH_CALL(64), MH_CALL(128))
#undef MH_CALL
}

int sslrec_rmha_bwd_rel_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                            const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest,
                            const int32_t *long_ptr, int32_t n_long, const float *G, const float *X, const float *T, int32_t d, const uint8_t *keep,
                            const float *alpha, const float *dl, float *dR, float *part, void *stream) {
    if (!mh_list_ok(ptr, ia, ib, eid, n_dest, n_slots, chunk_dest, chunk_begin, n_chunks, long_dest, long_ptr, n_long, part, d))
        return SSLREC_E_BADARG;
    if (!G || !X || !T || !dR || (n_slots > 0 && (!alpha || !dl))) return SSLREC_E_BADARG;
    if (!mh_aligned(G) || !mh_aligned(X) || !mh_aligned(T) || !mh_aligned(dR)) return SSLREC_E_BADARG;
    const MhList ls = {ptr, ia, ib, eid, chunk_dest, chunk_begin, n_dest, n_chunks};
    const MhLong lg = {long_dest, long_ptr, n_long};
    hipStream_t st = (hipStream_t)stream;
#define MH_CALL(D) mh_bwd_walk<D, false>(ls, lg, G, X, T, (const float *)nullptr, 0, false, keep, alpha, dl, dR, (float *)nullptr, part, st)
    MH_SWITCH(d, MH_CALL(32), MH_CALL(64), MH_CALL(128))
#undef MH_CALL
}

int sslrec_rmha_score_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                          const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest,
                          const int32_t *long_ptr, int32_t n_long, const float *T, const float *R, int32_t n_rel, int32_t d, const uint8_t *keep,
                          float *logit, float *score, float *mean_head, float *part_mz, int32_t *part_cnt, void *stream) {
    if (!ptr || n_dest < 1 || n_slots < 0 || n_slots >= 0x3fffffffLL || n_chunks < 0 || n_long < 0 || !mh_dim_ok(d)) return SSLREC_E_BADARG;
    if (n_slots > 0 && (!ia || !ib || !eid || !logit || !score)) return SSLREC_E_BADARG;
    if ((n_chunks > 0) != (n_long > 0)) return SSLREC_E_BADARG;
    if (n_chunks > 0 && (!chunk_dest || !chunk_begin || !long_dest || !long_ptr || !part_mz || !part_cnt)) return SSLREC_E_BADARG;
    if (!T || !R || !mean_head || n_rel < 1 || !mh_aligned(T) || !mh_aligned(R)) return SSLREC_E_BADARG;
    const MhList ls = {ptr, ia, ib, eid, chunk_dest, chunk_begin, n_dest, n_chunks};
    const MhLong lg = {long_dest, long_ptr, n_long};
    const bool lds = mh_lds(n_rel, d);
    hipStream_t st = (hipStream_t)stream;
#define MH_CALL(D) mh_score<D>(ls, lg, T, R, n_rel, lds, keep, logit, score, mean_head, part_mz, part_cnt, st)
    MH_SWITCH(d, MH_CALL(32), MH_CALL(64), MH_CALL(128))
#undef MH_CALL
}

int sslrec_rmha_mean_f32(const int32_t *ptr, const int32_t *ia, const int32_t *ib, const int32_t *eid, int32_t n_dest, int64_t n_slots,
                         const int32_t *chunk_dest, const int32_t *chunk_begin, int32_t n_chunks, const int32_t *long_dest, const int32_t *long_ptr,
                         int32_t n_long, const uint8_t *keep, const float *score, float *mean, float *part_sum, int32_t *part_cnt, void *stream) {
    (void)ia;
    (void)ib;
    if (!ptr || n_dest < 1 || n_slots < 0 || n_slots >= 0x3fffffffLL || n_chunks < 0 || n_long < 0 || !mean) return SSLREC_E_BADARG;
    if (n_slots > 0 && (!eid || !score)) return SSLREC_E_BADARG;
    if ((n_chunks > 0) != (n_long > 0)) return SSLREC_E_BADARG;
    if (n_chunks > 0 && (!chunk_dest || !chunk_begin || !long_dest || !long_ptr || !part_sum || !part_cnt)) return SSLREC_E_BADARG;
    const MhList ls = {ptr, ia, ib, eid, chunk_dest, chunk_begin, n_dest, n_chunks};
    const MhLong lg = {long_dest, long_ptr, n_long};
    hipStream_t st = (hipStream_t)stream;
    const long long items = (long long)n_dest + n_chunks;
    const long long b = (items + MH_THREADS - 1) / MH_THREADS;
    hipLaunchKernelGGL(mh_mean_kernel, dim3((unsigned)(b > MH_MAX_BLOCKS ? MH_MAX_BLOCKS : b)), dim3(MH_THREADS), 0, st, ls, keep, score, mean,
                       part_sum, part_cnt);
    if (n_long > 0)
        hipLaunchKernelGGL(mh_mean_finish_kernel, dim3((unsigned)((n_long + MH_THREADS - 1) / MH_THREADS)), dim3(MH_THREADS), 0, st, lg,
                           (const float *)part_sum, (const int32_t *)part_cnt, mean);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

}      // extern "C"
