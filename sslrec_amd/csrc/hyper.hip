// Hypergraph layer of HCCF (reference models/general_cf/hccf.py:43-44, 48-49, 105-107) on the stacked tables [users; items]:
//   A = dropout(E_r W * mult, p = 1 - keep_rate)   [rows, K]      W = W_u for rows [0, n_split), W_i for rows [n_split, N), [d, K] row-major
//   H = act(A^T X_r)                               [K, d]         act = LeakyReLU(leaky), one H per row range
//   Y = act(A H)                                   [rows, d]
// forward and backward for both row ranges per launch, without anything of size N x K in global memory: A is recomputed from E, W and
// the dropout mask wherever it is needed, and the mask is computed, never stored.
//
// Dropout.  keep(row, k) = floor(u + keep_rate) != 0 with u the Philox uniform (philox.h) of element
//       index = row * 4 ceil(K / 4) + k            (row = the row of the STACKED table, so both ranges share one call's stream)
// of call `philox_stream` at the state's current step: philox_uniform4(row * ceil(K / 4) + k / 4) holds the four consecutive k a lane has
// in registers 4 q .. 4 q + 3 of an accumulator block (k = 32 kb + 8 q + 4 half + j).  A kept element is scaled by mult / keep_rate.
// Every kernel below recomputes the same bits, so both uses of A in the forward and the backward agree.  keep_rate == 1 (philox_state
// == NULL) draws nothing.
//
// Layout and helpers: rowtile.h (4-wave workgroups that belong to one row range, transposed exact-fp32 32x32x2 MFMAs, slabs).  H, dH
// and dW are [d, K]-sized sums over rows and go through per-workgroup slabs that a small kernel adds in a fixed order: no atomics, two
// runs give the same bits.  H and dQ are kept TRANSPOSED, [d, K] row-major like W, so all three load into LDS the same way.
//
//   forward   1. hyper_slab_kernel<.., 0>: slab = X^T A                     -> hyper_reduce_kernel: Ht = act(sum)
//             2. hyper_y_kernel:           Y = act(A H)                     (W and Ht in LDS)
//   backward  1. hyper_slab_kernel<.., 1>: slab = dP^T A, dP = dY act'(Y)   -> hyper_reduce_kernel: dQt = sum * act'(Ht)
//             2. hyper_grad_kernel:        dA = dP H^T + X dQ^T,  dZ = dA * mask * mult / keep_rate,
//                                          dX = A dQ,  dE = dZ W^T,  slab = E^T dZ   -> hyper_reduce_kernel: dW = sum
// act' comes from the sign of the saved output (the slope is positive; at exactly 0 it is `leaky`, as in torch).
// Step 2 of the backward needs W, Ht and dQt.  Where the three do not fit the 160 KB of LDS together (d = 128 with K > 64, d = 64 with
// K > 128) it runs as TWO launches of two matrices each -- dZ is linear in dA: TERM 1 takes dA = dP H^T (W, Ht), TERM 2 takes
// dA = X dQ^T (W, dQt), writes dX and ADDS its share to dE; their slabs are summed together.  d = 128 with K > 128 does not fit even
// two and is refused.
#include "common.h"
#include "philox.h"
#include "rowtile.h"

namespace {

constexpr int HY_CAP = 256;                      // workgroups per row range at most: one [d, K] slab of the workspace each
constexpr size_t HY_LDS_MAX = 160 * 1024;
constexpr int HY_TILE_FLOATS = IN_WAVES * 32 * IN_TSTRIDE;

struct HyDrop {
    const uint64_t *state;                       // NULL: keep everything
    uint32_t stream;
    float keep, scale;                           // keep_rate, mult / keep_rate
    int kq;                                      // ceil(K / 4): float4 groups per row of the mask
};

template <int D, int KB> struct HyCfg {
    using In = InCfg<D, KB>;
    static constexpr int C = In::C_FLOATS;
    static constexpr size_t SLAB_LDS = In::BWD_LDS;
    static constexpr size_t Y_LDS = (size_t)2 * C * 4;
    static constexpr size_t grad_lds(int mats) {
        return (size_t)((mats * C > In::RED_FLOATS ? mats * C : In::RED_FLOATS) + HY_TILE_FLOATS) * 4;
    }
    static constexpr bool SPLIT = grad_lds(3) > HY_LDS_MAX;
    static constexpr bool FITS = grad_lds(2) <= HY_LDS_MAX && Y_LDS <= HY_LDS_MAX;
};

__device__ __forceinline__ float hy_act(float x, float leaky) { return x > 0.f ? x : x * leaky; }
__device__ __forceinline__ float hy_slope(float y, float leaky) { return y > 0.f ? 1.f : leaky; }

// bit r of bits[kb]: element (row, k(kb, r, half)) is kept
template <int KB>
__device__ __forceinline__ void hy_keep_bits(const HyDrop &dr, const PhiloxKey &key, long long row, int half, int K, uint32_t (&bits)[KB]) {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
        uint32_t b = 0xffffu;
        if (dr.state) {
            b = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k0 = kb * 32 + 8 * q + 4 * half;
                if (k0 < K) {
                    const float4 u = philox_uniform4(key, (uint64_t)row * (uint64_t)dr.kq + (uint64_t)(k0 >> 2), dr.stream);
                    b |= (floorf(u.x + dr.keep) != 0.f ? 1u : 0u) << (4 * q);
                    b |= (floorf(u.y + dr.keep) != 0.f ? 1u : 0u) << (4 * q + 1);
                    b |= (floorf(u.z + dr.keep) != 0.f ? 1u : 0u) << (4 * q + 2);
                    b |= (floorf(u.w + dr.keep) != 0.f ? 1u : 0u) << (4 * q + 3);
                }
            }
        }
        bits[kb] = b;
    }
}

template <int KB>
__device__ __forceinline__ void hy_apply(in_f32x16 (&z)[KB], const uint32_t (&bits)[KB], float scale) {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) z[kb][r] = ((bits[kb] >> r) & 1u) ? z[kb][r] * scale : 0.f;
}

// this lane's half of row `row` of dP = dY * act'(Y)
template <int D>
__device__ __forceinline__ void hy_load_dp_half_row(const float *__restrict__ dY, const float *__restrict__ Y, long long row, bool valid,
                                                    int half, float leaky, float (&v)[D / 2]) {
    float y[D / 2];
    in_load_half_row<D>(dY, row, valid, half, v);
    in_load_half_row<D>(Y, row, valid, half, y);
#pragma unroll
    for (int j = 0; j < D / 2; ++j) v[j] *= hy_slope(y[j], leaky);
}

// out[row, :] = / act of / += sum_k W[row, k] C[:, k]       EPI 0: store, 1: LeakyReLU then store, 2: add to what is there
template <int D, int KB, int EPI>
__device__ __forceinline__ void hy_project(const float *lds, const in_f32x16 (&w)[KB], int l32, int half, float *__restrict__ out, long long row,
                                           bool valid, float leaky) {
#pragma unroll
    for (int ib = 0; ib < D / 32; ++ib) {
        const in_f32x16 y = in_project_block<D, KB>(lds, w, ib, l32, half);
        if (valid) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                in_f32x4 *at = reinterpret_cast<in_f32x4 *>(out + (size_t)row * D + ib * 32 + 8 * q + 4 * half);
                in_f32x4 o = {y[4 * q], y[4 * q + 1], y[4 * q + 2], y[4 * q + 3]};
                if constexpr (EPI == 1) {
                    o.x = hy_act(o.x, leaky); o.y = hy_act(o.y, leaky); o.z = hy_act(o.z, leaky); o.w = hy_act(o.w, leaky);
                }
                if constexpr (EPI == 2) o += *at;
                *at = o;
            }
        }
    }
}

// slab[i, k] = sum over the workgroup's rows of T[row, i] A[row, k];  MODE 0: T = X (-> H),  MODE 1: T = dP = dY act'(Y) (-> dH)
template <int D, int KB, int MODE>
__global__ __launch_bounds__(256) void hyper_slab_kernel(const float *__restrict__ E, const float *__restrict__ T, const float *__restrict__ Yact,
                                                         int N, int n_split, const float *__restrict__ W_u, const float *__restrict__ W_i, int K,
                                                         int G_u, HyDrop dr, float leaky, float *__restrict__ ws) {
    using Cfg = InCfg<D, KB>;
    constexpr int DC = Cfg::DC, KP = KB * 32;
    extern __shared__ float in_lds[];
    const InRange rg = in_range(W_u, W_i, N, n_split, G_u);
    in_load_c<D, KB>(in_lds, rg.C, K);
    const int lane = threadIdx.x & 63, l32 = lane & 31, half = lane >> 5, wave = wave_in_block();
    const int chunk = blockIdx.y;
    float *tile = in_lds + Cfg::BWD_MAIN + wave * (32 * IN_TSTRIDE);
    PhiloxKey key = {0, 0, 0};
    if (dr.state) key = philox_load(dr.state);
    in_f32x16 dc[DC][KB];
#pragma unroll
    for (int a = 0; a < DC; ++a)
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) dc[a][kb][r] = 0.f;
    const int tiles = (rg.hi - rg.lo + 31) / 32;
    for (int t = rg.g * IN_WAVES + wave; t < tiles; t += rg.G * IN_WAVES) {
        const long long row0 = (long long)rg.lo + (long long)t * 32, row = row0 + l32;
        const bool valid = row < rg.hi;
        in_f32x16 a_[KB];
        {
            float eb[D / 2];
            in_load_half_row<D>(E, row, valid, half, eb);
            in_logits<D, KB>(in_lds, eb, l32, half, a_);
            uint32_t bits[KB];
            hy_keep_bits<KB>(dr, key, row, half, K, bits);
            hy_apply<KB>(a_, bits, dr.scale);
        }
        float ta[DC][16];
#pragma unroll
        for (int a = 0; a < DC; ++a)
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const long long rr = row0 + 2 * s + half;
                const size_t at = (size_t)rr * D + (chunk * DC + a) * 32 + l32;
                const bool ok = rr < rg.hi;
                float v = ok ? T[at] : 0.f;
                if constexpr (MODE == 1) v *= hy_slope(ok ? Yact[at] : 0.f, leaky);
                ta[a][s] = v;
            }
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) in_rowsum_block<DC, KB>(tile, a_[kb], ta, l32, half, dc, kb);
    }
    in_slab_store<D, KB>(in_lds, dc, chunk, ws + (size_t)blockIdx.x * (D * KP));
}

// Y = act(A H)
template <int D, int KB>
__global__ __launch_bounds__(256) void hyper_y_kernel(const float *__restrict__ E, int N, int n_split, const float *__restrict__ W_u,
                                                      const float *__restrict__ W_i, const float *__restrict__ Ht_u,
                                                      const float *__restrict__ Ht_i, int K, int G_u, HyDrop dr, float leaky,
                                                      float *__restrict__ Y) {
    constexpr int C = InCfg<D, KB>::C_FLOATS;
    extern __shared__ float in_lds[];
    const InRange rg = in_range(W_u, W_i, N, n_split, G_u);
    in_load_c<D, KB>(in_lds, rg.C, K);
    in_load_c<D, KB>(in_lds + C, (int)blockIdx.x < G_u ? Ht_u : Ht_i, K);
    const int lane = threadIdx.x & 63, l32 = lane & 31, half = lane >> 5, wave = wave_in_block();
    PhiloxKey key = {0, 0, 0};
    if (dr.state) key = philox_load(dr.state);
    const int tiles = (rg.hi - rg.lo + 31) / 32;
    for (int t = rg.g * IN_WAVES + wave; t < tiles; t += rg.G * IN_WAVES) {
        const long long row = (long long)rg.lo + (long long)t * 32 + l32;
        const bool valid = row < rg.hi;
        float eb[D / 2];
        in_load_half_row<D>(E, row, valid, half, eb);
        in_f32x16 a_[KB];
        in_logits<D, KB>(in_lds, eb, l32, half, a_);
        uint32_t bits[KB];
        hy_keep_bits<KB>(dr, key, row, half, K, bits);
        hy_apply<KB>(a_, bits, dr.scale);
        hy_project<D, KB, 1>(in_lds + C, a_, l32, half, Y, row, valid, leaky);
    }
}

// TERM 0: everything;  TERM 1: the dP H^T share of dA (dE stored, no dX);  TERM 2: the X dQ^T share (dX stored, dE added to)
template <int D, int KB, int TERM>
__global__ __launch_bounds__(256) void hyper_grad_kernel(const float *__restrict__ E, const float *__restrict__ X, const float *__restrict__ dY,
                                                         const float *__restrict__ Yact, int N, int n_split, const float *__restrict__ W_u,
                                                         const float *__restrict__ W_i, const float *__restrict__ Ht_u,
                                                         const float *__restrict__ Ht_i, const float *__restrict__ dQt_u,
                                                         const float *__restrict__ dQt_i, int K, int G_u, HyDrop dr, float leaky,
                                                         float *__restrict__ dX, float *__restrict__ dE, float *__restrict__ ws) {
    using Cfg = InCfg<D, KB>;
    constexpr int DC = Cfg::DC, KP = KB * 32, C = Cfg::C_FLOATS, MATS = TERM == 0 ? 3 : 2;
    constexpr int MAIN = MATS * C > Cfg::RED_FLOATS ? MATS * C : Cfg::RED_FLOATS;
    extern __shared__ float in_lds[];
    const InRange rg = in_range(W_u, W_i, N, n_split, G_u);
    const bool users = (int)blockIdx.x < G_u;
    const float *ldsW = in_lds, *ldsH = in_lds + C, *ldsQ = in_lds + (TERM == 0 ? 2 * C : C);
    in_load_c<D, KB>(in_lds, rg.C, K);
    if constexpr (TERM != 2) in_load_c<D, KB>(in_lds + C, users ? Ht_u : Ht_i, K);
    if constexpr (TERM != 1) in_load_c<D, KB>(in_lds + (TERM == 0 ? 2 * C : C), users ? dQt_u : dQt_i, K);
    const int lane = threadIdx.x & 63, l32 = lane & 31, half = lane >> 5, wave = wave_in_block();
    const int chunk = blockIdx.y;                              // which DC row blocks of dW this workgroup sums; chunk 0 also writes dX and dE
    float *tile = in_lds + MAIN + wave * (32 * IN_TSTRIDE);
    PhiloxKey key = {0, 0, 0};
    if (dr.state) key = philox_load(dr.state);
    in_f32x16 dc[DC][KB];
#pragma unroll
    for (int a = 0; a < DC; ++a)
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) dc[a][kb][r] = 0.f;
    const int tiles = (rg.hi - rg.lo + 31) / 32;
    for (int t = rg.g * IN_WAVES + wave; t < tiles; t += rg.G * IN_WAVES) {
        const long long row0 = (long long)rg.lo + (long long)t * 32, row = row0 + l32;
        const bool valid = row < rg.hi;
        uint32_t bits[KB];
        hy_keep_bits<KB>(dr, key, row, half, K, bits);
        in_f32x16 dz[KB];
        if constexpr (TERM != 2) {
            float gp[D / 2];
            hy_load_dp_half_row<D>(dY, Yact, row, valid, half, leaky, gp);
            in_logits<D, KB>(ldsH, gp, l32, half, dz);                            // dP H^T
        }
        if constexpr (TERM != 1) {
            float xb[D / 2];
            in_load_half_row<D>(X, row, valid, half, xb);
            in_logits<D, KB, TERM == 2>(ldsQ, xb, l32, half, dz);                 // (+) X dQ^T
        }
        hy_apply<KB>(dz, bits, dr.scale);
        if (chunk == 0) {
            if constexpr (TERM != 1) {
                float eb[D / 2];
                in_load_half_row<D>(E, row, valid, half, eb);
                in_f32x16 a_[KB];
                in_logits<D, KB>(ldsW, eb, l32, half, a_);
                hy_apply<KB>(a_, bits, dr.scale);
                hy_project<D, KB, 0>(ldsQ, a_, l32, half, dX, row, valid, leaky);     // dX = A dQ
            }
            hy_project<D, KB, TERM == 2 ? 2 : 0>(ldsW, dz, l32, half, dE, row, valid, leaky);      // dE (+)= dZ W^T
        }
        float ta[DC][16];
#pragma unroll
        for (int a = 0; a < DC; ++a)
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const long long rr = row0 + 2 * s + half;
                ta[a][s] = rr < rg.hi ? E[(size_t)rr * D + (chunk * DC + a) * 32 + l32] : 0.f;
            }
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) in_rowsum_block<DC, KB>(tile, dz[kb], ta, l32, half, dc, kb);
    }
    in_slab_store<D, KB>(in_lds, dc, chunk, ws + (size_t)blockIdx.x * (D * KP));
}

// out[i, k] = f(sum over the range's slabs in index order, set after set; four interleaved partial sums combined in a fixed order)
//   mode 0: f = act(s)      mode 1: f = s * act'(ref[i, k])      mode 2: f = s
__global__ __launch_bounds__(256) void hyper_reduce_kernel(const float *__restrict__ ws, int G_u, int G_i, int n_sets, size_t set_stride, int d,
                                                           int K, int KP, int mode, float leaky, const float *__restrict__ ref_u,
                                                           const float *__restrict__ ref_i, float *__restrict__ out_u,
                                                           float *__restrict__ out_i) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= d * K) return;
    const int which = blockIdx.y;
    float *out = which == 0 ? out_u : out_i;
    if (!out) return;
    const float *ref = which == 0 ? ref_u : ref_i;
    const int g0 = which == 0 ? 0 : G_u, G = which == 0 ? G_u : G_i;
    const int i = e / K, k = e - i * K;
    const size_t step = (size_t)d * KP;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int set = 0; set < n_sets; ++set) {
        const float *src = ws + (size_t)set * set_stride + (size_t)g0 * step + (size_t)i * KP + k;
        int g = 0;
        for (; g + 4 <= G; g += 4) {
            s0 += src[(size_t)g * step];
            s1 += src[(size_t)(g + 1) * step];
            s2 += src[(size_t)(g + 2) * step];
            s3 += src[(size_t)(g + 3) * step];
        }
        for (; g < G; ++g) s0 += src[(size_t)g * step];
    }
    float s = (s0 + s1) + (s2 + s3);
    if (mode == 0) s = hy_act(s, leaky);
    if (mode == 1) s = (G > 0 && ref) ? s * hy_slope(ref[e], leaky) : 0.f;
    out[e] = s;
}

inline bool hy_shape_ok(int d, int K) {
    if ((d != 32 && d != 64 && d != 128) || K < 1 || K > 256) return false;
    return !(d == 128 && K > 128);                            // HyCfg<128, 8>::FITS is false
}

inline bool hy_args_ok(int64_t N, int64_t n_split, int d, int K, const void *W_u, const void *W_i, float leaky, float keep_rate,
                       const void *philox_state) {
    if (N < 0 || N > 0x7fffffff || n_split < 0 || n_split > N || !hy_shape_ok(d, K)) return false;
    if (!(leaky > 0.f) || !(keep_rate > 0.f) || !(keep_rate <= 1.f)) return false;
    if (keep_rate < 1.f && !philox_state) return false;
    if (n_split > 0 && !W_u) return false;
    if (n_split < N && !W_i) return false;
    return true;
}

inline HyDrop hy_drop(const uint64_t *state, uint32_t stream, float mult, float keep_rate, int K) {
    HyDrop dr;
    dr.state = keep_rate < 1.f ? state : nullptr;
    dr.stream = stream;
    dr.keep = keep_rate;
    dr.scale = mult / keep_rate;
    dr.kq = (K + 3) / 4;
    return dr;
}

template <typename Kern>
inline hipError_t hy_allow_lds(Kern kern, size_t lds) {
    if (lds <= 65536) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

#define SSLREC_HYPER_DISPATCH(d, kb, CALL)                                                            \
    switch ((d) * 16 + (kb)) {                                                                        \
    case 32 * 16 + 1: CALL(32, 1); break;                                                             \
    case 32 * 16 + 2: CALL(32, 2); break;                                                             \
    case 32 * 16 + 4: CALL(32, 4); break;                                                             \
    case 32 * 16 + 8: CALL(32, 8); break;                                                             \
    case 64 * 16 + 1: CALL(64, 1); break;                                                             \
    case 64 * 16 + 2: CALL(64, 2); break;                                                             \
    case 64 * 16 + 4: CALL(64, 4); break;                                                             \
    case 64 * 16 + 8: CALL(64, 8); break;                                                             \
    case 128 * 16 + 1: CALL(128, 1); break;                                                           \
    case 128 * 16 + 2: CALL(128, 2); break;                                                           \
    case 128 * 16 + 4: CALL(128, 4); break;                                                           \
    default: return SSLREC_E_BADARG;                                                                  \
    }

static_assert(HyCfg<128, 4>::FITS && HyCfg<64, 8>::FITS && !HyCfg<128, 8>::FITS, "hy_shape_ok must agree with the LDS budget");

struct HyWs {
    size_t set_stride;                           // floats of one set of slabs
    float *slabs, *dQ_u, *dQ_i;
};

inline size_t hy_ws_floats(int64_t N, int64_t n_split, int d, int K) {
    const size_t G = (size_t)in_groups(n_split, HY_CAP) + (size_t)in_groups(N - n_split, HY_CAP);
    return 2 * G * (size_t)d * (size_t)(in_kb(K) * 32) + 2 * (size_t)d * (size_t)K;
}

inline HyWs hy_ws(void *ws, int64_t N, int64_t n_split, int d, int K) {
    const size_t G = (size_t)in_groups(n_split, HY_CAP) + (size_t)in_groups(N - n_split, HY_CAP);
    HyWs w;
    w.set_stride = G * (size_t)d * (size_t)(in_kb(K) * 32);
    w.slabs = (float *)ws;
    w.dQ_u = w.slabs + 2 * w.set_stride;
    w.dQ_i = w.dQ_u + (size_t)d * K;
    return w;
}

template <int D, int KB, int TERM>
inline int hy_grad_term(hipStream_t st, const float *E, const float *X, const float *dY, const float *Y, int N, int n_split, const float *W_u,
                        const float *W_i, const float *H_u, const float *H_i, int K, int G_u, int G_i, const HyDrop &dr, float leaky, float *dX,
                        float *dE, const HyWs &w, float *slabs) {
    constexpr size_t lds = HyCfg<D, KB>::grad_lds(TERM == 0 ? 3 : 2);
    hipError_t e = hy_allow_lds(hyper_grad_kernel<D, KB, TERM>, lds);
    if (e != hipSuccess) return (int)e;
    constexpr unsigned chunks = InCfg<D, KB>::CHUNKS;
    hipLaunchKernelGGL((hyper_grad_kernel<D, KB, TERM>), dim3((unsigned)(G_u + G_i), chunks), dim3(IN_WAVES * 64), lds, st,
                       E, X, dY, Y, N, n_split, W_u, W_i, H_u, H_i, (const float *)w.dQ_u, (const float *)w.dQ_i, K, G_u, dr, leaky, dX, dE, slabs);
    return 0;
}

// step 2 of the backward: one launch where W, Ht and dQt fit LDS together, else the two terms of dA one after the other
template <int D, int KB>
inline int hy_grad_launch(hipStream_t st, const float *E, const float *X, const float *dY, const float *Y, int N, int n_split, const float *W_u,
                          const float *W_i, const float *H_u, const float *H_i, int K, int G_u, int G_i, const HyDrop &dr, float leaky,
                          float *dX, float *dE, const HyWs &w, int *n_sets) {
    if constexpr (HyCfg<D, KB>::SPLIT) {
        *n_sets = 2;
        const int rc = hy_grad_term<D, KB, 1>(st, E, X, dY, Y, N, n_split, W_u, W_i, H_u, H_i, K, G_u, G_i, dr, leaky, dX, dE, w, w.slabs);
        if (rc != 0) return rc;
        return hy_grad_term<D, KB, 2>(st, E, X, dY, Y, N, n_split, W_u, W_i, H_u, H_i, K, G_u, G_i, dr, leaky, dX, dE, w, w.slabs + w.set_stride);
    } else {
        *n_sets = 1;
        return hy_grad_term<D, KB, 0>(st, E, X, dY, Y, N, n_split, W_u, W_i, H_u, H_i, K, G_u, G_i, dr, leaky, dX, dE, w, w.slabs);
    }
}

}      // namespace

extern "C" {

size_t sslrec_hyper_ws_bytes(int32_t N, int32_t n_split, int32_t d, int32_t K) {
    if (N < 0 || n_split < 0 || n_split > N || !hy_shape_ok(d, K)) return 0;
    return hy_ws_floats(N, n_split, d, K) * sizeof(float);
}

int sslrec_hyper_fwd_f32(const float *X, const float *E, int32_t N, int32_t n_split, int32_t d, const float *W_u, const float *W_i, int32_t K,
                         float mult, float leaky, float keep_rate, const uint64_t *philox_state, uint32_t philox_stream, float *H_u,
                         float *H_i, float *Y, void *ws, void *stream) {
    if (!hy_args_ok(N, n_split, d, K, W_u, W_i, leaky, keep_rate, philox_state) || !X || !E || !Y) return SSLREC_E_BADARG;
    if ((n_split > 0 && !H_u) || (n_split < N && !H_i) || (N > 0 && !ws)) return SSLREC_E_BADARG;
    if (N == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int G_u = in_groups(n_split, HY_CAP), G_i = in_groups((long long)N - n_split, HY_CAP);
    const int kb = in_kb(K);
    const HyDrop dr = hy_drop(philox_state, philox_stream, mult, keep_rate, K);
    const HyWs w = hy_ws(ws, N, n_split, d, K);
#define CALL(D, KB)                                                                                                                       \
    {                                                                                                                                     \
        constexpr size_t lds = HyCfg<D, KB>::SLAB_LDS;                                                                                    \
        constexpr unsigned chunks = InCfg<D, KB>::CHUNKS;                                                                                 \
        hipError_t e = hy_allow_lds(hyper_slab_kernel<D, KB, 0>, lds);                                                                    \
        if (e != hipSuccess) return (int)e;                                                                                               \
        hipLaunchKernelGGL((hyper_slab_kernel<D, KB, 0>), dim3((unsigned)(G_u + G_i), chunks), dim3(IN_WAVES * 64), lds, st,     \
                           E, X, (const float *)nullptr, (int)N, (int)n_split, W_u, W_i, (int)K, G_u, dr, leaky, \
                           w.slabs);                                                                                                      \
    }
    SSLREC_HYPER_DISPATCH(d, kb, CALL)
#undef CALL
    hipLaunchKernelGGL(hyper_reduce_kernel, dim3((unsigned)((d * K + 255) / 256), 2), dim3(256), 0, st, (const float *)w.slabs, G_u, G_i, 1,
                       w.set_stride, (int)d, (int)K, kb * 32, 0, leaky, (const float *)nullptr, (const float *)nullptr, n_split > 0 ? H_u : nullptr,
                       n_split < N ? H_i : nullptr);
#define CALL(D, KB)                                                                                                                       \
    {                                                                                                                                     \
        constexpr size_t lds = HyCfg<D, KB>::Y_LDS;                                                                                       \
        hipError_t e = hy_allow_lds(hyper_y_kernel<D, KB>, lds);                                                                          \
        if (e != hipSuccess) return (int)e;                                                                                               \
        hipLaunchKernelGGL((hyper_y_kernel<D, KB>), dim3((unsigned)(G_u + G_i)), dim3(IN_WAVES * 64), lds, st, E, (int)N,   \
                           (int)n_split, W_u, W_i, (const float *)H_u, (const float *)H_i, (int)K, G_u, dr, leaky, Y);                    \
    }
    SSLREC_HYPER_DISPATCH(d, kb, CALL)
#undef CALL
    SSLREC_LAUNCH_CHECK();
    return 0;
}

int sslrec_hyper_bwd_f32(const float *X, const float *E, const float *dY, const float *Y, int32_t N, int32_t n_split, int32_t d,
                         const float *W_u, const float *W_i, const float *H_u, const float *H_i, int32_t K, float mult, float leaky,
                         float keep_rate, const uint64_t *philox_state, uint32_t philox_stream, float *dX, float *dE, float *dW_u,
                         float *dW_i, void *ws, void *stream) {
    if (!hy_args_ok(N, n_split, d, K, W_u, W_i, leaky, keep_rate, philox_state) || !X || !E || !dY || !Y || !dX || !dE) return SSLREC_E_BADARG;
    if ((n_split > 0 && (!H_u || !dW_u)) || (n_split < N && (!H_i || !dW_i)) || (N > 0 && !ws)) return SSLREC_E_BADARG;
    if (N == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int G_u = in_groups(n_split, HY_CAP), G_i = in_groups((long long)N - n_split, HY_CAP);
    const int kb = in_kb(K);
    const HyDrop dr = hy_drop(philox_state, philox_stream, mult, keep_rate, K);
    const HyWs w = hy_ws(ws, N, n_split, d, K);
    int n_sets = 1;
#define CALL(D, KB)                                                                                                                       \
    {                                                                                                                                     \
        constexpr size_t lds = HyCfg<D, KB>::SLAB_LDS;                                                                                    \
        constexpr unsigned chunks = InCfg<D, KB>::CHUNKS;                                                                                 \
        hipError_t e = hy_allow_lds(hyper_slab_kernel<D, KB, 1>, lds);                                                                    \
        if (e != hipSuccess) return (int)e;                                                                                               \
        hipLaunchKernelGGL((hyper_slab_kernel<D, KB, 1>), dim3((unsigned)(G_u + G_i), chunks), dim3(IN_WAVES * 64), lds, st,     \
                           E, dY, Y, (int)N, (int)n_split, W_u, W_i, (int)K, G_u, dr, leaky, w.slabs);        \
    }
    SSLREC_HYPER_DISPATCH(d, kb, CALL)
#undef CALL
    hipLaunchKernelGGL(hyper_reduce_kernel, dim3((unsigned)((d * K + 255) / 256), 2), dim3(256), 0, st, (const float *)w.slabs, G_u, G_i, 1,
                       w.set_stride, (int)d, (int)K, kb * 32, 1, leaky, H_u, H_i, w.dQ_u, w.dQ_i);
#define CALL(D, KB)                                                                                                                       \
    {                                                                                                                                     \
        const int rc = hy_grad_launch<D, KB>(st, E, X, dY, Y, N, n_split, W_u, W_i, H_u, H_i, K, G_u, G_i, dr, leaky, dX, dE, w, &n_sets); \
        if (rc != 0) return rc;                                                                                                           \
    }
    SSLREC_HYPER_DISPATCH(d, kb, CALL)
#undef CALL
    hipLaunchKernelGGL(hyper_reduce_kernel, dim3((unsigned)((d * K + 255) / 256), 2), dim3(256), 0, st, (const float *)w.slabs, G_u, G_i, n_sets,
                       w.set_stride, (int)d, (int)K, kb * 32, 2, leaky, (const float *)nullptr, (const float *)nullptr, dW_u, dW_i);
    SSLREC_LAUNCH_CHECK();
    return 0;
}

}      // extern "C"
