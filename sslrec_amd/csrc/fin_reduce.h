// One-launch deterministic sum of per-workgroup partials: the workgroup that finishes LAST adds them (losses.hip, spmm_swept.hip).
#pragma once
#include "common.h"

// The block that finishes LAST adds the partials -- thread t adds partials t, t + 256, ..., then a 256-wide tree: a fixed order, so the
// value does not depend on which block that is (and equals what the separate finishing kernel of rounds 1-3 produced) -- and writes
// out[0] = mul * total / div (and out[1] = out[0] + *add_in): one launch instead of two.
// "Last" is found with TWO levels of ticket counters: a block takes a ticket of its group of <= 16 blocks, the last block of a group a
// ticket of the top counter.  (One counter for all blocks was measured first: 1024 increments of one address serialize at ~22 ns each
// -- sumsq_kernel went from 6.8 to 29 us, profiles/r04.)  No fence: the partial is published by a RETURNING device-scope atomic
// exchange that the lane waits for before it takes its ticket, so it has reached the coherence point before any later ticket can
// be observed; the reader uses device-scope atomic loads.  (An agent-scope release fence would write back the XCD's whole L2.)
// ws (floats): [0] top ticket, [32 (g + 1)] ticket of group g, [FIN_PART0 + b] partial of block b; every ticket must be 0 at entry and is
// 0 again afterwards (atomicInc wraps).
//  The ordering above is a property of the HARDWARE, not of the HSA memory model: on gfx942 / gfx950 a returning device-scope
// atomic completes at the coherence point and the sc1 loads of the last block bypass the (non-coherent) L2s.  Any other target must
// use a release on the ticket and an acquire in the last block instead; tests/test_gpu_round5.py hammers the one-launch form against
// the two-launch form (thousands of back-to-back launches) so that a toolchain change cannot break it silently.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#error "finish_by_last_block relies on gfx942 / gfx950 atomics completing at the coherence point: use release / acquire on this target"
#endif
#define FIN_GROUPS 64
#define FIN_PART0 (32 * (FIN_GROUPS + 1))

// The one-launch form with its scratch LDS handed in by the caller: s = 256 floats, is_last = one int (kernels that have no static LDS
// to spare lend a dead part of their dynamic allocation).  Every thread of the workgroup calls it; nobody may still use s / is_last.
__device__ __forceinline__ void finish_by_last_block_lds(float *ws, float block_partial, int n_blocks, float mul, float div, const float *add_in,
                                                         float *out, float *s, int *is_last) {
    float *part = ws + FIN_PART0;
    if (threadIdx.x == 0) {
        const int gs = (n_blocks + FIN_GROUPS - 1) / FIN_GROUPS, g = blockIdx.x / gs, n_groups = (n_blocks + gs - 1) / gs;
        const int size_g = min(gs, n_blocks - g * gs);
        (void)__hip_atomic_exchange(part + blockIdx.x, block_partial, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        int last = 0;
        if (atomicInc(reinterpret_cast<unsigned *>(ws + 32 * (g + 1)), (unsigned)size_g - 1u) == (unsigned)size_g - 1u)
            last = atomicInc(reinterpret_cast<unsigned *>(ws), (unsigned)n_groups - 1u) == (unsigned)n_groups - 1u;
        *is_last = last;
    }
    __syncthreads();
    if (!*is_last) return;
    if (threadIdx.x < 256) {      // (the first 256 threads add, whatever the workgroup's size: bpr_fwd_staged_kernel has 1024)
        float v = 0.f;
        for (int i = threadIdx.x; i < n_blocks; i += 256) v += __hip_atomic_load(part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s[threadIdx.x] = v;
    }
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float r = (mul * s[0]) / div;
        out[0] = r;
        if (add_in) out[1] = r + add_in[0];
    }
}

// one_launch = 0: the partial is stored plainly and a second one-workgroup launch adds them (finish_partials_kernel, losses.hip)
__device__ __forceinline__ void finish_by_last_block(float *ws, float block_partial, int n_blocks, float mul, float div, const float *add_in,
                                                     float *out, int one_launch) {
    __shared__ float s[256];
    __shared__ int is_last;
    if (!one_launch) {
        if (threadIdx.x == 0) ws[FIN_PART0 + blockIdx.x] = block_partial;
        return;
    }
    finish_by_last_block_lds(ws, block_partial, n_blocks, mul, div, add_in, out, s, &is_last);
}
