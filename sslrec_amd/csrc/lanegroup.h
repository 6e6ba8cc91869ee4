// Lane-group helpers shared by the per-entry kernels (sddmm.hip: SDDMM and the row normalizations; gt.hip: the graph-transformer
// layer).  A LANE GROUP of L lanes owns one row of d = 4 L floats, one float4 per lane; sums over an aligned group of lanes are DPP
// permutes inside a 16-lane DPP row and ds_bpermute beyond it.  All lanes of the group must be active together.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float dpp_add(float v, const int ctrl_sel) {
    // (ctrl must be an immediate: one call site per pattern)
    switch (ctrl_sel) {
    case 0: return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));       // quad_perm [1,0,3,2]
    case 1: return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));       // quad_perm [2,3,0,1]
    case 2: return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));      // row_half_mirror
    default: return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));     // row_mirror
    }
}

// sum over an aligned group of L lanes (L = 1 .. 64, a power of two); every lane of the group receives the total.  After the quad steps
// all lanes of a quad hold the same value, so the mirrors (lane i <- lane 7 - i, lane i <- lane 15 - i) add the OTHER half's sum.
template <int L>
__device__ __forceinline__ float group_sum(float v) {
    if constexpr (L >= 2) v = dpp_add(v, 0);
    if constexpr (L >= 4) v = dpp_add(v, 1);
    if constexpr (L >= 8) v = dpp_add(v, 2);
    if constexpr (L >= 16) v = dpp_add(v, 3);
    if constexpr (L >= 32) v += __shfl_xor(v, 16, 64);
    if constexpr (L >= 64) v += __shfl_xor(v, 32, 64);
    return v;
}

__device__ __forceinline__ float dot4(const float4 a, const float4 b) {
    return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)));
}

}      // namespace
