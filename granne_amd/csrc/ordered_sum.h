// ordered_sum.h -- the reference's sum of its 32 accumulators (src/math.rs:5-52: r = 0.0, then r += acc[i] for i = 0 .. 31)
// over a group of eight lanes, lane `sub` holding acc[4 sub .. 4 sub + 3]: the one place that order lives for the
// eight-lanes-per-row distance routines (dists_kernel in util_kernels.h, refine_kernel.h, f16.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace granne_hip {

__device__ __forceinline__ float lane_shr1(float v) { // value of lane-1 (within a 16-lane row)
#if GRANNE_HIP_USE_DPP
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111 /* row_shr:1 */, 0xf, 0xf, false));
#else
    return __shfl_up(v, 1, 64);
#endif
}

// acc[0] + acc[1] + ... + acc[31] in that order, starting from 0.0: the sum runs down the eight lanes of a group, lane
// `sub` is right after step `sub`, and every lane of the group returns lane 7's value. Every lane of the wave calls it.
__device__ __forceinline__ float ordered_sum8(float a0, float a1, float a2, float a3, uint32_t lane) {
    float s = 0.0f;
#pragma unroll
    for (int ps = 0; ps < 8; ++ps) {
        float u = (ps == 0) ? 0.0f : lane_shr1(s);
        u = u + a0; u = u + a1; u = u + a2; u = u + a3;
        s = u;
    }
    return __shfl(s, (int)(lane | 7u), 64);
}

} // namespace granne_hip
