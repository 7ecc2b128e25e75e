// wrap_device.h — angles on the circle, shared by the escape loop (traj_kernels.hip) and the motion calls (motion_prep.hip,
// motion_tile.h, motion_cost_reduce.hip): one definition, one rounding (include/dcx.h pins it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dcx {

// utils.py:51-52 on fp32 tensors: (pi + q) % (2 pi) - pi, Python's %.  Range [-pi, pi) up to the last subtraction's rounding.
__device__ __forceinline__ float wrap2pi_f32(float q) {
    const float pi = 3.14159265358979323846f, two_pi = 6.28318530717958647692f;
    float r = fmodf(pi + q, two_pi);
    if (r != 0.f && r < 0.f) r += two_pi;
    return r - pi;
}

// the delta of coordinate j of a motion qa -> qb: the rounded difference, along the shortest arc where bit j of the mask is set
// (a difference of exactly pi goes the negative way, as utils.anglin's)
__device__ __forceinline__ float motion_delta(float qa, float qb, uint64_t wrap_mask, int j) {
    const float d = __fsub_rn(qb, qa);
    return ((wrap_mask >> j) & 1ull) ? wrap2pi_f32(d) : d;
}

}  // namespace dcx
