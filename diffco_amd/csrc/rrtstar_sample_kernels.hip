// rrtstar_sample_kernels.hip — one round's samples of dcx_rrtstar_sample / dcx_rrtstar_run_sampled (include/dcx.h, "batched
// RRT*: samples drawn on the device"; rrtstar_kernel.h): one thread per slot (r, p) reads its problem's status, goal node and best
// cost as they stand at the start of the round and writes the slot's sample row and its info word.
//   goal:      the goal row's bits while the problem has no goal node, with probability goal_bias
//   uniform:   lo + span * u per coordinate, one rounded product and one rounded sum
//   informed:  a uniform point of the unit ball (a Gaussian direction from Box-Muller pairs, the radius u^(1/dof)), scaled to the
//              prolate ellipsoid of the best cost c around the segment start -> goal and turned onto it by ONE Householder
//              reflection, O(dof) per try; the first try inside the limits is taken, else the uniform point
// Random numbers are Philox4x32-10 blocks keyed by the seed and counted by (round, slot, try, block): a draw is a function of
// (seed, g, r, p) and the snapshot alone.  Nothing per coordinate is kept in an array: a pass that needs the Gaussians again
// draws their block again (with DOF known the passes unroll and the compiler keeps one copy in registers), so no dof is slower
// for indexing and nothing spills.  Plain vector stores, no atomics, no LDS.
#include <hip/hip_runtime.h>
#include <math.h>
#include "rrtstar_kernel.h"
#include "philox_device.h"
#include "wrap_device.h"

namespace dcx {
namespace {

struct SampleCounter {   // the fixed part of a slot's Philox counter and the key
    uint32_t g, slot, k0, k1;
    __device__ __forceinline__ Philox4 block(uint32_t t, uint32_t b) const { return philox4x32_10(g, slot, t, b, k0, k1); }
};

// f(j, u_j) for the uniforms of blocks 1 .. 8 (try 0): coordinate j is word j % 4 of block 1 + j / 4
template <int DOF, class F>
__device__ __forceinline__ void each_uniform(const SampleCounter& s, int dof, F f) {
#pragma unroll
    for (int b = 0; b < (DOF > 0 ? (DOF + 3) / 4 : DCX_MAX_DOF / 4); ++b) {
        if (DOF == 0 && b * 4 >= dof) break;
        const Philox4 h = s.block(0u, 1u + b);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (b * 4 + i < dof) f(b * 4 + i, philox_u01(h.w[i]));
    }
}

// f(j, z_j) for the Gaussians of try t, blocks 10 .. 17: words (0, 1) and (2, 3) of block 10 + j / 4 are the Box-Muller pairs of
// coordinates (4 b, 4 b + 1) and (4 b + 2, 4 b + 3): rad = sqrt(-2 ln u1) with u1 in (0, 1], then rad cos(2 pi u2), rad sin(2 pi u2)
template <int DOF, class F>
__device__ __forceinline__ void each_gauss(const SampleCounter& s, uint32_t t, int dof, F f) {
#pragma unroll
    for (int b = 0; b < (DOF > 0 ? (DOF + 3) / 4 : DCX_MAX_DOF / 4); ++b) {
        if (DOF == 0 && b * 4 >= dof) break;
        const Philox4 h = s.block(t, 10u + b);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float rad = sqrtf(-2.0f * logf(philox_u01_open0(h.w[2 * i])));
            float sn, cs;
            sincospif(2.0f * philox_u01(h.w[2 * i + 1]), &sn, &cs);
            if (b * 4 + 2 * i < dof) f(b * 4 + 2 * i, rad * cs);
            if (b * 4 + 2 * i + 1 < dof) f(b * 4 + 2 * i + 1, rad * sn);
        }
    }
}

template <int DOF>
__global__ __launch_bounds__(kRrtStarSampleThreads) void rrtstar_sample_kernel(const RrtStarSampleArgs a) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * kRrtStarSampleThreads + threadIdx.x;
    if (e >= (int64_t)a.R * a.P) return;
    const int64_t r = e / a.P;
    const int dof = DOF > 0 ? DOF : a.dof;
    const float* const start = a.nodes + r * (int64_t)a.cap * dof;   // node 0
    const float* const goal = a.goals + r * dof;
    const float* const lim = a.limits;
    const uint64_t mask = a.wrap_mask;
    float* const out = a.samples + e * dof;
    int info = -1;
    if (a.status[r] != 0) {   // not running: the start row
        for (int j = 0; j < dof; ++j) out[j] = start[j];
    } else {
        const SampleCounter s{(uint32_t)a.round, (uint32_t)r * 16u + (uint32_t)(e - r * a.P), (uint32_t)a.seed, (uint32_t)(a.seed >> 32)};
        const Philox4 h0 = s.block(0u, 0u);
        const int gn = a.goal_node[r];
        if (gn == -1 && philox_u01(h0.w[0]) < a.goal_bias) {
            for (int j = 0; j < dof; ++j) out[j] = goal[j];
            info = 1;
        } else {
            info = 0;
            // (a goal_node outside the tree is the caller's error: such a problem is sampled uniformly, nothing is read there)
            if (gn >= 0 && gn < a.cap && a.mode == 1 && !(philox_u01(h0.w[1]) < a.uniform_mix)) {
                const float c = a.cost[r * (int64_t)a.cap + gn];
                float l2 = 0.0f;
                for (int j = 0; j < dof; ++j) {
                    const float d = motion_delta(start[j], goal[j], mask, j);
                    l2 = l2 + d * d;
                }
                const float cmin = sqrtf(l2);
                if (cmin > 0.0f) {
                    // c^2 - c_min^2 as (c - c_min)(c + c_min): the difference of two near costs is exact, that of their squares is not
                    const float r1 = 0.5f * c, r2 = 0.5f * sqrtf(fmaxf((c - cmin) * (c + cmin), 0.0f));
                    const float sgn = motion_delta(start[0], goal[0], mask, 0) < 0.0f ? -1.0f : 1.0f;
                    // v = a^ + sign(a^_0) e_0
                    const auto v_of = [&](int j) {
                        const float ah = motion_delta(start[j], goal[j], mask, j) / cmin;
                        return j == 0 ? ah + sgn : ah;
                    };
                    float vv = 0.0f;
                    for (int j = 0; j < dof; ++j) vv = vv + v_of(j) * v_of(j);
                    info = 2 + a.tries;
                    for (int t = 0; t < a.tries; ++t) {
                        float n2 = 0.0f;
                        each_gauss<DOF>(s, (uint32_t)t, dof, [&](int, float z) { n2 = n2 + z * z; });
                        const float scale = n2 > 0.0f ? powf(philox_u01(s.block((uint32_t)t, 9u).w[0]), 1.0f / (float)dof) / sqrtf(n2) : 0.0f;
                        float vy = 0.0f;
                        each_gauss<DOF>(s, (uint32_t)t, dof, [&](int j, float z) { vy = vy + v_of(j) * ((j == 0 ? r1 : r2) * (scale * z)); });
                        const float k = 2.0f * vy / vv;
                        bool ok = true;
                        each_gauss<DOF>(s, (uint32_t)t, dof, [&](int j, float z) {
                            const float y = (j == 0 ? r1 : r2) * (scale * z);
                            const float centre = start[j] + 0.5f * motion_delta(start[j], goal[j], mask, j);
                            float x = centre + (y - k * v_of(j));
                            if ((mask >> j) & 1ull) x = wrap2pi_f32(x);
                            ok = ok && lim[2 * j] <= x && x < lim[2 * j + 1];   // (a NaN fails)
                            out[j] = x;
                        });
                        if (ok) {
                            info = 2 + t;
                            break;
                        }
                    }
                }
            }
            if (info == 0 || info == 2 + a.tries) {
                each_uniform<DOF>(s, dof, [&](int j, float u) {
                    const float lo = lim[2 * j];
                    const float span = lim[2 * j + 1] - lo;
                    const float pr = span * u;
                    out[j] = lo + pr;
                });
            }
        }
    }
    if (a.info) a.info[e] = info;
}

template <int DOF>
hipError_t sample(const RrtStarSampleArgs& a, hipStream_t st) {
    const int64_t E = (int64_t)a.R * a.P;
    rrtstar_sample_kernel<DOF><<<dim3((unsigned)((E + kRrtStarSampleThreads - 1) / kRrtStarSampleThreads)), dim3(kRrtStarSampleThreads), 0, st>>>(a);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_rrtstar_sample(const RrtStarSampleArgs& a, hipStream_t st) {
    switch (a.dof <= kRrtRegDof ? a.dof : 0) {
#define DCX_CASE(D) case D: return sample<D>(a, st);
        DCX_CASE(1) DCX_CASE(2) DCX_CASE(3) DCX_CASE(4) DCX_CASE(5) DCX_CASE(6) DCX_CASE(7) DCX_CASE(8)
#undef DCX_CASE
    default: return sample<0>(a, st);
    }
}

}  // namespace dcx
