// motion_worst_finish.hip — the launches of dcx_motion_worst behind its sweep (motion_worst_kernel.h).
//   finish: one thread per edge decodes keys[e] into worst / worst_idx / worst_class (NaN / -2 / -1 for an edge over max_samples)
//           and, when gradients are asked for, writes the worst sample x*[e] - motion_coord on the edge's endpoints, the bits the
//           sweep scored - and a one-hot upstream row for the library's score+gradient launch on those E points.
//   chain:  one thread per (edge, joint), the edges of a block side by side: g = d score_c* / dq at x* chained to the endpoints
//           with motion_cost_reduce's per-sample coefficients (the same u, L and u . g arithmetic, for ONE sample):
//             res rule, t = k / res:            grad_b = t g,  grad_a = (1 - t) g
//             max_step rule, interior sample:   grad_b = P (t g),  grad_a = g - grad_b,  t = k max_step / L,  P = I - u u^T
//             max_step rule, the target:        grad_b = g,  grad_a = 0
//           u = delta / L from the wrapped delta of the masked coordinates; the sample count is a constant.
// No atomics and no order of arrival anywhere: the same bits every call.
#include <hip/hip_runtime.h>
#include <math.h>
#include "motion_worst_kernel.h"
#include "wrap_device.h"

namespace dcx {
namespace {
constexpr int kFinishThreads = 256;
constexpr int kChainThreads = 256;

__global__ __launch_bounds__(kFinishThreads) void motion_worst_finish_kernel(const MotionWorstFinishArgs f) {
    const int64_t e = (int64_t)blockIdx.x * kFinishThreads + threadIdx.x;
    if (e >= f.E) return;
    const bool bad = f.status[e] == -2;
    const unsigned long long key = f.keys[e];
    const int k = bad ? 0 : (int)(0xffffffu - (unsigned int)((key >> 8) & 0xffffffull));
    const int c = bad ? 0 : (int)(0xffu - (unsigned int)(key & 0xffull));
    f.worst[e] = bad ? __builtin_nanf("") : __uint_as_float(motion_worst_unorder((uint32_t)(key >> 32)));
    f.worst_idx[e] = bad ? -2 : k;
    if (f.worst_class) f.worst_class[e] = bad ? -1 : c;
    if (f.xstar) {
        // (an edge over max_samples stages its start: a valid point whose gradient row the chain replaces by NaN)
        const int dof = f.dof;
        const int64_t n = f.offs[e + 1] - f.offs[e];
        for (int j = 0; j < dof; ++j) {
            const float qa = f.qa[e * dof + j], qb = f.qb[e * dof + j];
            f.xstar[e * dof + j] = bad ? qa : motion_coord(qa, qb, k, f.res, k == (int)n - 1, f.frac + e, (f.wrap_mask >> j) & 1ull);
        }
    }
    if (f.up)
        for (int i = 0; i < f.C; ++i) f.up[e * f.C + i] = (!bad && i == c) ? 1.0f : 0.0f;
}

__global__ __launch_bounds__(kChainThreads) void motion_worst_chain_kernel(const MotionWorstFinishArgs f) {
    __shared__ float sUT[kChainThreads];
    const int dof = f.dof;
    const int per = kChainThreads / dof;   // edges per block (dof <= DCX_MAX_DOF = 32)
    const int t = threadIdx.x;
    const int le = t / dof, j = t - le * dof;
    const int64_t e = (int64_t)blockIdx.x * per + le;
    const bool mine = le < per && e < f.E;
    float ga = 0.0f, gb = 0.0f, uj = 0.0f;
    bool bad = false, target = false;
    if (mine) {
        bad = f.status[e] == -2;
        const float g = f.g[e * dof + j];
        const int k = bad ? 0 : f.worst_idx[e];
        const int64_t n = f.offs[e + 1] - f.offs[e];
        if (f.res > 0) {
            const float tk = __fdiv_rn((float)k, (float)f.res);
            gb = tk * g;
            ga = (1.0f - tk) * g;
        } else if (k == (int)n - 1) {   // the closed rule's last sample is qb itself
            target = true;
            gb = g;
        } else {
#pragma clang fp contract(off)
            ga = g;
            gb = ((float)k * f.frac[e]) * g;
            float l2 = 0.0f;   // u = delta / L with L as motion_prep computed it (L > 0: there are interior samples)
            for (int i = 0; i < dof; ++i) {
                const float d = motion_delta(f.qa[e * dof + i], f.qb[e * dof + i], f.wrap_mask, i);
                l2 = l2 + d * d;
            }
            uj = motion_delta(f.qa[e * dof + j], f.qb[e * dof + j], f.wrap_mask, j) / sqrtf(l2);
        }
    }
    if (f.res <= 0) {   // (kernel-uniform) P T = T - u (u . T): u . T summed over the edge's joints in order
        sUT[t] = uj * gb;
        __syncthreads();
        if (mine && !target) {
            float ut = 0.0f;
            for (int i = 0; i < dof; ++i) ut += sUT[le * dof + i];
            const float pt = gb - uj * ut;
            gb = pt;
            ga = ga - pt;
        }
    }
    if (mine) {
        const float nan = __builtin_nanf("");
        f.grad_a[e * dof + j] = bad ? nan : ga;
        f.grad_b[e * dof + j] = bad ? nan : gb;
    }
}
}  // namespace

hipError_t launch_motion_worst_finish(const MotionWorstFinishArgs& f, hipStream_t stream) {
    motion_worst_finish_kernel<<<(unsigned)((f.E + kFinishThreads - 1) / kFinishThreads), kFinishThreads, 0, stream>>>(f);
    return hipGetLastError();
}

hipError_t launch_motion_worst_chain(const MotionWorstFinishArgs& f, hipStream_t stream) {
    const int per = kChainThreads / f.dof;
    motion_worst_chain_kernel<<<(unsigned)((f.E + per - 1) / per), kChainThreads, 0, stream>>>(f);
    return hipGetLastError();
}
}  // namespace dcx
