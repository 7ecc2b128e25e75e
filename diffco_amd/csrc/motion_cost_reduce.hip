// motion_cost_reduce.hip — the last launch of dcx_motion_cost (motion_cost_kernel.h): per edge, its samples' hinge values h and
// gradients dq (d(weight * h)/dx, the sweep's output in the caller's workspace) summed in sample order, and the chain through the
// interpolation applied.  One thread per (edge, joint), the edges of a block side by side; no atomics: the same bits every call.
//   res rule:       x_k = qa + (k / res)(qb - qa)        grad_b = sum_k t_k g_k,  grad_a = sum_k (1 - t_k) g_k,  t_k = k / res
//   max_step rule:  x_k = qa + k max_step u, u = (qb - qa) / L, for the interior samples (d x_k / d qb = t_k (I - u u^T),
//                   t_k = k max_step / L, d x_k / d qa = I - d x_k / d qb); the target sample x = qb carries identity to grad_b:
//                   grad_b = P T + g_last,  grad_a = G - P T,  G = sum g_k, T = sum t_k g_k over the interior, P = I - u u^T
// With a wrap mask (include/dcx.h) the masked coordinates of qb - qa are the wrapped deltas, in u and in L; wrap2pi has slope 1,
// so nothing else of the chain changes.
// Sample counts are constants (as autograd through utils.dense_path holds them).  An edge over max_samples answers NaN.
#include <hip/hip_runtime.h>
#include <math.h>
#include "motion_cost_kernel.h"
#include "wrap_device.h"

namespace dcx {
namespace {
constexpr int kReduceThreads = 256;

__global__ __launch_bounds__(kReduceThreads) void motion_cost_reduce_kernel(const MotionReduceArgs r) {
    __shared__ float sUT[kReduceThreads];
    const int dof = r.dof;
    const int per = kReduceThreads / dof;   // edges per block (dof <= DCX_MAX_DOF = 32)
    const int t = threadIdx.x;
    const int le = t / dof, j = t - le * dof;
    const int64_t e = (int64_t)blockIdx.x * per + le;
    const bool mine = le < per && e < r.E;
    float ga = 0.0f, gb = 0.0f, cost = 0.0f;   // res rule: the gradients; max_step rule: G and T (the projection below)
    float glast = 0.0f, uj = 0.0f;
    bool bad = false;
    if (mine) {
        bad = r.status[e] == -2;
        const int64_t o = r.offs[e], n = r.offs[e + 1] - o;
        // interior samples; the closed max_step rule's last sample is qb itself
        const int64_t n_in = (r.res > 0 || r.open_end) ? n : n - 1;
        const float fr = r.res > 0 ? 0.0f : r.frac[e];
        for (int64_t k = 0; k < n; ++k) {
            const float hv = r.h[o + k];
            cost += hv;
            if (!(hv > 0.0f)) continue;   // no class above its margin: the sample's gradient is zero (and dq was not written)
            const float g = r.dq[(o + k) * dof + j];
            if (r.res > 0) {
                const float tk = __fdiv_rn((float)k, (float)r.res);
                gb += tk * g;
                ga += (1.0f - tk) * g;
            } else if (k < n_in) {
                ga += g;
                gb += ((float)k * fr) * g;
            } else {
                glast = g;
            }
        }
        if (r.res <= 0 && n_in > 0) {   // u = (qb - qa) / L with L as motion_prep computed it (L > 0: there are interior samples)
#pragma clang fp contract(off)
            float l2 = 0.0f;
            for (int i = 0; i < dof; ++i) {
                const float d = motion_delta(r.qa[e * dof + i], r.qb[e * dof + i], r.wrap_mask, i);
                l2 = l2 + d * d;
            }
            uj = motion_delta(r.qa[e * dof + j], r.qb[e * dof + j], r.wrap_mask, j) / sqrtf(l2);   // (correctly rounded, as motion_prep's L)
        }
    }
    if (r.res <= 0) {   // (kernel-uniform) P T = T - u (u . T): u . T summed over the edge's joints in order
        sUT[t] = uj * gb;
        __syncthreads();
        if (mine) {
            float ut = 0.0f;
            for (int i = 0; i < dof; ++i) ut += sUT[le * dof + i];
            const float pt = gb - uj * ut;
            gb = pt + glast;
            ga = ga - pt;
        }
    }
    if (mine) {
        const float nan = __builtin_nanf("");
        if (j == 0) r.cost[e] = bad ? nan : r.weight * cost;
        r.grad_a[e * dof + j] = bad ? nan : ga;
        r.grad_b[e * dof + j] = bad ? nan : gb;
    }
}
}  // namespace

hipError_t launch_motion_cost_reduce(const MotionReduceArgs& r, hipStream_t stream) {
    const int per = kReduceThreads / r.dof;
    const int64_t nblk = (r.E + per - 1) / per;
    motion_cost_reduce_kernel<<<(unsigned)nblk, kReduceThreads, 0, stream>>>(r);
    return hipGetLastError();
}
}  // namespace dcx
