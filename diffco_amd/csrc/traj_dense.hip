// traj_dense.hip — the dense-check Adam trajectory step (include/dcx.h dcx_traj_dense_run): traj_adam_step_kernel
// (traj_kernels.hip) with the collision hinge charged along the segments instead of at the waypoints.
//
// The collision term arrives as dcx_motion_cost_ex's per-edge outputs (layout e = r * W + w, slot W - 1 the closed zero-length
// edge on the last waypoint): a waypoint's collision gradient is grad_a of the edge it starts plus grad_b of the edge it ends,
// the path's collision value and sample count are block sums of edge_cost and n_samples.  Everything else of the step - FK of
// the waypoints, path length, max-move, joint limits, J^T, Adam, the bookkeeping - is traj_adam_step_kernel's arithmetic through
// the same helpers (traj_fused.h), on the same mapping: one block per path, one lane per waypoint, a wave's 64 waypoints keep
// their control points in its LDS slab.  New per lane: the move mask, the wrap after the update, the history row, the sample
// counter and the stop on the constraint value.  No polling, no exchange between blocks, no atomics.
#include <algorithm>
#include <cmath>

#include "traj_dense.h"
#include "wrap_device.h"

namespace dcx {
namespace {

struct TrajDenseArgs {
    const FkProg* fk;
    dcx_traj_state st;
    dcx_traj_opts opt;
    dcx_traj_dense_opts dopt;
    dcx_traj_dense_io io;
    int32_t dof, d_fk, n_points, point_dim, frame_floats;
    int32_t coord_major;  // features laid out [point_dim][n_points] (DCX_FK_TREE, t_coord_major) instead of [n_points][point_dim]
    float bias1, bias2_sqrt;  // 1 - beta1^t, sqrt(1 - beta2^t)
    int32_t n_class;          // C of the normalisation W / (N_r * C)
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(1024) void traj_dense_step_kernel(const TrajDenseArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int W = a.st.n_waypoints, dof = a.dof, D = a.d_fk;
    const float* path = a.st.path + (size_t)r * W * dof;
    float* hist = a.io.history ? a.io.history + (size_t)r * W * dof : nullptr;
    if (a.st.done[r]) {  // frozen path: its history row repeats
        if (hist)
            for (int i = tid; i < W * dof; i += blockDim.x) hist[i] = path[i];
        return;
    }
    const int w = tid;                       // this lane's waypoint
    const bool live = w < W;
    const size_t e = (size_t)r * W + w;      // ... and the edge it starts (w == W - 1: the closed edge on it)

    // LDS carve: q rows [nw*64][dof] | gq rows | per-wave slabs X, G, F | reduction scratch | program (variable size)
    float* sQ = smem;
    float* sGQ = sQ + nw * 64 * dof;
    float* sX = sGQ + nw * 64 * dof;
    float* sG = sX + nw * 64 * D;
    float* sF = sG + nw * 64 * D;
    float* sR = sF + nw * 64 * a.frame_floats;  // [8][16] partial sums; [96] the bookkeeping flags
    float* sP = sR + 128;

    // ---- the path's collision value and sample count: block sums in waypoint order ---------------------------------------
    {
        const float ec = live ? a.io.edge_cost[e] : 0.f;
        const int ns = live ? a.io.n_samples[e] : 0;
        // an edge over max_samples (dcx_motion_cost_ex: NaN cost, n_samples the count it would need) or a NaN cost
        const int bad = (ec != ec || ns > a.dopt.max_samples) ? 1 : 0;
        const float s = wave_sum(bad ? 0.f : ec);
        const int n = wave_sum(bad ? 0 : ns), b = wave_sum(bad);
        if (lane == 0) {
            sR[5 * 16 + wave] = s;
            sR[6 * 16 + wave] = __int_as_float(n);
            sR[7 * 16 + wave] = __int_as_float(b);
        }
    }
    __syncthreads();
    float coll_sum = 0.f;
    int n_r = 0, n_bad = 0;
    for (int k = 0; k < nw; ++k) {
        coll_sum += sR[5 * 16 + k];
        n_r += __float_as_int(sR[6 * 16 + k]);
        n_bad += __float_as_int(sR[7 * 16 + k]);
    }
    if (n_bad) {  // no step: the path, its moments and counters stay as they are
        if (tid == 0) {
            a.st.done[r] = 1;
            a.st.stats[(size_t)r * 8 + 7] = -2.f;
        }
        if (hist)
            for (int i = tid; i < W * dof; i += blockDim.x) hist[i] = path[i];
        return;
    }
    // (no sample at all - only caller-filled arrays of dcx_traj_dense_step can say so: a mean over nothing is taken as 0)
    const float f_r = a.dopt.normalize ? (n_r > 0 ? (float)W / ((float)n_r * (float)a.n_class) : 0.f) : 1.f;
    const float collision = coll_sum * f_r;
    const float g_scale = a.opt.w_collision * f_r;

    const fk_cptr fk = stage_fk_prog(a.fk, sP, tid, blockDim.x);
    for (int i = tid; i < nw * 64 * dof; i += blockDim.x) sQ[i] = path[i < W * dof ? i : (i % dof) + (W - 1) * dof];
    __syncthreads();

    float* myQ = sQ + (wave * 64 + lane) * dof;
    float* myX = sX + wave * 64 * D + lane;
    float* myG = sG + wave * 64 * D + lane;
    float* myF = sF + wave * 64 * a.frame_floats + lane;
    fk_forward_trig(fk, myQ, myF, 0, 1);
    fk_forward_chain(fk, myQ, myX, myF);
    __syncthreads();

    // control point coordinate k of waypoint v
    auto X = [&](int k, int v) { return sX[(v >> 6) * 64 * D + k * 64 + (v & 63)]; };

    // ---- path-length and max-move terms: gradient w.r.t. this waypoint's control points ---------------
    const float ms = a.opt.max_speed;
    float obj = 0.f, mmv = 0.f;
    const int pd = a.point_dim;
    for (int p = 0; p < a.n_points; ++p) {
        float dn[3] = {0.f, 0.f, 0.f}, dp[3] = {0.f, 0.f, 0.f};
        float n2n = 0.f, n2p = 0.f;
        for (int c = 0; c < pd; ++c) {
            const int k = a.coord_major ? c * a.n_points + p : p * pd + c;
            const float xc = live ? X(k, w) : 0.f;
            if (live && w + 1 < W) { dn[c] = X(k, w + 1) - xc; n2n = fmaf(dn[c], dn[c], n2n); }
            if (live && w >= 1)    { dp[c] = xc - X(k, w - 1); n2p = fmaf(dp[c], dp[c], n2p); }
        }
        const float mn = traj_excess(n2n, ms), mp = traj_excess(n2p, ms);
        if (live && w + 1 < W) {   // each segment is counted once, by its left waypoint
            obj += n2n;
            if (mn > 0.f) mmv += mn;
        }
        const float cn = 2.f * (a.opt.w_diff + (mn > 0.f ? a.opt.w_max_move : 0.f));
        const float cp = 2.f * (a.opt.w_diff + (mp > 0.f ? a.opt.w_max_move : 0.f));
        for (int c = 0; c < pd; ++c) myG[(a.coord_major ? c * a.n_points + p : p * pd + c) * 64] = traj_path_grad(cp, dp[c], cn, dn[c]);
    }
    // J^T of that gradient (per lane; frames of this lane are in its slab)
    float* myGQ = sGQ + (wave * 64 + lane) * dof;
    fk_vjp(fk, myQ, myF, myG, myGQ);

    // ---- joint limits, collision gradient, move mask, Adam, wrap --------------------------------------
    float jl = 0.f, gn2 = 0.f;
    if (live) {
        const size_t base = e * dof;
        const bool fixed = a.io.move ? a.io.move[w] == 0 : (w == 0) || (w == W - 1);
        for (int i = 0; i < dof; ++i) {
            const float q = myQ[i];
            const float lo = a.st.limits[2 * i], hi = a.st.limits[2 * i + 1];
            // the edge this waypoint starts, the edge it ends, and - last waypoint - the closed edge's sample on it
            float gc = a.io.grad_a[base + i];
            if (w >= 1) gc += a.io.grad_b[base - dof + i];
            if (w == W - 1) gc += a.io.grad_b[base + i];
            float g = myGQ[i] + g_scale * gc;
            if (q < lo) { jl += lo - q; g -= a.opt.w_joint_limit; }
            if (q > hi) { jl += q - hi; g += a.opt.w_joint_limit; }
            if (fixed) g = 0.f;
            gn2 = fmaf(g, g, gn2);
            float m = a.st.adam_m[base + i], v = a.st.adam_v[base + i];
            m = fmaf(a.opt.beta1, m, (1.f - a.opt.beta1) * g);
            v = fmaf(a.opt.beta2, v, (1.f - a.opt.beta2) * g * g);
            const float denom = sqrtf(v) / a.bias2_sqrt + a.opt.eps;
            float qn = traj_adam_q(q, a.opt.lr, a.bias1, m, denom);
            if ((a.dopt.rewrap_mask >> i) & 1ull) qn = wrap2pi_f32(qn);
            a.st.adam_m[base + i] = m;
            a.st.adam_v[base + i] = v;
            a.st.path[base + i] = qn;
            myQ[i] = qn;  // keep the new row for the history and bookkeeping copies below
        }
    }

    // ---- block sums -> loss terms ------------------------------------------------------------------------
    float part[4] = {obj, mmv, jl, gn2};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float s = wave_sum(part[t]);
        if (lane == 0) sR[t * 16 + wave] = s;
    }
    __syncthreads();
    if (tid == 0) {
        float tot[4];
        for (int t = 0; t < 4; ++t) {
            float s = 0.f;
            for (int k = 0; k < nw; ++k) s += sR[t * 16 + k];
            tot[t] = s;
        }
        const float objective = a.opt.w_diff * tot[0];
        const float constraint = traj_constraint(a.opt.w_collision, collision, a.opt.w_max_move, tot[1], a.opt.w_joint_limit, tot[2]);
        const float loss = objective + constraint;
        const float gnorm = sqrtf(tot[3]);
        float* st = a.st.stats + (size_t)r * 8;
        st[0] = loss; st[1] = objective; st[2] = constraint; st[3] = gnorm; st[4] = collision; st[5] = tot[1]; st[6] = tot[2];
        st[7] = 0.f;
        int flags = 0;
        if (loss < a.st.lowest_loss[r]) {
            a.st.lowest_loss[r] = loss;
            a.st.lowest_obj[r] = objective;
            flags |= 1;
        }
        if (constraint <= a.opt.valid_tol) {
            if (objective < a.st.best_valid_obj[r]) {
                a.st.best_valid_obj[r] = objective;
                flags |= 2;
            }
            if (gnorm < a.opt.grad_tol) a.st.done[r] = 1;
        }
        // Weighted's `if constraint_loss <= 0.5: break` behind opt.step(): this step was taken, no further one
        if (a.dopt.stop_tol > 0.f && constraint <= a.dopt.stop_tol) a.st.done[r] = 1;
        a.st.steps[r] += 1;
        a.io.n_checks[r] += (int64_t)n_r;
        sR[96] = __int_as_float(flags);
    }
    __syncthreads();
    const int flags = __float_as_int(sR[96]);
    if (flags || hist) {
        float* lo = a.st.lowest_path + (size_t)r * W * dof;
        float* bv = a.st.best_valid_path + (size_t)r * W * dof;
        for (int i = tid; i < W * dof; i += blockDim.x) {
            const float v = sQ[i];
            if (flags & 1) lo[i] = v;
            if (flags & 2) bv[i] = v;
            if (hist) hist[i] = v;
        }
    }
}

__global__ __launch_bounds__(256) void traj_dense_edges_kernel(const TrajDenseEdgeArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a.margin_fill && i < a.C) a.margin_fill[i] = a.margin_value;
    if (i >= (int64_t)a.R * a.W * a.dof) return;
    const int64_t e = i / a.dof;
    const int j = (int)(i - e * a.dof);
    const int w = (int)(e % a.W);
    const int64_t r = e / a.W;
    if (w + 1 < a.W) {
        a.qb[i] = a.path[i + a.dof];
    } else {
        const float v = a.path[i];
        a.qb[i] = v;
        a.q_last[r * a.dof + j] = v;
    }
}

__global__ __launch_bounds__(256) void traj_dense_close_kernel(const TrajDenseCloseArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)a.R * a.dof) return;
    const int64_t r = i / a.dof;
    const int j = (int)(i - r * a.dof);
    const int64_t e = r * a.W + a.W - 1;
    a.io.grad_a[e * a.dof + j] = a.grad_a[i];
    a.io.grad_b[e * a.dof + j] = a.grad_b[i];
    if (j == 0) {
        a.io.edge_cost[e] = a.cost[r];
        a.io.n_samples[e] = a.n_samples[r];
    }
}

size_t traj_dense_lds_bytes(const dcx_fk_desc& fk, int nw) {
    const int d_fk = fk.n_points * fk.point_dim;
    return sizeof(float) * (fk_prog_floats(fk) + 2 * nw * 64 * fk.dof + 2 * nw * 64 * d_fk + nw * 64 * fk_frame_floats(fk) + 128);
}

}  // namespace

hipError_t launch_traj_dense_edges(const TrajDenseEdgeArgs& a, hipStream_t stream) {
    const int64_t n = std::max<int64_t>((int64_t)a.R * a.W * a.dof, a.C);
    if (n == 0) return hipSuccess;
    traj_dense_edges_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(a);
    return hipGetLastError();
}

hipError_t launch_traj_dense_close(const TrajDenseCloseArgs& a, hipStream_t stream) {
    const int64_t n = (int64_t)a.R * a.dof;
    if (n == 0) return hipSuccess;
    traj_dense_close_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(a);
    return hipGetLastError();
}

hipError_t launch_traj_dense_step(const FkProg* fk_dev, const dcx_fk_desc& fk, const dcx_traj_state& st, const dcx_traj_opts& opt,
                                  const dcx_traj_dense_opts& dopt, const dcx_traj_dense_io& io, int n_class, int step,
                                  hipStream_t stream) {
    if (st.n_paths == 0) return hipSuccess;
    TrajDenseArgs a;
    a.fk = fk_dev;
    a.st = st;
    a.opt = opt;
    a.dopt = dopt;
    a.io = io;
    a.dof = fk.dof;
    a.d_fk = fk.n_points * fk.point_dim;
    a.n_points = fk.n_points;
    a.point_dim = fk.point_dim;
    a.coord_major = (fk.kind == DCX_FK_TREE && fk.t_coord_major) ? 1 : 0;
    a.frame_floats = fk_frame_floats(fk);
    a.bias1 = (float)(1.0 - pow((double)opt.beta1, (double)step));
    a.bias2_sqrt = (float)sqrt(1.0 - pow((double)opt.beta2, (double)step));
    a.n_class = n_class;
    const int nw = (st.n_waypoints + 63) / 64;
    const size_t lds = traj_dense_lds_bytes(fk, nw);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)traj_dense_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    traj_dense_step_kernel<<<dim3((unsigned)st.n_paths), dim3(64 * nw), lds, stream>>>(a);
    return hipGetLastError();
}

}  // namespace dcx
