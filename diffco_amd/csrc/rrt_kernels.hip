// rrt_kernels.hip — the tree logic of dcx_rrt_connect_run (include/dcx.h, "batched RRT-Connect"; rrt_kernel.h): R planning
// problems grown in lockstep, P slots per problem and round.  The edge checks between these launches are dcx_check_motions_ex's.
//   nearest + steer: one block per problem.  Its waves divide the searched tree's nodes, lanes across nodes; a node row is read
//           once and measured against all P queries (the round's samples, or phase 1's new nodes), each lane keeping its P best
//           64-bit keys bits(dist2) << 32 | index in registers - dcx_knn's distance statement by statement (knn_kernels.hip) and
//           its order.  A wave-wide 64-bit minimum by __shfl_xor per slot, then the waves' minima through LDS; slot threads
//           steer towards the sample (phase 1) or pass the new node through (phase 2) and write the slot's edge.
//   commit: one wave per problem, slot p on lane p: a ballot of the slots that append and the popcount of the lower lanes give
//           the append indices in slot order.  Phase 2 appends the last free sample of a blocked connect edge - motion_coord's
//           point with the motion prep's own step fraction - and settles link, status and solved_round.
// Keys are unique and totally ordered and no atomic decides anything: the state after a round is a function of the state before
// it and the round's samples.
#include <hip/hip_runtime.h>
#include <math.h>
#include "rrt_kernel.h"
#include "motion_tile.h"
#include "wrap_device.h"

namespace dcx {
namespace {
typedef unsigned long long u64;

// dcx_knn's dist2 of the edge query -> point (knn_kernels.hip): subtract, (wrap,) multiply, add, each rounded on its own
template <int DOF, bool WRAP>
__device__ __forceinline__ float rrt_dist2(const float* q, const float* pt, int dof, uint64_t mask) {
#pragma clang fp contract(off)
    float l2 = 0.0f;
    if constexpr (DOF > 0) {
#pragma unroll
        for (int j = 0; j < DOF; ++j) {
            const float d = WRAP ? motion_delta(q[j], pt[j], mask, j) : __fsub_rn(pt[j], q[j]);
            l2 = l2 + d * d;
        }
    } else {
        for (int j = 0; j < dof; ++j) {
            const float d = WRAP ? motion_delta(q[j], pt[j], mask, j) : __fsub_rn(pt[j], q[j]);
            l2 = l2 + d * d;
        }
    }
    return l2;
}

// The slot's edge near -> qb towards the sample s (include/dcx.h): motion_count_kernel's length of the edge near -> s, then the
// sample itself within `range`, else the point at `range` along the (wrapped) delta.  False: no edge (a length that is not > 0).
__device__ __forceinline__ bool rrt_steer(const float* near, const float* s, int dof, uint64_t mask, float range, float* qb) {
#pragma clang fp contract(off)
    float l2 = 0.0f;
    for (int j = 0; j < dof; ++j) {
        const float d = motion_delta(near[j], s[j], mask, j);
        l2 = l2 + d * d;
    }
    const float L = sqrtf(l2);   // correctly rounded, as motion_prep.hip's
    if (!(L > 0.0f)) return false;
    if (L <= range) {
        for (int j = 0; j < dof; ++j) qb[j] = s[j];
        return true;
    }
    const float f = __fdiv_rn(range, L);
    for (int j = 0; j < dof; ++j) {
        const float d = motion_delta(near[j], s[j], mask, j);
        const float p = d * f;
        const float x = near[j] + p;
        qb[j] = ((mask >> j) & 1ull) ? wrap2pi_f32(x) : x;
    }
    return true;
}

// DOF 1 .. kRrtRegDof: the node row in registers while the P slots read it.  DOF 0: any dof, the row read where it is used
// (the slots after the first find it in the L1).
template <int DOF, bool WRAP>
__global__ __launch_bounds__(kRrtWaves * 64) void rrt_nearest_steer_kernel(const RrtArgs a) {
    __shared__ float sQ[kRrtMaxSlots * DCX_MAX_DOF];   // the P queries, [p][dof]
    __shared__ u64 sKey[kRrtWaves][kRrtMaxSlots];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t r = blockIdx.x;
    const int P = a.P, dof = DOF > 0 ? DOF : a.dof, cap = a.cap;
    const int searched = a.phase == 1 ? a.tree : 1 - a.tree;
    const float* const tree0 = a.nodes + r * a.trees * (int64_t)cap * dof;      // the problem's tree 0; its node 0 is the start
    const float* const pts = tree0 + (int64_t)searched * cap * dof;
    const float* const grown = tree0 + (int64_t)a.tree * cap * dof;             // tree a: phase 1's new nodes live here
    const bool running = a.status[r] == 0;
    const int n = running ? min(a.count[r * a.trees + searched], cap) : 0;   // (a count beyond cap is the caller's error: never read past the tree)
    const uint64_t mask = a.wrap_mask;

    // which slots search (block-uniform), and their queries
    unsigned active = 0;
    if (running)
        for (int p = 0; p < P; ++p)
            if (a.phase == 1 || a.added[r * P + p] >= 0) active |= 1u << p;
    for (int i = tid; i < P * dof; i += kRrtWaves * 64) {
        const int p = i / dof, j = i - p * dof;
        float v = 0.0f;
        if (a.phase == 1) {
            v = a.samples[(r * P + p) * dof + j];
        } else {
            const int at = a.added[r * P + p];
            if (at >= 0) v = grown[(int64_t)at * dof + j];
        }
        sQ[i] = v;
    }
    __syncthreads();

    u64 best[kRrtMaxSlots];
#pragma unroll
    for (int p = 0; p < kRrtMaxSlots; ++p) best[p] = kRrtEmpty;
    if (active) {
        for (int i = tid; i < n; i += kRrtWaves * 64) {
            const float* row = pts + (int64_t)i * dof;
            float pt[DOF > 0 ? DOF : 1];
            if constexpr (DOF > 0) {
#pragma unroll
                for (int j = 0; j < DOF; ++j) pt[j] = row[j];
            }
#pragma unroll
            for (int p = 0; p < kRrtMaxSlots; ++p) {
                if (p < P && ((active >> p) & 1u)) {
                    const float l2 = rrt_dist2<DOF, WRAP>(sQ + p * dof, DOF > 0 ? pt : row, dof, mask);
                    // a NaN fails the comparison; dist2 is never negative or -0, so its bits order like its value
                    if (l2 <= INFINITY) {
                        const u64 key = ((u64)__float_as_uint(l2) << 32) | (u64)(uint32_t)i;
                        best[p] = key < best[p] ? key : best[p];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < kRrtMaxSlots; ++p) {
        if (p < P) {
            u64 m = best[p];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                const u64 o = __shfl_xor(m, d, 64);
                m = o < m ? o : m;
            }
            if (lane == 0) sKey[wave][p] = m;
        }
    }
    __syncthreads();
    if (tid >= P) return;

    // slot thread p: its edge
    const int p = tid;
    const int64_t e = r * P + p;
    u64 key = sKey[0][p];
    for (int w = 1; w < kRrtWaves; ++w) key = sKey[w][p] < key ? sKey[w][p] : key;
    bool go = ((active >> p) & 1u) && key != kRrtEmpty;
    const int at = (int)(uint32_t)key;
    float* const qa = a.qa + e * dof;
    float* const qb = a.qb + e * dof;
    if (go) {
        const float* near = pts + (int64_t)at * dof;
        if (a.phase == 1) {
            go = rrt_steer(near, sQ + p * dof, dof, mask, a.range, qb);
        } else {
            for (int j = 0; j < dof; ++j) qb[j] = sQ[p * dof + j];
        }
        if (go)
            for (int j = 0; j < dof; ++j) qa[j] = near[j];
    }
    if (!go) {   // nothing to check: the zero-length edge on the start node, one sample, its verdict ignored
        for (int j = 0; j < dof; ++j) {
            qa[j] = tree0[j];
            qb[j] = tree0[j];
        }
    }
    a.near[e] = go ? at : -1;
}

__global__ __launch_bounds__(64) void rrt_commit_kernel(const RrtArgs a) {
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int P = a.P, dof = a.dof, cap = a.cap;
    const int written = a.phase == 1 ? a.tree : 1 - a.tree;
    const int64_t e = r * P + lane;
    const bool slot = lane < P;
    const bool running = a.status[r] == 0;
    const int c0 = max(0, min(a.count[r * 2 + written], cap));
    const int near = slot ? a.near[e] : -1;
    const int h = slot ? a.first_hit[e] : 0;
    const int grown = (slot && a.phase == 2) ? a.added[e] : -1;
    const bool full1 = a.phase == 2 && a.full[r] != 0;
    const bool valid = running && near >= 0;
    // phase 1: a free edge appends its end;  phase 2: an edge blocked at sample h >= 2 appends sample h - 1
    const bool app = valid && (a.phase == 1 ? h == -1 : h >= 2);
    const u64 bal = __ballot(app);
    const int total = __popcll(bal);
    const int at = c0 + __popcll(bal & ((1ull << lane) - 1ull));
    const bool fits = app && at < cap;
    if (fits) {
        float* out = a.nodes + ((r * 2 + written) * (int64_t)cap + at) * dof;
        const float* qa = a.qa + e * dof;
        const float* qb = a.qb + e * dof;
        for (int j = 0; j < dof; ++j)
            out[j] = a.phase == 1 ? qb[j] : motion_coord(qa[j], qb[j], h - 1, 0, false, a.frac + e, (a.wrap_mask >> j) & 1ull);
        a.parent[(r * 2 + written) * (int64_t)cap + at] = near;
    }
    const bool over = c0 + total > cap;   // a slot of this phase did not fit
    if (a.phase == 1) {
        if (slot) a.added[e] = fits ? at : -1;
        if (lane == 0 && running) {
            a.count[r * 2 + written] = over ? cap : c0 + total;
            a.full[r] = over ? 1 : 0;
        }
        if (lane == 0 && !running) a.full[r] = 0;
        return;
    }
    const u64 joined = __ballot(valid && h == -1);
    if (!running) return;   // (wave-uniform)
    if (lane == 0) a.count[r * 2 + written] = over ? cap : c0 + total;
    if (joined) {
        if (lane == __ffsll((long long)joined) - 1) {   // the joining slot with the lowest p; solved wins over full
            a.link[r * 2 + a.tree] = grown;
            a.link[r * 2 + written] = near;
            a.solved_round[r] = a.round;
            a.status[r] = 1;
        }
    } else if (lane == 0 && (over || full1)) {
        a.status[r] = 2;
    }
}

template <int DOF>
hipError_t nearest(const RrtArgs& a, hipStream_t st) {
    if (a.wrap_mask) rrt_nearest_steer_kernel<DOF, true><<<dim3((unsigned)a.R), dim3(kRrtWaves * 64), 0, st>>>(a);
    else rrt_nearest_steer_kernel<DOF, false><<<dim3((unsigned)a.R), dim3(kRrtWaves * 64), 0, st>>>(a);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_rrt_nearest(const RrtArgs& a, hipStream_t st) {
    switch (a.dof <= kRrtRegDof ? a.dof : 0) {
#define DCX_CASE(D) case D: return nearest<D>(a, st);
        DCX_CASE(1) DCX_CASE(2) DCX_CASE(3) DCX_CASE(4) DCX_CASE(5) DCX_CASE(6) DCX_CASE(7) DCX_CASE(8)
#undef DCX_CASE
    default: return nearest<0>(a, st);
    }
}

hipError_t launch_rrt_commit(const RrtArgs& a, hipStream_t st) {
    rrt_commit_kernel<<<dim3((unsigned)a.R), dim3(64), 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace dcx
