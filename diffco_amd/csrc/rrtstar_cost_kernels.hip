// rrtstar_cost_kernels.hip — the kernels dcx_rrtstar_run_cost adds to the round of rrtstar_kernels.hip (include/dcx.h, "batched
// RRT*: clearance-weighted edge costs"; rrtstar_cost_kernel.h has the round).  An edge with peak w = dcx_motion_worst's worst
// and length bits L costs C = L * (1 + gain * fmaxf(w + band, 0)) and is free where w <= 0.
//   extend settle:   one thread per slot (r, p): first_hit from worst0 (-1 free, -2 NaN, else 0), so that the length planner's
//                    near and rewire launches find their candidates where they look; C0 and c0 = cost[near] + C0 for the round.
//   choose prepare:  one thread per place (r, p, j): Lj, the lower bound cost[u_j] + Lj against the incumbent c0, the place's
//                    edge u_j -> x or the idle edge.
//   commit:          rrtstar_kernels.hip's, a wave per problem, slot p on lane p - with the candidates' Cj and cj formed from the
//                    places' worst, and a candidate taken only while (bits(cj), u_j) is still below (bits(c0), near).
//   rewire settle:   one thread per place, after the sweep of the edges the length planner's rewire prepare submitted on the
//                    lower bound: C' and c' = cost[x] + C' into place_len and place_cost, the verdict into place_hit, and the
//                    place stays submitted only where it is free and c' < cost[v].  The length planner's selection then picks
//                    the least (bits(c'), p) per v and writes elen[v] = C'.
// No atomics; every cost is formed with contraction off, one rounded operation at a time.
#include <hip/hip_runtime.h>
#include <math.h>
#include "rrtstar_cost_kernel.h"
#include "wrap_device.h"

namespace dcx {
namespace {
typedef unsigned long long u64;

// rrtstar_kernels.hip's star_len2: the squared length of the directed edge from -> to as the motion calls accumulate it
__device__ __forceinline__ float cost_len2(const float* from, const float* to, int dof, uint64_t mask) {
#pragma clang fp contract(off)
    float l2 = 0.0f;
    for (int j = 0; j < dof; ++j) {
        const float d = motion_delta(from[j], to[j], mask, j);
        l2 = l2 + d * d;
    }
    return l2;
}

// C = L * f(w): three operations, each rounded alone
__device__ __forceinline__ float edge_cost(float L, float w, float gain, float band) {
#pragma clang fp contract(off)
    const float pen = fmaxf(w + band, 0.0f);
    const float f = 1.0f + gain * pen;
    return L * f;
}

__device__ __forceinline__ bool cost_candidate(const RrtStarArgs& a, int64_t r, int64_t e) {
    return a.status[r] == 0 && a.near[e] >= 0 && a.first_hit[e] == -1;
}

__global__ __launch_bounds__(kRrtStarPlaceThreads) void rrtstar_cost_extend_settle_kernel(const RrtStarCostArgs c) {
#pragma clang fp contract(off)
    const RrtStarArgs& a = c.a;
    const int64_t e = (int64_t)blockIdx.x * kRrtStarPlaceThreads + threadIdx.x;
    if (e >= (int64_t)a.R * a.P) return;
    const int64_t r = e / a.P;
    const float w = c.worst0[e];
    const bool free = w <= 0.0f;   // (a NaN fails the comparison)
    c.first_hit[e] = free ? -1 : (w != w ? -2 : 0);
    float C0 = 0.0f, c0 = 0.0f;
    const int near = a.near[e];
    if (free && near >= 0 && a.status[r] == 0) {
        const float* const tree = a.nodes + r * (int64_t)a.cap * a.dof;
        C0 = edge_cost(sqrtf(cost_len2(tree + (int64_t)near * a.dof, a.qb + e * a.dof, a.dof, a.wrap_mask)), w, c.gain, c.band);
        c0 = a.cost[r * (int64_t)a.cap + near] + C0;
    }
    c.slot_len[e] = C0;
    c.slot_cost[e] = c0;
}

__global__ __launch_bounds__(kRrtStarPlaceThreads) void rrtstar_cost_choose_prepare_kernel(const RrtStarCostArgs c) {
#pragma clang fp contract(off)
    const RrtStarArgs& a = c.a;
    const int64_t i = (int64_t)blockIdx.x * kRrtStarPlaceThreads + threadIdx.x;
    if (i >= (int64_t)a.R * a.P * a.K) return;
    const int64_t e = i / a.K, r = e / a.P;
    const int dof = a.dof;
    const float* const tree = a.nodes + r * (int64_t)a.cap * dof;
    const int u = a.near_idx[i];
    bool submit = false;
    float lb = 0.0f, Lj = 0.0f;
    if (u >= 0 && cost_candidate(a, r, e)) {
        const int near = a.near[e];
        Lj = sqrtf(cost_len2(tree + (int64_t)u * dof, a.qb + e * dof, dof, a.wrap_mask));
        lb = a.cost[r * (int64_t)a.cap + u] + Lj;   // cj >= lb in bits: f >= 1, and the product and the sum are monotone
        const uint32_t bj = __float_as_uint(lb), b0 = __float_as_uint(c.slot_cost[e]);
        submit = bj < b0 || (bj == b0 && u < near);
    }
    float* const qa = a.pqa + i * dof;
    float* const qb = a.pqb + i * dof;
    const float* const from = tree + (int64_t)max(u, 0) * dof;
    const float* const x = a.qb + e * dof;
    for (int j = 0; j < dof; ++j) {   // the place's edge u_j -> x, or the zero-length edge on the problem's start node
        qa[j] = submit ? from[j] : tree[j];
        qb[j] = submit ? x[j] : tree[j];
    }
    a.submitted[i] = submit ? 1 : 0;
    a.place_cost[i] = lb;
    a.place_len[i] = Lj;
}

__global__ __launch_bounds__(64) void rrtstar_cost_commit_kernel(const RrtStarCostArgs c) {
#pragma clang fp contract(off)
    const RrtStarArgs& a = c.a;
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int P = a.P, K = a.K, dof = a.dof, cap = a.cap;
    const int64_t e = r * P + lane;
    const bool slot = lane < P;
    const bool running = a.status[r] == 0;
    const int c0n = max(0, min(a.count[r], cap));
    const bool app = slot && cost_candidate(a, r, e);
    const u64 bal = __ballot(app);
    const int total = __popcll(bal);
    const int at = c0n + __popcll(bal & ((1ull << lane) - 1ull));
    const bool fits = app && at < cap;
    bool is_goal = false;
    if (fits) {
        const float* const cost = a.cost + r * (int64_t)cap;
        const float* const x = a.qb + e * dof;
        int par = a.near[e];
        float len = c.slot_len[e];
        float cn = c.slot_cost[e];
        u64 bestk = ((u64)__float_as_uint(cn) << 32) | (u64)(uint32_t)par;   // the incumbent: a candidate has to stay below it
        for (int j = 0; j < K; ++j) {
            const int64_t i = e * K + j;
            if (!a.submitted[i]) continue;
            const float w = c.place_worst[i];
            if (!(w <= 0.0f)) continue;
            const int u = a.near_idx[i];
            const float Cj = edge_cost(a.place_len[i], w, c.gain, c.band);
            const float cj = cost[u] + Cj;
            const u64 key = ((u64)__float_as_uint(cj) << 32) | (u64)(uint32_t)u;
            if (key < bestk) {
                bestk = key;
                par = u;
                len = Cj;
                cn = cj;
            }
        }
        float* const out = a.nodes + (r * (int64_t)cap + at) * dof;
        const float* const goal = a.goals + r * dof;
        is_goal = true;
        for (int j = 0; j < dof; ++j) {
            out[j] = x[j];
            is_goal = is_goal && __float_as_uint(x[j]) == __float_as_uint(goal[j]);
        }
        a.parent[r * (int64_t)cap + at] = par;
        a.elen[r * (int64_t)cap + at] = len;
        a.cost[r * (int64_t)cap + at] = cn;
    }
    if (slot) a.added[e] = fits ? at : -1;
    const u64 goals = __ballot(is_goal);
    if (lane == 0) a.rewired[r] = 0;
    if (!running) return;   // (wave-uniform; nothing was appended)
    if (goals && lane == __ffsll((long long)goals) - 1 && a.goal_node[r] == -1) {
        a.goal_node[r] = at;
        a.first_round[r] = a.round;
    }
    if (lane == 0) {
        const bool over = c0n + total > cap;   // a slot did not fit
        a.count[r] = over ? cap : c0n + total;
        if (over) a.status[r] = 2;
    }
}

__global__ __launch_bounds__(kRrtStarPlaceThreads) void rrtstar_cost_rewire_settle_kernel(const RrtStarCostArgs c) {
#pragma clang fp contract(off)
    const RrtStarArgs& a = c.a;
    const int64_t i = (int64_t)blockIdx.x * kRrtStarPlaceThreads + threadIdx.x;
    if (i >= (int64_t)a.R * a.P * a.K) return;
    const int64_t e = i / a.K, r = e / a.P;
    bool keep = false, free = false;
    if (a.submitted[i]) {   // so added[e] >= 0 and near_idx[i] >= 0 (the rewire prepare's conditions)
        const float* const cost = a.cost + r * (int64_t)a.cap;
        const float w = c.place_worst[i];
        free = w <= 0.0f;
        if (free) {
            const float Cp = edge_cost(a.place_len[i], w, c.gain, c.band);
            const float cp = cost[a.added[e]] + Cp;
            keep = cp < cost[a.near_idx[i]];   // the snapshot's cost[v]: costs move only in the refresh
            a.place_len[i] = Cp;
            a.place_cost[i] = cp;
        }
    }
    c.place_hit[i] = free ? -1 : 0;
    a.submitted[i] = keep ? 1 : 0;
}

inline unsigned blocks_for(int64_t n) {
    return (unsigned)((n + kRrtStarPlaceThreads - 1) / kRrtStarPlaceThreads);
}
}  // namespace

hipError_t launch_rrtstar_cost_extend_settle(const RrtStarCostArgs& c, hipStream_t st) {
    rrtstar_cost_extend_settle_kernel<<<dim3(blocks_for((int64_t)c.a.R * c.a.P)), dim3(kRrtStarPlaceThreads), 0, st>>>(c);
    return hipGetLastError();
}

hipError_t launch_rrtstar_cost_choose_prepare(const RrtStarCostArgs& c, hipStream_t st) {
    rrtstar_cost_choose_prepare_kernel<<<dim3(blocks_for((int64_t)c.a.R * c.a.P * c.a.K)), dim3(kRrtStarPlaceThreads), 0, st>>>(c);
    return hipGetLastError();
}

hipError_t launch_rrtstar_cost_commit(const RrtStarCostArgs& c, hipStream_t st) {
    rrtstar_cost_commit_kernel<<<dim3((unsigned)c.a.R), dim3(64), 0, st>>>(c);
    return hipGetLastError();
}

hipError_t launch_rrtstar_cost_rewire_settle(const RrtStarCostArgs& c, hipStream_t st) {
    rrtstar_cost_rewire_settle_kernel<<<dim3(blocks_for((int64_t)c.a.R * c.a.P * c.a.K)), dim3(kRrtStarPlaceThreads), 0, st>>>(c);
    return hipGetLastError();
}

}  // namespace dcx
