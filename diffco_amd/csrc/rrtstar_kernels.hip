// rrtstar_kernels.hip — the tree logic of dcx_rrtstar_run and dcx_rrtstar_extract_paths (include/dcx.h, "batched RRT*";
// rrtstar_kernel.h): R planning problems, one tree each, grown in lockstep, P slots per problem and round, K near nodes per slot.
// The nearest + steer launch is rrt_kernels.hip's; the edge checks between these launches are dcx_check_motions_ex's.
//   near:            one wave per slot (r, p).  Lanes across the snapshot's nodes, each lane keeping its kRrtStarMaxNear best keys
//                    bits(dist2) << 32 | index sorted in registers (dcx_knn's distance statement by statement, and its order);
//                    then K wave-wide 64-bit minima by __shfl_xor, the lane that held the minimum dropping it.  Nothing of a
//                    Q x N matrix is ever written.
//   choose prepare:  one thread per place (r, p, j): Lj, cj against the incumbent c0, the place's edge u_j -> x or the idle edge.
//   commit:          one wave per problem, slot p on lane p: the free candidate with the least (bits(cj), u_j) or near; a ballot
//                    of the slots that append and the popcount of the lower lanes give the append indices in slot order; the
//                    goal's bits, count and status.
//   rewire prepare:  one thread per place: L' = sqrtf(dist2_j), c' = cost[x] + L' against the snapshot's cost[v], the edge x -> v.
//   rewire select:   one block per problem, a thread per place: the places' (v, bits(c') << 32 | p) in LDS, every free place
//                    compares itself with all others on the same v; the least key writes parent[v] and elen[v].
//   refresh:         one block per problem: passes of cost[i] = cost[parent[i]] + elen[i] over the tree until one changes nothing.
//   extract:         one wave per problem: the chain from goal_node is walked once for its depth and once more to write its rows.
// Keys are unique and totally ordered and no atomic decides anything: the state after a round is a function of the state before
// it, the goals and the round's samples.
#include <hip/hip_runtime.h>
#include <math.h>
#include "rrtstar_kernel.h"
#include "wrap_device.h"

namespace dcx {
namespace {
typedef unsigned long long u64;

// the squared length of the directed edge from -> to as the motion calls and dcx_knn accumulate it: subtract, (wrap,) multiply,
// add from +0 in coordinate order, each rounded on its own
__device__ __forceinline__ float star_len2(const float* from, const float* to, int dof, uint64_t mask) {
#pragma clang fp contract(off)
    float l2 = 0.0f;
    for (int j = 0; j < dof; ++j) {
        const float d = motion_delta(from[j], to[j], mask, j);
        l2 = l2 + d * d;
    }
    return l2;
}

__device__ __forceinline__ bool star_candidate(const RrtStarArgs& a, int64_t r, int64_t e) {
    return a.status[r] == 0 && a.near[e] >= 0 && a.first_hit[e] == -1;
}

__global__ __launch_bounds__(64) void rrtstar_near_kernel(const RrtStarArgs a) {
    __shared__ float sX[DCX_MAX_DOF];
    const int lane = threadIdx.x;
    const int64_t e = blockIdx.x;
    const int64_t r = e / a.P;
    const int K = a.K, dof = a.dof, cap = a.cap;
    int32_t* const out_idx = a.near_idx + e * K;
    float* const out_d2 = a.near_d2 + e * K;
    if (!star_candidate(a, r, e)) {   // (wave-uniform)
        if (lane < K) {
            out_idx[lane] = -1;
            out_d2[lane] = INFINITY;
        }
        return;
    }
    for (int j = lane; j < dof; j += 64) sX[j] = a.qb[e * dof + j];
    __syncthreads();
    const int n = max(0, min(a.count[r], cap));   // the snapshot: the commit of this round has not run yet
    const float* const pts = a.nodes + r * (int64_t)cap * dof;
    const uint64_t mask = a.wrap_mask;
    const float max_d2 = a.max_d2;

    u64 best[kRrtStarMaxNear];   // ascending
#pragma unroll
    for (int k = 0; k < kRrtStarMaxNear; ++k) best[k] = kRrtEmpty;
    for (int i = lane; i < n; i += 64) {
        const float l2 = star_len2(sX, pts + (int64_t)i * dof, dof, mask);
        if (!(l2 <= max_d2)) continue;   // (a NaN fails the comparison; dist2 is never negative or -0: its bits order like its value)
        const u64 key = ((u64)__float_as_uint(l2) << 32) | (u64)(uint32_t)i;
        if (key < best[kRrtStarMaxNear - 1]) {
#pragma unroll
            for (int k = kRrtStarMaxNear - 1; k > 0; --k)
                best[k] = key < best[k - 1] ? best[k - 1] : (key < best[k] ? key : best[k]);
            best[0] = key < best[0] ? key : best[0];
        }
    }
    for (int k = 0; k < K; ++k) {
        u64 m = best[0];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const u64 o = __shfl_xor(m, d, 64);
            m = o < m ? o : m;
        }
        if (lane == 0) {
            out_idx[k] = m == kRrtEmpty ? -1 : (int32_t)(uint32_t)m;
            out_d2[k] = m == kRrtEmpty ? INFINITY : __uint_as_float((uint32_t)(m >> 32));
        }
        if (m != kRrtEmpty && best[0] == m) {   // keys are unique: one lane drops its head
#pragma unroll
            for (int q = 0; q < kRrtStarMaxNear - 1; ++q) best[q] = best[q + 1];
            best[kRrtStarMaxNear - 1] = kRrtEmpty;
        }
    }
}

// the place's edge into the batch: from -> to, or the zero-length edge on the problem's start node
__device__ __forceinline__ void star_put_edge(const RrtStarArgs& a, int64_t i, const float* from, const float* to, const float* root,
                                              bool submit) {
    float* const qa = a.pqa + i * a.dof;
    float* const qb = a.pqb + i * a.dof;
    for (int j = 0; j < a.dof; ++j) {
        qa[j] = submit ? from[j] : root[j];
        qb[j] = submit ? to[j] : root[j];
    }
}

__global__ __launch_bounds__(kRrtStarPlaceThreads) void rrtstar_choose_prepare_kernel(const RrtStarArgs a) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kRrtStarPlaceThreads + threadIdx.x;
    if (i >= (int64_t)a.R * a.P * a.K) return;
    const int64_t e = i / a.K, r = e / a.P;
    const int dof = a.dof;
    const float* const tree = a.nodes + r * (int64_t)a.cap * dof;
    const int u = a.near_idx[i];
    bool submit = false;
    float cj = 0.0f, Lj = 0.0f;
    if (u >= 0 && star_candidate(a, r, e)) {
        const int near = a.near[e];
        const float* const x = a.qb + e * dof;
        const float* const cost = a.cost + r * (int64_t)a.cap;
        Lj = sqrtf(star_len2(tree + (int64_t)u * dof, x, dof, a.wrap_mask));
        cj = cost[u] + Lj;
        const float c0 = cost[near] + sqrtf(star_len2(tree + (int64_t)near * dof, x, dof, a.wrap_mask));
        const uint32_t bj = __float_as_uint(cj), b0 = __float_as_uint(c0);
        submit = bj < b0 || (bj == b0 && u < near);
    }
    star_put_edge(a, i, tree + (int64_t)max(u, 0) * dof, a.qb + e * dof, tree, submit);
    a.submitted[i] = submit ? 1 : 0;
    a.place_cost[i] = cj;
    a.place_len[i] = Lj;
}

__global__ __launch_bounds__(64) void rrtstar_commit_kernel(const RrtStarArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int P = a.P, K = a.K, dof = a.dof, cap = a.cap;
    const int64_t e = r * P + lane;
    const bool slot = lane < P;
    const bool running = a.status[r] == 0;
    const int c0n = max(0, min(a.count[r], cap));
    const bool app = slot && star_candidate(a, r, e);
    const u64 bal = __ballot(app);
    const int total = __popcll(bal);
    const int at = c0n + __popcll(bal & ((1ull << lane) - 1ull));
    const bool fits = app && at < cap;
    bool is_goal = false;
    if (fits) {
        const float* const tree = a.nodes + r * (int64_t)cap * dof;
        const float* const cost = a.cost + r * (int64_t)cap;
        const float* const x = a.qb + e * dof;
        int par = a.near[e];
        float len = sqrtf(star_len2(tree + (int64_t)par * dof, x, dof, a.wrap_mask));
        float c = cost[par] + len;
        u64 bestk = kRrtEmpty;
        for (int j = 0; j < K; ++j) {
            const int64_t i = e * K + j;
            if (a.submitted[i] && a.place_hit[i] == -1) {
                const u64 key = ((u64)__float_as_uint(a.place_cost[i]) << 32) | (u64)(uint32_t)a.near_idx[i];
                if (key < bestk) {
                    bestk = key;
                    par = a.near_idx[i];
                    len = a.place_len[i];
                    c = a.place_cost[i];
                }
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
        a.cost[r * (int64_t)cap + at] = c;
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

__global__ __launch_bounds__(kRrtStarPlaceThreads) void rrtstar_rewire_prepare_kernel(const RrtStarArgs a) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kRrtStarPlaceThreads + threadIdx.x;
    if (i >= (int64_t)a.R * a.P * a.K) return;
    const int64_t e = i / a.K, r = e / a.P;
    const int dof = a.dof;
    const float* const tree = a.nodes + r * (int64_t)a.cap * dof;
    const int v = a.near_idx[i];
    const int at = a.added[e];
    bool submit = false;
    float c = 0.0f, L = 0.0f;
    if (at >= 0 && v >= 0 && v != a.parent[r * (int64_t)a.cap + at]) {
        const float* const cost = a.cost + r * (int64_t)a.cap;
        L = sqrtf(a.near_d2[i]);   // correctly rounded: the length of the directed edge x -> v
        c = cost[at] + L;
        submit = c < cost[v];      // v is a node of the snapshot: its cost is the snapshot's until the refresh
    }
    star_put_edge(a, i, a.qb + e * dof, tree + (int64_t)max(v, 0) * dof, tree, submit);
    a.submitted[i] = submit ? 1 : 0;
    a.place_cost[i] = c;
    a.place_len[i] = L;
}

__global__ __launch_bounds__(kRrtStarPlaceThreads) void rrtstar_rewire_select_kernel(const RrtStarArgs a) {
    __shared__ int sV[kRrtStarPlaceThreads];
    __shared__ u64 sKey[kRrtStarPlaceThreads];
    const int t = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int places = a.P * a.K;
    int v = -1;
    u64 key = kRrtEmpty;
    int64_t i = 0;
    if (t < places) {
        i = r * places + t;
        if (a.submitted[i] && a.place_hit[i] == -1) {
            v = a.near_idx[i];
            key = ((u64)__float_as_uint(a.place_cost[i]) << 32) | (u64)(uint32_t)(t / a.K);   // (bits(c'), p)
        }
    }
    sV[t] = v;
    sKey[t] = key;
    __syncthreads();
    bool wins = v >= 0;
    if (wins)
        for (int o = 0; o < places; ++o)
            if (o != t && sV[o] == v && sKey[o] < key) wins = false;   // (the slots of one v differ in p: no two keys are equal)
    if (wins) {
        const int64_t e = i / a.K;
        a.parent[r * (int64_t)a.cap + v] = a.added[e];
        a.elen[r * (int64_t)a.cap + v] = a.place_len[i];
    }
    const int any = __syncthreads_or(wins ? 1 : 0);
    if (t == 0 && any) a.rewired[r] = 1;
}

__global__ __launch_bounds__(kRrtStarRefreshThreads) void rrtstar_refresh_kernel(const RrtStarArgs a) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    if (!a.rewired[r]) return;   // (block-uniform)
    const int n = max(0, min(a.count[r], a.cap));
    const int32_t* const parent = a.parent + r * (int64_t)a.cap;
    const float* const elen = a.elen + r * (int64_t)a.cap;
    float* const cost = a.cost + r * (int64_t)a.cap;
    // Every pass reads what the passes before it wrote (and maybe some of its own writes: either is a value on the way to the
    // fixed point).  A pass without a write has read the final values alone: every equation holds.  The parent graph is a tree,
    // so a node is final one pass after its parent: at most depth + 1 <= n + 1 passes.
    for (int pass = 0; pass <= n; ++pass) {
        int changed = 0;
        for (int i = tid; i < n; i += kRrtStarRefreshThreads) {
            const int p = parent[i];
            if (p < 0 || p >= n) continue;   // the root
            const float c = __hip_atomic_load(cost + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) + elen[i];
            if (__float_as_uint(c) != __float_as_uint(__hip_atomic_load(cost + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) {
                __hip_atomic_store(cost + i, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                changed = 1;
            }
        }
        __threadfence_block();
        if (!__syncthreads_or(changed)) break;
    }
}

__global__ __launch_bounds__(64) void rrtstar_extract_kernel(const RrtStarExtractArgs a) {
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int cap = a.cap, dof = a.dof;
    const int n = max(0, min(a.count[r], cap));
    const int start = a.goal_node[r];
    const int32_t* const par = a.parent + r * (int64_t)cap;
    // the chain's nodes, goal node .. root: at most count of them, every index inside the tree  (wave-uniform)
    int depth = 0;
    bool ok = start >= 0;
    for (int i = start; ok && i != -1; i = par[i]) {
        if (i < 0 || i >= n || depth >= n) {
            ok = false;
            break;
        }
        ++depth;
    }
    if (!ok || depth > a.W) {
        if (lane == 0) a.count_out[r] = ok ? -depth : 0;
        return;
    }
    const float* const nodes = a.nodes + r * (int64_t)cap * dof;
    float* const row = a.path + r * (int64_t)a.W * dof;
    int i = start;
    for (int h = 0; h < depth; ++h) {
        for (int j = lane; j < dof; j += 64) row[(int64_t)(depth - 1 - h) * dof + j] = nodes[(int64_t)i * dof + j];
        i = par[i];
    }
    if (lane == 0) a.count_out[r] = depth;
}

inline unsigned place_blocks(const RrtStarArgs& a) {
    return (unsigned)(((int64_t)a.R * a.P * a.K + kRrtStarPlaceThreads - 1) / kRrtStarPlaceThreads);
}
}  // namespace

hipError_t launch_rrtstar_near(const RrtStarArgs& a, hipStream_t st) {
    rrtstar_near_kernel<<<dim3((unsigned)((int64_t)a.R * a.P)), dim3(64), 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_rrtstar_choose_prepare(const RrtStarArgs& a, hipStream_t st) {
    rrtstar_choose_prepare_kernel<<<dim3(place_blocks(a)), dim3(kRrtStarPlaceThreads), 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_rrtstar_commit(const RrtStarArgs& a, hipStream_t st) {
    rrtstar_commit_kernel<<<dim3((unsigned)a.R), dim3(64), 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_rrtstar_rewire_prepare(const RrtStarArgs& a, hipStream_t st) {
    rrtstar_rewire_prepare_kernel<<<dim3(place_blocks(a)), dim3(kRrtStarPlaceThreads), 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_rrtstar_rewire_select(const RrtStarArgs& a, hipStream_t st) {
    rrtstar_rewire_select_kernel<<<dim3((unsigned)a.R), dim3(kRrtStarPlaceThreads), 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_rrtstar_refresh(const RrtStarArgs& a, hipStream_t st) {
    rrtstar_refresh_kernel<<<dim3((unsigned)a.R), dim3(kRrtStarRefreshThreads), 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_rrtstar_extract(const RrtStarExtractArgs& a, hipStream_t st) {
    rrtstar_extract_kernel<<<dim3((unsigned)a.R), dim3(64), 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace dcx
