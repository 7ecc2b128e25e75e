// shortcut_kernels.hip — the path logic of dcx_path_shortcut_run and dcx_rrt_extract_paths (include/dcx.h, "batched path
// shortcutting and RRT path extraction"; shortcut_kernel.h): R paths simplified in lockstep, P slots per path and round.  The
// edge checks between pick and commit are dcx_check_motions_ex's.
//   pick:    one thread per (r, p): the slot's waypoints (i, j) from the round's two draws, its edge into the batch.
//   commit:  one block per path.  The P picks and verdicts are block-uniform, so every thread selects the applied slots in
//            slot order by itself (at most 16 * 15 / 2 interval comparisons on uniform values).  A block with nothing applied
//            leaves at once.  The survivors are moved down in place, in ascending chunks: a chunk is read into registers, one
//            barrier, then written.  A waypoint never moves up, so what a chunk overwrites has been read by then - by this
//            chunk or an earlier one - and a waypoint's new index is a closed form of the applied intervals: no scan.  (The pick
//            and this compaction are shortcut_kernel.h's shortcut_pick_ij and shortcut_compact: the rounds under the clearance
//            objective, shortcut_cost_kernels.hip, run the same definitions.)
//   extract: one wave per problem, a half-wave per tree: each chain is walked once for its depth and once more to write its
//            rows, the half's lanes across the coordinates.
// Waypoints are copied, never recomputed, and no atomic decides anything: the state after a round is a function of the state
// before it and the round's draws.
#include <hip/hip_runtime.h>
#include <limits.h>
#include "shortcut_kernel.h"

namespace dcx {
namespace {

__global__ __launch_bounds__(kShortcutThreads) void shortcut_pick_kernel(const ShortcutArgs a) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * kShortcutThreads + threadIdx.x;
    if (e >= (int64_t)a.R * a.P) return;
    const int64_t r = e / a.P;
    const int dof = a.dof;
    const int n = max(0, min(a.count[r], a.W));   // (a count beyond W is the caller's error: never read past the row)
    const float u0 = a.draws[e * 2], u1 = a.draws[e * 2 + 1];
    int i, j;
    shortcut_pick_ij(n, u0, u1, i, j);
    // an idle slot: the zero-length edge on the path's first row, one sample, its verdict ignored
    const float* const row = a.path + r * (int64_t)a.W * dof;
    const float* const wa = row + (int64_t)max(i, 0) * dof;
    const float* const wb = row + (int64_t)max(j, 0) * dof;
    float* const qa = a.qa + e * dof;
    float* const qb = a.qb + e * dof;
    for (int c = 0; c < dof; ++c) {
        qa[c] = wa[c];
        qb[c] = wb[c];
    }
    a.picks[e * 2] = i;
    a.picks[e * 2 + 1] = j;
}

__global__ __launch_bounds__(kShortcutThreads) void shortcut_commit_kernel(const ShortcutArgs a) {
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int P = a.P, dof = a.dof;
    const int n = max(0, min(a.count[r], a.W));

    // the applied slots, in slot order (block-uniform).  A slot that is not applied keeps the empty interval (INT_MAX, INT_MAX):
    // it lies inside no waypoint's past and crosses nothing.
    int si[kShortcutMaxSlots], sj[kShortcutMaxSlots];
    int applied = 0, removed = 0, lo = INT_MAX;
#pragma unroll
    for (int p = 0; p < kShortcutMaxSlots; ++p) {
        si[p] = INT_MAX;
        sj[p] = INT_MAX;
        if (p < P) {
            const int64_t e = r * P + p;
            const int i = a.picks[e * 2], j = a.picks[e * 2 + 1];
            bool ok = a.first_hit[e] == -1 && i >= 0 && i + 2 <= j && j <= n - 1;
#pragma unroll
            for (int q = 0; q < p; ++q) ok = ok && (j <= si[q] || sj[q] <= i);
            if (ok) {
                si[p] = i;
                sj[p] = j;
                ++applied;
                removed += j - i - 1;
                lo = min(lo, i);
            }
        }
    }
    if (applied == 0) return;   // (block-uniform) the common case late in a run

    // waypoints 0 .. lo stay where they are; the floats of the rest in ascending chunks
    float* const row = a.path + r * (int64_t)a.W * dof;
    shortcut_compact<false>(row, (lo + 1) * dof, n * dof, dof, si, sj);   // (W * dof <= 65536 * DCX_MAX_DOF)
    __syncthreads();   // every thread has read count[r]
    if (tid == 0) {
        a.count[r] = n - removed;
        a.accepted[r] += applied;
    }
}

__global__ __launch_bounds__(64) void rrt_extract_kernel(const ExtractArgs a) {
    const int lane = threadIdx.x, t = lane >> 5, sub = lane & 31;   // lanes 0 .. 31 walk tree 0, lanes 32 .. 63 tree 1
    const int64_t r = blockIdx.x;
    const int cap = a.cap, dof = a.dof;
    if (a.status[r] != 1) {   // (wave-uniform)
        if (lane == 0) a.count[r] = 0;
        return;
    }
    const int32_t* const par = a.parent + (r * 2 + t) * (int64_t)cap;
    const int start = a.link[r * 2 + t];
    // the chain's nodes, start .. root: at most cap of them, every index inside the tree
    int depth = 0;
    bool ok = true;
    for (int i = start; i != -1; i = par[i]) {
        if (i < 0 || i >= cap || depth >= cap) {
            ok = false;
            break;
        }
        ++depth;
    }
    ok = ok && depth >= 1;
    const int d0 = __shfl(depth, 0, 64), d1 = __shfl(depth, 32, 64);
    const bool both = __shfl((int)ok, 0, 64) != 0 && __shfl((int)ok, 32, 64) != 0;
    const int n = d0 + d1;
    if (!both || n > a.W) {   // (wave-uniform)
        if (lane == 0) a.count[r] = both ? -n : 0;
        return;
    }
    // tree 0's chain ends the first d0 rows (its root first), tree 1's begins the rest (its link node first)
    const float* const nodes = a.nodes + (r * 2 + t) * (int64_t)cap * dof;
    float* const row = a.path + r * (int64_t)a.W * dof;
    int i = start;
    for (int h = 0; h < depth; ++h) {
        const int at = t == 0 ? d0 - 1 - h : d0 + h;
        for (int c = sub; c < dof; c += 32) row[(int64_t)at * dof + c] = nodes[(int64_t)i * dof + c];
        i = par[i];
    }
    if (lane == 0) a.count[r] = n;
}
}  // namespace

hipError_t launch_shortcut_pick(const ShortcutArgs& a, hipStream_t st) {
    const int64_t E = (int64_t)a.R * a.P;
    shortcut_pick_kernel<<<dim3((unsigned)((E + kShortcutThreads - 1) / kShortcutThreads)), dim3(kShortcutThreads), 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_shortcut_commit(const ShortcutArgs& a, hipStream_t st) {
    shortcut_commit_kernel<<<dim3((unsigned)a.R), dim3(kShortcutThreads), 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_rrt_extract(const ExtractArgs& a, hipStream_t st) {
    rrt_extract_kernel<<<dim3((unsigned)a.R), dim3(64), 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace dcx
