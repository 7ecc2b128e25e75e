// shortcut_partial_kernels.hip — the path logic of dcx_path_shortcut_partial_run (include/dcx.h, "Partial shortcuts";
// shortcut_partial_kernel.h): R paths simplified in lockstep, P slots per path and round, each slot a chord between two points
// inside segments.  The edge checks between pick and commit are dcx_check_motions_ex's.
//   pick:    one block per path.  The four arc-length phases of arclen_device.h (the resampler's, the same definition), then one
//            thread per float of the slots' two points (p, end, j): the two binary searches over c and the interpolation, the
//            point into the edge batch (coalesced), (ea, eb) into the picks.  The 2 * dof threads of a slot repeat the searches
//            (<= 16 reads of c each) instead of sharing them through another barrier.  A path of fewer than three waypoints
//            skips the arc length (block-uniform) and idles its slots.
//   commit:  one block per path.  The P picks and verdicts are block-uniform, so every thread selects the applied slots in
//            slot order by itself (at most 16 * 15 / 2 interval comparisons plus the running count).  A block with nothing
//            applied leaves at once.  The vertex mode's in-place compaction does not carry over: it relies on a waypoint never
//            moving up, and here a waypoint moves up by as much as the number of growing slots (eb = ea + 1) before it, so an
//            ascending in-place copy would overwrite rows that have not been read yet.  The rewritten tail - the survivors
//            after the first applied slot and the slots' xa, xb - is therefore written to the path's own row of a [R, W, dof]
//            stage in the workspace, one barrier, then copied back by the same block: no row of the path is written before
//            every read of the path is done.  A survivor's new index is a closed form of the applied intervals: no scan.
// Waypoints are copied, the two points of a slot computed once (by the pick; what was checked is what is written), and no
// atomic decides anything: the state after a round is a function of the state before it and the round's draws.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include "shortcut_partial_kernel.h"
#include "arclen_device.h"

namespace dcx {
namespace {

// the slots of path r: `live` (block-uniform) says whether the path has an arc length to draw on
template <bool kLds>
__device__ __forceinline__ void partial_slots(const ShortcutPartialArgs& a, const int64_t r, const int n, const bool live, const float L,
                                              const float* const c, const float* const ln) {
#pragma clang fp contract(off)
    const int dof = a.dof, P = a.P;
    const uint64_t mask = a.wrap_mask;
    const float* const row = a.path + r * (int64_t)a.W * dof;
    const int total = P * 2 * dof;   // (<= 16 * 2 * DCX_MAX_DOF)
    for (int i = threadIdx.x; i < total; i += kResampleThreads) {
        const int p = i / (2 * dof), rem = i - p * 2 * dof;
        const int end = rem / dof, j = rem - end * dof;
        const int64_t e = r * P + p;
        const float u0 = a.draws[e * 2], u1 = a.draws[e * 2 + 1];
        int ea, eb;
        float sa, sb;
        const bool ok = arc_pick<kLds>(c, n, live, L, u0, u1, ea, eb, sa, sb);
        // an idle slot: the zero-length edge on the path's first row, one sample, its verdict ignored
        float v = row[j];
        if (ok) v = end ? arc_point<kLds>(row, c, ln, dof, mask, eb, sb, j) : arc_point<kLds>(row, c, ln, dof, mask, ea, sa, j);
        (end ? a.qb : a.qa)[e * dof + j] = v;
        if (rem == 0) {
            a.picks[e * 2] = ok ? ea : -1;
            a.picks[e * 2 + 1] = ok ? eb : -1;
        }
    }
}

template <bool kLds>
__device__ __forceinline__ void partial_pick_path(const ShortcutPartialArgs& a, const int64_t r, const int n, float* const c,
                                                  float* const ln, float* const sB) {
    path_arc_length<kLds>(a.path + r * (int64_t)a.W * a.dof, n, a.dof, a.wrap_mask, c, ln, sB);
    const float L = c[arc_slot<kLds>(n - 1)];
    partial_slots<kLds>(a, r, n, L > 0.0f && L < INFINITY, L, c, ln);   // (block-uniform; a NaN fails it)
}

__global__ __launch_bounds__(kResampleThreads) void shortcut_partial_pick_kernel(const ShortcutPartialArgs a) {
    constexpr int kSlots = kResampleLdsWaypoints + kResampleLdsWaypoints / kResampleChunk;
    __shared__ float sC[kSlots];
    __shared__ float sLen[kSlots];
    __shared__ float sB[kResampleMaxChunks];
    const int64_t r = blockIdx.x;
    const int n = max(0, min(a.count[r], a.W));   // (a count beyond W is the caller's error: never read past the row)
    if (n < 3) partial_slots<true>(a, r, n, false, 0.0f, sC, sLen);   // (block-uniform: no barrier is skipped by a part of the block)
    else if (n <= kResampleLdsWaypoints) partial_pick_path<true>(a, r, n, sC, sLen, sB);
    else partial_pick_path<false>(a, r, n, a.work_c + r * (int64_t)a.W, a.work_len + r * (int64_t)a.W, sB);
}

__global__ __launch_bounds__(kShortcutThreads) void shortcut_partial_commit_kernel(const ShortcutPartialArgs a) {
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int P = a.P, dof = a.dof, W = a.W;
    const int n = max(0, min(a.count[r], W));

    // the applied slots, in slot order (block-uniform).  A slot that is not applied keeps the empty interval (INT_MAX, INT_MAX):
    // it removes no waypoint, lies before no waypoint and shares a segment with nothing.
    int sa[kShortcutMaxSlots], sb[kShortcutMaxSlots];
    int applied = 0, cnt = n, lo = INT_MAX;
#pragma unroll
    for (int p = 0; p < kShortcutMaxSlots; ++p) {
        sa[p] = INT_MAX;
        sb[p] = INT_MAX;
        if (p < P) {
            const int64_t e = r * P + p;
            const int ea = a.picks[e * 2], eb = a.picks[e * 2 + 1];
            bool ok = a.first_hit[e] == -1 && ea >= 0 && ea < eb && eb + 1 <= n - 1;
#pragma unroll
            for (int q = 0; q < p; ++q) ok = ok && (eb < sa[q] || sb[q] < ea);
            ok = ok && cnt + 2 - (eb - ea) <= W;
            if (ok) {
                sa[p] = ea;
                sb[p] = eb;
                ++applied;
                cnt += 2 - (eb - ea);
                lo = min(lo, ea);
            }
        }
    }
    if (applied == 0) return;   // (block-uniform) the common case late in a run

    // waypoints 0 .. lo stay where they are.  The survivors beyond them into the stage, at their new index ...
    float* const row = a.path + r * (int64_t)W * dof;
    float* const stage = a.stage + r * (int64_t)W * dof;
    const int begin = (lo + 1) * dof;   // (W * dof <= 65536 * DCX_MAX_DOF)
    for (int at = begin + tid; at < n * dof; at += kShortcutThreads) {
        const int k = at / dof;
        bool dead = false;
        int shift = 0;
#pragma unroll
        for (int p = 0; p < kShortcutMaxSlots; ++p) {
            dead = dead || (sa[p] < k && k <= sb[p]);
            shift += sb[p] < k ? 2 - (sb[p] - sa[p]) : 0;
        }
        if (!dead) stage[at + shift * dof] = row[at];   // (new index k + shift in lo + 3 .. cnt - 1)
    }
    // ... and every applied slot's xa, xb behind its waypoint ea
#pragma unroll
    for (int p = 0; p < kShortcutMaxSlots; ++p) {
        if (sa[p] == INT_MAX) continue;   // (block-uniform)
        int at = sa[p] + 1;
#pragma unroll
        for (int q = 0; q < kShortcutMaxSlots; ++q) at += sb[q] < sa[p] ? 2 - (sb[q] - sa[q]) : 0;
        const int64_t e = r * P + p;
        for (int i = tid; i < 2 * dof; i += kShortcutThreads)
            stage[at * dof + i] = i < dof ? a.qa[e * dof + i] : a.qb[e * dof + i - dof];   // (rows at, at + 1 <= cnt - 2)
    }
    __syncthreads();   // every read of the path's row (and of count[r]) is done; the stage is written
    for (int at = begin + tid; at < cnt * dof; at += kShortcutThreads) row[at] = stage[at];
    if (tid == 0) {
        a.count[r] = cnt;
        a.accepted[r] += applied;
    }
}
}  // namespace

hipError_t launch_shortcut_partial_pick(const ShortcutPartialArgs& a, hipStream_t st) {
    shortcut_partial_pick_kernel<<<dim3((unsigned)a.R), dim3(kResampleThreads), 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_shortcut_partial_commit(const ShortcutPartialArgs& a, hipStream_t st) {
    shortcut_partial_commit_kernel<<<dim3((unsigned)a.R), dim3(kShortcutThreads), 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace dcx
