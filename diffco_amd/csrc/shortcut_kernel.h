// shortcut_kernel.h — what dcx_path_shortcut_run's and dcx_rrt_extract_paths' host side (dcx_api.hip) and their kernels
// (shortcut_kernels.hip) share: the launches' arguments and THE plan of the workspace.  dcx_path_shortcut_work_bytes and
// dcx_path_shortcut_run both call shortcut_plan, so the workspace a caller was told to bring is the one the rounds use.  The
// call shares its host body with the partial mode (dcx_api.hip shortcut_run) and its checks with RRT-Connect (PlannerCheck).
//
// One round of R paths is three steps on the caller's stream (include/dcx.h, "batched path shortcutting"):
//   pick -> dcx_check_motions_ex on the R * P edges -> commit
// The edge batch always has R * P edges in (r, p) order; an idle slot submits the zero-length edge on the path's first
// waypoint, so the motion sweep's geometry never depends on the state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dcx.h"
#include "work_layout.h"

namespace dcx {

constexpr int kShortcutMaxSlots = DCX_SHORTCUT_MAX_SLOTS;   // P: the commit's selection is at most P * (P - 1) / 2 comparisons
constexpr int kShortcutThreads = 256;   // threads of a commit block
constexpr int kShortcutChunk = 4;       // floats a commit thread holds in registers between a chunk's reads and its writes

// the workspace (work_layout.h): dcx_check_motions' for E = R * P edges first (motion_work's offsets), then the per-slot scratch
struct ShortcutPlan {
    size_t qa, qb;        // [E, dof] floats: the edge batch
    size_t first_hit;     // [E] int32: the motion check's answers
    size_t picks;         // [E, 2] int32: the slot's (i, j), (-1, -1) for an idle slot
    size_t total;
};

inline ShortcutPlan shortcut_plan(int64_t R, int32_t P, int32_t dof, size_t motion_bytes) {
    const size_t E = (size_t)R * (size_t)P;
    WorkCarve c;
    c.take(motion_bytes);   // dcx_check_motions' workspace, at the head
    ShortcutPlan w;
    w.qa = c.take_n<float>(E * dof);
    w.qb = c.take_n<float>(E * dof);
    w.first_hit = c.take_n<int32_t>(E);
    w.picks = c.take_n<int32_t>(E * 2);
    w.total = c.at;
    return w;
}

struct ShortcutArgs {
    // the caller's state (dcx_shortcut_state)
    float* path;              // [R, W, dof]
    int32_t* count;           // [R]
    int32_t* accepted;        // [R]
    const float* draws;       // [R, P, 2]: this round's draws
    // the workspace
    float* qa;
    float* qb;
    const int32_t* first_hit;
    int32_t* picks;
    int32_t R, P, W, dof;
};

struct ExtractArgs {
    // the planner's state (dcx_rrt_state)
    const float* nodes;       // [R, 2, cap, dof]
    const int32_t* parent;    // [R, 2, cap]
    const int32_t* status;    // [R]
    const int32_t* link;      // [R, 2]
    float* path;              // [R, W, dof]
    int32_t* count;           // [R]
    int32_t R, cap, dof, W;
};

// THE pick of include/dcx.h's step 1 (dcx_path_shortcut_run and dcx_path_shortcut_run_cost draw the same (i, j) from the same
// draws): (-1, -1) for an idle slot
__device__ __forceinline__ void shortcut_pick_ij(const int n, const float u0, const float u1, int& i, int& j) {
#pragma clang fp contract(off)
    i = -1;
    j = -1;
    if (n >= 3 && u0 >= 0.0f && u0 < 1.0f && u1 >= 0.0f && u1 < 1.0f) {   // (a NaN fails the comparisons)
        i = min((int)(u0 * (float)(n - 2)), n - 3);
        const int m = n - 2 - i;
        j = i + 2 + min((int)(u1 * (float)m), m - 1);
    }
}

// THE in-place compaction of the vertex modes: the floats [begin, end) of `row`, `width` floats per entry, moved down past the
// applied intervals (si, sj) (INT_MAX, INT_MAX where a slot is not applied) in ascending chunks - a chunk is read into registers,
// one barrier, then written.  An entry never moves up, so what a chunk overwrites has been read by then, by this chunk or an
// earlier one; an entry's new index is a closed form of the intervals: no scan.  Waypoint k dies where si < k < sj; with
// kSegments the entries are segments k -> k + 1, which die where si <= k < sj (the chord's own cost goes to si afterwards).
// Every thread of the block calls it (begin and end are block-uniform).  On return every read of the row is done.
template <bool kSegments>
__device__ __forceinline__ void shortcut_compact(float* const row, const int begin, const int end, const int width,
                                                 const int (&si)[kShortcutMaxSlots], const int (&sj)[kShortcutMaxSlots]) {
    const int tid = threadIdx.x;
    for (int base = begin; base < end; base += kShortcutThreads * kShortcutChunk) {
        float v[kShortcutChunk];
        int dst[kShortcutChunk];
#pragma unroll
        for (int u = 0; u < kShortcutChunk; ++u) {
            const int at = base + u * kShortcutThreads + tid;
            dst[u] = -1;
            v[u] = 0.0f;
            if (at < end) {
                const int k = at / width;
                bool dead = false;
                int shift = 0;
#pragma unroll
                for (int p = 0; p < kShortcutMaxSlots; ++p) {
                    dead = dead || ((kSegments ? si[p] <= k : si[p] < k) && k < sj[p]);
                    shift += sj[p] <= k ? sj[p] - si[p] - 1 : 0;
                }
                if (!dead) {
                    v[u] = row[at];
                    dst[u] = at - shift * width;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kShortcutChunk; ++u)
            if (dst[u] >= 0) row[dst[u]] = v[u];
    }
}

hipError_t launch_shortcut_pick(const ShortcutArgs& a, hipStream_t stream);
hipError_t launch_shortcut_commit(const ShortcutArgs& a, hipStream_t stream);
hipError_t launch_rrt_extract(const ExtractArgs& a, hipStream_t stream);

}  // namespace dcx
