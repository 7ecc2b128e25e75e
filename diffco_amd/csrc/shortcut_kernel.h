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

hipError_t launch_shortcut_pick(const ShortcutArgs& a, hipStream_t stream);
hipError_t launch_shortcut_commit(const ShortcutArgs& a, hipStream_t stream);
hipError_t launch_rrt_extract(const ExtractArgs& a, hipStream_t stream);

}  // namespace dcx
