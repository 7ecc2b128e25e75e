// shortcut_partial_kernel.h — what dcx_path_shortcut_partial_run's host side (dcx_api.hip) and its kernels
// (shortcut_partial_kernels.hip) share: the launches' arguments and THE plan of the workspace.
// dcx_path_shortcut_partial_work_bytes and dcx_path_shortcut_partial_run both call shortcut_partial_plan, so the workspace a
// caller was told to bring is the one the rounds use.  The host body is the vertex mode's (dcx_api.hip shortcut_run).
//
// One round of R paths is three steps on the caller's stream (include/dcx.h, "Partial shortcuts"):
//   pick -> dcx_check_motions_ex on the R * P edges -> commit
// as the vertex mode's (shortcut_kernel.h), with the same fixed batch.  The slot's pick is (ea, eb) in `picks` and the two
// points xa, xb in the edge batch itself (qa, qb): the commit reads them from there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "resample_kernel.h"
#include "shortcut_kernel.h"

namespace dcx {

// the workspace: the vertex mode's (dcx_check_motions' for E = R * P edges, qa, qb, first_hit, picks), then the stage of the
// rewritten rows, then c and len of the rows that do not fit the pick block's LDS (nothing where no row can be that long)
struct ShortcutPartialPlan {
    ShortcutPlan slot;
    size_t stage;         // [R, W, dof] floats
    size_t c, len;        // [R, W] floats each, W > kResampleLdsWaypoints only
    size_t total;
};

inline ShortcutPartialPlan shortcut_partial_plan(int64_t R, int32_t P, int32_t W, int32_t dof, size_t motion_bytes) {
    const size_t rows = (size_t)R * (size_t)W;
    const size_t arc = W > kResampleLdsWaypoints ? rows : 0;
    ShortcutPartialPlan w;
    w.slot = shortcut_plan(R, P, dof, motion_bytes);
    WorkCarve c{w.slot.total};   // the vertex mode's workspace, at the head
    w.stage = c.take_n<float>(rows * (size_t)dof);
    w.c = c.take_n<float>(arc);
    w.len = c.take_n<float>(arc);
    w.total = c.at;
    return w;
}

struct ShortcutPartialArgs {
    // the caller's state (dcx_shortcut_state)
    float* path;              // [R, W, dof]
    int32_t* count;           // [R]
    int32_t* accepted;        // [R]
    const float* draws;       // [R, P, 2]: this round's draws
    // the workspace
    float* qa;                // [E, dof]: xa, or path[r, 0] of an idle slot
    float* qb;                // [E, dof]: xb
    const int32_t* first_hit;
    int32_t* picks;           // [E, 2]: (ea, eb), (-1, -1) for an idle slot
    float* stage;             // [R, W, dof]
    float* work_c;            // [R, W]
    float* work_len;          // [R, W]
    uint64_t wrap_mask;
    int32_t R, P, W, dof;
};

hipError_t launch_shortcut_partial_pick(const ShortcutPartialArgs& a, hipStream_t stream);
hipError_t launch_shortcut_partial_commit(const ShortcutPartialArgs& a, hipStream_t stream);

}  // namespace dcx
