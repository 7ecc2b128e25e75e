// shortcut_cost_kernel.h — what dcx_path_shortcut_run_cost's and dcx_path_shortcut_partial_run_cost's host side (dcx_api.hip) and
// their kernels (shortcut_cost_kernels.hip) share: the launches' arguments and THE plan of the workspace (include/dcx.h,
// "path shortcuts under the clearance objective").  The size queries and the calls all go through shortcut_cost_plan, so the
// workspace a caller was told to bring is the one the rounds use.  The host body is the length modes' (dcx_api.hip shortcut_run).
//
// One round of R paths is three steps on the caller's stream:
//   pick (the slots' edges and their lengths L) -> dcx_motion_worst on the R * P * pieces edges -> price and commit
// pieces = 1 in the vertex mode (the chord path[i] -> path[j]) and 3 in the partial mode (path[ea] -> xa, xa -> xb,
// xb -> path[eb + 1]).  The batch is fixed: an idle slot submits `pieces` zero-length edges on the path's first waypoint.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "shortcut_partial_kernel.h"

namespace dcx {

// a block of the price-and-commit kernels holds the seg row of a path of at most this many waypoints in LDS for the slots' sums
// of the removed span; a longer path's sums read the row from global memory
constexpr int kShortcutCostLdsWaypoints = 2048;

// the workspace: dcx_motion_worst's for E * pieces edges at the head, then the edge batch, its peaks (dcx_motion_worst wants a
// worst_idx beside them), the pieces' lengths, the picks and - the partial mode's alone, nothing in the vertex mode - the stages of
// the rewritten rows and of their seg, and c and len of the rows that do not fit the pick block's LDS
struct ShortcutCostPlan {
    size_t qa, qb;        // [E * pieces, dof] floats: the edge batch
    size_t worst;         // [E * pieces] float
    size_t widx;          // [E * pieces] int32
    size_t len;           // [E * pieces] float: L of every piece
    size_t picks;         // [E, 2] int32: (i, j) or (ea, eb), (-1, -1) for an idle slot
    size_t stage;         // [R, W, dof] floats
    size_t stage_seg;     // [R, W] floats
    size_t arc_c, arc_len;   // [R, W] floats each, W > kResampleLdsWaypoints only
    size_t total;
};

// W = 0: the vertex mode (no stage)
inline ShortcutCostPlan shortcut_cost_plan(int64_t R, int32_t P, int32_t W, int32_t dof, int32_t pieces, size_t worst_bytes) {
    const size_t E = (size_t)R * (size_t)P * (size_t)pieces;
    const size_t rows = (size_t)R * (size_t)W;
    const size_t arc = W > kResampleLdsWaypoints ? rows : 0;
    WorkCarve c;
    c.take(worst_bytes);   // dcx_motion_worst's workspace, at the head
    ShortcutCostPlan w;
    w.qa = c.take_n<float>(E * dof);
    w.qb = c.take_n<float>(E * dof);
    w.worst = c.take_n<float>(E);
    w.widx = c.take_n<int32_t>(E);
    w.len = c.take_n<float>(E);
    w.picks = c.take_n<int32_t>((size_t)R * (size_t)P * 2);
    w.stage = c.take_n<float>(rows * (size_t)dof);
    w.stage_seg = c.take_n<float>(rows);
    w.arc_c = c.take_n<float>(arc);
    w.arc_len = c.take_n<float>(arc);
    w.total = c.at;
    return w;
}

struct ShortcutCostArgs {
    ShortcutPartialArgs a;    // the length modes' arguments (first_hit unused; qa and qb hold `pieces` edges per slot)
    float* seg;               // [R, W]: the caller's segment costs
    float* len;               // [E * pieces]
    const float* worst;       // [E * pieces]
    float* stage_seg;         // [R, W]
    float gain, band;
};

hipError_t launch_shortcut_cost_pick(const ShortcutCostArgs& c, hipStream_t stream);
hipError_t launch_shortcut_cost_commit(const ShortcutCostArgs& c, hipStream_t stream);
hipError_t launch_shortcut_partial_cost_pick(const ShortcutCostArgs& c, hipStream_t stream);
hipError_t launch_shortcut_partial_cost_commit(const ShortcutCostArgs& c, hipStream_t stream);

}  // namespace dcx
