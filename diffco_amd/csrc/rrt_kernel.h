// rrt_kernel.h — what dcx_rrt_connect_run's host side (dcx_api.hip) and its kernels (rrt_kernels.hip) share: the launches'
// arguments and THE plan of the workspace.  dcx_rrt_work_bytes and dcx_rrt_connect_run both call rrt_plan, so the workspace a
// caller was told to bring is the one the rounds use.  (The planners' shared checks: dcx_api.hip PlannerCheck, PlannerEdges.)
//
// One round of R problems is six steps on the caller's stream (include/dcx.h, "batched RRT-Connect"):
//   nearest + steer (phase 1) -> dcx_check_motions_ex on the R * P edges -> commit (phase 1)
//   nearest         (phase 2) -> dcx_check_motions_ex on the R * P edges -> commit (phase 2)
// The edge batch always has R * P edges in (r, p) order; a slot with nothing to check submits the zero-length edge on the
// problem's start node, so the motion sweep's geometry never depends on the state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dcx.h"
#include "work_layout.h"

namespace dcx {

constexpr int kRrtWaves = 4;        // waves of a nearest block: they divide the tree's nodes, lanes across nodes
constexpr int kRrtMaxSlots = DCX_RRT_MAX_SLOTS;   // P: a lane's best keys are kRrtMaxSlots 64-bit registers
constexpr int kRrtRegDof = 8;       // node rows of up to this many coordinates sit in registers while the P slots read them
constexpr unsigned long long kRrtEmpty = ~0ull;   // "no admissible node": above every real key (knn_kernel.h kKnnEmpty)

// the workspace (work_layout.h): dcx_check_motions' for E = R * P edges first (motion_work's offsets), then the per-slot scratch
struct RrtPlan {
    size_t qa, qb;        // [E, dof] floats: the edge batch
    size_t near;          // [E] int32: the edge's start node in its tree, -1 for a slot with nothing to check
    size_t added;         // [E] int32: phase 1's append index of the slot's new node in tree a, -1 none
    size_t first_hit;     // [E] int32: the motion check's answers
    size_t full;          // [R] int32: a slot of this round did not fit
    size_t total;
};

inline RrtPlan rrt_plan(int64_t R, int32_t P, int32_t dof, size_t motion_bytes) {
    const size_t E = (size_t)R * (size_t)P;
    WorkCarve c;
    c.take(motion_bytes);   // dcx_check_motions' workspace, at the head
    RrtPlan w;
    w.qa = c.take_n<float>(E * dof);
    w.qb = c.take_n<float>(E * dof);
    w.near = c.take_n<int32_t>(E);
    w.added = c.take_n<int32_t>(E);
    w.first_hit = c.take_n<int32_t>(E);
    w.full = c.take_n<int32_t>((size_t)R);
    w.total = c.at;
    return w;
}

struct RrtArgs {
    // the caller's state (dcx_rrt_state; RRT* searches and steers with trees = 1: nodes [R, cap, dof], count [R], phase 1 alone)
    float* nodes;             // [R, trees, cap, dof]
    int32_t* parent;          // [R, 2, cap]
    int32_t* count;           // [R, trees]
    int32_t* status;          // [R]
    int32_t* link;            // [R, 2]
    int32_t* solved_round;    // [R]
    const float* samples;     // [R, P, dof]: this round's targets
    // the workspace
    float* qa;
    float* qb;
    int32_t* near;
    int32_t* added;
    const int32_t* first_hit;
    int32_t* full;
    const float* frac;        // [E]: the motion prep's step fractions of the batch just checked (commit of phase 2)
    int32_t R, P, cap, dof;
    int32_t trees;            // 2: RRT-Connect's pair;  1: RRT*'s one tree (rrtstar_kernel.h), nearest + steer only
    int32_t phase;            // 1: extend tree a towards the samples;  2: connect tree b to phase 1's new nodes
    int32_t tree;             // a = g & 1
    int32_t round;            // g
    float range;
    uint64_t wrap_mask;
};

hipError_t launch_rrt_nearest(const RrtArgs& a, hipStream_t stream);
hipError_t launch_rrt_commit(const RrtArgs& a, hipStream_t stream);

}  // namespace dcx
