// rrtstar_kernel.h — what dcx_rrtstar_run's host side (dcx_api.hip) and its kernels (rrtstar_kernels.hip) share: the launches'
// arguments and THE plan of the workspace.  dcx_rrtstar_work_bytes and dcx_rrtstar_run both call rrtstar_plan.
//
// One round of R problems on the caller's stream (include/dcx.h, "batched RRT*"); E = R * P slots, K = opts->near:
//   nearest + steer (rrt_kernels.hip's, on the one tree) -> dcx_check_motions_ex on the E edges near -> x
//   near (top K within the radius, K > 0) -> choose prepare -> dcx_check_motions_ex on the E * K edges u_j -> x
//   commit (parent choice, append, goal)
//   rewire prepare -> dcx_check_motions_ex on the E * K edges x -> u_j -> rewire select (K > 0)
//   refresh
// Every batch has its fixed size; a place with nothing to check submits the zero-length edge on the problem's start node.
// dcx_rrtstar_run_sampled puts the sample launch (rrtstar_sample_kernels.hip) in front of each round: the same round otherwise.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dcx.h"
#include "rrt_kernel.h"
#include "work_layout.h"

namespace dcx {

constexpr int kRrtStarMaxNear = DCX_RRTSTAR_MAX_NEAR;   // K: a lane of the near search keeps this many 64-bit keys in registers
constexpr int kRrtStarPlaceThreads = 256;               // the per-place kernels' block; also the most places of one problem (16 * 16)
constexpr int kRrtStarRefreshThreads = 1024;            // the refresh: one block per problem
constexpr int kRrtStarSampleThreads = 256;              // the sample kernel's block: one thread per slot
static_assert(kRrtMaxSlots * kRrtStarMaxNear <= kRrtStarPlaceThreads, "the rewire selection holds a problem's places in one block");

// the workspace (work_layout.h): dcx_check_motions' for the larger batch first (motion_work's offsets; the smaller batch's layout
// is a prefix of it), then the slot scratch [E] and the place scratch [E * K]
struct RrtStarPlan {
    size_t qa, qb;          // [E, dof] floats: the extend batch; qb is the slot's new point x
    size_t near;            // [E] int32: the extend edge's start node, -1 for an idle slot
    size_t first_hit;       // [E] int32: the extend batch's verdicts
    size_t added;           // [E] int32: the append index of the slot's new node, -1 none
    size_t rewired;         // [R] int32: the round changed a parent of this problem
    size_t near_idx;        // [E * K] int32: u_j, -1 unfilled
    size_t near_d2;         // [E * K] floats: dist2_j
    size_t pqa, pqb;        // [E * K, dof] floats: the choose batch, then the rewire batch
    size_t place_hit;       // [E * K] int32: that batch's verdicts
    size_t submitted;       // [E * K] int32: the place is a candidate of the batch
    size_t place_cost;      // [E * K] floats: cj, then c'
    size_t place_len;       // [E * K] floats: Lj, then L'
    size_t total;
};

inline RrtStarPlan rrtstar_plan(int64_t R, int32_t P, int32_t K, int32_t dof, size_t motion_bytes) {
    const size_t E = (size_t)R * (size_t)P, EK = E * (size_t)K;
    WorkCarve c;
    c.take(motion_bytes);   // dcx_check_motions' workspace, at the head
    RrtStarPlan w;
    w.qa = c.take_n<float>(E * dof);
    w.qb = c.take_n<float>(E * dof);
    w.near = c.take_n<int32_t>(E);
    w.first_hit = c.take_n<int32_t>(E);
    w.added = c.take_n<int32_t>(E);
    w.rewired = c.take_n<int32_t>((size_t)R);
    w.near_idx = c.take_n<int32_t>(EK);
    w.near_d2 = c.take_n<float>(EK);
    w.pqa = c.take_n<float>(EK * dof);
    w.pqb = c.take_n<float>(EK * dof);
    w.place_hit = c.take_n<int32_t>(EK);
    w.submitted = c.take_n<int32_t>(EK);
    w.place_cost = c.take_n<float>(EK);
    w.place_len = c.take_n<float>(EK);
    w.total = c.at;
    return w;
}

// dcx_rrtstar_run_sampled's workspace: dcx_rrtstar_run's, then one round's sample rows (used where the caller keeps none)
struct RrtStarSampledPlan {
    RrtStarPlan run;
    size_t samples;         // [E, dof] floats
    size_t total;
};

inline RrtStarSampledPlan rrtstar_sampled_plan(int64_t R, int32_t P, int32_t K, int32_t dof, size_t motion_bytes) {
    RrtStarSampledPlan w;
    w.run = rrtstar_plan(R, P, K, dof, motion_bytes);
    WorkCarve c;
    c.take(w.run.total);
    w.samples = c.take_n<float>((size_t)R * (size_t)P * dof);
    w.total = c.at;
    return w;
}

struct RrtStarArgs {
    // the caller's state (dcx_rrtstar_state)
    float* nodes;             // [R, cap, dof]
    int32_t* parent;          // [R, cap]
    float* elen;              // [R, cap]
    float* cost;              // [R, cap]
    int32_t* count;           // [R]
    int32_t* status;          // [R]
    int32_t* goal_node;       // [R]
    int32_t* first_round;     // [R]
    const float* goals;       // [R, dof]
    // the workspace
    const float* qa;
    const float* qb;
    const int32_t* near;
    const int32_t* first_hit;
    int32_t* added;
    int32_t* rewired;
    int32_t* near_idx;
    float* near_d2;
    float* pqa;
    float* pqb;
    const int32_t* place_hit;
    int32_t* submitted;
    float* place_cost;
    float* place_len;
    int32_t R, P, K, cap, dof;
    int32_t round;            // g
    float max_d2;             // radius * radius
    uint64_t wrap_mask;
};

struct RrtStarExtractArgs {
    const float* nodes;
    const int32_t* parent;
    const int32_t* count;
    const int32_t* goal_node;
    float* path;              // [R, W, dof]
    int32_t* count_out;       // [R]
    int32_t R, cap, dof, W;
};

// one round's samples (rrtstar_sample_kernels.hip; include/dcx.h, "batched RRT*: samples drawn on the device")
struct RrtStarSampleArgs {
    const float* nodes;        // [R, cap, dof]: node 0 is the start
    const float* cost;         // [R, cap]
    const int32_t* status;     // [R]
    const int32_t* goal_node;  // [R]
    const float* goals;        // [R, dof]
    const float* limits;       // [dof, 2]
    float* samples;            // [R, P, dof]
    int32_t* info;             // [R, P] or NULL
    uint64_t seed;
    uint64_t wrap_mask;
    int32_t R, P, cap, dof;
    int32_t round;             // g
    int32_t mode, tries;
    float goal_bias, uniform_mix;
};

hipError_t launch_rrtstar_sample(const RrtStarSampleArgs& a, hipStream_t stream);
hipError_t launch_rrtstar_near(const RrtStarArgs& a, hipStream_t stream);
hipError_t launch_rrtstar_choose_prepare(const RrtStarArgs& a, hipStream_t stream);
hipError_t launch_rrtstar_commit(const RrtStarArgs& a, hipStream_t stream);
hipError_t launch_rrtstar_rewire_prepare(const RrtStarArgs& a, hipStream_t stream);
hipError_t launch_rrtstar_rewire_select(const RrtStarArgs& a, hipStream_t stream);
hipError_t launch_rrtstar_refresh(const RrtStarArgs& a, hipStream_t stream);
hipError_t launch_rrtstar_extract(const RrtStarExtractArgs& a, hipStream_t stream);

}  // namespace dcx
