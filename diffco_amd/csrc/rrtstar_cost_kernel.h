// rrtstar_cost_kernel.h — what dcx_rrtstar_run_cost's host side (dcx_api.hip) and its kernels (rrtstar_cost_kernels.hip) share:
// the launches' arguments and THE plan of the workspace (include/dcx.h, "batched RRT*: clearance-weighted edge costs").
//
// One round; E = R * P slots, K = opts->near.  (*) marks the launches of the length planner, taken as they are:
//   nearest + steer (*) -> dcx_motion_worst on the E edges near -> x -> extend settle (first_hit from worst0; C0, c0)
//   near (*) -> choose prepare (the lower bound against c0) -> dcx_motion_worst on the E * K edges u_j -> x
//   commit (Cj, cj from the places' worst; parent choice, append, goal)
//   rewire prepare (*; its test IS the lower bound cost[x] + L' < cost[v]) -> dcx_motion_worst on the E * K edges x -> u_j
//   -> rewire settle (place_len = C', place_cost = c', place_hit, submitted from the places' worst) -> rewire select (*)
//   refresh (*)
// The settle kernels rewrite the words the length planner's launches read, so those launches run unchanged.
#pragma once
#include "rrtstar_kernel.h"

namespace dcx {

// the workspace: dcx_rrtstar_run's (rrtstar_plan, with dcx_motion_worst's workspace for the larger batch at its head), then the
// batches' worst arrays (dcx_motion_worst wants a worst_idx beside each) and the slots' own edge costs
struct RrtStarCostPlan {
    RrtStarPlan run;
    size_t worst0, widx0;     // [E] float, int32: the extend batch's worst and worst_idx
    size_t slot_len;          // [E] float: C0
    size_t slot_cost;         // [E] float: c0
    size_t place_worst;       // [E * K] float: the choose batch's worst, then the rewire batch's
    size_t place_widx;        // [E * K] int32
    size_t total;
};

inline RrtStarCostPlan rrtstar_cost_plan(int64_t R, int32_t P, int32_t K, int32_t dof, size_t worst_bytes) {
    const size_t E = (size_t)R * (size_t)P, EK = E * (size_t)K;
    RrtStarCostPlan w;
    w.run = rrtstar_plan(R, P, K, dof, worst_bytes);
    WorkCarve c;
    c.take(w.run.total);
    w.worst0 = c.take_n<float>(E);
    w.widx0 = c.take_n<int32_t>(E);
    w.slot_len = c.take_n<float>(E);
    w.slot_cost = c.take_n<float>(E);
    w.place_worst = c.take_n<float>(EK);
    w.place_widx = c.take_n<int32_t>(EK);
    w.total = c.at;
    return w;
}

// dcx_rrtstar_run_sampled_cost's workspace: the above, then one round's sample rows
struct RrtStarSampledCostPlan {
    RrtStarCostPlan run;
    size_t samples;           // [E, dof] floats
    size_t total;
};

inline RrtStarSampledCostPlan rrtstar_sampled_cost_plan(int64_t R, int32_t P, int32_t K, int32_t dof, size_t worst_bytes) {
    RrtStarSampledCostPlan w;
    w.run = rrtstar_cost_plan(R, P, K, dof, worst_bytes);
    WorkCarve c;
    c.take(w.run.total);
    w.samples = c.take_n<float>((size_t)R * (size_t)P * dof);
    w.total = c.at;
    return w;
}

struct RrtStarCostArgs {
    RrtStarArgs a;             // the length planner's arguments over run's slots: what its launches take
    int32_t* first_hit;        // a.first_hit and a.place_hit, writable: the settle kernels form them from the worst arrays
    int32_t* place_hit;
    const float* worst0;       // [E]
    float* slot_len;           // [E]
    float* slot_cost;          // [E]
    const float* place_worst;  // [E * K]
    float gain, band;
};

hipError_t launch_rrtstar_cost_extend_settle(const RrtStarCostArgs& c, hipStream_t stream);
hipError_t launch_rrtstar_cost_choose_prepare(const RrtStarCostArgs& c, hipStream_t stream);
hipError_t launch_rrtstar_cost_commit(const RrtStarCostArgs& c, hipStream_t stream);
hipError_t launch_rrtstar_cost_rewire_settle(const RrtStarCostArgs& c, hipStream_t stream);

}  // namespace dcx
