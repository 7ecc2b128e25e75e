// sssp_lazy_kernel.h — what dcx_sssp_mark_routes' and dcx_graph_apply_checks' host side (dcx_api.hip) and their kernels
// (sssp_lazy_kernels.hip) share: the launches' arguments, their geometry and THE plan of the workspace (include/dcx.h, "lazy
// roadmap queries").  dcx_sssp_mark_routes_work_bytes and dcx_sssp_mark_routes both call lazy_plan.
//
// The marks are bytes, one per edge, taken kLazyGroup at a time: the scan adds a group's 16 marks from one 16-byte load and
// keeps one offset per GROUP, and the scatter's thread lays its group's marked ids behind that offset in id order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dcx.h"
#include "work_layout.h"

namespace dcx {

constexpr int kLazyLanes = 64;          // the mark kernel's block: one wave, one query
constexpr int kLazyGroup = 16;          // marks per group: one 16-byte load
constexpr int kLazyScanThreads = 1024;  // the scan's one workgroup: 1024 groups (16384 edges) per step
constexpr int kLazyThreads = 256;       // threads of the zero, scatter and apply blocks
constexpr int kLazyApplyBlocks = 1024;  // the apply grid's cap: its threads stride over the list

struct LazyPlan {   // offsets into the workspace
    size_t mark;    // uint8 [groups * kLazyGroup]: the marks, padded with zeros to whole groups
    size_t offs;    // int32 [groups + 1]: marked edges before each group
    size_t total;
    int64_t groups;
};

inline LazyPlan lazy_plan(int64_t M) {
    LazyPlan p{};
    p.groups = (M + kLazyGroup - 1) / kLazyGroup;
    WorkCarve w;
    p.mark = w.take_n<uint8_t>((size_t)p.groups * kLazyGroup);
    p.offs = w.take_n<int32_t>((size_t)p.groups + 1);
    p.total = w.at;
    return p;
}

struct LazyMarkArgs {
    // the graph (dcx_graph) and its edges (dcx_lazy_graph)
    const int32_t* rowptr;    // [N + 1]
    const int32_t* col;       // [nnz]
    const int32_t* eid;       // [nnz]
    const int32_t* ends;      // [M, 2]
    const uint8_t* state;     // [M]
    const float* nodes;       // [N, dof]
    // the relaxation's state and the goal links
    const float* dist;        // [N, Q]: the buffer the last round wrote
    const int32_t* pred;      // [N, Q]
    const int32_t* mode;      // [Q]
    const int32_t* goal_idx;  // [Q, k]
    const float* goal_len;    // [Q, k]
    // what the call writes
    int32_t* pending;         // [Q]
    int32_t* list;            // [capacity]
    float* qa;                // [capacity, dof]
    float* qb;                // [capacity, dof]
    int32_t* n_out;           // [2]
    uint8_t* mark;            // the workspace: [groups * kLazyGroup]
    int32_t* offs;            //                [groups + 1]
    int64_t groups, capacity;
    int32_t N, nnz, M, Q, k, dof;
};

struct LazyApplyArgs {
    float* weight;            // [nnz]: written
    const int32_t* ent;       // [M, 2]
    uint8_t* state;           // [M]: written
    const int32_t* list;      // [n_out[1]]
    const int32_t* n_out;     // [2]
    const uint8_t* hit;       // [n_out[1]]
    int32_t* any_blocked;     // [1]
    int32_t nnz, M;
};

// the four launches of dcx_sssp_mark_routes: the marks zeroed, a wave per query, the scan, the scatter
hipError_t launch_lazy_mark_routes(const LazyMarkArgs& a, hipStream_t stream);
// the two launches of dcx_graph_apply_checks: the flag zeroed, a thread per listed edge
hipError_t launch_lazy_apply(const LazyApplyArgs& a, hipStream_t stream);

}  // namespace dcx
