// sssp_kernel.h — what dcx_sssp_run's and dcx_sssp_extract_paths' host side (dcx_api.hip) and their kernels (sssp_kernels.hip)
// share: the launches' arguments and their geometry (include/dcx.h, "roadmap queries").
//
// The state is node-major and query-minor, dist[b][v][q] and pred[v][q]: lanes are queries, so every neighbour of a node costs a
// wave one coalesced 256-B read, and the row of the CSR (col, weight) is the same for the whole wave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dcx.h"

namespace dcx {

constexpr int kSsspLanes = 64;          // queries of a wave
constexpr int kSsspWaves = 4;           // waves of a relaxation block: consecutive nodes, the same 64 queries
constexpr int kSsspUnroll = 8;          // neighbour rows a wave has in flight
constexpr int kSsspFillThreads = 256;   // threads of the round-0 fill and scatter blocks
constexpr int64_t kSsspMaxGridY = 65535;

struct SsspArgs {
    // the graph (dcx_graph)
    const int32_t* rowptr;    // [N + 1]
    const int32_t* col;       // [nnz]
    const float* weight;      // [nnz]
    // the start links (round 0 only)
    const int32_t* link_idx;  // [Q, k]
    const float* link_len;    // [Q, k]
    // the state (dcx_sssp_state)
    float* dist;              // [2, N, Q]
    int32_t* pred;            // [N, Q]
    int32_t N, nnz, Q, k;
};

struct SsspExtractArgs {
    const float* nodes;       // [N, dof]
    const float* dist;        // [N, Q]: the buffer the last round wrote
    const int32_t* pred;      // [N, Q]
    const int32_t* mode;      // [Q]
    const float* starts;      // [Q, dof]
    const float* goals;       // [Q, dof]
    const int32_t* goal_idx;  // [Q, k]
    const float* goal_len;    // [Q, k]
    const float* direct_len;  // [Q]
    float* path;              // [Q, W, dof]
    int32_t* count;           // [Q]
    float* length;            // [Q]
    int32_t N, Q, k, dof, W;
};

// whether the relaxation's grid (a block per kSsspWaves nodes x 64 queries) fits one launch
inline bool sssp_grid_ok(int64_t N, int64_t Q) {
    return (Q + kSsspLanes - 1) / kSsspLanes <= kSsspMaxGridY && (N + kSsspWaves - 1) / kSsspWaves <= INT32_MAX;
}

// changed[0 .. n - 1] = 0 (n >= 1)
hipError_t launch_sssp_zero(int32_t* changed, int32_t n, hipStream_t stream);
// round 0: the fill of both dist buffers and pred, then the scatter of the links; *changed = 1 iff a link is real
hipError_t launch_sssp_init(const SsspArgs& a, int32_t* changed, hipStream_t stream);
// round t >= 1: prev == nullptr for the first round of a call, else the previous round's flag (0: return at once)
hipError_t launch_sssp_relax(const SsspArgs& a, int32_t t, const int32_t* prev, int32_t* changed, hipStream_t stream);
hipError_t launch_sssp_extract(const SsspExtractArgs& a, hipStream_t stream);

}  // namespace dcx
