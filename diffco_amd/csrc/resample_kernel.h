// resample_kernel.h — what dcx_path_resample's host side (dcx_api.hip) and its kernel (resample_kernels.hip) share: the launch's
// arguments and THE plan of the workspace.  dcx_path_resample_work_bytes and dcx_path_resample both call resample_plan, so the
// workspace a caller was told to bring is the one the launch uses.
//
// One block per path (include/dcx.h, "batched path resampling"): the segment lengths, the arc length at the waypoints in the
// contract's fixed association (chunks of DCX_RESAMPLE_CHUNK segments added in order, the chunk totals added in order), then the
// T output waypoints by a binary search over that arc length.  The arc length c and the lengths len of a path of at most
// kResampleLdsWaypoints waypoints live in the block's LDS, those of a longer path in the workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dcx.h"
#include "work_layout.h"

namespace dcx {

constexpr int kResampleChunk = DCX_RESAMPLE_CHUNK;
// 256 threads = one wave per SIMD of a CU: the block's phases are short, barrier-separated loops over segments, chunks and
// output floats, and more waves per block only lengthen the barriers.
constexpr int kResampleThreads = 256;
// c and len of 2048 waypoints (each chunk of 32 padded by one word, so that the threads that walk one chunk each hit different
// banks) and the 2048 chunk totals of the longest path (65536 / 32) are 16.5 + 8 KB of LDS: 6 blocks, 24 waves, fit a CU's
// 160 KB.  Planner and shortcut paths are tens to hundreds of waypoints; a longer one pays the workspace's L2 latency.
constexpr int kResampleLdsWaypoints = 2048;
constexpr int kResampleMaxChunks = DCX_SHORTCUT_MAX_WAYPOINTS / kResampleChunk;

// the workspace: c and len of the rows that do not fit the LDS, [R, W] floats each (nothing where no row can be that long)
struct ResamplePlan {
    size_t c, len;
    size_t total;
};

inline ResamplePlan resample_plan(int64_t R, int32_t W) {
    const size_t rows = W > kResampleLdsWaypoints ? (size_t)R * (size_t)W : 0;
    WorkCarve c;
    ResamplePlan w;
    w.c = c.take_n<float>(rows);
    w.len = c.take_n<float>(rows);
    w.total = c.at;
    if (R > 0 && w.total == 0) w.total = 256;   // (never 0 for a call that launches: `work` is a real pointer)
    return w;
}

struct ResampleArgs {
    const float* path;        // [R, W, dof]
    const int32_t* count;     // [R]
    float* out;               // [R, T, dof]
    int32_t* out_count;       // [R]
    float* length;            // [R] or NULL
    // the workspace
    float* work_c;            // [R, W]
    float* work_len;          // [R, W]
    uint64_t wrap_mask;
    int32_t R, W, dof, T;
};

hipError_t launch_path_resample(const ResampleArgs& a, hipStream_t stream);

}  // namespace dcx
