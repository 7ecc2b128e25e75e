// knn_kernel.h — what dcx_knn's host side (dcx_api.hip) and its kernels (knn_kernels.hip) share: the launch's arguments and
// THE plan of its geometry.  dcx_knn_work_bytes and dcx_knn both call knn_plan, so the workspace a caller was told to bring
// is the one the launch uses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "../../include/dcx.h"

namespace dcx {

constexpr int kKnnWaves = 4;              // waves per block: each takes a quarter of the block's point range.  Four
                                          // columns of k = DCX_KNN_MAX_K keys are 128 KB of a CU's 160 KB
constexpr int kKnnMaxDof = 64;            // a wrap mask has 64 bits (the motion calls' own ceiling, DCX_MAX_DOF, lies below)
constexpr int kKnnRegDof = 16;            // queries of up to this many coordinates sit in registers, longer ones in LDS
constexpr int kKnnCus = 256;              // the only target's CU count: the plan takes no device (dcx_knn_work_bytes has none)
constexpr int kKnnTargetBlocks = 2 * kKnnCus;   // a small Q splits the points until this many blocks exist ...
constexpr int kKnnMinSplitPoints = 1024;  // ... each with at least this many points (256 per wave)
constexpr int kKnnMaxSplits = 1024;       // the ceiling of the plan and of the knn_split knob
constexpr unsigned long long kKnnEmpty = ~0ull;   // an unfilled slot's key: above every real key (0xFFFFFFFF is a NaN's pattern,
                                                  // and a NaN distance is never admitted)

struct KnnPlan {
    bool ok;            // false: the sizes are beyond one launch
    int64_t tiles;      // 64-query tiles = grid.x of the search
    int32_t splits;     // point splits = grid.y; 1: the search writes idx / dist2 itself and the merge does not run
    size_t lds_bytes;   // of the search: kKnnWaves key columns, then the query tile where dof > kKnnRegDof
    size_t work_bytes;  // what dcx_knn_work_bytes reports
};

// `knob`: dcx_debug_set("knn_split"), <= 0: this rule.  A tile count of at least kKnnTargetBlocks runs unsplit; below it the
// points are split until the grid has kKnnTargetBlocks blocks, while a split keeps kKnnMinSplitPoints points.
// The reported size is a bound on tiles * splits * 64 key lists that never shrinks as Q or N grow (tiles * ceil(T / tiles)
// itself is not monotone in tiles): min(tiles + T, tiles * ceil(N / kKnnMinSplitPoints)) lists of k keys per lane.
inline KnnPlan knn_plan(int64_t Q, int64_t N, int32_t dof, int32_t k, int64_t knob) {
    KnnPlan p{};
    p.tiles = (Q + 63) / 64;
    const int64_t by_n = std::max<int64_t>(1, (N + kKnnMinSplitPoints - 1) / kKnnMinSplitPoints);
    const int64_t by_q = p.tiles > 0 ? (kKnnTargetBlocks + p.tiles - 1) / p.tiles : 1;
    int64_t lists;
    if (knob > 0) {
        p.splits = (int32_t)std::min<int64_t>(knob, kKnnMaxSplits);
        lists = p.tiles <= (INT64_MAX >> 8) / p.splits ? p.tiles * p.splits : -1;
    } else {
        p.splits = (int32_t)std::min<int64_t>(std::min(by_q, by_n), kKnnMaxSplits);
        lists = std::min(p.tiles + kKnnTargetBlocks, p.tiles <= (INT64_MAX >> 8) / by_n ? p.tiles * by_n : INT64_MAX);
    }
    p.lds_bytes = (size_t)kKnnWaves * k * 64 * sizeof(unsigned long long) + (dof > kKnnRegDof ? (size_t)dof * 64 * sizeof(float) : 0);
    // one launch: grid.x * grid.y blocks below 2^31, point indices in 32 bits, the workspace in a size_t with room to spare
    p.ok = N <= INT32_MAX && p.tiles <= INT32_MAX / p.splits && lists >= 0 && lists <= (int64_t)1 << 40 &&
           (p.splits == 1 || Q <= (int64_t)INT32_MAX * kKnnWaves);   // (the merge takes a wave per query)
    p.work_bytes = p.ok ? (size_t)std::max<int64_t>(lists, 1) * 64 * k * sizeof(unsigned long long) : 0;
    return p;
}

struct KnnArgs {
    const float* queries;   // [Q, dof]
    const float* points;    // [N, dof]
    int64_t Q;
    int32_t N, dof, k, splits;
    uint64_t wrap_mask;
    float max_dist2;
    int64_t self_offset;
    int32_t* idx;           // [Q, k]
    float* dist2;           // [Q, k]
    unsigned long long* part;   // [Q, splits, k] sorted keys, splits > 1 only
};

hipError_t launch_knn(const KnnArgs& a, const KnnPlan& p, hipStream_t stream);

}  // namespace dcx
