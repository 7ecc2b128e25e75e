// resample_kernels.hip — dcx_path_resample (include/dcx.h, "batched path resampling"; resample_kernel.h): R paths of uneven
// length resampled to T waypoints each, equally spaced in arc length.  One block per path, five barrier-separated phases:
//   lengths, chunks, totals, finish: the arc length c_e at the waypoints in the contract's association; L = c_{n-1}.  They
//            are arclen_device.h's path_arc_length, which the partial shortcut's pick kernel runs too: one definition
//   outputs: one thread per output float (t, j), so the stores are coalesced: the largest e with c_e <= s by a binary search
//            over c (non-decreasing: the header says why), then the interpolation (arc_locate, arc_point).  The dof threads
//            of one waypoint repeat the search (<= 16 reads of c each) instead of sharing it through another barrier.
// Every loop runs the block over its range: neither n nor T is bounded by the block size.  c and len live in LDS (each chunk
// of 32 padded by one word: the chunk threads' stride becomes 33 banks) or, for a path of more than kResampleLdsWaypoints
// waypoints, in the workspace.  Nothing is atomic and nothing depends on the launch geometry: repeated calls give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include "resample_kernel.h"
#include "arclen_device.h"

namespace dcx {
namespace {

// c, ln: n entries each (arc_slot's layout); sB: the chunk totals, then their exclusive sums
template <bool kLds>
__device__ __forceinline__ void resample_path(const ResampleArgs& a, const int64_t r, const int n, float* const c, float* const ln,
                                              float* const sB) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, dof = a.dof, T = a.T;
    const uint64_t mask = a.wrap_mask;
    const float* const row = a.path + r * (int64_t)a.W * dof;

    path_arc_length<kLds>(row, n, dof, mask, c, ln, sB);   // lengths, chunks, totals, finish (arclen_device.h)

    const float L = c[arc_slot<kLds>(n - 1)];
    const bool ok = L < INFINITY;   // (block-uniform; a NaN fails it)
    if (tid == 0) {
        a.out_count[r] = ok ? T : 0;
        if (a.length) a.length[r] = L != L ? NAN : L;   // (whatever NaN the sums made: the one quiet NaN)
    }
    if (!ok) return;

    // outputs
    const float step = __fdiv_rn(L, (float)(T - 1));
    float* const out = a.out + r * (int64_t)T * dof;
    const int total = T * dof;   // (<= 65536 * DCX_MAX_DOF)
    for (int i = tid; i < total; i += kResampleThreads) {
        const int t = i / dof, j = i - t * dof;
        if (t == 0) {
            out[i] = row[j];
            continue;
        }
        if (t == T - 1) {
            out[i] = row[(int64_t)(n - 1) * dof + j];
            continue;
        }
        const float s = (float)t * step;
        out[i] = arc_point<kLds>(row, c, ln, dof, mask, arc_locate<kLds>(c, n, s), s, j);
    }
}

__global__ __launch_bounds__(kResampleThreads) void path_resample_kernel(const ResampleArgs a) {
    constexpr int kSlots = kResampleLdsWaypoints + kResampleLdsWaypoints / kResampleChunk;
    __shared__ float sC[kSlots];
    __shared__ float sLen[kSlots];
    __shared__ float sB[kResampleMaxChunks];
    const int64_t r = blockIdx.x;
    const int n = min(a.count[r], a.W);
    if (n < 2) {   // (block-uniform)
        if (threadIdx.x == 0) {
            a.out_count[r] = 0;
            if (a.length) a.length[r] = NAN;
        }
        return;
    }
    if (n <= kResampleLdsWaypoints) resample_path<true>(a, r, n, sC, sLen, sB);
    else resample_path<false>(a, r, n, a.work_c + r * (int64_t)a.W, a.work_len + r * (int64_t)a.W, sB);
}
}  // namespace

hipError_t launch_path_resample(const ResampleArgs& a, hipStream_t st) {
    path_resample_kernel<<<dim3((unsigned)a.R), dim3(kResampleThreads), 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace dcx
