// motion_band_finish.hip — the launches of dcx_motion_band behind its sweep (motion_band_kernel.h).
//   edges:   one thread per edge reads the edge's codes in sample order: verdict (1 at a sure hit, else 2 at an uncertain sample,
//            else 0; -2 from motion_prep's status word for an edge over max_samples), first_hit (the smallest sample with code 1)
//            and the edge's uncertain count - 0 unless the verdict is 2: an edge with a sure hit is decided.
//   scan:    the exclusive scan of those counts into int64 offsets [E + 1], in place: motion_prep's scan shape (one workgroup,
//            chunks of 1024 counts, each scanned by wave shuffles and one pass over the 16 wave totals).
//   scatter: one wave per edge; an edge with a non-zero count walks its codes again, 64 samples per step, and the lane of an
//            uncertain sample writes entry offset + i (i from a ballot and a popcount: sample order) - (edge, sample) and, on
//            request, the sample's configuration: motion_coord on the edge's endpoints, the bits the sweep scored (the way
//            motion_worst_finish forms x*) - while offset + i < unc_cap.  unc_total = offsets[E].
//            (One THREAD per edge was the first form: 139 us at E = 4096 with 12.7 k entries listed, each thread writing its
//            edge's ~19 rows one after the other.)
// The order of the list is the order of the offsets: no atomics and no order of arrival anywhere, the same bits every call.
#include <hip/hip_runtime.h>
#include "motion_band_kernel.h"
#include "wrap_device.h"

namespace dcx {
namespace {
constexpr int kEdgeThreads = 256;
constexpr int kScanThreads = 1024;

__global__ __launch_bounds__(kEdgeThreads) void motion_band_edges_kernel(const MotionBandFinishArgs f) {
    const int64_t e = (int64_t)blockIdx.x * kEdgeThreads + threadIdx.x;
    if (e >= f.E) return;
    int32_t verdict = -2, first = -2, unc = 0;
    if (f.status[e] != -2) {
        const int64_t s0 = f.offs[e];
        const int n = (int)(f.offs[e + 1] - s0);
        first = -1;
        for (int k = 0; k < n; ++k) {
            const int code = f.codes[s0 + k];
            if (code == 1) {
                first = k;
                break;
            }
            unc += code == 2 ? 1 : 0;
        }
        verdict = first >= 0 ? 1 : (unc > 0 ? 2 : 0);
        if (first >= 0) unc = 0;
    }
    f.verdict[e] = verdict;
    if (f.first_hit) f.first_hit[e] = first;
    if (f.n_uncertain) f.n_uncertain[e] = unc;
    f.uoffs[e + 1] = unc;   // the count, scanned in place below
}

__global__ __launch_bounds__(kScanThreads) void motion_band_scan_kernel(const MotionBandFinishArgs f) {
    __shared__ int64_t sWave[kScanThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) f.uoffs[0] = 0;
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < f.E; c0 += kScanThreads) {
        const int64_t e = c0 + t;
        int64_t v = e < f.E ? f.uoffs[e + 1] : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {   // inclusive scan of the wave's 64 counts
            const int64_t u = __shfl_up(v, d, 64);
            if (lane >= d) v += u;
        }
        if (lane == 63) sWave[wave] = v;
        __syncthreads();
        int64_t before = carry, total = carry;
        for (int w = 0; w < kScanThreads / 64; ++w) {
            if (w < wave) before += sWave[w];
            total += sWave[w];
        }
        if (e < f.E) f.uoffs[e + 1] = before + v;
        carry = total;
        __syncthreads();   // sWave is rewritten by the next chunk
    }
}

__global__ __launch_bounds__(kEdgeThreads) void motion_band_scatter_kernel(const MotionBandFinishArgs f) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * (kEdgeThreads / 64) + (threadIdx.x >> 6);   // one wave per edge
    if (e >= f.E) return;
    if (e == 0 && lane == 0) *f.unc_total = f.uoffs[f.E];
    int64_t j0 = f.uoffs[e];
    const int64_t end = f.uoffs[e + 1] < f.unc_cap ? f.uoffs[e + 1] : f.unc_cap;   // nothing at or beyond unc_cap
    if (j0 >= end) return;
    const int64_t s0 = f.offs[e];
    const int n = (int)(f.offs[e + 1] - s0);
    const int dof = f.dof;
    // 64 samples per step: a lane's entry lies behind those of the lanes below it (ballot and popcount: sample order)
    for (int k0 = 0; k0 < n && j0 < end; k0 += 64) {
        const int k = k0 + lane;
        const bool on = k < n && f.codes[s0 + k] == 2;
        const uint64_t mine = __builtin_amdgcn_ballot_w64(on);
        const int64_t j = j0 + __popcll(mine & ((1ull << lane) - 1ull));
        if (on && j < end) {
            f.unc_edge[j] = (int32_t)e;
            f.unc_sample[j] = k;
            if (f.unc_q)
                for (int i = 0; i < dof; ++i) {
                    const float qa = f.qa[e * dof + i], qb = f.qb[e * dof + i];
                    f.unc_q[j * dof + i] = motion_coord(qa, qb, k, f.res, k == n - 1, f.frac + e, (f.wrap_mask >> i) & 1ull);
                }
        }
        j0 += __popcll(mine);
    }
}
}  // namespace

hipError_t launch_motion_band_finish(const MotionBandFinishArgs& f, hipStream_t stream) {
    const unsigned blocks = (unsigned)((f.E + kEdgeThreads - 1) / kEdgeThreads);
    motion_band_edges_kernel<<<blocks, kEdgeThreads, 0, stream>>>(f);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    motion_band_scan_kernel<<<1, kScanThreads, 0, stream>>>(f);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned waves = (unsigned)((f.E + kEdgeThreads / 64 - 1) / (kEdgeThreads / 64));
    motion_band_scatter_kernel<<<waves, kEdgeThreads, 0, stream>>>(f);
    return hipGetLastError();
}
}  // namespace dcx
