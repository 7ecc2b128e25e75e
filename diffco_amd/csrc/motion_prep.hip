// motion_prep.hip — the first launches of the motion calls (motion_tile.h): per edge its sample count under the call's rule,
// the step fraction of the max_step rule, first_hit set to -1 (or -2 for an edge over max_samples), n_samples (one thread per
// edge over the whole chip), then the exclusive scan of the counts into the work list's offsets (one workgroup: chunks of 1024
// counts, each scanned by wave shuffles and one pass over the 16 wave totals) and the split launch's arrival counters zeroed.
// (The first form did both in ONE workgroup, each thread a contiguous run of edges: 420 us of a 2.9 ms call at E = 65536.)
#include <hip/hip_runtime.h>
#include "motion_tile.h"
#include "wrap_device.h"

namespace dcx {
namespace {
constexpr int kCountThreads = 256;
constexpr int kScanThreads = 1024;

__global__ __launch_bounds__(kCountThreads) void motion_count_kernel(const MotionPrepArgs p) {
    const int64_t e = (int64_t)blockIdx.x * kCountThreads + threadIdx.x;
    if (e >= p.E) return;
    int64_t n;
    if (p.res > 0) {
        n = p.res;
    } else {
#pragma clang fp contract(off)
        // dense_path's arithmetic (utils.py): L = |qb - qa|, n = ceil(L * (1 / max_step)) + 1 points, step fraction (1 / L) * max_step.
        // Each operation rounded on its own, with contraction off: -ffp-contract=fast fuses d * d + l2 into one FMA per joint
        // (__fmul_rn / __fadd_rn included: they are plain * and + in the HIP headers) - a different l2, and a count off by one
        // where L / max_step lies near an integer.  Masked coordinates enter with their wrapped delta (wrap_device.h).
        float l2 = 0.0f;
        for (int j = 0; j < p.dof; ++j) {
            const float d = motion_delta(p.qa[e * p.dof + j], p.qb[e * p.dof + j], p.wrap_mask, j);
            l2 = l2 + d * d;
        }
        // sqrtf, not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS the latter is the native v_sqrt_f32 (1 ulp); sqrtf is
        // correctly rounded (the compiler's default -fhip-fp32-correctly-rounded-divide-sqrt)
        const float L = sqrtf(l2);
        const float steps = ceilf(__fmul_rn(L, __frcp_rn(p.max_step)));
        p.frac[e] = __fmul_rn(__frcp_rn(L), p.max_step);
        if (p.open_end) n = (steps <= 2147483647.0f) ? (int64_t)steps : INT64_MAX;   // without the target (L = 0: none)
        else n = (steps + 1.0f <= 2147483647.0f) ? (int64_t)steps + 1 : INT64_MAX;   // (NaN and inf land here too)
    }
    const bool ok = n <= p.max_samples;
    if (p.n_samples) p.n_samples[e] = (int32_t)(n < INT32_MAX ? n : INT32_MAX);
    p.first_hit[e] = ok ? -1 : -2;
    p.offs[e + 1] = ok ? n : 0;   // the count, scanned in place below
}

__global__ __launch_bounds__(kScanThreads) void motion_scan_kernel(const MotionPrepArgs p) {
    __shared__ int64_t sWave[kScanThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int64_t i = t; i < (int64_t)p.n_counters * kCounterStride; i += kScanThreads) p.counters[i] = 0u;
    if (t == 0) p.offs[0] = 0;
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < p.E; c0 += kScanThreads) {
        const int64_t e = c0 + t;
        int64_t v = e < p.E ? p.offs[e + 1] : 0;
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
        if (e < p.E) p.offs[e + 1] = before + v;
        carry = total;
        __syncthreads();   // sWave is rewritten by the next chunk
    }
}
}  // namespace

hipError_t launch_motion_prep(const MotionPrepArgs& p, hipStream_t stream) {
    motion_count_kernel<<<(unsigned)((p.E + kCountThreads - 1) / kCountThreads), kCountThreads, 0, stream>>>(p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    motion_scan_kernel<<<1, kScanThreads, 0, stream>>>(p);
    return hipGetLastError();
}
}  // namespace dcx
