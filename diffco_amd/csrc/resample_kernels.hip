// resample_kernels.hip — dcx_path_resample (include/dcx.h, "batched path resampling"; resample_kernel.h): R paths of uneven
// length resampled to T waypoints each, equally spaced in arc length.  One block per path, five barrier-separated phases:
//   lengths: one thread per segment: len_e from the two rows (neighbouring threads share the rows' cache lines: a row leaves
//            HBM once)
//   chunks:  one thread per chunk of 32 segments, sequentially inside the chunk: the contract's p, and the chunk's total
//   totals:  one thread adds the chunk totals in order: the contract's b (at most 2048 dependent adds)
//   finish:  c_e = b + p, one thread per waypoint; L = c_{n-1}
//   outputs: one thread per output float (t, j), so the stores are coalesced: the largest e with c_e <= s by a binary search
//            over c (non-decreasing: the header says why), then the interpolation.  The dof threads of one waypoint repeat
//            the search (<= 16 reads of c each) instead of sharing it through another barrier.
// Every loop runs the block over its range: neither n nor T is bounded by the block size.  c and len live in LDS (each chunk
// of 32 padded by one word: the chunk threads' stride becomes 33 banks) or, for a path of more than kResampleLdsWaypoints
// waypoints, in the workspace.  Nothing is atomic and nothing depends on the launch geometry: repeated calls give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include "resample_kernel.h"
#include "wrap_device.h"

namespace dcx {
namespace {

template <bool kLds>
__device__ __forceinline__ int slot(int e) {
    return kLds ? e + (e >> 5) : e;
}

// c, ln: n entries each (slot()'s layout); sB: the chunk totals, then their exclusive sums
template <bool kLds>
__device__ __forceinline__ void resample_path(const ResampleArgs& a, const int64_t r, const int n, float* const c, float* const ln,
                                              float* const sB) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, dof = a.dof, T = a.T;
    const uint64_t mask = a.wrap_mask;
    const float* const row = a.path + r * (int64_t)a.W * dof;

    // lengths: motion_prep.hip's edge length, statement by statement
    for (int e = tid; e < n - 1; e += kResampleThreads) {
        const float* const qa = row + (int64_t)e * dof;
        float l2 = 0.0f;
        for (int j = 0; j < dof; ++j) {
            const float d = motion_delta(qa[j], qa[dof + j], mask, j);
            l2 = l2 + d * d;
        }
        ln[slot<kLds>(e)] = sqrtf(l2);   // (correctly rounded: motion_prep.hip says why not __fsqrt_rn)
    }
    __syncthreads();

    // chunks: p_{g,i} into c, the chunk's total into sB
    const int chunks = (n + kResampleChunk - 1) / kResampleChunk;   // (of the n entries of c; <= kResampleMaxChunks)
    for (int g = tid; g < chunks; g += kResampleThreads) {
        float p = 0.0f;
        const int e0 = g * kResampleChunk;
        for (int i = 0; i < kResampleChunk; ++i) {
            const int e = e0 + i;
            if (e < n) c[slot<kLds>(e)] = p;
            if (e < n - 1) p = p + ln[slot<kLds>(e)];
        }
        sB[g] = p;   // (the last chunk's total is never used)
    }
    __syncthreads();

    // totals: b_g in order
    if (tid == 0) {
        float b = 0.0f;
        for (int g0 = 0; g0 < chunks; g0 += 8) {   // eight totals per LDS round trip; the adds stay one chain
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = g0 + u < chunks ? sB[g0 + u] : 0.0f;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float before = b;
                b = b + t[u];
                t[u] = before;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (g0 + u < chunks) sB[g0 + u] = t[u];
        }
    }
    __syncthreads();

    // finish: c_e = b_{e / 32} + p_{e / 32, e % 32}
    for (int e = tid; e < n; e += kResampleThreads) c[slot<kLds>(e)] = sB[e / kResampleChunk] + c[slot<kLds>(e)];
    __syncthreads();

    const float L = c[slot<kLds>(n - 1)];
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
        int lo = 0, hi = n - 2;   // c_0 = +0 <= s
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (c[slot<kLds>(mid)] <= s) lo = mid;
            else hi = mid - 1;
        }
        const float arc = s - c[slot<kLds>(lo)];
        const float len = ln[slot<kLds>(lo)];
        const float qa = row[(int64_t)lo * dof + j], qb = row[(int64_t)(lo + 1) * dof + j];
        if (!(arc < len)) {
            out[i] = qb;
            continue;
        }
        const float f = __fdiv_rn(arc, len);
        const float d = motion_delta(qa, qb, mask, j);
        if ((mask >> j) & 1ull) {
            const float p = f * d;
            out[i] = wrap2pi_f32(qa + p);
        } else {
            out[i] = fmaf(f, d, qa);
        }
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
