// arclen_device.h — the arc length of one path at its waypoints, in THE fixed association of include/dcx.h ("batched path
// resampling"): what dcx_path_resample's kernel (resample_kernels.hip) and the partial shortcut's pick kernel
// (shortcut_partial_kernels.hip) both run first, one block of kResampleThreads threads per path.  One definition: the two
// contracts name the same c_e and len_e, bit for bit.
// Four barrier-separated phases (every thread of the block calls path_arc_length: n is block-uniform):
//   lengths: one thread per segment: len_e from the two rows (neighbouring threads share the rows' cache lines: a row leaves
//            HBM once)
//   chunks:  one thread per chunk of 32 segments, sequentially inside the chunk: the contract's p, and the chunk's total
//   totals:  one thread adds the chunk totals in order: the contract's b (at most 2048 dependent adds - the chain IS the contract)
//   finish:  c_e = b + p, one thread per waypoint
// c and ln live in LDS (each chunk of 32 padded by one word: the chunk threads' stride becomes 33 banks) or, for a path of more
// than kResampleLdsWaypoints waypoints, in the workspace; arc_slot<kLds> is the layout.  The last barrier is inside: c and ln are
// readable by every thread on return.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "resample_kernel.h"
#include "wrap_device.h"

namespace dcx {

template <bool kLds>
__device__ __forceinline__ int arc_slot(int e) {
    return kLds ? e + (e >> 5) : e;
}

// row: the path's n >= 2 waypoints [n, dof];  c, ln: n entries each (arc_slot's layout);  sB: the chunk totals, then their
// exclusive sums (kResampleMaxChunks floats of LDS)
template <bool kLds>
__device__ __forceinline__ void path_arc_length(const float* const row, const int n, const int dof, const uint64_t mask, float* const c,
                                                float* const ln, float* const sB) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;

    // lengths: motion_prep.hip's edge length, statement by statement
    for (int e = tid; e < n - 1; e += kResampleThreads) {
        const float* const qa = row + (int64_t)e * dof;
        float l2 = 0.0f;
        for (int j = 0; j < dof; ++j) {
            const float d = motion_delta(qa[j], qa[dof + j], mask, j);
            l2 = l2 + d * d;
        }
        ln[arc_slot<kLds>(e)] = sqrtf(l2);   // (correctly rounded: motion_prep.hip says why not __fsqrt_rn)
    }
    __syncthreads();

    // chunks: p_{g,i} into c, the chunk's total into sB
    const int chunks = (n + kResampleChunk - 1) / kResampleChunk;   // (of the n entries of c; <= kResampleMaxChunks)
    for (int g = tid; g < chunks; g += kResampleThreads) {
        float p = 0.0f;
        const int e0 = g * kResampleChunk;
        for (int i = 0; i < kResampleChunk; ++i) {
            const int e = e0 + i;
            if (e < n) c[arc_slot<kLds>(e)] = p;
            if (e < n - 1) p = p + ln[arc_slot<kLds>(e)];
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
    for (int e = tid; e < n; e += kResampleThreads) c[arc_slot<kLds>(e)] = sB[e / kResampleChunk] + c[arc_slot<kLds>(e)];
    __syncthreads();
}

// the point at arc length s of a path whose c and ln path_arc_length made: the largest e in 0 .. n - 2 with c_e <= s (c is
// non-decreasing and c_0 = +0 <= s: include/dcx.h says why), by a binary search of at most 16 reads of c
template <bool kLds>
__device__ __forceinline__ int arc_locate(const float* const c, const int n, const float s) {
    int lo = 0, hi = n - 2;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (c[arc_slot<kLds>(mid)] <= s) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// THE pick of the partial shortcuts (include/dcx.h, "Partial shortcuts" step 2): the two arc lengths sa <= sb of the draws
// (u0, u1) on a path of total length L and the segments ea <= eb they fall into; false for an idle slot (a path without an arc
// length to draw on, a spoilt draw, or ea == eb: a chord inside one straight segment gains nothing)
template <bool kLds>
__device__ __forceinline__ bool arc_pick(const float* const c, const int n, const bool live, const float L, const float u0, const float u1,
                                         int& ea, int& eb, float& sa, float& sb) {
#pragma clang fp contract(off)
    ea = -1;
    eb = -1;
    sa = 0.0f;
    sb = 0.0f;
    if (!(live && u0 >= 0.0f && u0 < 1.0f && u1 >= 0.0f && u1 < 1.0f)) return false;   // (a NaN fails the comparisons)
    const float s0 = u0 * L, s1 = u1 * L;
    sa = fminf(s0, s1);
    sb = fmaxf(s0, s1);
    ea = arc_locate<kLds>(c, n, sa);
    eb = arc_locate<kLds>(c, n, sb);
    return ea != eb;
}

// coordinate j of that point on segment e: the contract's interpolation (the bits of the segment's end where !(arc < len))
template <bool kLds>
__device__ __forceinline__ float arc_point(const float* const row, const float* const c, const float* const ln, const int dof,
                                           const uint64_t mask, const int e, const float s, const int j) {
#pragma clang fp contract(off)
    const float arc = s - c[arc_slot<kLds>(e)];
    const float len = ln[arc_slot<kLds>(e)];
    const float qa = row[(int64_t)e * dof + j], qb = row[(int64_t)(e + 1) * dof + j];
    if (!(arc < len)) return qb;
    const float f = __fdiv_rn(arc, len);
    const float d = motion_delta(qa, qb, mask, j);
    if ((mask >> j) & 1ull) {
        const float p = f * d;
        return wrap2pi_f32(qa + p);
    }
    return fmaf(f, d, qa);
}

}  // namespace dcx
