// shortcut_cost_kernels.hip — the path logic of dcx_path_shortcut_run_cost and dcx_path_shortcut_partial_run_cost (include/dcx.h,
// "path shortcuts under the clearance objective"; shortcut_cost_kernel.h has the round).  A piece with peak w = dcx_motion_worst's
// worst and length bits L costs C = L * (1 + gain * fmaxf(w + band, 0)) and is free where w <= 0; a slot is applied only where
// every piece of it is free and what it inserts costs less than the segments it removes.
//   picks:   the length modes' picks (shortcut_pick_ij, arc_pick: one definition each), which additionally write every piece's L -
//            the motion calls' own length bits of the edge as it stands in the batch.  Vertex mode: one thread per slot.  Partial
//            mode: one block per path, the arc length of arclen_device.h, one thread per slot for its pick (through LDS to the
//            rest), then one thread per float of the slots' three edges and one thread per piece for its L (it forms the piece's
//            two ends again: the same function of the same words).
//   commits: one block per path.  Lane p < P prices slot p: the sum of the removed span of seg, serial and ascending as the contract
//            has it, the P sums side by side, reading the row from LDS where the path has at most kShortcutCostLdsWaypoints
//            waypoints and from global memory where not.  The verdicts go through LDS; from there the selection is the length
//            modes' block-uniform slot-order loop, and a block with nothing applied leaves at once.  Vertex mode: the row and then
//            seg are compacted in place (shortcut_compact: an entry never moves up), and every applied chord's C is written once
//            the last chunk is through.  Partial mode: the rewritten tail of the row and of seg go to their stages in the
//            workspace, one barrier, then back: nothing is overwritten before it is read.
// No atomics; every cost is formed with contraction off, one rounded operation at a time.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include "shortcut_cost_kernel.h"
#include "arclen_device.h"

namespace dcx {
namespace {

// C = L * f(w): three operations, each rounded alone (rrtstar_cost_kernels.hip's edge_cost: the same objective)
__device__ __forceinline__ float piece_cost(float L, float w, float gain, float band) {
#pragma clang fp contract(off)
    const float pen = fmaxf(w + band, 0.0f);
    const float f = 1.0f + gain * pen;
    return L * f;
}

// seg[from] + seg[from + 1] + ... + seg[to], ascending from seg[from] (from <= to)
__device__ __forceinline__ float span_cost(const float* const seg, const int from, const int to) {
#pragma clang fp contract(off)
    float old = seg[from];
    for (int k = from + 1; k <= to; ++k) old = old + seg[k];
    return old;
}

// the seg row of a path of n waypoints into LDS where it fits (block-uniform); every thread calls it
__device__ __forceinline__ bool stage_seg_row(const float* const segrow, const int n, float* const sSeg) {
    const bool lds = n <= kShortcutCostLdsWaypoints;
    if (lds)
        for (int k = threadIdx.x; k < n - 1; k += kShortcutThreads) sSeg[k] = segrow[k];
    __syncthreads();
    return lds;
}

__global__ __launch_bounds__(kShortcutThreads) void shortcut_cost_pick_kernel(const ShortcutCostArgs c) {
#pragma clang fp contract(off)
    const ShortcutPartialArgs& a = c.a;
    const int64_t e = (int64_t)blockIdx.x * kShortcutThreads + threadIdx.x;
    if (e >= (int64_t)a.R * a.P) return;
    const int64_t r = e / a.P;
    const int dof = a.dof;
    const int n = max(0, min(a.count[r], a.W));   // (a count beyond W is the caller's error: never read past the row)
    int i, j;
    shortcut_pick_ij(n, a.draws[e * 2], a.draws[e * 2 + 1], i, j);
    // an idle slot: the zero-length edge on the path's first row, one sample, its peak ignored
    const float* const row = a.path + r * (int64_t)a.W * dof;
    const float* const wa = row + (int64_t)max(i, 0) * dof;
    const float* const wb = row + (int64_t)max(j, 0) * dof;
    float* const qa = a.qa + e * dof;
    float* const qb = a.qb + e * dof;
    float l2 = 0.0f;
    for (int k = 0; k < dof; ++k) {
        const float d = motion_delta(wa[k], wb[k], a.wrap_mask, k);
        l2 = l2 + d * d;
        qa[k] = wa[k];
        qb[k] = wb[k];
    }
    c.len[e] = sqrtf(l2);   // (correctly rounded: motion_prep.hip says why not __fsqrt_rn)
    a.picks[e * 2] = i;
    a.picks[e * 2 + 1] = j;
}

__global__ __launch_bounds__(kShortcutThreads) void shortcut_cost_commit_kernel(const ShortcutCostArgs c) {
#pragma clang fp contract(off)
    __shared__ float sSeg[kShortcutCostLdsWaypoints];
    __shared__ float sC[kShortcutMaxSlots];
    __shared__ int sGain[kShortcutMaxSlots];
    const ShortcutPartialArgs& a = c.a;
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int P = a.P, dof = a.dof;
    const int n = max(0, min(a.count[r], a.W));
    if (n < 3) return;   // (block-uniform) every slot of the path is idle
    float* const segrow = c.seg + r * (int64_t)a.W;
    const bool lds = stage_seg_row(segrow, n, sSeg);

    if (tid < P) {   // price slot tid
        const int64_t e = r * P + tid;
        const int i = a.picks[e * 2], j = a.picks[e * 2 + 1];
        float C = 0.0f;
        bool gainful = false;
        if (i >= 0 && i + 2 <= j && j <= n - 1) {
            const float w = c.worst[e];
            C = piece_cost(c.len[e], w, c.gain, c.band);
            const float old = lds ? span_cost(sSeg, i, j - 1) : span_cost(segrow, i, j - 1);
            gainful = w <= 0.0f && C < old;   // (a NaN fails either comparison)
        }
        sC[tid] = C;
        sGain[tid] = gainful ? 1 : 0;
    }
    __syncthreads();

    // the applied slots, in slot order (block-uniform), as shortcut_commit_kernel selects them - with "gainful" for "free"
    int si[kShortcutMaxSlots], sj[kShortcutMaxSlots];
    int applied = 0, removed = 0, lo = INT_MAX;
#pragma unroll
    for (int p = 0; p < kShortcutMaxSlots; ++p) {
        si[p] = INT_MAX;
        sj[p] = INT_MAX;
        if (p < P) {
            const int64_t e = r * P + p;
            const int i = a.picks[e * 2], j = a.picks[e * 2 + 1];
            bool ok = sGain[p] != 0;
#pragma unroll
            for (int q = 0; q < p; ++q) ok = ok && (j <= si[q] || sj[q] <= i);
            if (ok) {
                si[p] = i;
                sj[p] = j;
                ++applied;
                removed += j - i - 1;
                lo = min(lo, i);
            }
        }
    }
    if (applied == 0) return;   // (block-uniform)

    // waypoints 0 .. lo and segments 0 .. lo - 1 stay where they are
    shortcut_compact<false>(a.path + r * (int64_t)a.W * dof, (lo + 1) * dof, n * dof, dof, si, sj);
    __syncthreads();
    shortcut_compact<true>(segrow, lo + 1, n - 1, 1, si, sj);
    // every read of seg is done (each thread is past the last chunk's barrier): the chords' costs, at the new index of their i -
    // where no survivor lands
    if (tid < P && si[tid] != INT_MAX) {
        int at = si[tid];
#pragma unroll
        for (int q = 0; q < kShortcutMaxSlots; ++q) at -= sj[q] <= si[tid] ? sj[q] - si[q] - 1 : 0;
        segrow[at] = sC[tid];
    }
    if (tid == 0) {
        a.count[r] = n - removed;
        a.accepted[r] += applied;
    }
}

// coordinate j of end `end` of piece `piece` of a live slot: path[ea] -> xa, xa -> xb, xb -> path[eb + 1]
template <bool kLds>
__device__ __forceinline__ float piece_coord(const float* const row, const float* const c, const float* const ln, const int dof,
                                             const uint64_t mask, const int ea, const float sa, const int eb, const float sb,
                                             const int piece, const int end, const int j) {
    const int point = piece + end;   // 0: path[ea], 1: xa, 2: xb, 3: path[eb + 1]
    if (point == 0) return row[(int64_t)ea * dof + j];
    if (point == 3) return row[(int64_t)(eb + 1) * dof + j];
    return point == 1 ? arc_point<kLds>(row, c, ln, dof, mask, ea, sa, j) : arc_point<kLds>(row, c, ln, dof, mask, eb, sb, j);
}

// the slots of path r: `live` (block-uniform) says whether the path has an arc length to draw on
template <bool kLds>
__device__ __forceinline__ void partial_cost_slots(const ShortcutCostArgs& cc, const int64_t r, const int n, const bool live, const float L,
                                                   const float* const c, const float* const ln) {
#pragma clang fp contract(off)
    const ShortcutPartialArgs& a = cc.a;
    const int dof = a.dof, P = a.P;
    const uint64_t mask = a.wrap_mask;
    const float* const row = a.path + r * (int64_t)a.W * dof;
    // the slots' picks, once each (two binary searches over c), shared through LDS with the threads that write the edges
    __shared__ int sEa[kShortcutMaxSlots], sEb[kShortcutMaxSlots], sOk[kShortcutMaxSlots];
    __shared__ float sSa[kShortcutMaxSlots], sSb[kShortcutMaxSlots];
    if ((int)threadIdx.x < P) {
        const int p = threadIdx.x;
        const int64_t e = r * P + p;
        int ea, eb;
        float sa, sb;
        const bool ok = arc_pick<kLds>(c, n, live, L, a.draws[e * 2], a.draws[e * 2 + 1], ea, eb, sa, sb);
        sEa[p] = ea;
        sEb[p] = eb;
        sSa[p] = sa;
        sSb[p] = sb;
        sOk[p] = ok ? 1 : 0;
        a.picks[e * 2] = ok ? ea : -1;
        a.picks[e * 2 + 1] = ok ? eb : -1;
    }
    __syncthreads();   // (every thread of the block is here: n and live are block-uniform)
    const int per = 3 * 2 * dof;   // the floats of a slot's three edges
    for (int i = threadIdx.x; i < P * per; i += kResampleThreads) {
        const int p = i / per, rem = i - p * per;
        const int piece = rem / (2 * dof), rem2 = rem - piece * 2 * dof;
        const int end = rem2 / dof, j = rem2 - end * dof;
        const int64_t e = r * P + p;
        // an idle slot: three zero-length edges on the path's first row, one sample each, their peaks ignored
        const float v = sOk[p] ? piece_coord<kLds>(row, c, ln, dof, mask, sEa[p], sSa[p], sEb[p], sSb[p], piece, end, j) : row[j];
        (end ? a.qb : a.qa)[(e * 3 + piece) * dof + j] = v;
    }
    for (int i = threadIdx.x; i < P * 3; i += kResampleThreads) {
        const int p = i / 3, piece = i - p * 3;
        const int64_t e = r * P + p;
        float l2 = 0.0f;
        if (sOk[p]) {
            for (int j = 0; j < dof; ++j) {
                const float d = motion_delta(piece_coord<kLds>(row, c, ln, dof, mask, sEa[p], sSa[p], sEb[p], sSb[p], piece, 0, j),
                                             piece_coord<kLds>(row, c, ln, dof, mask, sEa[p], sSa[p], sEb[p], sSb[p], piece, 1, j), mask, j);
                l2 = l2 + d * d;
            }
        }
        cc.len[e * 3 + piece] = sqrtf(l2);
    }
}

template <bool kLds>
__device__ __forceinline__ void partial_cost_pick_path(const ShortcutCostArgs& cc, const int64_t r, const int n, float* const c,
                                                       float* const ln, float* const sB) {
    const ShortcutPartialArgs& a = cc.a;
    path_arc_length<kLds>(a.path + r * (int64_t)a.W * a.dof, n, a.dof, a.wrap_mask, c, ln, sB);
    const float L = c[arc_slot<kLds>(n - 1)];
    partial_cost_slots<kLds>(cc, r, n, L > 0.0f && L < INFINITY, L, c, ln);   // (block-uniform; a NaN fails it)
}

__global__ __launch_bounds__(kResampleThreads) void shortcut_partial_cost_pick_kernel(const ShortcutCostArgs cc) {
    constexpr int kSlots = kResampleLdsWaypoints + kResampleLdsWaypoints / kResampleChunk;
    __shared__ float sC[kSlots];
    __shared__ float sLen[kSlots];
    __shared__ float sB[kResampleMaxChunks];
    const ShortcutPartialArgs& a = cc.a;
    const int64_t r = blockIdx.x;
    const int n = max(0, min(a.count[r], a.W));   // (a count beyond W is the caller's error: never read past the row)
    if (n < 3) partial_cost_slots<true>(cc, r, n, false, 0.0f, sC, sLen);   // (block-uniform: no barrier is skipped by a part of the block)
    else if (n <= kResampleLdsWaypoints) partial_cost_pick_path<true>(cc, r, n, sC, sLen, sB);
    else partial_cost_pick_path<false>(cc, r, n, a.work_c + r * (int64_t)a.W, a.work_len + r * (int64_t)a.W, sB);
}

__global__ __launch_bounds__(kShortcutThreads) void shortcut_partial_cost_commit_kernel(const ShortcutCostArgs cc) {
#pragma clang fp contract(off)
    __shared__ float sSeg[kShortcutCostLdsWaypoints];
    __shared__ float sC[kShortcutMaxSlots * 3];
    __shared__ int sGain[kShortcutMaxSlots];
    const ShortcutPartialArgs& a = cc.a;
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int P = a.P, dof = a.dof, W = a.W;
    const int n = max(0, min(a.count[r], W));
    if (n < 3) return;   // (block-uniform) every slot of the path is idle
    float* const segrow = cc.seg + r * (int64_t)W;
    const bool lds = stage_seg_row(segrow, n, sSeg);

    if (tid < P) {   // price slot tid
        const int64_t e = r * P + tid;
        const int ea = a.picks[e * 2], eb = a.picks[e * 2 + 1];
        float C0 = 0.0f, C1 = 0.0f, C2 = 0.0f;
        bool gainful = false;
        if (ea >= 0 && ea < eb && eb + 1 <= n - 1) {
            const float w0 = cc.worst[e * 3], w1 = cc.worst[e * 3 + 1], w2 = cc.worst[e * 3 + 2];
            C0 = piece_cost(cc.len[e * 3], w0, cc.gain, cc.band);
            C1 = piece_cost(cc.len[e * 3 + 1], w1, cc.gain, cc.band);
            C2 = piece_cost(cc.len[e * 3 + 2], w2, cc.gain, cc.band);
            const float fresh = (C0 + C1) + C2;
            const float old = lds ? span_cost(sSeg, ea, eb) : span_cost(segrow, ea, eb);
            gainful = w0 <= 0.0f && w1 <= 0.0f && w2 <= 0.0f && fresh < old;   // (a NaN fails any of them)
        }
        sC[tid * 3] = C0;
        sC[tid * 3 + 1] = C1;
        sC[tid * 3 + 2] = C2;
        sGain[tid] = gainful ? 1 : 0;
    }
    __syncthreads();

    // the applied slots, in slot order (block-uniform), as shortcut_partial_commit_kernel selects them - "gainful" for "free"
    int sa[kShortcutMaxSlots], sb[kShortcutMaxSlots];
    int applied = 0, cnt = n, lo = INT_MAX;
#pragma unroll
    for (int p = 0; p < kShortcutMaxSlots; ++p) {
        sa[p] = INT_MAX;
        sb[p] = INT_MAX;
        if (p < P) {
            const int64_t e = r * P + p;
            const int ea = a.picks[e * 2], eb = a.picks[e * 2 + 1];
            bool ok = sGain[p] != 0;
#pragma unroll
            for (int q = 0; q < p; ++q) ok = ok && (eb < sa[q] || sb[q] < ea);
            ok = ok && cnt + 2 - (eb - ea) <= W;
            if (ok) {
                sa[p] = ea;
                sb[p] = eb;
                ++applied;
                cnt += 2 - (eb - ea);
                lo = min(lo, ea);
            }
        }
    }
    if (applied == 0) return;   // (block-uniform)

    // waypoints 0 .. lo and segments 0 .. lo - 1 stay where they are.  The survivors beyond them into the stages, at their new
    // index (a segment moves with its first waypoint; segments sa .. sb of an applied slot are gone) ...
    float* const row = a.path + r * (int64_t)W * dof;
    float* const stage = a.stage + r * (int64_t)W * dof;
    float* const stage_seg = cc.stage_seg + r * (int64_t)W;
    const int begin = (lo + 1) * dof;   // (W * dof <= 65536 * DCX_MAX_DOF)
    for (int at = begin + tid; at < n * dof; at += kShortcutThreads) {
        const int k = at / dof;
        bool dead = false;
        int shift = 0;
#pragma unroll
        for (int p = 0; p < kShortcutMaxSlots; ++p) {
            dead = dead || (sa[p] < k && k <= sb[p]);
            shift += sb[p] < k ? 2 - (sb[p] - sa[p]) : 0;
        }
        if (!dead) stage[at + shift * dof] = row[at];   // (new index k + shift in lo + 3 .. cnt - 1)
    }
    for (int k = lo + 1 + tid; k < n - 1; k += kShortcutThreads) {
        bool dead = false;
        int shift = 0;
#pragma unroll
        for (int p = 0; p < kShortcutMaxSlots; ++p) {
            dead = dead || (sa[p] <= k && k <= sb[p]);
            shift += sb[p] < k ? 2 - (sb[p] - sa[p]) : 0;
        }
        if (!dead) stage_seg[k + shift] = lds ? sSeg[k] : segrow[k];   // (new index in lo + 3 .. cnt - 2)
    }
    // ... and every applied slot's xa, xb behind its waypoint ea, its three costs from the new index of ea on
#pragma unroll
    for (int p = 0; p < kShortcutMaxSlots; ++p) {
        if (sa[p] == INT_MAX) continue;   // (block-uniform)
        int at = sa[p];
#pragma unroll
        for (int q = 0; q < kShortcutMaxSlots; ++q) at += sb[q] < sa[p] ? 2 - (sb[q] - sa[q]) : 0;
        const int64_t e = r * P + p;
        for (int i = tid; i < 2 * dof; i += kShortcutThreads)   // (rows at + 1, at + 2 <= cnt - 2: piece 1's two ends)
            stage[(at + 1) * dof + i] = i < dof ? a.qa[(e * 3 + 1) * dof + i] : a.qb[(e * 3 + 1) * dof + i - dof];
        if (tid < 3) stage_seg[at + tid] = sC[p * 3 + tid];   // (segments at .. at + 2 <= cnt - 2)
    }
    __syncthreads();   // every read of the path's row, of seg (and of count[r]) is done; the stages are written
    for (int at = begin + tid; at < cnt * dof; at += kShortcutThreads) row[at] = stage[at];
    for (int k = lo + tid; k < cnt - 1; k += kShortcutThreads) segrow[k] = stage_seg[k];
    if (tid == 0) {
        a.count[r] = cnt;
        a.accepted[r] += applied;
    }
}
}  // namespace

hipError_t launch_shortcut_cost_pick(const ShortcutCostArgs& c, hipStream_t st) {
    const int64_t E = (int64_t)c.a.R * c.a.P;
    shortcut_cost_pick_kernel<<<dim3((unsigned)((E + kShortcutThreads - 1) / kShortcutThreads)), dim3(kShortcutThreads), 0, st>>>(c);
    return hipGetLastError();
}

hipError_t launch_shortcut_cost_commit(const ShortcutCostArgs& c, hipStream_t st) {
    shortcut_cost_commit_kernel<<<dim3((unsigned)c.a.R), dim3(kShortcutThreads), 0, st>>>(c);
    return hipGetLastError();
}

hipError_t launch_shortcut_partial_cost_pick(const ShortcutCostArgs& c, hipStream_t st) {
    shortcut_partial_cost_pick_kernel<<<dim3((unsigned)c.a.R), dim3(kResampleThreads), 0, st>>>(c);
    return hipGetLastError();
}

hipError_t launch_shortcut_partial_cost_commit(const ShortcutCostArgs& c, hipStream_t st) {
    shortcut_partial_cost_commit_kernel<<<dim3((unsigned)c.a.R), dim3(kShortcutThreads), 0, st>>>(c);
    return hipGetLastError();
}

}  // namespace dcx
