// knn_kernels.hip — dcx_knn (include/dcx.h): the k nearest points of every query under the motion calls' metric, bit for bit
// the squared edge length motion_prep.hip accumulates (wrap_device.h motion_delta, every fp32 operation rounded on its own).
//   search: grid (64-query tiles) x (point splits), kKnnWaves waves per block.  One lane owns one query; the block's waves divide
//           the block's points.  A wave's point rows are wave-uniform: scalar loads.  A lane's best k so far are a column of
//           64-bit keys bits(dist2) << 32 | index in LDS ([k][64] per wave: the lanes side by side, no bank conflict), unsorted,
//           the largest of them and its slot in registers: a point that does not enter costs one compare; one that does takes
//           the largest's slot, and one pass over the column (k independent reads) finds the new largest.  (A sorted column
//           shifted on every entry is a chain of dependent LDS reads, and a wave pays it whenever ANY of its lanes admits a
//           point: 154 ms instead of this form's time at N = Q = 65536, k = 64.)
//           Wave 0 then folds the other waves' columns into its own, sorts it once and writes idx / dist2 (one split) or the
//           column (several).
//   merge:  one wave per query over the splits' columns: each lane folds its share of them into a sorted column of its own,
//           then k rounds of a wave-wide minimum over the 64 heads take the answer off in order.
// Keys are unique (the index is part of them) and totally ordered, so the result does not depend on the split, the wave count
// or the order anything arrives in; nothing here is atomic.
#include <hip/hip_runtime.h>
#include <math.h>
#include "knn_kernel.h"
#include "wrap_device.h"

namespace dcx {
namespace {
typedef unsigned long long u64;

// key into the lane's sorted column col[i * 64], i < k; the caller has checked key < col[(k - 1) * 64].  Returns the new k-th key.
__device__ __forceinline__ u64 knn_insert(u64* col, int k, u64 key) {
    int i = k - 1;
    while (i > 0) {
        const u64 prev = col[(i - 1) * 64];
        if (prev <= key) break;
        col[i * 64] = prev;
        --i;
    }
    col[i * 64] = key;
    return col[(k - 1) * 64];
}

// key into the lane's UNSORTED column in place of its largest key `kth` at slot `kpos` (the caller has checked key < kth), then
// the new largest and its slot.  Empty slots all hold kKnnEmpty: the first of them is found, which is as good as any.
__device__ __forceinline__ void knn_replace_max(u64* col, int k, u64 key, u64& kth, int& kpos) {
    col[kpos * 64] = key;
    u64 m = key;
    int at = kpos;
#pragma unroll 8
    for (int i = 0; i < k; ++i) {
        const u64 v = col[i * 64];
        if (v > m) {
            m = v;
            at = i;
        }
    }
    kth = m;
    kpos = at;
}

// the lane's column in ascending order (once per tile: an insertion sort)
__device__ __forceinline__ void knn_sort(u64* col, int k) {
    for (int i = 1; i < k; ++i) {
        const u64 key = col[i * 64];
        int j = i;
        while (j > 0) {
            const u64 prev = col[(j - 1) * 64];
            if (prev <= key) break;
            col[j * 64] = prev;
            --j;
        }
        col[j * 64] = key;
    }
}

// DOF 1 .. kKnnRegDof: the query in registers, the coordinate loop unrolled.  DOF 0: the query tile in LDS ([dof][64]), any dof.
template <int DOF, bool WRAP>
__global__ __launch_bounds__(kKnnWaves * 64) void knn_search_kernel(const KnnArgs a) {
    extern __shared__ u64 sm[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = a.k, dof = DOF > 0 ? DOF : a.dof;
    u64* const col = sm + (size_t)wave * k * 64 + lane;
    float* const sq = reinterpret_cast<float*>(sm + (size_t)kKnnWaves * k * 64) + lane;   // DOF 0: sq[j * 64]
    const int64_t q = (int64_t)blockIdx.x * 64 + lane;
    const bool live = q < a.Q;
    const float* qrow = a.queries + (live ? q : a.Q - 1) * dof;   // a lane past the end searches for the last query and writes nothing
    float qr[DOF > 0 ? DOF : 1];
    if constexpr (DOF > 0) {
#pragma unroll
        for (int j = 0; j < DOF; ++j) qr[j] = qrow[j];
    } else {
        for (int j = wave; j < dof; j += kKnnWaves) sq[j * 64] = qrow[j];
        __syncthreads();
    }
    for (int i = 0; i < k; ++i) col[i * 64] = kKnnEmpty;
    u64 kth = kKnnEmpty;
    int kpos = 0;

    // the block's share of the points, then the wave's share of that (either may be empty)
    const int64_t N = a.N, per = (N + a.splits - 1) / a.splits;
    const int64_t lo = std::min<int64_t>(N, (int64_t)blockIdx.y * per), hi = std::min<int64_t>(N, lo + per);
    const int64_t wper = (hi - lo + kKnnWaves - 1) / kKnnWaves;
    const int64_t wlo = std::min<int64_t>(hi, lo + wave * wper), whi = std::min<int64_t>(hi, wlo + wper);
    const int64_t self = a.self_offset >= 0 ? a.self_offset + q : -1;
    const uint64_t mask = a.wrap_mask;
    const float max_d2 = a.max_dist2;

    auto dist2 = [&](int64_t p) {
#pragma clang fp contract(off)
        // motion_prep.hip's accumulation for the edge query -> point: subtract, (wrap,) multiply, add, each rounded on its own
        const float* pt = a.points + p * dof;
        float l2 = 0.0f;
        if constexpr (DOF > 0) {
#pragma unroll
            for (int j = 0; j < DOF; ++j) {
                const float d = WRAP ? motion_delta(qr[j], pt[j], mask, j) : __fsub_rn(pt[j], qr[j]);
                l2 = l2 + d * d;
            }
        } else {
            for (int j = 0; j < dof; ++j) {
                const float d = WRAP ? motion_delta(sq[j * 64], pt[j], mask, j) : __fsub_rn(pt[j], sq[j * 64]);
                l2 = l2 + d * d;
            }
        }
        return l2;
    };
    auto consider = [&](float l2, int64_t p) {
        // a NaN fails the first comparison; dist2 is never negative or -0, so its bits order like its value
        if (l2 <= max_d2 && p != self) {
            const u64 key = ((u64)__float_as_uint(l2) << 32) | (u64)(uint32_t)p;
            if (key < kth) knn_replace_max(col, k, key, kth, kpos);
        }
    };
    int64_t p = wlo;
    for (; p + 4 <= whi; p += 4) {   // four rows' scalar loads in flight
        const float d0 = dist2(p), d1 = dist2(p + 1), d2 = dist2(p + 2), d3 = dist2(p + 3);
        consider(d0, p);
        consider(d1, p + 1);
        consider(d2, p + 2);
        consider(d3, p + 3);
    }
    for (; p < whi; ++p) consider(dist2(p), p);

    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < kKnnWaves; ++w) {
        const u64* other = sm + (size_t)w * k * 64 + lane;
        for (int i = 0; i < k; ++i) {   // (an empty slot never enters)
            const u64 key = other[i * 64];
            if (key < kth) knn_replace_max(col, k, key, kth, kpos);
        }
    }
    knn_sort(col, k);
    if (!live) return;
    if (a.splits == 1) {
        for (int i = 0; i < k; ++i) {
            const u64 key = col[i * 64];
            a.idx[q * k + i] = key == kKnnEmpty ? -1 : (int32_t)(uint32_t)key;
            a.dist2[q * k + i] = key == kKnnEmpty ? INFINITY : __uint_as_float((uint32_t)(key >> 32));
        }
    } else {
        u64* out = a.part + (q * a.splits + blockIdx.y) * k;
        for (int i = 0; i < k; ++i) out[i] = col[i * 64];
    }
}

__global__ __launch_bounds__(kKnnWaves * 64) void knn_merge_kernel(const KnnArgs a) {
    extern __shared__ u64 sm[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = a.k;
    const int64_t q = (int64_t)blockIdx.x * kKnnWaves + wave;
    if (q >= a.Q) return;   // wave-uniform; no barrier below
    u64* const col = sm + (size_t)wave * k * 64 + lane;
    for (int i = 0; i < k; ++i) col[i * 64] = kKnnEmpty;
    u64 kth = kKnnEmpty;
    for (int s = lane; s < a.splits; s += 64) {
        const u64* in = a.part + (q * a.splits + s) * k;
        for (int i = 0; i < k; ++i) {
            const u64 key = in[i];
            if (key >= kth) break;
            kth = knn_insert(col, k, key);
        }
    }
    // the 64 columns are sorted and their keys distinct: the wave's minimum head is the next neighbour, and exactly one lane
    // holds it.  Round r's key stays with lane r (k <= 64), so the row goes out in one store per array.
    int head = 0;
    u64 mine = kKnnEmpty;
    for (int r = 0; r < k; ++r) {
        const u64 h = head < k ? col[head * 64] : kKnnEmpty;
        u64 m = h;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const u64 o = __shfl_xor(m, d, 64);
            m = o < m ? o : m;
        }
        if (m == kKnnEmpty) break;   // nothing left anywhere: the remaining slots stay empty
        if (h == m) ++head;
        if (lane == r) mine = m;
    }
    if (lane < k) {
        a.idx[q * k + lane] = mine == kKnnEmpty ? -1 : (int32_t)(uint32_t)mine;
        a.dist2[q * k + lane] = mine == kKnnEmpty ? INFINITY : __uint_as_float((uint32_t)(mine >> 32));
    }
}

template <int DOF>
hipError_t search(const KnnArgs& a, const KnnPlan& p, hipStream_t st) {
    auto launch = [&](auto kern) {
        if (p.lds_bytes > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
            if (e != hipSuccess) return e;
        }
        kern<<<dim3((unsigned)p.tiles, (unsigned)p.splits), dim3(kKnnWaves * 64), p.lds_bytes, st>>>(a);
        return hipGetLastError();
    };
    return a.wrap_mask ? launch(knn_search_kernel<DOF, true>) : launch(knn_search_kernel<DOF, false>);
}
}  // namespace

hipError_t launch_knn(const KnnArgs& a, const KnnPlan& p, hipStream_t st) {
    hipError_t e;
    switch (a.dof <= kKnnRegDof ? a.dof : 0) {
#define DCX_CASE(D) case D: e = search<D>(a, p, st); break;
        DCX_CASE(1) DCX_CASE(2) DCX_CASE(3) DCX_CASE(4) DCX_CASE(5) DCX_CASE(6) DCX_CASE(7) DCX_CASE(8)
        DCX_CASE(9) DCX_CASE(10) DCX_CASE(11) DCX_CASE(12) DCX_CASE(13) DCX_CASE(14) DCX_CASE(15) DCX_CASE(16)
#undef DCX_CASE
    default: e = search<0>(a, p, st); break;
    }
    if (e != hipSuccess || p.splits == 1) return e;
    const size_t lds = (size_t)kKnnWaves * a.k * 64 * sizeof(u64);
    if (lds > 64 * 1024) {
        e = hipFuncSetAttribute((const void*)knn_merge_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    knn_merge_kernel<<<dim3((unsigned)((a.Q + kKnnWaves - 1) / kKnnWaves)), dim3(kKnnWaves * 64), lds, st>>>(a);
    return hipGetLastError();
}

}  // namespace dcx
