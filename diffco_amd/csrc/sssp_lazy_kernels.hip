// sssp_lazy_kernels.hip — the kernels of dcx_sssp_mark_routes and dcx_graph_apply_checks (include/dcx.h, "lazy roadmap
// queries"; sssp_lazy_kernel.h): which unchecked edges the current shortest routes stand on, as one ordered list ready for
// the motion checks, and the checks' verdicts written back into the graph.
//   zero:    the marks (whole groups, the padding included) and, for the apply call, its flag: a launch, not a memset node.
//   mark:    one wave per query, everything wave-uniform.  The goal slot and the walk along pred are sssp_extract_kernel's: the
//            chain is walked once for its depth (a walk that does not end within N nodes or leaves 0 .. N - 1 marks nothing)
//            and once more for its hops.  For a hop (v, u = pred[v][q]) the lanes look through row v together, 64 entries a
//            step, for the first entry whose col is u (a ballot); its edge, if still unknown, gets mark[m] = 1: a plain store
//            of the one value every other wave would store there.
//   scan:    one workgroup over the groups of 16 marks: a thread adds its group's marks from one 16-byte load (marks are 0 or
//            1: four popcounts), the 1024 sums are scanned by wave shuffles and one pass over the 16 wave totals, as
//            motion_band_finish.hip's scan.  It ends with the totals in n_out.
//   scatter: a thread per group lays its marked ids behind the group's offset in id order, with the two rows of nodes the
//            motion checks take, while the entry lies below capacity.
//   apply:   a thread per listed edge, striding: state, and +inf into both CSR entries of an edge that hit.
// No atomics and no order of arrival anywhere: the list is ordered by the offsets, the same bits every call.
#include <hip/hip_runtime.h>
#include <math.h>
#include "sssp_lazy_kernel.h"

namespace dcx {
namespace {

__global__ __launch_bounds__(kLazyThreads) void lazy_zero_kernel(uint32_t* const words, const int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kLazyThreads + threadIdx.x;
    if (i < n) words[i] = 0u;
}

__global__ __launch_bounds__(kLazyLanes) void sssp_mark_kernel(const LazyMarkArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const int q = blockIdx.x;   // (everything but the lane's entry of a row is wave-uniform)
    const int N = a.N, Q = a.Q;
    float best = INFINITY;
    int last = -1;
    if (a.mode[q] == 2) {
        for (int k = 0; k < a.k; ++k) {
            const int v = a.goal_idx[(int64_t)q * a.k + k];
            if ((uint32_t)v >= (uint32_t)N) continue;
            const float c = a.dist[(int64_t)(v * Q) + q] + a.goal_len[(int64_t)q * a.k + k];
            if (c < best) {
                best = c;
                last = v;
            }
        }
    }
    // the chain's nodes, last .. the linked one: at most N of them, every index a node's
    int depth = 0;
    bool ok = last >= 0;
    for (int i = last; ok && i != -1; i = a.pred[(int64_t)(i * Q) + q]) {
        if ((uint32_t)i >= (uint32_t)N || depth >= N) {
            ok = false;
            break;
        }
        ++depth;
    }
    int pend = 0;
    if (ok) {
        int v = last;
        for (int h = 0; h + 1 < depth; ++h) {   // depth nodes, depth - 1 hops; every node was seen to lie in 0 .. N - 1
            const int u = a.pred[(int64_t)(v * Q) + q];
            const int beg = max(a.rowptr[v], 0), end = min(a.rowptr[v + 1], a.nnz);
            int found = -1;
            for (int e0 = beg; e0 < end && found < 0; e0 += kLazyLanes) {
                const int e = e0 + lane;
                const uint64_t at = __builtin_amdgcn_ballot_w64(e < end && a.col[e] == u);
                if (at) found = e0 + (int)__builtin_ctzll(at);
            }
            if (found >= 0) {   // (a hop without an entry, or an entry without an edge, is skipped)
                const int m = a.eid[found];
                if ((uint32_t)m < (uint32_t)a.M && a.state[m] == 0) {
                    if (lane == 0) a.mark[m] = 1;
                    ++pend;
                }
            }
            v = u;
        }
    }
    if (lane == 0) a.pending[q] = pend;
}

__device__ inline int group_marks(const uint4 w) { return __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w); }

__global__ __launch_bounds__(kLazyScanThreads) void lazy_scan_kernel(const LazyMarkArgs a) {
    __shared__ int32_t sWave[kLazyScanThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint4* const marks = reinterpret_cast<const uint4*>(a.mark);
    int32_t carry = 0;
    for (int64_t g0 = 0; g0 < a.groups; g0 += kLazyScanThreads) {
        const int64_t g = g0 + t;
        const int32_t mine = g < a.groups ? group_marks(marks[g]) : 0;
        int32_t v = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {   // inclusive scan of the wave's 64 sums
            const int32_t u = __shfl_up(v, d, 64);
            if (lane >= d) v += u;
        }
        if (lane == 63) sWave[wave] = v;
        __syncthreads();
        int32_t before = carry, total = carry;
        for (int w = 0; w < kLazyScanThreads / 64; ++w) {
            if (w < wave) before += sWave[w];
            total += sWave[w];
        }
        if (g < a.groups) a.offs[g] = before + v - mine;
        carry = total;
        __syncthreads();   // sWave is rewritten by the next step
    }
    if (t == 0) {
        a.offs[a.groups] = carry;
        a.n_out[0] = carry;
        a.n_out[1] = (int32_t)((int64_t)carry < a.capacity ? (int64_t)carry : a.capacity);
    }
}

__global__ __launch_bounds__(kLazyThreads) void lazy_scatter_kernel(const LazyMarkArgs a) {
    const int64_t g = (int64_t)blockIdx.x * kLazyThreads + threadIdx.x;
    if (g >= a.groups) return;
    int64_t j = a.offs[g];
    if (j == a.offs[g + 1] || j >= a.capacity) return;
    const uint4 w = reinterpret_cast<const uint4*>(a.mark)[g];
    const uint32_t word[4] = {w.x, w.y, w.z, w.w};
    const int dof = a.dof;
#pragma unroll
    for (int b = 0; b < kLazyGroup; ++b) {
        if (((word[b >> 2] >> (8 * (b & 3))) & 0xffu) == 0u) continue;
        if (j >= a.capacity) return;
        const int32_t m = (int32_t)(g * kLazyGroup + b);   // (a padding byte is zero: m < M)
        a.list[j] = m;
        const int32_t ea = a.ends[2 * (int64_t)m], eb = a.ends[2 * (int64_t)m + 1];
        if ((uint32_t)ea < (uint32_t)a.N)   // (an end that is no node: the row stays as it is)
            for (int c = 0; c < dof; ++c) a.qa[j * dof + c] = a.nodes[(int64_t)ea * dof + c];
        if ((uint32_t)eb < (uint32_t)a.N)
            for (int c = 0; c < dof; ++c) a.qb[j * dof + c] = a.nodes[(int64_t)eb * dof + c];
        ++j;
    }
}

__global__ __launch_bounds__(kLazyThreads) void graph_apply_kernel(const LazyApplyArgs a) {
    const int32_t n = min(max(a.n_out[1], 0), a.M);   // (the list holds distinct edges: never more than M)
    for (int64_t i = (int64_t)blockIdx.x * kLazyThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kLazyThreads) {
        const int32_t m = a.list[i];
        if ((uint32_t)m >= (uint32_t)a.M) continue;
        const bool hit = a.hit[i] != 0;
        a.state[m] = hit ? 2 : 1;
        if (!hit) continue;
        const int32_t e0 = a.ent[2 * (int64_t)m], e1 = a.ent[2 * (int64_t)m + 1];
        if ((uint32_t)e0 < (uint32_t)a.nnz) a.weight[e0] = INFINITY;
        if ((uint32_t)e1 < (uint32_t)a.nnz) a.weight[e1] = INFINITY;
        *a.any_blocked = 1;
    }
}
}  // namespace

hipError_t launch_lazy_mark_routes(const LazyMarkArgs& a, hipStream_t st) {
    const int64_t words = a.groups * (kLazyGroup / 4);
    lazy_zero_kernel<<<dim3((unsigned)((words + kLazyThreads - 1) / kLazyThreads)), dim3(kLazyThreads), 0, st>>>(
        reinterpret_cast<uint32_t*>(a.mark), words);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    sssp_mark_kernel<<<dim3((unsigned)a.Q), dim3(kLazyLanes), 0, st>>>(a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    lazy_scan_kernel<<<dim3(1), dim3(kLazyScanThreads), 0, st>>>(a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    lazy_scatter_kernel<<<dim3((unsigned)((a.groups + kLazyThreads - 1) / kLazyThreads)), dim3(kLazyThreads), 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_lazy_apply(const LazyApplyArgs& a, hipStream_t st) {
    lazy_zero_kernel<<<dim3(1), dim3(kLazyThreads), 0, st>>>(reinterpret_cast<uint32_t*>(a.any_blocked), 1);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t blocks = ((int64_t)a.M + kLazyThreads - 1) / kLazyThreads;
    graph_apply_kernel<<<dim3((unsigned)(blocks < kLazyApplyBlocks ? blocks : kLazyApplyBlocks)), dim3(kLazyThreads), 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace dcx
