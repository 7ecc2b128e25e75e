// sssp_kernels.hip — the kernels of dcx_sssp_run and dcx_sssp_extract_paths (include/dcx.h, "roadmap queries"; sssp_kernel.h):
// shortest paths over a roadmap for Q start/goal pairs at once, by synchronous min-plus relaxation in fp32.
//   fill, scatter: round 0.  One thread per (v, q) writes +inf into both dist buffers and -1 into pred; then one thread per
//            (q, s) writes its link's length into buffer 0.  A query's real link indices are distinct, so no two threads write
//            one element.
//   relax:   round t >= 1.  Lanes are queries: a wave owns (node v, 64 consecutive queries), the four waves of a block own four
//            consecutive nodes.  v is wave-uniform, so rowptr, col and weight are scalar loads; every neighbour u contributes one
//            coalesced 256-B read of dist_old[u][q0 .. q0 + 63], an add, a compare and two selects.  kSsspUnroll neighbour
//            rows are in flight per wave.  The wave ends with one coalesced store of dist_new and a predicated store of pred.
//            It pulls over the symmetric CSR, the row being its own inverted index: no atomic, and dist_old is never written.
//   extract: one wave per query.  The goal slot, the walk along pred and the sizes are wave-uniform; the lanes run across the
//            coordinates of a row.  The chain is walked once for its depth and once more to write its rows.
// The sums are single rounded adds (fp contract off; there is no multiply to fuse with, the pragma states the contract).
#include <hip/hip_runtime.h>
#include <math.h>
#include "sssp_kernel.h"

namespace dcx {
namespace {

// the call's flags, zeroed by a launch of its own: a memset node of a captured call was seen to replay other bytes than zeros
__global__ __launch_bounds__(kSsspFillThreads) void sssp_zero_kernel(int32_t* const changed, const int32_t n) {
    const int64_t i = (int64_t)blockIdx.x * kSsspFillThreads + threadIdx.x;
    if (i < n) changed[i] = 0;
}

__global__ __launch_bounds__(kSsspFillThreads) void sssp_fill_kernel(const SsspArgs a) {
    const int64_t NQ = (int64_t)a.N * a.Q;
    const int64_t i = (int64_t)blockIdx.x * kSsspFillThreads + threadIdx.x;
    if (i >= NQ) return;
    a.dist[i] = INFINITY;
    a.dist[NQ + i] = INFINITY;
    a.pred[i] = -1;
}

__global__ __launch_bounds__(kSsspFillThreads) void sssp_scatter_kernel(const SsspArgs a, int32_t* const changed) {
    const int64_t j = (int64_t)blockIdx.x * kSsspFillThreads + threadIdx.x;
    if (j >= (int64_t)a.Q * a.k) return;
    const int64_t q = j / a.k;
    const int32_t v = a.link_idx[j];
    if ((uint32_t)v < (uint32_t)a.N) {   // (-1, and whatever else is no node: no link)
        a.dist[(int64_t)v * a.Q + q] = a.link_len[j];
        *changed = 1;
    }
}

__global__ __launch_bounds__(kSsspWaves* kSsspLanes) void sssp_relax_kernel(const SsspArgs a, const float* __restrict__ const old,
                                                                           float* __restrict__ const nw, const int32_t* const prev,
                                                                           int32_t* const changed) {
#pragma clang fp contract(off)
    if (prev != nullptr && *prev == 0) return;   // (grid-uniform) the round before changed nothing: both buffers are equal
    const int v = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kSsspWaves + (threadIdx.x >> 6)));
    const int q = (int)blockIdx.y * kSsspLanes + (int)(threadIdx.x & (kSsspLanes - 1));
    const int N = a.N, Q = a.Q;
    if (v >= N || q >= Q) return;   // (v: wave-uniform; q: the tail lanes of the last query block do nothing)
    const int beg = max(a.rowptr[v], 0), end = min(a.rowptr[v + 1], a.nnz);
    const float* const oq = old + q;   // column q of dist_old: N * Q <= 2^31 - 1, so u * Q is an int
    const float d0 = oq[(int64_t)(v * Q)];
    float best = INFINITY;
    int bu = -1;
    int e = beg;
    for (; e + kSsspUnroll <= end; e += kSsspUnroll) {
        int u[kSsspUnroll];
        float w[kSsspUnroll], d[kSsspUnroll];
#pragma unroll
        for (int j = 0; j < kSsspUnroll; ++j) {
            const int c = a.col[e + j];
            const bool ok = (uint32_t)c < (uint32_t)N;   // (an entry that is no node is skipped: its candidate is +inf)
            const float wj = a.weight[e + j];   // (loaded whatever ok says: a select, not a branch per entry)
            u[j] = ok ? c : v;
            w[j] = ok ? wj : INFINITY;
        }
#pragma unroll
        for (int j = 0; j < kSsspUnroll; ++j) d[j] = oq[(int64_t)(u[j] * Q)];
#pragma unroll
        for (int j = 0; j < kSsspUnroll; ++j) {
            const float c = d[j] + w[j];
            if (c < best) {   // strict: the first entry that attains the minimum keeps it; inf and NaN never win
                best = c;
                bu = u[j];
            }
        }
    }
    for (; e < end; ++e) {
        const int c0 = a.col[e];
        const bool ok = (uint32_t)c0 < (uint32_t)N;
        const float w0 = a.weight[e];
        const int u = ok ? c0 : v;
        const float w = ok ? w0 : INFINITY;
        const float c = oq[(int64_t)(u * Q)] + w;
        if (c < best) {
            best = c;
            bu = u;
        }
    }
    const int64_t at = (int64_t)(v * Q) + q;
    if (best < d0) {
        nw[at] = best;
        a.pred[at] = bu;
        *changed = 1;
    } else {
        nw[at] = d0;
    }
}

__global__ __launch_bounds__(kSsspLanes) void sssp_extract_kernel(const SsspExtractArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const int q = blockIdx.x;   // (everything but the lane's coordinate is wave-uniform)
    const int N = a.N, Q = a.Q, dof = a.dof, W = a.W;
    const int mode = a.mode[q];
    float* const row = a.path + (int64_t)q * W * dof;
    const float* const s = a.starts + (int64_t)q * dof;
    const float* const g = a.goals + (int64_t)q * dof;
    if (mode == 1) {
        if (W >= 2)
            for (int c = lane; c < dof; c += kSsspLanes) {
                row[c] = s[c];
                row[dof + c] = g[c];
            }
        if (lane == 0) {
            a.count[q] = W >= 2 ? 2 : -2;
            a.length[q] = a.direct_len[q];
        }
        return;
    }
    float best = INFINITY;
    int last = -1;
    if (mode == 2) {
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
    if (!ok) {
        if (lane == 0) {
            a.count[q] = 0;
            a.length[q] = INFINITY;
        }
        return;
    }
    const int n = depth + 2;
    if (n <= W) {
        for (int c = lane; c < dof; c += kSsspLanes) {
            row[c] = s[c];
            row[(int64_t)(n - 1) * dof + c] = g[c];
        }
        int i = last;
        for (int h = 0; h < depth; ++h) {   // the walk runs goal -> start: its node h is waypoint depth - h
            for (int c = lane; c < dof; c += kSsspLanes) row[(int64_t)(depth - h) * dof + c] = a.nodes[(int64_t)i * dof + c];
            i = a.pred[(int64_t)(i * Q) + q];
        }
    }
    if (lane == 0) {
        a.count[q] = n <= W ? n : -n;
        a.length[q] = best;
    }
}
}  // namespace

hipError_t launch_sssp_zero(int32_t* changed, int32_t n, hipStream_t st) {
    sssp_zero_kernel<<<dim3((unsigned)((n + kSsspFillThreads - 1) / kSsspFillThreads)), dim3(kSsspFillThreads), 0, st>>>(changed, n);
    return hipGetLastError();
}

hipError_t launch_sssp_init(const SsspArgs& a, int32_t* changed, hipStream_t st) {
    const int64_t NQ = (int64_t)a.N * a.Q, L = (int64_t)a.Q * a.k;
    sssp_fill_kernel<<<dim3((unsigned)((NQ + kSsspFillThreads - 1) / kSsspFillThreads)), dim3(kSsspFillThreads), 0, st>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    sssp_scatter_kernel<<<dim3((unsigned)((L + kSsspFillThreads - 1) / kSsspFillThreads)), dim3(kSsspFillThreads), 0, st>>>(a, changed);
    return hipGetLastError();
}

hipError_t launch_sssp_relax(const SsspArgs& a, int32_t t, const int32_t* prev, int32_t* changed, hipStream_t st) {
    const int64_t NQ = (int64_t)a.N * a.Q;
    const float* const old = a.dist + (int64_t)((t - 1) & 1) * NQ;
    float* const nw = a.dist + (int64_t)(t & 1) * NQ;
    const dim3 grid((unsigned)((a.N + kSsspWaves - 1) / kSsspWaves), (unsigned)((a.Q + kSsspLanes - 1) / kSsspLanes));
    sssp_relax_kernel<<<grid, dim3(kSsspWaves * kSsspLanes), 0, st>>>(a, old, nw, prev, changed);
    return hipGetLastError();
}

hipError_t launch_sssp_extract(const SsspExtractArgs& a, hipStream_t st) {
    sssp_extract_kernel<<<dim3((unsigned)a.Q), dim3(kSsspLanes), 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace dcx
