// motion_cost_kernel.h — differentiable motion costs (dcx_motion_cost): for E straight joint-space motions qa[e] -> qb[e],
//     cost[e] = weight * sum over the edge's samples x_k of sum_c max(0, score_c(x_k) - margin_c)
// and its gradients with respect to qa[e] and qb[e] through the interpolation (the optimisers' collision term, reference
// optim.py:88-89 and :708-711, summed over dcx_check_motions' sample set).
//
// The work list is dcx_check_motions' (motion_kernel.h): motion_prep.hip counts and scans the samples, a 64-sample tile takes 64
// consecutive flat samples, one tile per block, the grid sized from E * max_samples (surplus blocks leave at once).  Each tile
// interpolates its rows, runs FK and the sweep of dcx_score_grad (score_kernel.h sweep_rows: the same rows, slices, wave-group
// shares and split launches), and writes PER FLAT SAMPLE its hinge value h and dq = d(weight * h)/dx (J^T applied) into the
// caller's workspace.  A separate small kernel (motion_cost_reduce) sums each edge's samples in sample order and applies the
// chain coefficients of the interpolation: no floating-point atomics, the same bits on every call.
//   C == 1: one sweep (MODE_GRAD_ROW) whose folded gradient is scaled by weight * 1[s - m > 0] (ScoreArgs::hinge == 1's rule).
//   C > 1:  two passes, as dcx_score_hinge_grad_mc runs them: a score-only pass (MODE_SCORE) stores the class scores and h
//           per flat sample and marks the tiles holding a sample with h > 0; then the gradient sweep (MODE_GRAD_UP, upstream
//           weight * 1[s_c > m_c]) on the marked tiles only - the others leave before staging anything.
// The reduction reads dq only where h > 0 (h > 0 iff some class's indicator is 1), so an unmarked tile's dq is never read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "motion_kernel.h"

namespace dcx {

struct MotionCostArgs {
    ScoreArgs sc;             // the sweep's arguments (first: reload_kernargs reads them at offset 0).  sc.q / score / grad unused;
                              // sc.partial / sc.tile_done: the split launch's partial rows and arrival counters (caller's work)
    const float* qa;          // [E][dof]
    const float* qb;          // [E][dof]
    const int64_t* offs;      // [E + 1] exclusive scan of the sample counts (motion_prep.hip)
    const float* frac;        // [E] max_step rule: (1 / L) * max_step
    const float* margin;      // [c_out] or null (0)
    float* h;                 // [E * max_samples] per flat sample: sum_c max(0, s_c - m_c)
    float* dq;                // [E * max_samples][dof] per flat sample: d(weight * h)/dx
    float* scores;            // C > 1: [E * max_samples][c_out] the score pass's class scores, read by the gradient pass
    int32_t* tile_on;         // C > 1: [tiles] 1 if the tile holds a sample with h > 0 (written by the score pass)
    int64_t E;
    float weight;
    int32_t res;              // > 0: the res rule; 0: the max_step rule
    int32_t open_end;         // max_step rule: the target qb is not a sample
    uint64_t wrap_mask;       // bit j: coordinate j is an angle, the edge runs along its shortest arc (motion_kernel.h motion_coord)
};

// one entry point per compiled width (motion_cost_inst.hip); mode: MODE_GRAD_ROW (C == 1), MODE_SCORE / MODE_GRAD_UP (C > 1)
typedef hipError_t (*motion_cost_fn)(int kf, int cc, int mode, int nw, size_t lds, int64_t n_blocks, const MotionCostArgs& a,
                                     hipStream_t stream);
#define DCX_DECLARE_MOTION_COST(D) \
    hipError_t launch_motion_cost_D##D(int, int, int, int, size_t, int64_t, const MotionCostArgs&, hipStream_t);
DCX_DECLARE_MOTION_COST(2)  DCX_DECLARE_MOTION_COST(4)  DCX_DECLARE_MOTION_COST(6)  DCX_DECLARE_MOTION_COST(8)
DCX_DECLARE_MOTION_COST(12) DCX_DECLARE_MOTION_COST(16) DCX_DECLARE_MOTION_COST(18) DCX_DECLARE_MOTION_COST(21)
DCX_DECLARE_MOTION_COST(24) DCX_DECLARE_MOTION_COST(27) DCX_DECLARE_MOTION_COST(30) DCX_DECLARE_MOTION_COST(32)
DCX_DECLARE_MOTION_COST(36) DCX_DECLARE_MOTION_COST(42) DCX_DECLARE_MOTION_COST(48) DCX_DECLARE_MOTION_COST(54)
DCX_DECLARE_MOTION_COST(60) DCX_DECLARE_MOTION_COST(64) DCX_DECLARE_MOTION_COST(72) DCX_DECLARE_MOTION_COST(84)
DCX_DECLARE_MOTION_COST(96)
#undef DCX_DECLARE_MOTION_COST

// the per-edge reduction (motion_prep.hip): cost, grad_a, grad_b from h / dq; status[e] == -2 (over max_samples) gives NaN
struct MotionReduceArgs {
    const float* qa;
    const float* qb;
    const int64_t* offs;
    const float* frac;
    const int32_t* status;    // motion_prep's first_hit: -1, or -2 for an edge over max_samples
    const float* h;
    const float* dq;
    float* cost;              // [E]
    float* grad_a;            // [E][dof]
    float* grad_b;            // [E][dof]
    int64_t E;
    int32_t dof, res, open_end;
    float weight;
    uint64_t wrap_mask;       // u = delta / L from the wrapped delta of the masked coordinates (motion_prep's L)
};
hipError_t launch_motion_cost_reduce(const MotionReduceArgs& r, hipStream_t stream);

#ifdef __HIPCC__
// LDS behind the sweep's plan and the FK program: per lane its edge, sample index and count, the 64 edge ends (int64), a flag
constexpr int kMotionCostLdsFloats = kMotionLdsFloats;

// Wave 0: the edge, sample index and sample count of each lane of the tile starting at flat sample `base` (nb samples), into
// sEdge / sK / sN (dcx_check_motions' lookup: a 64-ary search in offs for the first edge, then a binary search in LDS over the
// next 64 edge ends, a global one when more than 64 edges end inside the tile)
__device__ __forceinline__ void motion_tile_lookup(const int64_t* offs, int64_t E, int64_t base, int nb, int64_t* sEnd,
                                                   int32_t* sEdge, int32_t* sK, int32_t* sN) {
    const int lane = threadIdx.x & 63;
    int64_t lo = 0, hi = E;
    while (hi - lo > 1) {
        const int64_t step = (hi - lo + 63) / 64;
        const int64_t idx = lo + (int64_t)lane * step;
        const bool le = idx < hi && offs[idx] <= base;
        const int p = __popcll(__builtin_amdgcn_ballot_w64(le));
        const int64_t nlo = lo + (int64_t)(p - 1) * step;
        hi = (lo + (int64_t)p * step < hi) ? lo + (int64_t)p * step : hi;
        lo = nlo;
    }
    const int64_t e0 = lo;
    sEnd[lane] = (e0 + 1 + lane <= E) ? offs[e0 + 1 + lane] : INT64_MAX;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    const int64_t s = base + (lane < nb ? lane : nb - 1);
    int64_t e, start;
    if (sEnd[63] > s) {
        int j = 0;
#pragma unroll
        for (int hh = 32; hh >= 1; hh >>= 1)
            if (sEnd[j + hh - 1] <= s) j += hh;
        e = e0 + j;
        start = j ? sEnd[j - 1] : offs[e0];
    } else {
        int64_t l2 = e0 + 64, h2 = E;
        while (h2 - l2 > 1) {
            const int64_t md = (l2 + h2) / 2;
            if (offs[md] <= s) l2 = md; else h2 = md;
        }
        e = l2;
        start = offs[l2];
    }
    sEdge[lane] = (int32_t)e;
    sK[lane] = (int32_t)(s - start);
    sN[lane] = (int32_t)(offs[e + 1] - start);
}

// One configuration per lane.  LDS: lds_plan(dof, d_fk, frame_floats, red_slots, ACC, true).total + prog_floats rounded to 4,
// then kMotionCostLdsFloats (mc_off).
template <int D, int KF, int CC, int MODE, int MAXT, int XF = 0 /* 1: the expanded form, 2: its spare-slot form (score_kernel.h sweep_rows SP) */>
__global__ __launch_bounds__(MAXT, sweep_min_waves(D, CC, KF)) void motion_cost_kernel(const MotionCostArgs m, int32_t mc_off) {
    static_assert((CC == 1) == (MODE == MODE_GRAD_ROW), "one class: the hinge sweep; several: the score and gradient passes");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr bool GRAD = MODE != MODE_SCORE;
    constexpr int ACC = (GRAD ? D : 0) + CC;
    const ScoreArgs& a = m.sc;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nw = blockDim.x >> 6;
    const int dof = a.dof;
    const LdsPlan lp = lds_plan(dof, a.d_fk, a.frame_floats, nw > 1 ? a.red_slots : 0, ACC, true);
    float* sQ = smem + lp.q;
    float* sX = smem + lp.x;
    float* sF = smem + lp.f;
    int64_t* sEnd = reinterpret_cast<int64_t*>(smem + mc_off);   // [64]
    int32_t* sEdge = reinterpret_cast<int32_t*>(smem + mc_off + 128);
    int32_t* sK = sEdge + 64;
    int32_t* sN = sEdge + 128;

    const int64_t E = m.E;
    const int64_t total = m.offs[E];
    const int64_t tile = blockIdx.x;
    if (tile * 64 >= total) return;   // past the end of the work list: before any staging
    if constexpr (MODE == MODE_GRAD_UP) {
        if (m.tile_on[tile] == 0) return;   // no sample of this tile is in collision: its gradient is zero, never read
    }
    const FkWalk fw = fk_stage_sel(a.fkk, a.fk, a.fk_dwords, a.dh, smem + lp.fk, threadIdx.x, blockDim.x);
    const int64_t base = tile * 64;
    const int nb = (int)((total - base) < 64 ? (total - base) : 64);
    if (wave == 0) motion_tile_lookup(m.offs, E, base, nb, sEnd, sEdge, sK, sN);
    __syncthreads();
    // ---- the rows of sQ: this tile's samples, interpolated from their edges (dcx_check_motions' arithmetic) ----
    for (int i = threadIdx.x; i < 64 * dof; i += blockDim.x) {
        const int l = i / dof, j = i - l * dof;
        const int64_t e = sEdge[l];
        const int k = sK[l];
        const float qa = m.qa[e * dof + j], qb = m.qb[e * dof + j];
        sQ[i] = motion_coord(qa, qb, k, m.res, !m.open_end && k == sN[l] - 1, m.frac + e, (m.wrap_mask >> j) & 1ull);
    }
    __syncthreads();
    {
        const int lane = threadIdx.x & 63;
        fk_trig_sel(fw, a.dh, sQ + lane * dof, sF + lane, wave, nw);
        __syncthreads();
        if (a.fkk == 2 && a.jt_rows) dh2_chain_rows_sel(fw.dh, a.dh, sX + lane, sF + lane, wave);
        else if (wave == 0) fk_chain_sel(fw, a.dh, sQ + lane * dof, sX + lane, sF + lane);
        __syncthreads();
    }
    const int lane0 = threadIdx.x & 63;
    float x[D];
    if (a.d_fk == D) {
#pragma unroll
        for (int k = 0; k < D; ++k) x[k] = sX[k * 64 + lane0];
    } else {
#pragma unroll
        for (int k = 0; k < D; ++k) x[k] = (k < a.d_fk) ? sX[k * 64 + lane0] : 0.0f;
    }
    if constexpr (XF != 0) {
        cfloat_ptr cen = (cfloat_ptr)(uintptr_t)a.centre;
#pragma unroll
        for (int k = 0; k < D; ++k) x[k] -= cen[k];
    }
    if (nw > 1) __syncthreads();   // X is dead: the partial sums reuse its LDS
    float up[CC];
#pragma unroll
    for (int c = 0; c < CC; ++c) up[c] = 0.0f;
    if constexpr (MODE == MODE_GRAD_UP) {   // the hinge's upstream from the score pass: weight * 1[s_c - m_c > 0]
        const int64_t s = base + (lane0 < nb ? lane0 : nb - 1);
#pragma unroll
        for (int c = 0; c < CC; ++c)
            if (c < a.c_out) up[c] = (m.scores[s * a.c_out + c] - (m.margin ? m.margin[c] : 0.0f) > 0.0f) ? m.weight : 0.0f;
    }
    float sc[CC];
    float gx[D];
#pragma unroll
    for (int c = 0; c < CC; ++c) sc[c] = 0.0f;
#pragma unroll
    for (int k = 0; k < D; ++k) gx[k] = 0.0f;
    const int ybase = blockIdx.y * a.s_super;
    const int yend = (ybase + a.s_super < a.S) ? (ybase + a.s_super) : a.S;
    int j0, j1;
    wave_slice(wave, nw, a.s_chunk, a.s_skew, ybase, yend, j0, j1);
    sweep_rows<D, KF, CC, MODE, XF != 0, 0, false, XF == 2>(a, x, up, j0, j1, sc, gx);

    // ---- epilogue: arguments read afresh (score_kernel.h reload_args); the block's partial sums meet on wave 0 ----
    const auto& b = reload_kernargs<MotionCostArgs>();
    const int lane = fresh_lane();
    const LdsPlan lq = lds_plan(b.sc.dof, b.sc.d_fk, b.sc.frame_floats, nw > 1 ? b.sc.red_slots : 0, ACC, true);
    float* sRed = smem + lq.red;
    if (nw > 1 && b.sc.red_slots == nw) {
        float* mine = sRed + (size_t)wave * ACC * 64 + lane;
#pragma unroll
        for (int c = 0; c < CC; ++c) mine[c * 64] = sc[c];
        if constexpr (GRAD) {
#pragma unroll
            for (int k = 0; k < D; ++k) mine[(CC + k) * 64] = gx[k];
        }
        __syncthreads();
        fold_partial_rows<ACC>(sRed, wave, lane, nw);
        __syncthreads();
        if (wave != 0) return;
#pragma unroll
        for (int c = 0; c < CC; ++c) sc[c] = sRed[c * 64 + lane];
        if constexpr (GRAD) {
#pragma unroll
            for (int k = 0; k < D; ++k) gx[k] = sRed[(CC + k) * 64 + lane];
        }
    } else if (nw > 1) {
        for (int w = 1; w < nw; ++w) {   // one LDS row: the waves hand their sums to wave 0 in turn
            if (wave == w) {
#pragma unroll
                for (int c = 0; c < CC; ++c) sRed[c * 64 + lane] = sc[c];
                if constexpr (GRAD) {
#pragma unroll
                    for (int k = 0; k < D; ++k) sRed[(CC + k) * 64 + lane] = gx[k];
                }
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int c = 0; c < CC; ++c) sc[c] += sRed[c * 64 + lane];
                if constexpr (GRAD) {
#pragma unroll
                    for (int k = 0; k < D; ++k) gx[k] += sRed[(CC + k) * 64 + lane];
                }
            }
            __syncthreads();
        }
        if (wave != 0) return;
    }
    const int64_t t = blockIdx.x;
    if (b.sc.partial != nullptr) {
        // the split launch's in-launch hand-over on wave 0 (score_kernel.h's one-wave form): publish write-through, drain,
        // count; the last block of the tile to arrive adds the ys rows in the order y = 0, 1, ... and finishes the tile
        float* out = b.sc.partial + (t * b.sc.ys + blockIdx.y) * ACC * 64 + lane;
#pragma unroll
        for (int c = 0; c < CC; ++c) __hip_atomic_store(out + c * 64, sc[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (GRAD) {
#pragma unroll
            for (int k = 0; k < D; ++k) __hip_atomic_store(out + (CC + k) * 64, gx[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned int arrived = 0;
        if (lane == 0) arrived = __hip_atomic_fetch_add(b.sc.tile_done + t * kCounterStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        arrived = __builtin_amdgcn_readfirstlane(arrived);
        if (arrived != (unsigned int)b.sc.ys - 1u) return;
        if (lane == 0) b.sc.tile_done[t * kCounterStride] = 0u;   // ready for the next launch on this work buffer
        asm volatile("" ::: "memory");
        const float* part = b.sc.partial + t * b.sc.ys * ACC * 64 + lane;
#pragma unroll
        for (int c = 0; c < CC; ++c) sc[c] = 0.0f;
        if constexpr (GRAD) {
#pragma unroll
            for (int k = 0; k < D; ++k) gx[k] = 0.0f;
        }
        for (int y = 0; y < b.sc.ys; ++y) {
#pragma unroll
            for (int c = 0; c < CC; ++c) sc[c] += __hip_atomic_load(part + ((size_t)y * ACC + c) * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if constexpr (GRAD) {
#pragma unroll
                for (int k = 0; k < D; ++k)
                    gx[k] += __hip_atomic_load(part + ((size_t)y * ACC + CC + k) * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    // ---- wave 0 alone: the tile's scores are final ----
    const int64_t tot = b.offs[b.E];
    const int64_t s0 = t * 64;
    const int n = (int)((tot - s0) < 64 ? (tot - s0) : 64);
    float hv = 0.0f;
#pragma unroll
    for (int c = 0; c < CC; ++c) {
        const float d = sc[c] - (b.margin ? b.margin[c] : 0.0f);
        if (c < b.sc.c_out && d > 0.0f) hv += d;
    }
    if constexpr (MODE == MODE_SCORE) {   // C > 1, first pass: class scores and h per sample, the tile's mark
        if (lane < n) {
#pragma unroll
            for (int c = 0; c < CC; ++c)
                if (c < b.sc.c_out) b.scores[(s0 + lane) * b.sc.c_out + c] = sc[c];
            b.h[s0 + lane] = hv;
        }
        const bool any = __builtin_amdgcn_ballot_w64(lane < n && hv > 0.0f) != 0;
        if (lane == 0) b.tile_on[t] = any ? 1 : 0;
    } else {
        float scale = 1.0f;
        if constexpr (MODE == MODE_GRAD_ROW) {
            scale = hv > 0.0f ? b.weight : 0.0f;
            if (lane < n) b.h[s0 + lane] = hv;
            // a wave with no active lane skips J^T: its rows are never read (the reduction reads dq where h > 0 only)
            if (__builtin_amdgcn_ballot_w64(lane < n && hv > 0.0f) == 0) return;
        }
        const int dofb = b.sc.dof;
        float* sG = smem + lq.g;
        float* sQb = smem + lq.q;
        float* sFb = smem + lq.f;
        if (b.sc.d_fk == D) {
#pragma unroll
            for (int k = 0; k < D; ++k) sG[k * 64 + lane] = gx[k] * scale;
        } else {
#pragma unroll
            for (int k = 0; k < D; ++k)
                if (k < b.sc.d_fk) sG[k * 64 + lane] = gx[k] * scale;
        }
        DhArgs dhb;
        DCX_COPY_DH(dhb, b.sc.dh);
        FkWalk fwb;
        fwb.fkk = b.sc.fkk;
        fwb.g = b.sc.fk;
        fwb.fk = (fk_cptr)(uintptr_t)(uint32_t)(uintptr_t)(smem + lq.fk);
        fwb.dh = (dh_cptr)(uintptr_t)(uint32_t)(uintptr_t)(smem + lq.fk);
        // J^T per lane, the gradient row built in place of the lane's q row (score_kernel.h)
        float* gq = sQb;
        fk_vjp_sel(fwb, dhb, sQb + lane * dofb, sFb + lane, sG + lane, gq + lane * dofb, dofb);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        float* gdst = b.dq + s0 * dofb;
        const int nn = n * dofb;
        for (int i = lane; i < nn; i += 64) gdst[i] = gq[i];
    }
}
#endif  // __HIPCC__

}  // namespace dcx
