// motion_cost_kernel.h — differentiable motion costs (dcx_motion_cost): for E straight joint-space motions qa[e] -> qb[e],
//     cost[e] = weight * sum over the edge's samples x_k of sum_c max(0, score_c(x_k) - margin_c)
// and its gradients with respect to qa[e] and qb[e] through the interpolation (the optimisers' collision term, reference
// optim.py:88-89 and :708-711, summed over dcx_check_motions' sample set).
//
// The work list and the tile are dcx_check_motions' (motion_tile.h), the sweep dcx_score_grad's.  Each tile writes PER FLAT
// SAMPLE its hinge value h and dq = d(weight * h)/dx (J^T applied) into the caller's workspace.  A separate small kernel
// (motion_cost_reduce) sums each edge's samples in sample order and applies the chain coefficients of the interpolation: no
// floating-point atomics, the same bits on every call.
//   C == 1: one sweep (MODE_GRAD_ROW) whose folded gradient is scaled by weight * 1[s - m > 0] (ScoreArgs::hinge == 1's rule).
//   C > 1:  two passes, as dcx_score_hinge_grad_mc runs them: a score-only pass (MODE_SCORE) stores the class scores and h
//           per flat sample and marks the tiles holding a sample with h > 0; then the gradient sweep (MODE_GRAD_UP, upstream
//           weight * 1[s_c > m_c]) on the marked tiles only - the others leave before staging anything.
// The reduction reads dq only where h > 0 (h > 0 iff some class's indicator is 1), so an unmarked tile's dq is never read.
#pragma once
#include "dcx_internal.h"
#include "motion_tile.h"

namespace dcx {

struct MotionCostArgs : MotionEdgeArgs {
    const float* margin;      // [c_out] or null (0)
    float* h;                 // [E * max_samples] per flat sample: sum_c max(0, s_c - m_c)
    float* dq;                // [E * max_samples][dof] per flat sample: d(weight * h)/dx
    float* scores;            // C > 1: [E * max_samples][c_out] the score pass's class scores, read by the gradient pass
    int32_t* tile_on;         // C > 1: [tiles] 1 if the tile holds a sample with h > 0 (written by the score pass)
    float weight;
    int32_t open_end;         // max_step rule: the target qb is not a sample
};

// one entry point per compiled width (motion_cost_inst.hip); mode: MODE_GRAD_ROW (C == 1), MODE_SCORE / MODE_GRAD_UP (C > 1)
typedef hipError_t (*motion_cost_fn)(int kf, int cc, int mode, int nw, size_t lds, int64_t n_blocks, const MotionCostArgs& a,
                                     hipStream_t stream);
#define DCX_DECLARE_MOTION_COST(D) \
    hipError_t launch_motion_cost_D##D(int, int, int, int, size_t, int64_t, const MotionCostArgs&, hipStream_t);
DCX_FOREACH_WIDTH(DCX_DECLARE_MOTION_COST)
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
// One configuration per lane.  The block's partial sums (CC scores, and D gradient entries in the gradient passes) fold as
// score_kernel folds them (motion_tile.h motion_fold_block, TREE).
template <int D, int KF, int CC, int MODE, int MAXT, int XF = 0 /* motion_tile.h motion_sweep */>
__global__ __launch_bounds__(MAXT, sweep_min_waves(D, CC, KF)) void motion_cost_kernel(const MotionCostArgs m, int32_t mo_off) {
    static_assert((CC == 1) == (MODE == MODE_GRAD_ROW), "one class: the hinge sweep; several: the score and gradient passes");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NG = MODE != MODE_SCORE ? D : 0;
    constexpr int ACC = NG + CC;
    const ScoreArgs& a = m.sc;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nw = blockDim.x >> 6;
    const LdsPlan lp = lds_plan(a.dof, a.d_fk, a.frame_floats, nw > 1 ? a.red_slots : 0, ACC, true);
    const MotionTile mt = motion_tile_view(smem, lp, mo_off);
    const int64_t total = m.offs[m.E];
    const int64_t tile = blockIdx.x;
    if (tile * 64 >= total) return;   // past the end of the work list: before any staging
    if constexpr (MODE == MODE_GRAD_UP) {
        if (m.tile_on[tile] == 0) return;   // no sample of this tile is in collision: its gradient is zero, never read
    }
    const FkWalk fw = fk_stage_sel(a.fkk, a.fk, a.fk_dwords, a.dh, smem + lp.fk, threadIdx.x, blockDim.x);
    const int64_t base = tile * 64;
    const int nb = (int)((total - base) < 64 ? (total - base) : 64);
    if (wave == 0) motion_tile_lookup(m.offs, m.E, base, nb, mt);
    __syncthreads();
    float x[D];
    motion_tile_features<D, XF>(m, mt, fw, m.open_end != 0, wave, nw, x);
    float up[CC];
#pragma unroll
    for (int c = 0; c < CC; ++c) up[c] = 0.0f;
    if constexpr (MODE == MODE_GRAD_UP) {   // the hinge's upstream from the score pass: weight * 1[s_c - m_c > 0]
        const int lane0 = threadIdx.x & 63;
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
    motion_sweep<D, KF, CC, MODE, XF>(a, x, up, wave, nw, sc, gx);

    // ---- epilogue: arguments read afresh (score_kernel.h reload_args) ----
    const auto& b = reload_kernargs<MotionCostArgs>();
    const int lane = fresh_lane();
    const LdsPlan lq = lds_plan(b.sc.dof, b.sc.d_fk, b.sc.frame_floats, nw > 1 ? b.sc.red_slots : 0, ACC, true);
    if (!motion_fold_block<CC, NG, true>(smem + lq.red, b.sc.red_slots, wave, lane, nw, sc, gx)) return;
    const int64_t t = blockIdx.x;
    if (!motion_split_handover<CC, NG>(b.sc, t, lane, sc, gx)) return;
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
