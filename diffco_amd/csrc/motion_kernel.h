// motion_kernel.h — batched motion checks (dcx_check_motions): is the straight joint-space motion qa -> qb free, and if not,
// which of its samples is the first to collide?  Two small prep launches (sample counts, their exclusive scan, the edges' answers
// initialised) and ONE sweep launch over the tiles of the work list (motion_tile.h: the score-only sweep of dcx_score), which
// folds each finished score into first_hit[e] with a ballot and one atomicMin per edge and wave.
//
// Early exit: before a tile stages anything, wave 0 reads first_hit of its lanes' edges; a tile none of whose samples lies
// before its edge's current first hit skips the FK and the sweep.  first_hit only decreases (unsigned atomicMin, -1 = "free"
// is the largest unsigned value), so a skip decided on an older value is still right.  A skipped tile of a split launch still
// takes part in the tile's hand-over, with zero sums.
// Answer step (wave 0, or the last block of a split tile: where the scores are final): a sample collides iff
// score_c - margin_c > 0 for some class; the first colliding lane of each edge segment of the wave lowers first_hit[e].
#pragma once
#include "dcx_internal.h"
#include "motion_tile.h"

namespace dcx {

struct MotionArgs : MotionEdgeArgs {
    unsigned int* first_hit;  // [E] int32 answers, compared unsigned (-1 = free is the largest value)
    const float* margin;      // [c_out] or null (0)
    int32_t early_exit;       // 0: every tile sweeps (developer knob motion_early_exit; the bound the benchmark compares against)
};

// one entry point per compiled width (motion_inst.hip)
typedef hipError_t (*motion_fn)(int kf, int cc, int nw, size_t lds, int64_t n_blocks, const MotionArgs& a, hipStream_t stream);
#define DCX_DECLARE_MOTION(D) hipError_t launch_motion_D##D(int, int, int, size_t, int64_t, const MotionArgs&, hipStream_t);
DCX_FOREACH_WIDTH(DCX_DECLARE_MOTION)
#undef DCX_DECLARE_MOTION

#ifdef __HIPCC__
template <int D, int KF, int CC, int MAXT, int XF = 0 /* motion_tile.h motion_sweep */>
__global__ __launch_bounds__(MAXT, sweep_min_waves(D, CC, KF)) void motion_kernel(const MotionArgs m, int32_t mo_off) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const ScoreArgs& a = m.sc;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nw = blockDim.x >> 6;
    const LdsPlan lp = lds_plan(a.dof, a.d_fk, a.frame_floats, nw > 1 ? a.red_slots : 0, CC, true);
    const MotionTile t = motion_tile_view(smem, lp, mo_off);
    const int64_t total = m.offs[m.E];
    const int64_t tile = blockIdx.x;
    if (tile * 64 >= total) return;   // past the end of the work list: before any staging
    const FkWalk fw = fk_stage_sel(a.fkk, a.fk, a.fk_dwords, a.dh, smem + lp.fk, threadIdx.x, blockDim.x);
    const int64_t base = tile * 64;
    const int nb = (int)((total - base) < 64 ? (total - base) : 64);
    if (wave == 0) {
        const int lane = threadIdx.x & 63;
        const MotionLane l = motion_tile_lookup(m.offs, m.E, base, nb, t);
        // early exit: is any sample of this tile still before its edge's first hit?
        const unsigned int fh = m.early_exit ? __hip_atomic_load(m.first_hit + l.e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0xffffffffu;
        const bool any_live = __builtin_amdgcn_ballot_w64(lane < nb && (unsigned int)l.k < fh) != 0;
        if (lane == 0) *t.sFlag = any_live ? 1 : 0;
    }
    __syncthreads();
    const bool live = *t.sFlag != 0;
    if (!live && a.partial == nullptr) return;   // (block-uniform; a split launch's blocks still take part in the tile's hand-over)
    float sc[CC];
#pragma unroll
    for (int c = 0; c < CC; ++c) sc[c] = 0.0f;
    if (live) {
        float x[D], gx[D], up[CC];
#pragma unroll
        for (int c = 0; c < CC; ++c) up[c] = 0.0f;
        motion_tile_features<D, XF>(m, t, fw, false, wave, nw, x);
        motion_sweep<D, KF, CC, MODE_SCORE, XF>(a, x, up, wave, nw, sc, gx);
    }
    const auto& b = reload_kernargs<MotionArgs>();
    const int lane = fresh_lane();
    if (!motion_fold_block<CC, 0, false>(t.sRed, b.sc.red_slots, wave, lane, nw, sc, nullptr)) return;
    if (!motion_split_handover<CC, 0>(b.sc, tile, lane, sc, nullptr)) return;
    bool hit = false;
#pragma unroll
    for (int c = 0; c < CC; ++c)
        if (c < b.sc.c_out) hit = hit || (sc[c] - (b.margin ? b.margin[c] : 0.0f) > 0.0f);
    hit = hit && lane < nb;
    const int k = t.sK[lane];
    const uint64_t hits = __builtin_amdgcn_ballot_w64(hit);
    uint64_t starts;
    const int seg0 = motion_segment_start(k, lane, starts);
    const uint64_t before = hits & ((1ull << lane) - 1ull) & ~((1ull << seg0) - 1ull);
    if (hit && before == 0) atomicMin(b.first_hit + t.sEdge[lane], (unsigned int)k);
}
#endif  // __HIPCC__

}  // namespace dcx
