// motion_band_kernel.h — hybrid motion checks (dcx_motion_band): for E straight joint-space motions qa[e] -> qb[e] and two
// thresholds per class, lo and hi, every sample x_k gets a code
//     1 (sure hit)    some c has score_c(x_k) - hi_c > 0        (dcx_check_motions' comparison with margin = hi)
//     0 (sure clear)  no hit, and every c has score_c(x_k) - lo_c <= 0
//     2 (uncertain)   neither: inside the band, or a NaN class score
// and every edge a verdict, its first sure hit and - for an edge without a sure hit - the ordered list of its uncertain
// samples with their configurations, ready for a ground-truth checker.
//
// The tiles are scored as dcx_check_motions scores them (motion_tile.h: the same bits for the same (model, E, max_samples));
// no early exit, every tile sweeps.
//
// Answer step (wave 0, or the last block of a split tile: where the scores are final).  Lane < nb writes its code as ONE byte
// to codes[tile * 64 + lane] in the caller's workspace: 64 consecutive bytes per tile, flat sample s at codes[s].  No shuffle,
// no atomic, every byte below offs[E] written exactly once per call: the same bits every call.
//
// motion_band_finish.hip reads the codes per edge in sample order, scans the per-edge counts and scatters the list.
#pragma once
#include "dcx_internal.h"
#include "motion_tile.h"

namespace dcx {

struct MotionBandArgs : MotionEdgeArgs {
    uint8_t* codes;           // [offs[E]] one code per flat sample (room for E * max_samples rounded up to whole tiles)
    const float* lo;          // [c_out] or null (0)
    const float* hi;          // [c_out] or null (0)
};

// one entry point per compiled width (motion_band_inst.hip)
typedef hipError_t (*motion_band_fn)(int kf, int cc, int nw, size_t lds, int64_t n_blocks, const MotionBandArgs& a, hipStream_t stream);
#define DCX_DECLARE_MOTION_BAND(D) \
    hipError_t launch_motion_band_D##D(int, int, int, size_t, int64_t, const MotionBandArgs&, hipStream_t);
DCX_FOREACH_WIDTH(DCX_DECLARE_MOTION_BAND)
#undef DCX_DECLARE_MOTION_BAND

// the finish (motion_band_finish.hip): the codes folded per edge, the counts scanned, the list scattered
struct MotionBandFinishArgs {
    const float* qa;
    const float* qb;
    const int64_t* offs;
    const float* frac;
    const int32_t* status;    // motion_prep's first_hit: -1, or -2 for an edge over max_samples
    const uint8_t* codes;
    int32_t* verdict;         // [E]
    int32_t* first_hit;       // [E] or null
    int32_t* n_uncertain;     // [E] or null
    int64_t* uoffs;           // [E + 1] workspace: the edges' uncertain counts (0 unless the verdict is 2), scanned in place
    int64_t* unc_total;       // [1]
    int32_t* unc_edge;        // [unc_cap]
    int32_t* unc_sample;      // [unc_cap]
    float* unc_q;             // [unc_cap][dof] or null
    int64_t unc_cap;
    int64_t E;
    int32_t dof, res;
    uint64_t wrap_mask;
};
hipError_t launch_motion_band_finish(const MotionBandFinishArgs& f, hipStream_t stream);

#ifdef __HIPCC__
template <int D, int KF, int CC, int MAXT, int XF = 0 /* motion_tile.h motion_sweep */>
__global__ __launch_bounds__(MAXT, sweep_min_waves(D, CC, KF)) void motion_band_kernel(const MotionBandArgs m, int32_t mo_off) {
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
    const bool split = a.partial != nullptr;   // (read before the sweep, as the fold and hand-over below were written)
    const int64_t base = tile * 64;
    const int nb = (int)((total - base) < 64 ? (total - base) : 64);
    if (wave == 0) motion_tile_lookup(m.offs, m.E, base, nb, t);
    __syncthreads();
    float sc[CC], up[CC], x[D], gx[D];
#pragma unroll
    for (int c = 0; c < CC; ++c) sc[c] = up[c] = 0.0f;
    motion_tile_features<D, XF>(m, t, fw, false, wave, nw, x);
    motion_sweep<D, KF, CC, MODE_SCORE, XF>(a, x, up, wave, nw, sc, gx);
    // The fold and the hand-over stand here as text, not as motion_fold_block<CC, 0, false> / motion_split_handover<CC, 0>
    // (motion_tile.h), whose bodies they repeat word for word, as in motion_worst_kernel: with the two as inlined calls the compiler schedules this
    // kernel's sweep in another order, 1.2 - 1.7 % slower at E = 65536 (profiles/r18_motion_refactor_timing.txt).
    const auto& b = reload_kernargs<MotionBandArgs>();
    const int lane = fresh_lane();
    float* sRed = t.sRed;
    if (nw > 1 && b.sc.red_slots == nw) {
        float* mine = sRed + (size_t)wave * CC * 64 + lane;
#pragma unroll
        for (int c = 0; c < CC; ++c) mine[c * 64] = sc[c];
        __syncthreads();
        if (wave == 0) {
            for (int w = 1; w < nw; ++w)
#pragma unroll
                for (int c = 0; c < CC; ++c) sc[c] += sRed[((size_t)w * CC + c) * 64 + lane];
        }
    } else if (nw > 1) {
        for (int w = 1; w < nw; ++w) {
            if (wave == w) {
#pragma unroll
                for (int c = 0; c < CC; ++c) sRed[c * 64 + lane] = sc[c];
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int c = 0; c < CC; ++c) sc[c] += sRed[c * 64 + lane];
            }
            __syncthreads();
        }
    }
    if (wave != 0) return;
    if (split) {
        float* out = b.sc.partial + (tile * b.sc.ys + blockIdx.y) * CC * 64 + lane;
#pragma unroll
        for (int c = 0; c < CC; ++c) __hip_atomic_store(out + c * 64, sc[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned int arrived = 0;
        if (lane == 0) arrived = __hip_atomic_fetch_add(b.sc.tile_done + tile * kCounterStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        arrived = __builtin_amdgcn_readfirstlane(arrived);
        if (arrived != (unsigned int)b.sc.ys - 1u) return;
        if (lane == 0) b.sc.tile_done[tile * kCounterStride] = 0u;   // ready for the next launch on this work buffer
        asm volatile("" ::: "memory");
        const float* part = b.sc.partial + tile * b.sc.ys * CC * 64 + lane;
#pragma unroll
        for (int c = 0; c < CC; ++c) sc[c] = 0.0f;
        for (int y = 0; y < b.sc.ys; ++y)
#pragma unroll
            for (int c = 0; c < CC; ++c) sc[c] += __hip_atomic_load(part + ((size_t)y * CC + c) * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // ---- the answer: the sample's code from its class scores.  hit: motion_kernel's comparison against hi.  clear: every
    // class at or below lo - written as "not (s - lo <= 0)" so that a NaN score is neither ----
    bool hit = false, clear = true;
#pragma unroll
    for (int c = 0; c < CC; ++c) {
        if (c < b.sc.c_out) {
            const float dh = sc[c] - (b.hi ? b.hi[c] : 0.0f);
            const float dl = sc[c] - (b.lo ? b.lo[c] : 0.0f);
            hit = hit || dh > 0.0f;
            clear = clear && dl <= 0.0f;
        }
    }
    // (the lanes behind the work list's end repeat its last sample and write nothing; tile * 64 + lane < offs[E] for the rest)
    if (lane < nb) b.codes[base + lane] = hit ? (uint8_t)1 : (clear ? (uint8_t)0 : (uint8_t)2);
}
#endif  // __HIPCC__

}  // namespace dcx
