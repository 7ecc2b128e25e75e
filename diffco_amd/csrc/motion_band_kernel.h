// motion_band_kernel.h — hybrid motion checks (dcx_motion_band): for E straight joint-space motions qa[e] -> qb[e] and two
// thresholds per class, lo and hi, every sample x_k gets a code
//     1 (sure hit)    some c has score_c(x_k) - hi_c > 0        (dcx_check_motions' comparison with margin = hi)
//     0 (sure clear)  no hit, and every c has score_c(x_k) - lo_c <= 0
//     2 (uncertain)   neither: inside the band, or a NaN class score
// and every edge a verdict, its first sure hit and - for an edge without a sure hit - the ordered list of its uncertain
// samples with their configurations, ready for a ground-truth checker.
//
// The work list, the tile lookup (motion_cost_kernel.h motion_tile_lookup), the interpolation (motion_kernel.h motion_coord)
// and the sweep are dcx_check_motions': the same rows, slices, wave-group shares and split launches for the same
// (model, E, max_samples), so a sample's class scores are the bits the check compares.  The kernel is motion_worst_kernel up
// to the point where the scores are final (no early exit: every tile sweeps); only the answer step differs.
//
// Answer step (wave 0, or the last block of a split tile: where the scores are final).  Lane < nb writes its code as ONE byte
// to codes[tile * 64 + lane] in the caller's workspace: 64 consecutive bytes per tile, flat sample s at codes[s].  No shuffle,
// no atomic, every byte below offs[E] written exactly once per call: the same bits every call.
//
// motion_band_finish.hip reads the codes per edge in sample order, scans the per-edge counts and scatters the list.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "motion_cost_kernel.h"

namespace dcx {

struct MotionBandArgs {
    ScoreArgs sc;             // the sweep's arguments (first: reload_kernargs reads them at offset 0), as MotionArgs::sc
    const float* qa;          // [E][dof]
    const float* qb;          // [E][dof]
    const int64_t* offs;      // [E + 1] exclusive scan of the sample counts (motion_prep.hip)
    const float* frac;        // [E] max_step rule: (1 / L) * max_step
    uint8_t* codes;           // [offs[E]] one code per flat sample (room for E * max_samples rounded up to whole tiles)
    const float* lo;          // [c_out] or null (0)
    const float* hi;          // [c_out] or null (0)
    int64_t E;
    int32_t res;              // > 0: the res rule; 0: the closed max_step rule
    uint64_t wrap_mask;       // as MotionArgs::wrap_mask
};

// one entry point per compiled width (motion_band_inst.hip)
typedef hipError_t (*motion_band_fn)(int kf, int cc, int nw, size_t lds, int64_t n_blocks, const MotionBandArgs& a, hipStream_t stream);
#define DCX_DECLARE_MOTION_BAND(D) \
    hipError_t launch_motion_band_D##D(int, int, int, size_t, int64_t, const MotionBandArgs&, hipStream_t);
DCX_DECLARE_MOTION_BAND(2)  DCX_DECLARE_MOTION_BAND(4)  DCX_DECLARE_MOTION_BAND(6)  DCX_DECLARE_MOTION_BAND(8)
DCX_DECLARE_MOTION_BAND(12) DCX_DECLARE_MOTION_BAND(16) DCX_DECLARE_MOTION_BAND(18) DCX_DECLARE_MOTION_BAND(21)
DCX_DECLARE_MOTION_BAND(24) DCX_DECLARE_MOTION_BAND(27) DCX_DECLARE_MOTION_BAND(30) DCX_DECLARE_MOTION_BAND(32)
DCX_DECLARE_MOTION_BAND(36) DCX_DECLARE_MOTION_BAND(42) DCX_DECLARE_MOTION_BAND(48) DCX_DECLARE_MOTION_BAND(54)
DCX_DECLARE_MOTION_BAND(60) DCX_DECLARE_MOTION_BAND(64) DCX_DECLARE_MOTION_BAND(72) DCX_DECLARE_MOTION_BAND(84)
DCX_DECLARE_MOTION_BAND(96)
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
// one configuration per lane: motion_worst_kernel up to the final scores, then one code byte per sample.
// LDS: lds_plan(...).total + prog_floats rounded to 4, then kMotionLdsFloats (mo_off), as motion_kernel.
template <int D, int KF, int CC, int MAXT, int XF = 0 /* 1: the expanded form, 2: its spare-slot form (score_kernel.h sweep_rows SP) */>
__global__ __launch_bounds__(MAXT, sweep_min_waves(D, CC, KF)) void motion_band_kernel(const MotionBandArgs m, int32_t mo_off) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const ScoreArgs& a = m.sc;
    constexpr int ACC = CC;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nw = blockDim.x >> 6;
    const int dof = a.dof;
    const LdsPlan lp = lds_plan(dof, a.d_fk, a.frame_floats, nw > 1 ? a.red_slots : 0, ACC, true);
    float* sQ = smem + lp.q;
    float* sX = smem + lp.x;
    float* sF = smem + lp.f;
    float* sRed = smem + lp.red;
    int64_t* sEnd = reinterpret_cast<int64_t*>(smem + mo_off);   // [64]
    int32_t* sEdge = reinterpret_cast<int32_t*>(smem + mo_off + 128);
    int32_t* sK = sEdge + 64;
    int32_t* sN = sEdge + 128;

    const int64_t E = m.E;
    const int64_t total = m.offs[E];
    const int64_t tile = blockIdx.x;
    if (tile * 64 >= total) return;   // past the end of the work list (the grid is sized from E * max_samples): before any staging
    const FkWalk fw = fk_stage_sel(a.fkk, a.fk, a.fk_dwords, a.dh, smem + lp.fk, threadIdx.x, blockDim.x);
    const bool split = a.partial != nullptr;
    const int64_t base = tile * 64;
    const int nb = (int)((total - base) < 64 ? (total - base) : 64);
    if (wave == 0) motion_tile_lookup(m.offs, E, base, nb, sEnd, sEdge, sK, sN);
    __syncthreads();
    float sc[CC];
#pragma unroll
    for (int c = 0; c < CC; ++c) sc[c] = 0.0f;
    {
        // ---- the rows of sQ: this tile's 64 samples, interpolated from their edges (motion_kernel's prologue) ----
        for (int i = threadIdx.x; i < 64 * dof; i += blockDim.x) {
            const int l = i / dof, j = i - l * dof;
            const int64_t e = sEdge[l];
            const int k = sK[l];
            const float qa = m.qa[e * dof + j], qb = m.qb[e * dof + j];
            sQ[i] = motion_coord(qa, qb, k, m.res, k == sN[l] - 1, m.frac + e, (m.wrap_mask >> j) & 1ull);
        }
        __syncthreads();
        const int lane = threadIdx.x & 63;
        fk_trig_sel(fw, a.dh, sQ + lane * dof, sF + lane, wave, nw);
        __syncthreads();
        if (a.fkk == 2 && a.jt_rows) dh2_chain_rows_sel(fw.dh, a.dh, sX + lane, sF + lane, wave);   // (score_kernel's two forms)
        else if (wave == 0) fk_chain_sel(fw, a.dh, sQ + lane * dof, sX + lane, sF + lane);
        __syncthreads();
        float x[D];
        if (a.d_fk == D) {
#pragma unroll
            for (int k = 0; k < D; ++k) x[k] = sX[k * 64 + lane];
        } else {
#pragma unroll
            for (int k = 0; k < D; ++k) x[k] = (k < a.d_fk) ? sX[k * 64 + lane] : 0.0f;
        }
        if constexpr (XF != 0) {   // the expanded form's centred features (score_kernel.h)
            cfloat_ptr cen = (cfloat_ptr)(uintptr_t)a.centre;
#pragma unroll
            for (int k = 0; k < D; ++k) x[k] -= cen[k];
        }
        if (nw > 1) __syncthreads();   // X is dead: the partial sums reuse its LDS
        const int ybase = blockIdx.y * a.s_super;
        const int yend = (ybase + a.s_super < a.S) ? (ybase + a.s_super) : a.S;
        int j0, j1;
        wave_slice(wave, nw, a.s_chunk, a.s_skew, ybase, yend, j0, j1);
        float up[CC];
        float gx[D];
#pragma unroll
        for (int c = 0; c < CC; ++c) up[c] = 0.0f;
        sweep_rows<D, KF, CC, MODE_SCORE, XF != 0, 0, false, XF == 2>(a, x, up, j0, j1, sc, gx);
    }
    // ---- epilogue: the block's partial sums meet on wave 0 in motion_kernel's order (the same bits as the check's scores) ----
    const auto& b = reload_kernargs<MotionBandArgs>();
    const int lane = fresh_lane();
    if (nw > 1 && b.sc.red_slots == nw) {
        float* mine = sRed + (size_t)wave * ACC * 64 + lane;
#pragma unroll
        for (int c = 0; c < CC; ++c) mine[c * 64] = sc[c];
        __syncthreads();
        if (wave == 0) {
            for (int w = 1; w < nw; ++w)
#pragma unroll
                for (int c = 0; c < CC; ++c) sc[c] += sRed[((size_t)w * ACC + c) * 64 + lane];
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
        // motion_kernel's in-launch hand-over: publish write-through, drain, count; the last block of the tile to arrive adds
        // the ys rows in the order y = 0, 1, ... and answers for the tile
        float* out = b.sc.partial + (tile * b.sc.ys + blockIdx.y) * ACC * 64 + lane;
#pragma unroll
        for (int c = 0; c < CC; ++c) __hip_atomic_store(out + c * 64, sc[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned int arrived = 0;
        if (lane == 0) arrived = __hip_atomic_fetch_add(b.sc.tile_done + tile * kCounterStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        arrived = __builtin_amdgcn_readfirstlane(arrived);
        if (arrived != (unsigned int)b.sc.ys - 1u) return;
        if (lane == 0) b.sc.tile_done[tile * kCounterStride] = 0u;   // ready for the next launch on this work buffer
        asm volatile("" ::: "memory");
        const float* part = b.sc.partial + tile * b.sc.ys * ACC * 64 + lane;
#pragma unroll
        for (int c = 0; c < CC; ++c) sc[c] = 0.0f;
        for (int y = 0; y < b.sc.ys; ++y)
#pragma unroll
            for (int c = 0; c < CC; ++c) sc[c] += __hip_atomic_load(part + ((size_t)y * ACC + c) * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
