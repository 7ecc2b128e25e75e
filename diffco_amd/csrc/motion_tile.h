// motion_tile.h — what the motion calls share on the device (dcx_check_motions, dcx_motion_cost, dcx_motion_worst,
// dcx_motion_band): the work list, the tile's LDS, its prologue, the sweep, the block's fold and the split launch's hand-over.
// The four kernels differ in their early returns and in the answer step alone, so for the same (model, E, max_samples) they
// score a sample to the same bits: that contract is carried by the functions below, once.
//
// Work list: the samples of all edges in flat order, sample i of edge e at offs[e] + i (offs: the exclusive scan of the sample
// counts, made on the device by motion_prep.hip).  A 64-configuration tile takes 64 consecutive flat samples, so short edges
// share a tile and long ones span several.  The tile finds its first edge by a 64-ary search in offs (three dependent loads at
// E = 65536) and the edge of every lane by a binary search in LDS over the next 64 edge ends.
// Grid: one tile per block, sized from the upper bound E * max_samples / 64 (the host cannot read the total sample count back:
// the calls are capturable); the kernel reads offs[E] and blocks past the end of the work list leave at once.  (A persistent grid
// striding over the tiles was the first form: the loop around the sweep kept its state live across it, and at the sweep's
// 64-VGPR budget the compiler spilled 12 VGPRs to scratch and parked 133 SGPRs - 1.9x the time of dcx_score on the same points.)
// A kernel is then: early returns, motion_tile_lookup, motion_tile_features (interpolation, FK, the features in registers),
// motion_sweep (score_kernel.h sweep_rows: the rows, slices, wave-group shares and split launches of dcx_score),
// motion_fold_block (the block's partial sums meet on wave 0), motion_split_handover (the last block of a split tile to arrive
// adds the tile's rows), and its own answer step on wave 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "score_kernel.h"
#ifdef __HIPCC__
#include "wrap_device.h"
#endif

namespace dcx {

// The head of every motion kernel's arguments; each kernel's struct derives from it and adds only its own fields.
struct MotionEdgeArgs {
    ScoreArgs sc;             // the sweep's arguments (first: reload_kernargs reads them at offset 0).  sc.q / score / grad unused;
                              // sc.partial / sc.tile_done: the split launch's partial rows and arrival counters (caller's work)
    const float* qa;          // [E][dof]
    const float* qb;          // [E][dof]
    const int64_t* offs;      // [E + 1] exclusive scan of the sample counts (motion_prep.hip)
    const float* frac;        // [E] max_step rule: the step as a fraction of the edge, (1 / L) * max_step (dense_path's arithmetic)
    int64_t E;
    int32_t res;              // > 0: the res rule (qa + (k / res)(qb - qa), k < res); 0: the max_step rule
    uint64_t wrap_mask;       // bit j: coordinate j is an angle, the edge runs along its shortest arc (0: straight, every bit as before)
};

// LDS a motion kernel needs behind the sweep's plan and the FK program: per lane its edge, sample index, count, and the
// 64 edge ends the lookup searches (int64), plus the block's flag
constexpr int kMotionLdsFloats = 64 * 2 + 64 * 3 + 4;

struct MotionPrepArgs {
    const float* qa;
    const float* qb;
    int64_t E;
    int32_t dof, res, max_samples;
    float max_step;
    int64_t* offs;
    float* frac;
    int32_t* first_hit;
    int32_t* n_samples;       // or null
    unsigned int* counters;   // split-launch arrival counters zeroed here (n_counters * kCounterStride words), or null
    int32_t n_counters;
    int32_t open_end;         // max_step rule: 1 drops the target qb from the samples (dcx_motion_cost; the other calls: 0)
    uint64_t wrap_mask;       // the edge's length is taken from the wrapped delta of the masked coordinates
};
hipError_t launch_motion_prep(const MotionPrepArgs& p, hipStream_t stream);

#ifdef __HIPCC__
// Coordinate j of sample k of the edge qa -> qb (one joint's values): the sQ prologue of the motion kernels.
//   res > 0:  qa + d (k / res);   res == 0:  qa + k (d frac), the target (`target`: the closed rule's last sample) qb itself.
// Unmasked coordinates: d = qb - qa, the expression as it always stood (the compiler contracts its last product and sum).
// Masked coordinates (include/dcx.h): d = wrap2pi(qb - qa), product and sum rounded one by one, then wrap2pi - a point one
// ulp to the other side of the seam is 2 pi away in a raw feature, so this path leaves the compiler no choice.
__device__ __forceinline__ float motion_coord(float qa, float qb, int k, int res, bool target, const float* frac_e, bool masked) {
    if (masked) {
#pragma clang fp contract(off)
        const float d = wrap2pi_f32(__fsub_rn(qb, qa));
        if (res > 0) {
            const float p = d * __fdiv_rn((float)k, (float)res);
            return wrap2pi_f32(qa + p);
        }
        if (target) return qb;
        const float s = d * *frac_e;
        const float p = (float)k * s;
        return wrap2pi_f32(qa + p);
    }
    const float d = __fsub_rn(qb, qa);
    if (res > 0) return __fadd_rn(qa, __fmul_rn(d, __fdiv_rn((float)k, (float)res)));
    if (target) return qb;   // the target closes the max_step rule's point set
    return __fadd_rn(qa, __fmul_rn((float)k, __fmul_rn(d, *frac_e)));
}

// The tile's LDS: the sweep's plan (lds_plan(dof, d_fk, frame_floats, red_slots, ACC, true)), the FK program rounded to 4 floats,
// then kMotionLdsFloats at mo_off (the launcher passes it: motion_inst_common.h).
struct MotionTile {
    float *sQ, *sX, *sF, *sRed;
    int64_t* sEnd;            // [64] the ends of the 64 edges from the tile's first
    int32_t *sEdge, *sK, *sN; // [64] per lane: its edge, its sample's index in the edge, the edge's sample count
    int32_t* sFlag;           // the block's flag (dcx_check_motions' early exit)
};
__device__ __forceinline__ MotionTile motion_tile_view(float* smem, const LdsPlan& lp, int32_t mo_off) {
    MotionTile t;
    t.sQ = smem + lp.q;
    t.sX = smem + lp.x;
    t.sF = smem + lp.f;
    t.sRed = smem + lp.red;
    t.sEnd = reinterpret_cast<int64_t*>(smem + mo_off);
    t.sEdge = reinterpret_cast<int32_t*>(smem + mo_off + 128);
    t.sK = t.sEdge + 64;
    t.sN = t.sEdge + 128;
    t.sFlag = t.sEdge + 192;
    return t;
}

// Wave 0: the edge, sample index and sample count of each lane of the tile starting at flat sample `base` (nb samples), into
// sEdge / sK / sN; returns the lane's edge and sample index.  The first edge is the largest e with offs[e] <= base (offs[0] = 0 <= base <
// offs[E]): a 64-ary search; then a binary search in LDS over the next 64 edge ends, a global one when more than 64 edges end
// inside the tile (edges over max_samples have no samples).
struct MotionLane {
    int64_t e;
    int k;
};
__device__ __forceinline__ MotionLane motion_tile_lookup(const int64_t* offs, int64_t E, int64_t base, int nb, const MotionTile& t) {
    const int lane = threadIdx.x & 63;
    int64_t lo = 0, hi = E;
    while (hi - lo > 1) {
        const int64_t step = (hi - lo + 63) / 64;
        const int64_t idx = lo + (int64_t)lane * step;
        const bool le = idx < hi && offs[idx] <= base;
        const int p = __popcll(__builtin_amdgcn_ballot_w64(le));   // >= 1: lane 0 reads offs[lo]
        const int64_t nlo = lo + (int64_t)(p - 1) * step;
        hi = (lo + (int64_t)p * step < hi) ? lo + (int64_t)p * step : hi;
        lo = nlo;
    }
    const int64_t e0 = lo;
    t.sEnd[lane] = (e0 + 1 + lane <= E) ? offs[e0 + 1 + lane] : INT64_MAX;   // end of edge e0 + lane
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    const int64_t s = base + (lane < nb ? lane : nb - 1);
    int64_t e, start;
    if (t.sEnd[63] > s) {   // the usual case: this lane's edge is among the next 64 (first j with end > s)
        int j = 0;
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1)
            if (t.sEnd[j + h - 1] <= s) j += h;
        e = e0 + j;
        start = j ? t.sEnd[j - 1] : offs[e0];
    } else {
        int64_t l2 = e0 + 64, h2 = E;   // offs[l2] <= s < offs[h2]
        while (h2 - l2 > 1) {
            const int64_t md = (l2 + h2) / 2;
            if (offs[md] <= s) l2 = md; else h2 = md;
        }
        e = l2;
        start = offs[l2];
    }
    t.sEdge[lane] = (int32_t)e;
    const int k = (int)(s - start);
    t.sK[lane] = k;
    t.sN[lane] = (int32_t)(offs[e + 1] - start);
    return MotionLane{e, k};
}

// The tile's prologue, all waves: the rows of sQ interpolated from their edges (dense_path / line_predict arithmetic; with
// `open_end` the max_step rule has no target sample), trig, the FK chain in either of score_kernel's forms, and the lane's
// features in x[], centred for the expanded form (XF != 0).  Ends behind the barrier after which X is dead.
template <int D, int XF>
__device__ __forceinline__ void motion_tile_features(const MotionEdgeArgs& m, const MotionTile& t, const FkWalk& fw, bool open_end,
                                                     int wave, int nw, float (&x)[D]) {
    const ScoreArgs& a = m.sc;
    const int dof = a.dof;
    for (int i = threadIdx.x; i < 64 * dof; i += blockDim.x) {
        const int l = i / dof, j = i - l * dof;
        const int64_t e = t.sEdge[l];
        const int k = t.sK[l];
        const float qa = m.qa[e * dof + j], qb = m.qb[e * dof + j];
        t.sQ[i] = motion_coord(qa, qb, k, m.res, !open_end && k == t.sN[l] - 1, m.frac + e, (m.wrap_mask >> j) & 1ull);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    fk_trig_sel(fw, a.dh, t.sQ + lane * dof, t.sF + lane, wave, nw);
    __syncthreads();
    if (a.fkk == 2 && a.jt_rows) dh2_chain_rows_sel(fw.dh, a.dh, t.sX + lane, t.sF + lane, wave);   // (score_kernel's two forms)
    else if (wave == 0) fk_chain_sel(fw, a.dh, t.sQ + lane * dof, t.sX + lane, t.sF + lane);
    __syncthreads();
    // (the lane's column as ONE base: written t.sX[k * 64 + lane] in here, the guarded loads of the D = 96, four- and eight-class
    // kernels each kept an address of their own - 22 VGPRs, one occupancy step)
    const float* xl = t.sX + lane;
    if (a.d_fk == D) {
#pragma unroll
        for (int k = 0; k < D; ++k) x[k] = xl[k * 64];
    } else {
#pragma unroll
        for (int k = 0; k < D; ++k) x[k] = (k < a.d_fk) ? xl[k * 64] : 0.0f;
    }
    if constexpr (XF != 0) {   // the expanded form's centred features (score_kernel.h)
        cfloat_ptr cen = (cfloat_ptr)(uintptr_t)a.centre;
#pragma unroll
        for (int k = 0; k < D; ++k) x[k] -= cen[k];
    }
    if (nw > 1) __syncthreads();   // X is dead: the partial sums reuse its LDS
}

// This wave's slice of the block's rows (blockIdx.y's super-chunk of a split launch), swept: score_kernel.h's sweep.
// XF: 1 the expanded form, 2 its spare-slot form (sweep_rows SP).
template <int D, int KF, int CC, int MODE, int XF>
__device__ __forceinline__ void motion_sweep(const ScoreArgs& a, const float (&x)[D], const float (&up)[CC], int wave, int nw,
                                             float (&sc)[CC], float (&gx)[D]) {
    const int ybase = blockIdx.y * a.s_super;
    const int yend = (ybase + a.s_super < a.S) ? (ybase + a.s_super) : a.S;
    int j0, j1;
    wave_slice(wave, nw, a.s_chunk, a.s_skew, ybase, yend, j0, j1);
    sweep_rows<D, KF, CC, MODE, XF != 0, 0, false, XF == 2>(a, x, up, j0, j1, sc, gx);
}

// The block's partial sums (CC class scores, then NG gradient entries: 0 or D) meet on wave 0; returns whether this wave is
// wave 0.  red_slots == nw: every wave has a row of its own in sRed; otherwise one row, the waves hand over in turn.  With a row
// per wave the sums are taken in one of TWO orders, and the bits depend on which: TREE (the cost passes) folds as
// score_kernel's fold_partial_rows does, every wave taking part; otherwise (the score-only kernels) wave 0 adds the rows
// w = 1 ... nw - 1 one after the other.
template <int CC, int NG, bool TREE>
__device__ __forceinline__ bool motion_fold_block(float* sRed, int red_slots, int wave, int lane, int nw, float (&sc)[CC], float* gx) {
    constexpr int ACC = CC + NG;
    if (nw > 1 && red_slots == nw) {
        float* mine = sRed + (size_t)wave * ACC * 64 + lane;
#pragma unroll
        for (int c = 0; c < CC; ++c) mine[c * 64] = sc[c];
#pragma unroll
        for (int k = 0; k < NG; ++k) mine[(CC + k) * 64] = gx[k];
        __syncthreads();
        if constexpr (TREE) {
            fold_partial_rows<ACC>(sRed, wave, lane, nw);
            __syncthreads();
            if (wave != 0) return false;
#pragma unroll
            for (int c = 0; c < CC; ++c) sc[c] = sRed[c * 64 + lane];
#pragma unroll
            for (int k = 0; k < NG; ++k) gx[k] = sRed[(CC + k) * 64 + lane];
        } else if (wave == 0) {
            for (int w = 1; w < nw; ++w) {
#pragma unroll
                for (int c = 0; c < CC; ++c) sc[c] += sRed[((size_t)w * ACC + c) * 64 + lane];
#pragma unroll
                for (int k = 0; k < NG; ++k) gx[k] += sRed[((size_t)w * ACC + CC + k) * 64 + lane];
            }
        }
    } else if (nw > 1) {
        for (int w = 1; w < nw; ++w) {
            if (wave == w) {
#pragma unroll
                for (int c = 0; c < CC; ++c) sRed[c * 64 + lane] = sc[c];
#pragma unroll
                for (int k = 0; k < NG; ++k) sRed[(CC + k) * 64 + lane] = gx[k];
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int c = 0; c < CC; ++c) sc[c] += sRed[c * 64 + lane];
#pragma unroll
                for (int k = 0; k < NG; ++k) gx[k] += sRed[(CC + k) * 64 + lane];
            }
            __syncthreads();
        }
    }
    return wave == 0;
}

// Wave 0 of a split launch (b.partial set; an unsplit one returns true at once): the in-launch hand-over of score_kernel's
// one-wave form.  The block publishes its sums write-through, drains, counts; the last block of the tile to arrive resets the
// counter for the next launch on this work buffer, adds the ys rows in the order y = 0, 1, ... and answers for the tile (true).
// b: the sweep's arguments read afresh (reload_kernargs: they live in the constant address space).
template <int CC, int NG>
__device__ __forceinline__ bool motion_split_handover(const __attribute__((address_space(4))) ScoreArgs& b, int64_t tile, int lane,
                                                      float (&sc)[CC], float* gx) {
    constexpr int ACC = CC + NG;
    if (b.partial == nullptr) return true;
    float* out = b.partial + (tile * b.ys + blockIdx.y) * ACC * 64 + lane;
#pragma unroll
    for (int c = 0; c < CC; ++c) __hip_atomic_store(out + c * 64, sc[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int k = 0; k < NG; ++k) __hip_atomic_store(out + (CC + k) * 64, gx[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned int arrived = 0;
    if (lane == 0) arrived = __hip_atomic_fetch_add(b.tile_done + tile * kCounterStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    arrived = __builtin_amdgcn_readfirstlane(arrived);
    if (arrived != (unsigned int)b.ys - 1u) return false;
    if (lane == 0) b.tile_done[tile * kCounterStride] = 0u;
    asm volatile("" ::: "memory");
    const float* part = b.partial + tile * b.ys * ACC * 64 + lane;
#pragma unroll
    for (int c = 0; c < CC; ++c) sc[c] = 0.0f;
#pragma unroll
    for (int k = 0; k < NG; ++k) gx[k] = 0.0f;
    for (int y = 0; y < b.ys; ++y) {
#pragma unroll
        for (int c = 0; c < CC; ++c) sc[c] += __hip_atomic_load(part + ((size_t)y * ACC + c) * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int k = 0; k < NG; ++k)
            gx[k] += __hip_atomic_load(part + ((size_t)y * ACC + CC + k) * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return true;
}

// The lanes of an edge are consecutive in the wave, its sample index k rising with the lane: the first lane of this lane's
// edge segment, and in `starts` the mask of the lanes that begin a segment.
__device__ __forceinline__ int motion_segment_start(int k, int lane, uint64_t& starts) {
    starts = __builtin_amdgcn_ballot_w64(k == 0 || lane == 0);
    const uint64_t upto = (lane == 63) ? ~0ull : ((1ull << (lane + 1)) - 1ull);
    return 63 - __clzll(starts & upto);
}
#endif  // __HIPCC__

}  // namespace dcx
