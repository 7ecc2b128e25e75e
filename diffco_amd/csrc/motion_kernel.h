// motion_kernel.h — batched motion checks (dcx_check_motions): is the straight joint-space motion qa -> qb free, and if not,
// which of its samples is the first to collide?  Two small prep launches (sample counts, their exclusive scan, the edges' answers
// initialised) and ONE sweep launch whose blocks interpolate their configurations from the edge endpoints, run the score-only
// sweep of dcx_score (score_kernel.h sweep_rows, MODE_SCORE: the same rows, slices, wave-group shares and split launches) and
// fold each finished score into first_hit[e] with a ballot and one atomicMin per edge and wave.
//
// Work list: the samples of all edges in flat order, sample i of edge e at offs[e] + i (offs: the exclusive scan of the sample
// counts, made on the device by motion_prep.hip).  A 64-configuration tile takes 64 consecutive flat samples, so short edges
// share a tile and long ones span several.  The tile finds its first edge by a 64-ary search in offs (three dependent loads at
// E = 65536) and the edge of every lane by a binary search in LDS over the next 64 edge ends.
// Early exit: before a tile stages anything, wave 0 reads first_hit of its lanes' edges; a tile none of whose samples lies
// before its edge's current first hit skips the FK and the sweep.  first_hit only decreases (unsigned atomicMin, -1 = "free"
// is the largest unsigned value), so a skip decided on an older value is still right.
// Grid: one tile per block, sized from the upper bound E * max_samples / 64 (the host cannot read the total sample count back:
// the call is capturable); the kernel reads offs[E] and blocks past the end of the work list leave at once.  (A persistent grid
// striding over the tiles was the first form: the loop around the sweep kept its state live across it, and at the sweep's
// 64-VGPR budget the compiler spilled 12 VGPRs to scratch and parked 133 SGPRs - 1.9x the time of dcx_score on the same points.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "score_kernel.h"
#ifdef __HIPCC__
#include "wrap_device.h"
#endif

namespace dcx {

struct MotionArgs {
    ScoreArgs sc;             // the sweep's arguments (first: reload_kernargs reads them at offset 0).  sc.q / score / grad unused;
                              // sc.partial / sc.tile_done: the split launch's partial rows and arrival counters (caller's work)
    const float* qa;          // [E][dof]
    const float* qb;          // [E][dof]
    const int64_t* offs;      // [E + 1] exclusive scan of the sample counts (motion_prep.hip)
    const float* frac;        // [E] max_step rule: the step as a fraction of the edge, (1 / L) * max_step (dense_path's arithmetic)
    unsigned int* first_hit;  // [E] int32 answers, compared unsigned (-1 = free is the largest value)
    const float* margin;      // [c_out] or null (0)
    int64_t E;
    int32_t res;              // > 0: the res rule (qa + (k / res)(qb - qa), k < res); 0: the max_step rule
    int32_t early_exit;       // 0: every tile sweeps (developer knob motion_early_exit; the bound the benchmark compares against)
    uint64_t wrap_mask;       // bit j: coordinate j is an angle, the edge runs along its shortest arc (0: straight, every bit as before)
};

// LDS the motion kernel needs behind the sweep's plan and the FK program: per lane its edge, sample index, count, and the
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
    int32_t open_end;         // max_step rule: 1 drops the target qb from the samples (dcx_motion_cost; dcx_check_motions: 0)
    uint64_t wrap_mask;       // the edge's length is taken from the wrapped delta of the masked coordinates
};
hipError_t launch_motion_prep(const MotionPrepArgs& p, hipStream_t stream);

// one entry point per compiled width (motion_inst.hip)
typedef hipError_t (*motion_fn)(int kf, int cc, int nw, size_t lds, int64_t n_blocks, const MotionArgs& a, hipStream_t stream);
#define DCX_DECLARE_MOTION(D) hipError_t launch_motion_D##D(int, int, int, size_t, int64_t, const MotionArgs&, hipStream_t);
DCX_DECLARE_MOTION(2)  DCX_DECLARE_MOTION(4)  DCX_DECLARE_MOTION(6)  DCX_DECLARE_MOTION(8)
DCX_DECLARE_MOTION(12) DCX_DECLARE_MOTION(16) DCX_DECLARE_MOTION(18) DCX_DECLARE_MOTION(21)
DCX_DECLARE_MOTION(24) DCX_DECLARE_MOTION(27) DCX_DECLARE_MOTION(30) DCX_DECLARE_MOTION(32)
DCX_DECLARE_MOTION(36) DCX_DECLARE_MOTION(42) DCX_DECLARE_MOTION(48) DCX_DECLARE_MOTION(54)
DCX_DECLARE_MOTION(60) DCX_DECLARE_MOTION(64) DCX_DECLARE_MOTION(72) DCX_DECLARE_MOTION(84)
DCX_DECLARE_MOTION(96)
#undef DCX_DECLARE_MOTION

#ifdef __HIPCC__
// Coordinate j of sample k of the edge qa -> qb (one joint's values): the sQ prologue of both motion kernels.
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

// one configuration per lane: the score-only sweep of score_kernel (its prologue, with the rows of sQ interpolated from the
// edges instead of read from q), then the compare against the margins.  LDS: lds_plan(...).total + prog_floats (the FK
// program) rounded to 4, then kMotionLdsFloats (mo_off below).
template <int D, int KF, int CC, int MAXT, int XF = 0 /* 1: the expanded form, 2: its spare-slot form (score_kernel.h sweep_rows SP) */>
__global__ __launch_bounds__(MAXT, sweep_min_waves(D, CC, KF)) void motion_kernel(const MotionArgs m, int32_t mo_off) {
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
    int32_t* sFlag = sEdge + 192;

    const int64_t E = m.E;
    const int64_t total = m.offs[E];
    const int64_t tile = blockIdx.x;
    if (tile * 64 >= total) return;   // past the end of the work list (the grid is sized from E * max_samples): before any staging
    const FkWalk fw = fk_stage_sel(a.fkk, a.fk, a.fk_dwords, a.dh, smem + lp.fk, threadIdx.x, blockDim.x);
    const bool split = a.partial != nullptr;
    do {   // one tile per block (`continue` leaves)
        const int64_t base = tile * 64;
        const int nb = (int)((total - base) < 64 ? (total - base) : 64);
        if (wave == 0) {
            const int lane = threadIdx.x & 63;
            // the edge holding sample `base`: largest e with offs[e] <= base (offs[0] = 0 <= base < offs[E] = total)
            int64_t lo = 0, hi = E;
            while (hi - lo > 1) {
                const int64_t step = (hi - lo + 63) / 64;
                const int64_t idx = lo + (int64_t)lane * step;
                const bool le = idx < hi && m.offs[idx] <= base;
                const int p = __popcll(__builtin_amdgcn_ballot_w64(le));   // >= 1: lane 0 reads offs[lo]
                const int64_t nlo = lo + (int64_t)(p - 1) * step;
                hi = (lo + (int64_t)p * step < hi) ? lo + (int64_t)p * step : hi;
                lo = nlo;
            }
            const int64_t e0 = lo;
            sEnd[lane] = (e0 + 1 + lane <= E) ? m.offs[e0 + 1 + lane] : INT64_MAX;   // end of edge e0 + lane
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            const int64_t s = base + (lane < nb ? lane : nb - 1);
            int64_t e, start;
            if (sEnd[63] > s) {   // the usual case: this lane's edge is among the next 64 (first j with end > s)
                int j = 0;
#pragma unroll
                for (int h = 32; h >= 1; h >>= 1)
                    if (sEnd[j + h - 1] <= s) j += h;
                e = e0 + j;
                start = j ? sEnd[j - 1] : m.offs[e0];
            } else {              // more than 64 edges end inside this tile (edges over max_samples have no samples): global search
                int64_t l2 = e0 + 64, h2 = E;   // offs[l2] <= s < offs[h2]
                while (h2 - l2 > 1) {
                    const int64_t md = (l2 + h2) / 2;
                    if (m.offs[md] <= s) l2 = md; else h2 = md;
                }
                e = l2;
                start = m.offs[l2];
            }
            const int k = (int)(s - start);
            sEdge[lane] = (int32_t)e;
            sK[lane] = k;
            sN[lane] = (int32_t)(m.offs[e + 1] - start);
            // early exit: is any sample of this tile still before its edge's first hit?
            const unsigned int fh = m.early_exit ? __hip_atomic_load(m.first_hit + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0xffffffffu;
            const bool any_live = __builtin_amdgcn_ballot_w64(lane < nb && (unsigned int)k < fh) != 0;
            if (lane == 0) *sFlag = any_live ? 1 : 0;
        }
        __syncthreads();
        const bool live = *sFlag != 0;
        if (!live && !split) continue;   // (block-uniform; a split launch's blocks still take part in the tile's hand-over)
        float sc[CC];
#pragma unroll
        for (int c = 0; c < CC; ++c) sc[c] = 0.0f;
        if (live) {
            // ---- the rows of sQ: this tile's 64 samples, interpolated from their edges (dense_path / line_predict arithmetic) ----
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
        // ---- epilogue: the block's partial sums meet on wave 0 (rows in wave order, as score_kernel folds them) ----
        const auto& b = reload_kernargs<MotionArgs>();
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
        if (wave != 0) continue;
        if (split) {
            // the in-launch hand-over of score_kernel's one-wave form: publish write-through, drain, count; the last block of the
            // tile to arrive adds the ys rows in the order y = 0, 1, ... and answers for the tile
            float* out = b.sc.partial + (tile * b.sc.ys + blockIdx.y) * ACC * 64 + lane;
#pragma unroll
            for (int c = 0; c < CC; ++c) __hip_atomic_store(out + c * 64, sc[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            unsigned int arrived = 0;
            if (lane == 0) arrived = __hip_atomic_fetch_add(b.sc.tile_done + tile * kCounterStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            arrived = __builtin_amdgcn_readfirstlane(arrived);
            if (arrived != (unsigned int)b.sc.ys - 1u) continue;
            if (lane == 0) b.sc.tile_done[tile * kCounterStride] = 0u;   // ready for the next launch on this work buffer
            asm volatile("" ::: "memory");
            const float* part = b.sc.partial + tile * b.sc.ys * ACC * 64 + lane;
#pragma unroll
            for (int c = 0; c < CC; ++c) sc[c] = 0.0f;
            for (int y = 0; y < b.sc.ys; ++y)
#pragma unroll
                for (int c = 0; c < CC; ++c) sc[c] += __hip_atomic_load(part + ((size_t)y * ACC + c) * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // ---- the answer: collides iff score_c - margin_c > 0 for some class; the first colliding lane of each edge segment of
        // the wave lowers first_hit[e] (the lanes of an edge are consecutive, its sample index rising with the lane) ----
        bool hit = false;
#pragma unroll
        for (int c = 0; c < CC; ++c)
            if (c < b.sc.c_out) hit = hit || (sc[c] - (b.margin ? b.margin[c] : 0.0f) > 0.0f);
        hit = hit && lane < nb;
        const int k = sK[lane];
        const uint64_t hits = __builtin_amdgcn_ballot_w64(hit);
        const uint64_t starts = __builtin_amdgcn_ballot_w64(k == 0 || lane == 0);
        const uint64_t upto = (lane == 63) ? ~0ull : ((1ull << (lane + 1)) - 1ull);
        const int seg0 = 63 - __clzll(starts & upto);              // first lane of this lane's edge in the wave
        const uint64_t before = hits & ((1ull << lane) - 1ull) & ~((1ull << seg0) - 1ull);
        if (hit && before == 0) atomicMin(b.first_hit + sEdge[lane], (unsigned int)k);
    } while (0);
}
#endif  // __HIPCC__

}  // namespace dcx
