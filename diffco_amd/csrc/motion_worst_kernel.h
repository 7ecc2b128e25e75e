// motion_worst_kernel.h — worst-sample motion queries (dcx_motion_worst): for E straight joint-space motions qa[e] -> qb[e],
//     worst[e] = max over the edge's samples x_k of v_k,   v_k = max over classes c of (score_c(x_k) - margin_c)
// with the smallest k that attains it, the smallest c that attains v_k there and, on request, the gradient of worst[e] with
// respect to qa[e] and qb[e] through that sample.
//
// The tiles are scored as dcx_check_motions scores them (motion_tile.h: the same bits for the same (model, E, max_samples));
// no early exit, every tile sweeps.
//
// Answer step (wave 0, or the last block of a split tile: where the scores are final).  Each live lane packs
//     key = orderable(v) << 32 | (0xffffff - k) << 8 | (0xff - c)
// (orderable: the monotone map of a float onto unsigned; a NaN class score counts as -inf, -0 as +0), so the larger key is the
// larger value, then the smaller sample index, then the smaller class.  The lanes of an edge are consecutive in the wave, so a
// segmented max-scan over wave shuffles leaves the segment's key in its last lane, which sends ONE 64-bit atomicMax to
// keys[e] (the caller's workspace, zeroed on the stream before the sweep).  Key 0 is "no sample yet": the key of -inf is
// 0x007fffff << 32 | ..., above it.  max over packed keys does not depend on the order of arrival: the same bits every call.
//
// motion_worst_finish.hip decodes the keys (one thread per edge), stages the worst sample and a one-hot upstream row for the
// library's own score+gradient launch on those E points, and chains that gradient to the endpoints.
#pragma once
#include "dcx_internal.h"
#include "motion_tile.h"

namespace dcx {

// The key's fields: 24 bits of sample index, 8 bits of class.  dcx_motion_worst refuses max_samples above the limit below at run
// time - that check is what protects the sample field.  (The assert beside it only records, for the reader, that the Python
// layer's default bound MOTION_MAX_SAMPLES = 10000 lies far inside it: it cannot see that constant change.)
constexpr int kMotionWorstSampleLimit = (1 << 24) - 1;
static_assert(10000 <= kMotionWorstSampleLimit, "documentation only: the Python layer's default max_samples fits the sample field");
static_assert(DCX_MAX_C <= 256, "the key holds the class in 8 bits");

struct MotionWorstArgs : MotionEdgeArgs {
    unsigned long long* keys; // [E] packed (value, sample, class) maxima; 0 = no sample yet
    const float* margin;      // [c_out] or null (0)
};

// one entry point per compiled width (motion_worst_inst.hip)
typedef hipError_t (*motion_worst_fn)(int kf, int cc, int nw, size_t lds, int64_t n_blocks, const MotionWorstArgs& a, hipStream_t stream);
#define DCX_DECLARE_MOTION_WORST(D) \
    hipError_t launch_motion_worst_D##D(int, int, int, size_t, int64_t, const MotionWorstArgs&, hipStream_t);
DCX_FOREACH_WIDTH(DCX_DECLARE_MOTION_WORST)
#undef DCX_DECLARE_MOTION_WORST

// the finish (motion_worst_finish.hip): keys decoded into the answers; with gradients, the worst samples and their one-hot
// upstream rows staged for the score+gradient launch, and afterwards the chain to the endpoints
struct MotionWorstFinishArgs {
    const float* qa;
    const float* qb;
    const int64_t* offs;
    const float* frac;
    const int32_t* status;    // motion_prep's first_hit: -1, or -2 for an edge over max_samples
    const unsigned long long* keys;
    float* worst;             // [E]
    int32_t* worst_idx;       // [E]
    int32_t* worst_class;     // [E] or null
    float* xstar;             // [E][dof] the worst samples, or null (no gradients)
    float* up;                // [E][C] one-hot upstream rows (C > 1 with gradients), or null
    const float* g;           // chain: [E][dof] d score_c* / dq at the worst sample
    float* grad_a;            // chain: [E][dof]
    float* grad_b;            // chain: [E][dof]
    int64_t E;
    int32_t dof, res, C;
    uint64_t wrap_mask;
};
hipError_t launch_motion_worst_finish(const MotionWorstFinishArgs& f, hipStream_t stream);
hipError_t launch_motion_worst_chain(const MotionWorstFinishArgs& f, hipStream_t stream);

// the key's fields (both sides of the atomic use these)
__host__ __device__ inline uint32_t motion_worst_orderable(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
__host__ __device__ inline uint32_t motion_worst_unorder(uint32_t o) { return (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o; }

#ifdef __HIPCC__
template <int D, int KF, int CC, int MAXT, int XF = 0 /* motion_tile.h motion_sweep */>
__global__ __launch_bounds__(MAXT, sweep_min_waves(D, CC, KF)) void motion_worst_kernel(const MotionWorstArgs m, int32_t mo_off) {
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
    // (motion_tile.h), whose bodies they repeat word for word: with the two as inlined calls the compiler schedules this
    // kernel's sweep in another order, 1.7 - 2.1 % slower at E = 65536 (profiles/r18_motion_refactor_timing.txt).
    const auto& b = reload_kernargs<MotionWorstArgs>();
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
    // ---- the answer: v = max_c (score_c - margin_c) and the first class that attains it (a NaN difference never wins: it
    // counts as -inf); the key, its maximum over the lane's edge segment, one atomic per segment ----
    float v = -__builtin_inff();
    int cbest = 0;
#pragma unroll
    for (int c = 0; c < CC; ++c) {
        const float d = sc[c] - (b.margin ? b.margin[c] : 0.0f);
        if (c < b.sc.c_out && d > v) {
            v = d;
            cbest = c;
        }
    }
    v += 0.0f;   // -0 becomes +0: equal values, equal keys
    const int k = t.sK[lane];
    const bool on = lane < nb;   // (the lanes behind the work list's end repeat its last sample)
    unsigned long long key = 0ull;
    if (on)
        key = ((unsigned long long)motion_worst_orderable(__float_as_uint(v)) << 32) |
              ((unsigned long long)(0xffffffu - (unsigned int)k) << 8) | (unsigned long long)(0xffu - (unsigned int)cbest);
    uint64_t starts;
    const int seg0 = motion_segment_start(k, lane, starts);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {   // inclusive max-scan inside the segment
        const unsigned long long o = __shfl_up(key, d, 64);
        if (lane - d >= seg0 && o > key) key = o;
    }
    const bool seg_last = lane == 63 || ((starts >> (lane + 1)) & 1ull) != 0;
    if (seg_last && key != 0ull) atomicMax(b.keys + t.sEdge[lane], key);
}
#endif  // __HIPCC__

}  // namespace dcx
