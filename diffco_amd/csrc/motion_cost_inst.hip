// motion_cost_inst.hip — instantiates the motion-cost kernel (motion_cost_kernel.h) for ONE feature width (-DDCX_INST_D=<D>) and
// every kernel function and class count dcx_score compiles, in the direct form and (where score_kernel.h xf_applies) the
// expanded form: C == 1 the hinge sweep (MODE_GRAD_ROW), C > 1 the score pass (MODE_SCORE) and the gradient pass (MODE_GRAD_UP).
#include "dcx_internal.h"
#include "motion_cost_kernel.h"

#ifndef DCX_INST_D
#error "compile with -DDCX_INST_D=<feature width>"
#endif

namespace dcx {
#define DCX_CAT_(a, b) a##b
#define DCX_CAT(a, b) DCX_CAT_(a, b)
#ifdef DCX_STUB   // developer builds (Makefile ONLY_WIDTHS): this width is not compiled
hipError_t DCX_CAT(launch_motion_cost_D, DCX_INST_D)(int, int, int, int, size_t, int64_t, const MotionCostArgs&, hipStream_t) {
    return hipErrorNotSupported;
}
#else
namespace {
constexpr int kD = DCX_INST_D;
constexpr int kMaxT = kD <= 16 ? 1024 : (kD <= 48 ? 512 : 256);

template <int KF, int CC, int MODE>
hipError_t go(int nw, size_t lds, int64_t nblk, const MotionCostArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)nblk, (unsigned)(a.sc.ys > 1 ? a.sc.ys : 1));
    // the kernel's LDS of its own sits behind the sweep's plan and the FK program (motion_cost_kernel.h)
    const int32_t mc_off = (int32_t)(lds / sizeof(float)) - kMotionCostLdsFloats;
    auto launch = [&](auto kern) {
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        kern<<<grid, dim3(64 * nw), lds, st>>>(a, mc_off);
        return hipGetLastError();
    };
    if constexpr (spare_applies(kD, CC, KF)) {   // the spare-slot form of the expanded sweep (score_kernel.h)
        if (a.sc.xf && a.sc.spare > 0) return launch(motion_cost_kernel<kD, KF, CC, MODE, kMaxT, 2>);
    }
    if constexpr (xf_applies(kD, CC, KF)) {
        if (a.sc.xf) return launch(motion_cost_kernel<kD, KF, CC, MODE, kMaxT, 1>);
    }
    return launch(motion_cost_kernel<kD, KF, CC, MODE, kMaxT>);
}

template <int KF, int CC>
hipError_t passes(int mode, int nw, size_t lds, int64_t nblk, const MotionCostArgs& a, hipStream_t st) {
    if (mode == MODE_SCORE) return go<KF, CC, MODE_SCORE>(nw, lds, nblk, a, st);
    if (mode == MODE_GRAD_UP) return go<KF, CC, MODE_GRAD_UP>(nw, lds, nblk, a, st);
    return hipErrorInvalidValue;
}

template <int KF>
hipError_t by_cc(int cc, int mode, int nw, size_t lds, int64_t nblk, const MotionCostArgs& a, hipStream_t st) {
    switch (cc) {
    case 1: return mode == MODE_GRAD_ROW ? go<KF, 1, MODE_GRAD_ROW>(nw, lds, nblk, a, st) : hipErrorInvalidValue;
    case 5: return passes<KF, 5>(mode, nw, lds, nblk, a, st);
#ifndef DCX_DEV_FAST
    case 4: return passes<KF, 4>(mode, nw, lds, nblk, a, st);
    case 8: return passes<KF, 8>(mode, nw, lds, nblk, a, st);
#endif
    default: return hipErrorInvalidValue;
    }
}
}  // namespace

hipError_t DCX_CAT(launch_motion_cost_D, DCX_INST_D)(int kf, int cc, int mode, int nw, size_t lds, int64_t nblk,
                                                     const MotionCostArgs& a, hipStream_t st) {
    switch (kf) {
    case KF_RQ2: return by_cc<KF_RQ2>(cc, mode, nw, lds, nblk, a, st);
    case KF_POLY1: return by_cc<KF_POLY1>(cc, mode, nw, lds, nblk, a, st);
    case KF_GEN: return by_cc<KF_GEN>(cc, mode, nw, lds, nblk, a, st);
    default: return hipErrorInvalidValue;
    }
}
#endif  // DCX_STUB
}  // namespace dcx
