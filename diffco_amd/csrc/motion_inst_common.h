// motion_inst_common.h — what the four motion instantiation files share (motion_inst.hip, motion_cost_inst.hip,
// motion_worst_inst.hip, motion_band_inst.hip): each instantiates its kernel for ONE feature width (-DDCX_INST_D=<D>) and every
// kernel function and class count dcx_score compiles, in the direct form and (where score_kernel.h xf_applies / spare_applies)
// the expanded and spare-slot forms.  A file names its kernel in a traits type
//     struct T { using Args = ...; static constexpr bool kByMode = ...;
//                template <int KF, int CC, int MODE, int XF> static constexpr auto kernel() { return the_kernel<...>; } };
// (MODE: the cost kernel's pass, kByMode; the score-only kernels ignore it) and defines its launch_*_D<D> on motion_launch.
#pragma once
#include "dcx_internal.h"
#include "motion_tile.h"

#ifndef DCX_INST_D
#error "compile with -DDCX_INST_D=<feature width>"
#endif

namespace dcx {
#define DCX_CAT_(a, b) a##b
#define DCX_CAT(a, b) DCX_CAT_(a, b)
#ifndef DCX_STUB   // (developer builds, Makefile ONLY_WIDTHS: a width that is not compiled reports hipErrorNotSupported)
namespace {
constexpr int kD = DCX_INST_D;
constexpr int kMaxT = kD <= 16 ? 1024 : (kD <= 48 ? 512 : 256);

template <class T, int KF, int CC, int MODE>
hipError_t motion_go(int nw, size_t lds, int64_t nblk, const typename T::Args& a, hipStream_t st) {
    const dim3 grid((unsigned)nblk, (unsigned)(a.sc.ys > 1 ? a.sc.ys : 1));
    // the kernel's LDS of its own sits behind the sweep's plan and the FK program (motion_tile.h MotionTile)
    const int32_t mo_off = (int32_t)(lds / sizeof(float)) - kMotionLdsFloats;
    auto launch = [&](auto kern) {
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        kern<<<grid, dim3(64 * nw), lds, st>>>(a, mo_off);
        return hipGetLastError();
    };
    if constexpr (spare_applies(kD, CC, KF)) {   // the spare-slot form of the expanded sweep (score_kernel.h)
        if (a.sc.xf && a.sc.spare > 0) return launch(T::template kernel<KF, CC, MODE, 2>());
    }
    if constexpr (xf_applies(kD, CC, KF)) {
        if (a.sc.xf) return launch(T::template kernel<KF, CC, MODE, 1>());
    }
    return launch(T::template kernel<KF, CC, MODE, 0>());
}

// T::kByMode (the cost kernel): one class runs the hinge sweep (MODE_GRAD_ROW), several the score pass (MODE_SCORE) and the
// gradient pass (MODE_GRAD_UP), picked by `mode`; the score-only kernels ignore `mode`
template <class T, int KF, int CC>
hipError_t motion_pass(int mode, int nw, size_t lds, int64_t nblk, const typename T::Args& a, hipStream_t st) {
    if constexpr (!T::kByMode) {
        return motion_go<T, KF, CC, MODE_SCORE>(nw, lds, nblk, a, st);
    } else if constexpr (CC == 1) {
        return mode == MODE_GRAD_ROW ? motion_go<T, KF, 1, MODE_GRAD_ROW>(nw, lds, nblk, a, st) : hipErrorInvalidValue;
    } else {
        if (mode == MODE_SCORE) return motion_go<T, KF, CC, MODE_SCORE>(nw, lds, nblk, a, st);
        if (mode == MODE_GRAD_UP) return motion_go<T, KF, CC, MODE_GRAD_UP>(nw, lds, nblk, a, st);
        return hipErrorInvalidValue;
    }
}

template <class T, int KF>
hipError_t motion_by_cc(int cc, int mode, int nw, size_t lds, int64_t nblk, const typename T::Args& a, hipStream_t st) {
    switch (cc) {
    case 1: return motion_pass<T, KF, 1>(mode, nw, lds, nblk, a, st);
    case 5: return motion_pass<T, KF, 5>(mode, nw, lds, nblk, a, st);
#ifndef DCX_DEV_FAST
    case 4: return motion_pass<T, KF, 4>(mode, nw, lds, nblk, a, st);
    case 8: return motion_pass<T, KF, 8>(mode, nw, lds, nblk, a, st);
#endif
    default: return hipErrorInvalidValue;
    }
}

template <class T>
hipError_t motion_launch(int kf, int cc, int mode, int nw, size_t lds, int64_t nblk, const typename T::Args& a, hipStream_t st) {
    switch (kf) {
    case KF_RQ2: return motion_by_cc<T, KF_RQ2>(cc, mode, nw, lds, nblk, a, st);
    case KF_POLY1: return motion_by_cc<T, KF_POLY1>(cc, mode, nw, lds, nblk, a, st);
    case KF_GEN: return motion_by_cc<T, KF_GEN>(cc, mode, nw, lds, nblk, a, st);
    default: return hipErrorInvalidValue;
    }
}
}  // namespace
#endif  // DCX_STUB
}  // namespace dcx
