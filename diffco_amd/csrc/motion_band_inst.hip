// motion_band_inst.hip — instantiates the hybrid motion check kernel (motion_band_kernel.h) for ONE feature width
// (-DDCX_INST_D=<D>) and every kernel function and class count motion_inst.hip compiles, in the direct form and (where
// score_kernel.h xf_applies) the expanded form.  One object per width, the score-only sweep only.
#include "dcx_internal.h"
#include "motion_band_kernel.h"

#ifndef DCX_INST_D
#error "compile with -DDCX_INST_D=<feature width>"
#endif

namespace dcx {
#define DCX_CAT_(a, b) a##b
#define DCX_CAT(a, b) DCX_CAT_(a, b)
#ifdef DCX_STUB   // developer builds (Makefile ONLY_WIDTHS): this width is not compiled
hipError_t DCX_CAT(launch_motion_band_D, DCX_INST_D)(int, int, int, size_t, int64_t, const MotionBandArgs&, hipStream_t) { return hipErrorNotSupported; }
#else
namespace {
constexpr int kD = DCX_INST_D;
constexpr int kMaxT = kD <= 16 ? 1024 : (kD <= 48 ? 512 : 256);

template <int KF, int CC>
hipError_t go(int nw, size_t lds, int64_t nblk, const MotionBandArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)nblk, (unsigned)(a.sc.ys > 1 ? a.sc.ys : 1));
    // the kernel's LDS of its own sits behind the sweep's plan and the FK program (motion_kernel.h)
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
        if (a.sc.xf && a.sc.spare > 0) return launch(motion_band_kernel<kD, KF, CC, kMaxT, 2>);
    }
    if constexpr (xf_applies(kD, CC, KF)) {
        if (a.sc.xf) return launch(motion_band_kernel<kD, KF, CC, kMaxT, 1>);
    }
    return launch(motion_band_kernel<kD, KF, CC, kMaxT>);
}

template <int KF>
hipError_t by_cc(int cc, int nw, size_t lds, int64_t nblk, const MotionBandArgs& a, hipStream_t st) {
    switch (cc) {
    case 1: return go<KF, 1>(nw, lds, nblk, a, st);
    case 5: return go<KF, 5>(nw, lds, nblk, a, st);
#ifndef DCX_DEV_FAST
    case 4: return go<KF, 4>(nw, lds, nblk, a, st);
    case 8: return go<KF, 8>(nw, lds, nblk, a, st);
#endif
    default: return hipErrorInvalidValue;
    }
}
}  // namespace

hipError_t DCX_CAT(launch_motion_band_D, DCX_INST_D)(int kf, int cc, int nw, size_t lds, int64_t nblk, const MotionBandArgs& a,
                                                hipStream_t st) {
    switch (kf) {
    case KF_RQ2: return by_cc<KF_RQ2>(cc, nw, lds, nblk, a, st);
    case KF_POLY1: return by_cc<KF_POLY1>(cc, nw, lds, nblk, a, st);
    case KF_GEN: return by_cc<KF_GEN>(cc, nw, lds, nblk, a, st);
    default: return hipErrorInvalidValue;
    }
}
#endif  // DCX_STUB
}  // namespace dcx
