// motion_inst.hip — instantiates the motion-check kernel (motion_kernel.h)
// for ONE feature width; the launcher: motion_inst_common.h
#include "motion_kernel.h"
#include "motion_inst_common.h"

namespace dcx {
#ifdef DCX_STUB
hipError_t DCX_CAT(launch_motion_D, DCX_INST_D)(int, int, int, size_t, int64_t, const MotionArgs&, hipStream_t) {
    return hipErrorNotSupported;
}
#else
namespace {
struct Traits {
    using Args = MotionArgs;
    static constexpr bool kByMode = false;
    template <int KF, int CC, int MODE, int XF>
    static constexpr auto kernel() { return motion_kernel<kD, KF, CC, kMaxT, XF>; }
};
}  // namespace
hipError_t DCX_CAT(launch_motion_D, DCX_INST_D)(int kf, int cc, int nw, size_t lds, int64_t nblk, const MotionArgs& a,
        hipStream_t st) {
    return motion_launch<Traits>(kf, cc, MODE_SCORE, nw, lds, nblk, a, st);
}
#endif  // DCX_STUB
}  // namespace dcx
