// motion_cost_inst.hip — instantiates the motion-cost kernel's passes (motion_cost_kernel.h)
// for ONE feature width; the launcher: motion_inst_common.h
#include "motion_cost_kernel.h"
#include "motion_inst_common.h"

namespace dcx {
#ifdef DCX_STUB
hipError_t DCX_CAT(launch_motion_cost_D, DCX_INST_D)(int, int, int, int, size_t, int64_t, const MotionCostArgs&, hipStream_t) {
    return hipErrorNotSupported;
}
#else
namespace {
struct Traits {
    using Args = MotionCostArgs;
    static constexpr bool kByMode = true;
    template <int KF, int CC, int MODE, int XF>
    static constexpr auto kernel() { return motion_cost_kernel<kD, KF, CC, MODE, kMaxT, XF>; }
};
}  // namespace
hipError_t DCX_CAT(launch_motion_cost_D, DCX_INST_D)(int kf, int cc, int mode, int nw, size_t lds, int64_t nblk, const MotionCostArgs& a,
        hipStream_t st) {
    return motion_launch<Traits>(kf, cc, mode, nw, lds, nblk, a, st);
}
#endif  // DCX_STUB
}  // namespace dcx
