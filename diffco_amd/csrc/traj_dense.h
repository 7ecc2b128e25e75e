// traj_dense.h — the launches of the dense-check Adam trajectory loop (traj_dense.hip; include/dcx.h dcx_traj_dense_run).
#pragma once
#include "dcx_internal.h"

namespace dcx {

// per-edge layout everywhere: e = r * W + w; slot W - 1 of a path is the closed zero-length edge on its last waypoint

// before the motion costs of an iteration: qb[e] = p[min(w + 1, W - 1)] (qa is the path itself), q_last[r] = p[W - 1], and -
// margin_fill != nullptr - the C margins the caller left to opt->safety_margin
struct TrajDenseEdgeArgs {
    const float* path;   // [R, W, dof]
    float* qb;           // [R * W, dof]
    float* q_last;       // [R, dof]
    float* margin_fill;  // [C] or nullptr
    float margin_value;
    int32_t R, W, dof, C;
};
hipError_t launch_traj_dense_edges(const TrajDenseEdgeArgs& a, hipStream_t stream);

// after them: the R closed edges' results into slot W - 1 of the per-edge arrays
struct TrajDenseCloseArgs {
    const float *cost, *grad_a, *grad_b;   // [R], [R, dof], [R, dof]
    const int32_t* n_samples;              // [R]
    dcx_traj_dense_io io;
    int32_t R, W, dof;
};
hipError_t launch_traj_dense_close(const TrajDenseCloseArgs& a, hipStream_t stream);

// the dense step (one block per path, one lane per waypoint)
hipError_t launch_traj_dense_step(const FkProg* fk_dev, const dcx_fk_desc& fk, const dcx_traj_state& st, const dcx_traj_opts& opt,
                                  const dcx_traj_dense_opts& dopt, const dcx_traj_dense_io& io, int n_class, int step,
                                  hipStream_t stream);

}  // namespace dcx
