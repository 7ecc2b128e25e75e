// geom_kernel.h — the sphere-model ground truth (dcx_geom_clearance): what dcx_api.hip and geom_kernels.hip share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dcx.h"
#include "fk_device.h"

namespace dcx {

struct GeomArgs {
    const FkProg* fk;
    const float* radii;     // [M]
    const float* obst;      // [O] rows of 16 dwords (dcx_geom_obstacle)
    int64_t O;
    const float* q;         // [B, dof]
    int64_t B;
    float* clearance;       // [B, G]
    int32_t* witness;       // [B, G, 2] or nullptr
    float* grad;            // [B, dof] or nullptr
    int32_t dof, d_fk, n_points, point_dim, frame_floats;
    int32_t pt_stride, coord_stride;   // coordinate r of sphere k is feature k * pt_stride + r * coord_stride
    int32_t n_groups, sphere_base, accumulate;
};

// LDS floats of one block: q rows, the centres' columns (the gradient's seed afterwards), per-group minima and witnesses, the radii, frames,
// the staged program
inline size_t geom_lds_bytes(const dcx_fk_desc& fk, int n_groups) {
    const int d_fk = fk.n_points * fk.point_dim;
    return sizeof(float) * ((size_t)((64 * fk.dof + 3) & ~3) + 64 * d_fk + 3 * 64 * n_groups + DCX_MAX_POINTS + 64 * fk_frame_floats(fk) + fk_prog_floats(fk));
}
// what a launch may ask for without raising the kernel's dynamic LDS attribute
constexpr size_t kGeomMaxLdsBytes = 64 * 1024;

hipError_t launch_geom_clearance(const GeomArgs& a, size_t lds_bytes, hipStream_t stream);

}  // namespace dcx
