// geom_kernels.hip — the sphere-model ground truth: fused FK + signed distances of the robot's spheres to a world of primitives
// (stands in for the reference's FCL / trimesh labels, collision_interfaces/env_interface.py:35-122, and the checkers' calls
// into them, collision_checkers.py:28-125).
//
// One wave per block, one lane per configuration, as fkine_kernel: the FK program is staged into LDS, the lane's sphere centres
// are the description's control points and stay where the chain walk leaves them (LDS columns, one per lane: no bank conflict,
// no register indexed by a loop counter), the radii beside them (one broadcast read that queues with the centre's three; a scalar
// load indexed by the sphere would be waited for inside the loop).  The obstacles are the OUTER loop: a row is wave-uniform, so its 16 dwords arrive
// through scalar loads and sit in SGPRs while the M spheres of the lane pass by, and the primitive's type is one uniform branch
// per obstacle, not per pair.  (obstacle, sphere) is also the order the contract breaks ties in.
#include "geom_kernel.h"

namespace dcx {
namespace {

typedef const __attribute__((address_space(4))) float* geom_kf;
typedef const __attribute__((address_space(4))) int32_t* geom_ki;

constexpr float kGeomInf = __builtin_huge_valf();

__device__ __forceinline__ float geom_sign(float x) { return __builtin_copysignf(1.0f, x); }

// signed distance of the local point l to the solid of TYPE with parameters p; WN: its gradient in local coordinates as well
// (a unit vector, or zero where it is undefined: the centre of a sphere, the axis segment of a capsule, the axis of a cylinder's
// radial part; on a box's medial planes the first of x, y, z that attains the maximum, towards +)
template <int TYPE, bool WN>
__device__ __forceinline__ float geom_dist(float lx, float ly, float lz, float p0, float p1, float p2, float* n) {
    if (TYPE == DCX_GEOM_SPHERE) {
        const float r = sqrtf(fmaf(lx, lx, fmaf(ly, ly, lz * lz)));
        if (WN) {
            const float inv = r > 0.0f ? 1.0f / r : 0.0f;
            n[0] = lx * inv; n[1] = ly * inv; n[2] = lz * inv;
        }
        return r - p0;
    }
    if (TYPE == DCX_GEOM_BOX) {
        const float ux = fabsf(lx) - p0, uy = fabsf(ly) - p1, uz = fabsf(lz) - p2;
        const float mx = fmaxf(ux, 0.0f), my = fmaxf(uy, 0.0f), mz = fmaxf(uz, 0.0f);
        const float out = sqrtf(fmaf(mx, mx, fmaf(my, my, mz * mz)));
        const float in = fminf(fmaxf(ux, fmaxf(uy, uz)), 0.0f);
        if (WN) {
            if (out > 0.0f) {
                const float inv = 1.0f / out;
                n[0] = mx * inv * geom_sign(lx); n[1] = my * inv * geom_sign(ly); n[2] = mz * inv * geom_sign(lz);
            } else {
                int ax = 0;
                float best = ux;
                if (uy > best) { best = uy; ax = 1; }
                if (uz > best) { best = uz; ax = 2; }
                n[0] = ax == 0 ? geom_sign(lx) : 0.0f;
                n[1] = ax == 1 ? geom_sign(ly) : 0.0f;
                n[2] = ax == 2 ? geom_sign(lz) : 0.0f;
            }
        }
        return out + in;
    }
    if (TYPE == DCX_GEOM_CAPSULE) {
        const float vz = lz - fminf(fmaxf(lz, -p1), p1);
        const float r = sqrtf(fmaf(lx, lx, fmaf(ly, ly, vz * vz)));
        if (WN) {
            const float inv = r > 0.0f ? 1.0f / r : 0.0f;
            n[0] = lx * inv; n[1] = ly * inv; n[2] = vz * inv;
        }
        return r - p0;
    }
    // DCX_GEOM_CYLINDER
    const float h = sqrtf(fmaf(lx, lx, ly * ly));
    const float a = h - p0, b = fabsf(lz) - p1;
    const float ma = fmaxf(a, 0.0f), mb = fmaxf(b, 0.0f);
    const float out = sqrtf(fmaf(ma, ma, mb * mb));
    const float in = fminf(fmaxf(a, b), 0.0f);
    if (WN) {
        const float hinv = h > 0.0f ? 1.0f / h : 0.0f;
        const float rx = lx * hinv, ry = ly * hinv, sz = geom_sign(lz);
        if (out > 0.0f) {
            const float inv = 1.0f / out;
            n[0] = ma * inv * rx; n[1] = ma * inv * ry; n[2] = mb * inv * sz;
        } else if (a >= b) {
            n[0] = rx; n[1] = ry; n[2] = 0.0f;
        } else {
            n[0] = 0.0f; n[1] = 0.0f; n[2] = sz;
        }
    }
    return out + in;
}

struct GeomRow {
    float rt[9], c[3], p[3];
};

__device__ __forceinline__ void geom_local(const GeomRow& r, float px, float py, float pz, float& lx, float& ly, float& lz) {
    const float dx = px - r.c[0], dy = py - r.c[1], dz = pz - r.c[2];
    lx = fmaf(r.rt[0], dx, fmaf(r.rt[1], dy, r.rt[2] * dz));
    ly = fmaf(r.rt[3], dx, fmaf(r.rt[4], dy, r.rt[5] * dz));
    lz = fmaf(r.rt[6], dx, fmaf(r.rt[7], dy, r.rt[8] * dz));
}

// the lane's M spheres against one obstacle: the smallest d - r_k and the first k that attains it
template <int TYPE>
__device__ __forceinline__ void geom_scan(const GeomRow& r, const float* sXl, const float* rad, int M, int ps, int cs, bool three,
                                          float& dmin, int& kmin) {
    // (four spheres in flight: a lone wave per SIMD has nothing else to hide the LDS reads and the square roots behind)
#pragma unroll 4
    for (int k = 0; k < M; ++k) {
        const float* x = sXl + (k * ps) * 64;
        const float px = x[0], py = x[cs * 64], pz = three ? x[2 * cs * 64] : 0.0f;
        float lx, ly, lz;
        geom_local(r, px, py, pz, lx, ly, lz);
        const float d = geom_dist<TYPE, false>(lx, ly, lz, r.p[0], r.p[1], r.p[2], nullptr) - rad[k];
        if (d < dmin) {
            dmin = d;
            kmin = k;
        }
    }
}

__global__ __launch_bounds__(64) void geom_clearance_kernel(const GeomArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * 64;
    const int nb = (int)((a.B - b0) < 64 ? (a.B - b0) : 64);
    const int dof = a.dof, d_fk = a.d_fk, G = a.n_groups, M = a.n_points;
    float* sQ = smem;
    float* sX = sQ + ((64 * dof + 3) & ~3);
    float* sB = sX + 64 * d_fk;                             // [G][64] running minima
    int* sWo = reinterpret_cast<int*>(sB + 64 * G);         // [G][64] witness obstacle
    int* sWk = sWo + 64 * G;                                // [G][64] witness sphere
    float* sR = reinterpret_cast<float*>(sWk + 64 * G);     // [DCX_MAX_POINTS] radii: one broadcast read beside the centre's three
    float* sF = sR + DCX_MAX_POINTS;
    const fk_cptr fk = stage_fk_prog(a.fk, sF + 64 * a.frame_floats, lane, 64);  // program last (variable size)
    const float* qsrc = a.q + b0 * dof;
    const int n = nb * dof;
    for (int i = lane; i < 64 * dof; i += 64) sQ[i] = qsrc[i < n ? i : (i % dof) + (nb - 1) * dof];
    if (lane < M) sR[lane] = a.radii[lane];
    for (int g = 0; g < G; ++g) {
        sB[g * 64 + lane] = kGeomInf;
        sWo[g * 64 + lane] = -1;
        sWk[g * 64 + lane] = -1;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    fk_forward_trig(fk, sQ + lane * dof, sF + lane, 0, 1);
    fk_forward_chain(fk, sQ + lane * dof, sX + lane, sF + lane);
    // every lane reads back its own column only: program order is enough

    const int ps = a.pt_stride, cs = a.coord_stride;
    const bool three = a.point_dim == 3;
    const geom_kf rows = (geom_kf)(uintptr_t)a.obst;
    float dall = kGeomInf;
    int oall = -1, kall = -1;
    for (int64_t o = 0; o < a.O; ++o) {
        const geom_kf row = rows + o * 16;
        const int tg = ((geom_ki)row)[0];
        const int type = tg & 0xff, g = tg >> 8;
        if ((unsigned)g >= (unsigned)G || type > DCX_GEOM_CYLINDER) continue;   // wave-uniform
        GeomRow r;
#pragma unroll
        for (int i = 0; i < 9; ++i) r.rt[i] = row[1 + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            r.c[i] = row[10 + i];
            r.p[i] = row[13 + i];
        }
        float dmin = kGeomInf;
        int kmin = -1;
        if (type == DCX_GEOM_SPHERE) geom_scan<DCX_GEOM_SPHERE>(r, sX + lane, sR, M, ps, cs, three, dmin, kmin);
        else if (type == DCX_GEOM_BOX) geom_scan<DCX_GEOM_BOX>(r, sX + lane, sR, M, ps, cs, three, dmin, kmin);
        else if (type == DCX_GEOM_CAPSULE) geom_scan<DCX_GEOM_CAPSULE>(r, sX + lane, sR, M, ps, cs, three, dmin, kmin);
        else geom_scan<DCX_GEOM_CYLINDER>(r, sX + lane, sR, M, ps, cs, three, dmin, kmin);
        if (dmin < sB[g * 64 + lane]) {
            sB[g * 64 + lane] = dmin;
            sWo[g * 64 + lane] = (int)o;
            sWk[g * 64 + lane] = kmin;
        }
        if (dmin < dall) {
            dall = dmin;
            oall = (int)o;
            kall = kmin;
        }
    }

    // ---- results: a row's entries are overwritten unless this call accumulates and the entry there is not larger
    float prev_all = kGeomInf;
    if (lane < nb) {
        const int64_t b = b0 + lane;
        for (int g = 0; g < G; ++g) {
            const float v = sB[g * 64 + lane];
            bool take = true;
            if (a.accumulate) {
                const float old = a.clearance[b * G + g];
                prev_all = fminf(prev_all, old);
                take = v < old;
            }
            if (!take) continue;
            a.clearance[b * G + g] = v;
            if (a.witness != nullptr) {
                const int wk = sWk[g * 64 + lane];
                a.witness[(b * G + g) * 2] = sWo[g * 64 + lane];
                a.witness[(b * G + g) * 2 + 1] = wk < 0 ? -1 : wk + a.sphere_base;
            }
        }
    }
    if (a.grad == nullptr) return;

    // ---- d(overall minimum)/dq: the unit normal at the witness sphere, zeros elsewhere, through one reverse sweep
    float nw[3] = {0.0f, 0.0f, 0.0f};
    if (oall >= 0) {
        const float* row = a.obst + (int64_t)oall * 16;   // the lane's own witness: a vector load
        GeomRow r;
#pragma unroll
        for (int i = 0; i < 9; ++i) r.rt[i] = row[1 + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            r.c[i] = row[10 + i];
            r.p[i] = row[13 + i];
        }
        const int type = reinterpret_cast<const int32_t*>(row)[0] & 0xff;
        const float* x = sX + lane + (kall * ps) * 64;
        float lx, ly, lz, nl[3];
        geom_local(r, x[0], x[cs * 64], three ? x[2 * cs * 64] : 0.0f, lx, ly, lz);
        if (type == DCX_GEOM_SPHERE) geom_dist<DCX_GEOM_SPHERE, true>(lx, ly, lz, r.p[0], r.p[1], r.p[2], nl);
        else if (type == DCX_GEOM_BOX) geom_dist<DCX_GEOM_BOX, true>(lx, ly, lz, r.p[0], r.p[1], r.p[2], nl);
        else if (type == DCX_GEOM_CAPSULE) geom_dist<DCX_GEOM_CAPSULE, true>(lx, ly, lz, r.p[0], r.p[1], r.p[2], nl);
        else geom_dist<DCX_GEOM_CYLINDER, true>(lx, ly, lz, r.p[0], r.p[1], r.p[2], nl);
        // world normal = R nl, R = (R^T)^T
        nw[0] = fmaf(r.rt[0], nl[0], fmaf(r.rt[3], nl[1], r.rt[6] * nl[2]));
        nw[1] = fmaf(r.rt[1], nl[0], fmaf(r.rt[4], nl[1], r.rt[7] * nl[2]));
        nw[2] = fmaf(r.rt[2], nl[0], fmaf(r.rt[5], nl[1], r.rt[8] * nl[2]));
    }
    // the centres have served: their columns become the upstream of the reverse sweep (fk_vjp reads frames, not X)
    for (int i = 0; i < d_fk; ++i) sX[i * 64 + lane] = 0.0f;
    if (oall >= 0) {
        float* x = sX + lane + (kall * ps) * 64;
        x[0] = nw[0];
        x[cs * 64] = nw[1];
        if (three) x[2 * cs * 64] = nw[2];
    }
    sB[lane] = (!a.accumulate || dall < prev_all) ? 1.0f : 0.0f;   // this row's gradient is this call's
    fk_vjp(fk, sQ + lane * dof, sF + lane, sX + lane, sQ + lane * dof);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    float* dst = a.grad + b0 * dof;
    for (int i = lane; i < n; i += 64)
        if (sB[i / dof] != 0.0f) dst[i] = sQ[i];
}

}  // namespace

hipError_t launch_geom_clearance(const GeomArgs& a, size_t lds_bytes, hipStream_t st) {
    if (a.B == 0) return hipSuccess;
    geom_clearance_kernel<<<dim3((unsigned)((a.B + 63) / 64)), dim3(64), lds_bytes, st>>>(a);
    return hipGetLastError();
}

}  // namespace dcx
