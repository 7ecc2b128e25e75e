"""The sphere-model ground truth: the fused call (SphereWorldChecker, dcx_geom_clearance) against the torch composition with the
same contract (_ops.fkine on the sphere descriptions, then geometry.host_clearance_points, on GPU tensors) on the same GPU; the
fused call's pair-test rate against the VALU floor; and its cost per configuration beside the lazy roadmap's break-even.

    python tools/geom_clearance_bench.py [--iters 20] [--out profiles/r28_geom_clearance.txt] [--quick]

Cases: B in {1024, 65536}; the Panda URDF fixture with about 32 and about 64 spheres along its links; 16 and 64 obstacles (the four
primitive types in turn, in the arm's workspace); with and without the gradient (the composition's gradient: autograd through
fkine and the torch ops).  Microseconds per call from HIP events around each call on an idle stream; the two legs interleaved in
three rounds, the median of the three medians reported with the three.  The composition runs in slices of CHUNK configurations
(its [B, M, O, 3] intermediates would not fit otherwise).
The floor: B * M * O pair tests of VALU_PER_PAIR operations each over the chip's 256 CUs x 4 SIMDs x 16 lanes per clock, at the
shader clock dcx_debug_clock_probe measures during the run.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from knn_bench import LANES_PER_CLOCK, shader_mhz, timed   # noqa: E402

VALU_PER_PAIR = 25     # the analytic count: 3 subtracts, 9 for R^T (p - c), ~10 for the solid's closed form, the radius, the min
CHUNK = 8192
BREAK_EVEN_US = 0.09   # README: a lazy roadmap wins for any ground truth costlier than this per configuration


def spheres_near(robot, target, radius=0.06):
    """spheres_along_links with the spacing whose count comes nearest to `target`"""
    from diffco_amd import geometry
    best = None
    for spacing in np.linspace(0.2, 0.01, 96):
        s = geometry.spheres_along_links(robot, radius, float(spacing))
        if best is None or abs(len(s) - target) < abs(len(best) - target):
            best = s
    return best


def world_of(O, seed):
    from diffco_amd import geometry
    rng = np.random.default_rng(seed)
    w = geometry.World()
    for o in range(O):
        Q, R = np.linalg.qr(rng.standard_normal((3, 3)))
        Q = Q * np.sign(np.diag(R))
        if np.linalg.det(Q) < 0:
            Q[:, 0] = -Q[:, 0]
        T = np.eye(4)
        T[:3, :3] = Q
        T[:3, 3] = rng.uniform(-0.9, 0.9, 3) * np.array([1.0, 1.0, 0.6]) + np.array([0, 0, 0.5])
        s = rng.uniform(0.03, 0.12, 3)
        [lambda: w.add_sphere(f"s{o}", s[0], T), lambda: w.add_box(f"b{o}", 2 * s, T),
         lambda: w.add_capsule(f"c{o}", s[0], 2 * s[1], T), lambda: w.add_cylinder(f"y{o}", s[0], 2 * s[1], T)][o % 4]()
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_geom_clearance.txt"))
    ap.add_argument("--quick", action="store_true", help="the small batch only")
    ap.add_argument("--host-budget", type=float, default=4.0, help="seconds of composition timing per round and case")
    args = ap.parse_args()
    import helpers
    from diffco_amd import _lib, geometry
    lib = _lib.require_gpu()
    dev = torch.device("cuda", 0)
    rob = helpers.urdf_robot("urdf_panda")
    lines = []

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)

    for target in (32, 64):
        spheres = spheres_near(rob, target)
        radii = spheres.radii.to(dev)
        for O in (16, 64):
            world = world_of(O, O)
            checker = geometry.SphereWorldChecker(spheres, world)
            for B in ((1024,) if args.quick else (1024, 65536)):
                g = torch.Generator(device=dev).manual_seed(B)
                lo, hi = rob.limits[:, 0].to(dev), rob.limits[:, 1].to(dev)
                q = torch.rand((B, rob.dof), generator=g, device=dev) * (hi - lo) + lo
                for want_grad in (False, True):
                    def fused():
                        if not want_grad:
                            return checker.clearance(q)
                        qq = q.detach().requires_grad_(True)
                        c = checker.clearance(qq)
                        return c, torch.autograd.grad(c.sum(), qq)[0]

                    def host():
                        outs, grads = [], []
                        for i in range(0, B, CHUNK):
                            qq = q[i:i + CHUNK].detach().requires_grad_(want_grad)
                            c = geometry.host_clearance_points(spheres.centres(qq), radii, world, 1)[0][:, 0]
                            outs.append(c.detach())
                            if want_grad:
                                grads.append(torch.autograd.grad(c.sum(), qq)[0])
                        return (torch.cat(outs), torch.cat(grads)) if want_grad else torch.cat(outs)

                    a, b = fused(), host()
                    ca, cb = (a[0], b[0]) if want_grad else (a, b)
                    err = float((ca.detach() - cb).abs().max())
                    gerr = float((a[1] - b[1]).abs().max()) if want_grad else None
                    t_host = timed(host, 1, warmup=1)
                    host_iters = max(2, min(args.iters, int(args.host_budget * 1e6 / max(t_host, 1.0))))
                    f3, h3 = [], []
                    for _ in range(3):
                        f3.append(timed(fused, args.iters))
                        h3.append(timed(host, host_iters, warmup=1))
                    mhz = shader_mhz(lib, dev, fused)
                    med = lambda xs: sorted(xs)[1]   # noqa: E731
                    M = len(spheres)
                    res = dict(B=B, M=M, chunks=len(spheres.chunks), O=O, grad=want_grad, max_abs_diff=err, max_abs_grad_diff=gerr,
                               colliding=round(float((ca < 0).float().mean()), 3),
                               fused_us=round(med(f3), 1), fused_us_x3=[round(x, 1) for x in f3], host_us=round(med(h3), 1),
                               host_us_x3=[round(x, 1) for x in h3], host_iters=host_iters, speedup=round(med(h3) / med(f3), 2),
                               us_per_config=round(med(f3) / B, 5), break_even_us=BREAK_EVEN_US, shader_mhz=mhz and round(mhz))
                    if mhz:
                        floor = VALU_PER_PAIR * B * M * O / (LANES_PER_CLOCK * mhz)      # microseconds
                        res.update(pair_tests_per_us=round(B * M * O / med(f3)), valu_per_pair=VALU_PER_PAIR, floor_us=round(floor, 2),
                                   floor_ratio=round(med(f3) / floor, 2))
                    emit(res)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/geom_clearance_bench.py: microseconds per call, medians of three interleaved rounds (MI355X)\n"
                    + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
