"""The dense-check Adam trajectory loop (dcx_traj_dense_run) on the headline model (Baxter DH-7, Polyharmonic(1,1), S = 2000,
C = 1) and on cfg3's five-class model: R paths of W = 50 waypoints whose segments take 4 - 16 samples of max_step.  Microseconds
per iteration beside
  (a) the work it is made of: one dcx_motion_cost_ex call on the same R (W - 1) open edges plus one dcx_traj_adam_step,
  (b) the non-persistent waypoint-only loop (dcx_traj_adam_run with the traj_fused knob at 0): the difference is the price of
      the dense check,
  (c) the host composition: ScoreModel.path_cost + autograd + torch.optim.Adam + wrap2pi per iteration.
Every timing is the median of interleaved rounds (each a median over --iters calls of --steps iterations, CUDA events on an
idle stream, after warm-up calls).  lr is tiny and no stop rule is armed, so every call does the same work.

    python tools/traj_dense_bench.py [--paths 256 32] [--iters 20] [--models headline cfg3]
    python tools/traj_dense_bench.py --trace --models headline --paths 256     # ten iterations, for a kernel trace

One JSON line per (model, R) on stdout.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, nargs="+", default=[256, 32])
    ap.add_argument("--waypoints", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10, help="iterations per timed call")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--models", nargs="+", default=["headline", "cfg3"])
    ap.add_argument("--trace", action="store_true", help="warm up, then one call of --steps iterations and nothing else")
    args = ap.parse_args()
    import bench
    from diffco_amd import _lib
    from diffco_amd.utils import wrap2pi
    lib = _lib.require_gpu()
    dev = torch.device("cuda", 0)
    step, cap, W, K = 0.05, 24, args.waypoints, args.steps
    p = lambda t: C.c_void_p(t.data_ptr())
    for name in args.models:
        w = bench.make_workload(name, 1024, dev)
        m, lo, hi = w["model"], w["lo"].to(dev), w["hi"].to(dev)
        dof = m.dof
        for R in args.paths:
            g = torch.Generator(device=dev).manual_seed(R)
            dirn = torch.randn((R, W - 1, dof), generator=g, device=dev)
            dirn = dirn / dirn.norm(dim=2, keepdim=True)
            n_want = torch.randint(4, 17, (R, W - 1, 1), generator=g, device=dev).float()
            start = torch.rand((R, 1, dof), generator=g, device=dev) * (hi - lo) + lo
            paths = torch.cat([start, dirn * step * (n_want - 0.5)], dim=1).cumsum(dim=1).contiguous()   # ceil(L / step) = n_want
            scores = m.score_raw(paths.reshape(-1, dof))
            margin = torch.quantile(scores, 0.5, dim=0).contiguous()        # half the waypoints above their margin
            f32 = dict(device=dev, dtype=torch.float32)
            E = R * W

            def state():
                path = paths.clone()
                b = dict(path=path, adam_m=torch.zeros_like(path), adam_v=torch.zeros_like(path),
                         limits=torch.stack([lo, hi], dim=1).contiguous(), col_score=torch.zeros(E * m.C, **f32),
                         col_grad=torch.zeros((E, dof), **f32), stats=torch.zeros((R, 8), **f32),
                         lowest_loss=torch.full((R,), float("inf"), **f32), lowest_obj=torch.full((R,), float("inf"), **f32),
                         lowest_path=path.clone(), best_valid_obj=torch.full((R,), float("inf"), **f32),
                         best_valid_path=path.clone(), done=torch.zeros(R, device=dev, dtype=torch.int32),
                         steps=torch.zeros(R, device=dev, dtype=torch.int32))
                return _lib.TrajState(R, W, *(p(t) for t in b.values())), b

            opt = _lib.TrajOpts(1e-6, 0.9, 0.999, 1e-8, 1, 10, 10, 10, float(margin[0]), 0.3, -1.0, 0.0)   # no stop is armed
            dopt = _lib.TrajDenseOpts(step, cap, 0, 0, 0, 0.0)
            st_d, bd = state()
            n_checks = torch.zeros(R, device=dev, dtype=torch.int64)
            io = _lib.TrajDenseIO(None, None, p(n_checks), None, None, None, None)
            need = int(lib.dcx_traj_dense_work_bytes(m._h, R, W, cap))
            work = torch.empty(need, device=dev, dtype=torch.uint8)

            def dense():
                _lib.check(lib.dcx_traj_dense_run(m._h, C.byref(st_d), C.byref(opt), C.byref(dopt), C.byref(io), p(margin), 1, K,
                                                  p(work), need, m._st()))

            if args.trace:
                for _ in range(3):
                    dense()
                torch.cuda.synchronize()
                print(json.dumps(dict(model=name, R=R, W=W, traced_iterations=3 * K)), flush=True)
                continue

            # (a) its parts: the open edges' motion costs and the waypoint-only step
            Eo = R * (W - 1)
            qa, qb = paths[:, :-1].reshape(Eo, dof).contiguous(), paths[:, 1:].reshape(Eo, dof).contiguous()
            cost, ga, gb = torch.empty(Eo, **f32), torch.empty((Eo, dof), **f32), torch.empty((Eo, dof), **f32)
            ns = torch.empty(Eo, device=dev, dtype=torch.int32)
            mo = _lib.MotionCostOpts(0, step, cap, 1)
            mneed = int(lib.dcx_motion_cost_work_bytes(m._h, Eo, cap))
            mwork = torch.empty(mneed, device=dev, dtype=torch.uint8)
            st_s, bs = state()
            mhost = (C.c_float * m.C)(*margin.tolist())

            def parts():
                for _ in range(K):
                    _lib.check(lib.dcx_motion_cost_ex(m._h, p(qa), p(qb), Eo, C.byref(mo), p(margin), 1.0, p(cost), p(ga), p(gb), p(ns),
                                                      p(mwork), mneed, 0, m._st()))
                    _lib.check(lib.dcx_traj_adam_step_mc(dev.index or 0, C.byref(m.desc), C.byref(st_s), C.byref(opt), mhost, m.C, 1,
                                                         m._st()))

            # (b) the waypoint-only loop, launches per iteration
            st_w, bw = state()

            def waypoint():
                _lib.check(lib.dcx_traj_adam_run_mc(m._h, C.byref(st_w), C.byref(opt), mhost, 1, K, m._st()))

            # (c) the host composition
            ph = paths.clone().requires_grad_(True)
            adam = torch.optim.Adam([ph], lr=1e-6)
            mlist = margin.tolist()

            def host():
                for _ in range(K):
                    adam.zero_grad()
                    m.path_cost(ph, step, margin=mlist, max_samples=cap).sum().backward()
                    adam.step()
                    ph.data = wrap2pi(ph.data)

            dense()
            torch.cuda.synchronize()
            samples = int(n_checks.sum()) // K
            res = dict(model=name, C=m.C, R=R, W=W, samples_per_iteration=samples, frozen=int(bd["done"].sum()))
            calls = {"dense_run_us": dense, "motion_cost_plus_step_us": parts, "waypoint_loop_us": waypoint}
            rounds = {k: [] for k in list(calls) + ["host_composition_us"]}
            lib.dcx_debug_set(b"traj_fused", 0)      # (b) as launches per iteration, not the persistent kernel
            try:
                for _ in range(args.rounds):   # interleaved
                    for k, fn in calls.items():
                        rounds[k].append(timed(fn, args.iters) / K)
                    rounds["host_composition_us"].append(timed(host, max(3, args.iters // 5), warmup=1) / K)
            finally:
                lib.dcx_debug_set(b"traj_fused", -1)
            for k, v in rounds.items():
                res[k] = round(sorted(v)[len(v) // 2], 1)
                res[k.replace("_us", "_spread")] = round((max(v) - min(v)) / max(min(v), 1e-9), 3)
            res["dense_over_parts"] = round(res["dense_run_us"] / res["motion_cost_plus_step_us"], 3)
            res["price_of_dense_check_us"] = round(res["dense_run_us"] - res["waypoint_loop_us"], 1)
            res["speedup_vs_host"] = round(res["host_composition_us"] / res["dense_run_us"], 1)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
