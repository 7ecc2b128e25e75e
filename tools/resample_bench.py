"""Batched path resampling and the plan -> optimise hand-over: the fused call (resample.resample_paths, dcx_path_resample)
against the host composition of the same contract (resample.host_resample_paths: the torch ops a user would otherwise write) on
the same device tensors; and traj.optimize_paths - R problems in one DenseAdamRun - against a Python loop of one
fused_adam_traj_optimize(..., init_solution=...) per path, on the headline model.

    python tools/resample_bench.py [--iters 20] [--out profiles/r19_resample.txt] [--quick]

Resampling: R in {1, 32, 256} paths of {64, 512} waypoints (a straight motion between two uniform configurations in the joint
limits, its waypoints shaken by 0.2 rad) to T in {32, 128}.  Microseconds per CALL of the public entry - arguments checked,
outputs allocated, the launch(es), ended by a device synchronise - on a host clock; both legs warmed up, interleaved in three
rounds, the median of the three medians reported with the three.  launch_us: dcx_path_resample alone, on buffers allocated
once, between two HIP events.  same_bits: both legs return the same path, count and lengths.
Optimising: R in {8, 64} of those paths, 64 waypoints to T = 32, --maxiter dense-check Adam iterations: seconds per call of
optimize_paths against the loop (each of its runs reads its path back and restates the problem), and the largest difference of
the solutions relative to the largest coordinate."""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def wall(fn, iters, warmup=2):
    """median microseconds of fn() + synchronise on the host clock"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts.sort()
    return ts[len(ts) // 2]


def events(fn, iters, warmup=2):
    """median microseconds between two HIP events around fn()"""
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


def bits(t):
    return t.contiguous().view(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--maxiter", type=int, default=20, help="Adam iterations of the optimising legs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_resample.txt"))
    ap.add_argument("--quick", action="store_true", help="the small shapes only")
    args = ap.parse_args()
    import bench
    from diffco_amd import _lib, _ops, fused_adam_traj_optimize, optimize_paths
    from diffco_amd.resample import host_resample_paths, resample_paths
    lib = _lib.require_gpu()
    dev = torch.device("cuda", 0)
    w = bench.make_workload("headline", 1024, dev)
    m, rob, lo, hi = w["model"], w["rob"], w["lo"].to(dev), w["hi"].to(dev)
    dof = len(lo)
    lines = []
    med = lambda xs: sorted(xs)[1]   # noqa: E731

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)

    def paths_of(R, n, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        rand = lambda *shape: torch.rand(shape, generator=g, device=dev)   # noqa: E731
        a, b = lo + (hi - lo) * rand(R, 1, dof), lo + (hi - lo) * rand(R, 1, dof)
        s = torch.linspace(0, 1, n, device=dev)[None, :, None]
        inner = torch.ones(n, device=dev)
        inner[0] = inner[-1] = 0   # (the endpoints stay in the limits)
        path = (a + (b - a) * s + 0.2 * (2 * rand(R, n, dof) - 1) * inner[None, :, None]).contiguous()
        return path, torch.full((R,), n, dtype=torch.int32, device=dev)

    Rs, Ns, Ts = ((1, 32), (64,), (32,)) if args.quick else ((1, 32, 256), (64, 512), (32, 128))
    for n in Ns:
        for R in Rs:
            for T in Ts:
                path, count = paths_of(R, n, n + R + T)
                fused = lambda: resample_paths(path, count, n_waypoints=T)        # noqa: E731
                host = lambda: host_resample_paths(path, count, n_waypoints=T)    # noqa: E731
                out, out_count = torch.zeros((R, T, dof), device=dev), torch.zeros(R, dtype=torch.int32, device=dev)
                length = torch.zeros(R, device=dev)
                work = torch.empty(max(int(lib.dcx_path_resample_work_bytes(R, n)), 1), dtype=torch.uint8, device=dev)
                ptr = lambda t: ctypes.c_void_p(t.data_ptr())                    # noqa: E731
                launch = lambda: _lib.check(lib.dcx_path_resample(0, ptr(path), ptr(count), R, n, dof, 0, T, ptr(out), ptr(out_count),  # noqa: E731
                                                                  ptr(length), ptr(work), work.numel(), _ops._stream(dev)))
                a, b = fused(), host()
                same = bool(torch.equal(bits(a.path), bits(b.path)) and torch.equal(a.count, b.count)
                            and torch.equal(bits(a.lengths), bits(b.lengths))) and a.route == "fused" and b.route == "host"
                f3, h3, k3 = [], [], []
                for _ in range(3):
                    f3.append(wall(fused, args.iters))
                    h3.append(wall(host, max(3, args.iters // 4)))
                    k3.append(events(launch, args.iters))
                emit(dict(R=R, waypoints=n, T=T, dof=dof, same_bits=same, fused_us=round(med(f3), 1), fused_x3=[round(x, 1) for x in f3],
                          host_us=round(med(h3), 1), host_x3=[round(x, 1) for x in h3], launch_us=round(med(k3), 1),
                          launch_x3=[round(x, 1) for x in k3], speedup=round(med(h3) / med(f3), 1)))

    # ---- plan -> optimise: R problems in one run against one run per path ------------------------------------------------------
    T, n = 32, 64
    opts = {"MAXITER": args.maxiter, "max_speed": 0.3, "safety_margin": 0.0, "extra_optimizer_options": {"lr": 0.05},
            "dense_max_samples": 64, "fused_chunk": args.maxiter}
    for R in ((8,) if args.quick else (8, 64)):
        path, count = paths_of(R, n, 7 + R)
        got = {}

        def batched():
            got["recs"] = optimize_paths(rob, m, path, count, n_waypoints=T, options=dict(opts))

        def loop():   # what a user writes without it: resample, then walk the rows in Python
            res = resample_paths(path, count, n_waypoints=T)
            rows, out = res.path.cpu(), []
            for r in range(R):
                out.append(fused_adam_traj_optimize(rob, m, rows[r, 0], rows[r, -1],
                                                    dict(opts, NUM_RE_TRIALS=1, N_WAYPOINTS=T, seed=0, init_solution=rows[r],
                                                         dense_check=True)))
            got["loop"] = out

        b3, l3 = [], []
        for _ in range(3):
            b3.append(wall(batched, 3, warmup=1) / 1e6)
            l3.append(wall(loop, 2, warmup=1) / 1e6)
        sols = torch.stack([rec["solution"] for rec in got["recs"]]).cpu().double()
        ones = torch.tensor([rec["solution"] for rec in got["loop"]], dtype=torch.float64)
        emit(dict(optimize=True, R=R, waypoints=n, T=T, dof=dof, maxiter=args.maxiter,
                  same_success=[rec["success"] for rec in got["recs"]] == [rec["success"] for rec in got["loop"]],
                  max_rel_diff=float((sols - ones).abs().max() / ones.abs().max()),
                  batched_s=round(med(b3), 4), batched_x3=[round(x, 4) for x in b3], loop_s=round(med(l3), 4),
                  loop_x3=[round(x, 4) for x in l3], speedup=round(med(l3) / med(b3), 1)))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/resample_bench.py: microseconds per call (resampling) and seconds per call (optimising), medians of three "
                    "interleaved rounds (MI355X, headline model)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
