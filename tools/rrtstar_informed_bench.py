"""Batched RRT* with its samples drawn on the device (ScoreModel.rrtstar_run_sampled, dcx_rrtstar_run_sampled) against the
rounds fed from the host sampler (rrt_star's default: torch.rand per round, then ScoreModel.rrtstar_run), the sampler's own time
included; and what informed sampling buys in path length.

    python tools/rrtstar_informed_bench.py --baseline-lib PARENT/libdcx.so [--out profiles/r24_rrtstar_informed.txt] [--quick]
    python tools/rrtstar_informed_bench.py --leg timing|quality [--quick]        (one process, the library DCX_LIB names)

Timing: tools/rrtstar_bench.py's shapes (R in {1, 32, 256} x P in {1, 4, 8} x K in {0, 8, 16} x trees of {64, 4096} nodes, the
trees grown as there, every problem kept running).  Three legs per shape, interleaved in three rounds, the median of the three
medians reported with the three; microseconds per ROUND from HIP events around one chunk of --rounds rounds, and from the wall
clock around the same chunk with a synchronisation (the host sampler is host work: the events see it only as the stream's idle
time):
  host_fed          the chunk's samples from rrt_star's default sampler (goal bias 0.1), then rrtstar_run
  sampled_uniform   rrtstar_run_sampled, mode "uniform": the same distribution drawn on the device round by round
  sampled_informed  rrtstar_run_sampled, mode "informed", on the same trees with each problem's LAST node named its goal node
                    (a real node with its real cost, the goal row that node's): every draw is an informed one
The orchestrating call runs the timing leg in child processes, alternately under --baseline-lib (the parent commit's library:
host_fed alone, the baseline) and under the tree's own library (all three legs), tree size by tree size.

Quality: tools/rrtstar_bench.py's table again on the same 256 problems and budgets (accepted uniform configurations, seed 7;
slots 4, near 8), with rrt_star(sampling="informed") and rrt_star(sampling="device") beside the host-sampled rrt_star and
rrt_connect + shortcut_paths at the same number of submitted edges per problem.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STATE = ("nodes", "parent", "elen", "cost", "count", "status", "goal_node", "first_round")
RANGE, STEP, BIAS = 1.0, 0.25, 0.1


def timed(fn, reset, iters, warmup=1):
    """(median microseconds between HIP events, median wall microseconds) of fn() after reset()"""
    for _ in range(warmup):
        reset()
        fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(iters):
        reset()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6)
        ev.append(a.elapsed_time(b) * 1e3)
    return sorted(ev)[len(ev) // 2], sorted(wall)[len(wall) // 2]


def timing_leg(args, emit):
    import ctypes

    import bench
    from diffco_amd import _lib, rrtstar
    if os.environ.get("DCX_LIB"):   # an older library: bind what it exports (the loader insists on every symbol of its table)
        probe = ctypes.CDLL(_lib.LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name in [n for n in _lib.SYMBOLS if not hasattr(probe, n)]:
            del _lib.SYMBOLS[name]
    lib = _lib.require_gpu()
    has_sampled = hasattr(lib, "dcx_rrtstar_run_sampled") and hasattr(rrtstar, "host_device_samples")
    dev = torch.device("cuda", 0)
    w = bench.make_workload("headline", 1024, dev)
    m, lo, hi = w["model"], w["lo"].to(dev), w["hi"].to(dev)
    dof, T = len(lo), args.rounds
    limits = torch.stack([lo, hi], dim=1).contiguous()

    class Checker:
        def check_motions(self, a, b, max_step=None, wrap=None, max_samples=None, return_first=False):
            first, _ = m.check_motions(a, b, max_step=max_step, max_samples=max_samples, wrap=wrap)
            return first >= 0, first

    ck = Checker()

    def plan_of(R, P, K, cap, g):
        draw = lo + (hi - lo) * torch.rand((16 * R + 64, dof), generator=g, device=dev)
        draw = draw[m.check_motions(draw, draw, max_step=STEP, max_samples=2)[0] == -1]   # accepted configurations
        assert len(draw) >= 2 * R
        return rrtstar._StarPlan(ck, draw[:R], draw[R:2 * R], dev, RANGE, STEP, 2 * RANGE, K, None, P, cap, T, T, None, BIAS, limits, 0, None)

    def blank(R, cap, starts):
        st = dict(nodes=torch.zeros((R, cap, dof), device=dev), parent=torch.full((R, cap), -1, dtype=torch.int32, device=dev),
                  elen=torch.zeros((R, cap), device=dev), cost=torch.zeros((R, cap), device=dev),
                  count=torch.ones(R, dtype=torch.int32, device=dev), status=torch.zeros(R, dtype=torch.int32, device=dev),
                  goal_node=torch.full((R,), -1, dtype=torch.int32, device=dev),
                  first_round=torch.full((R,), -1, dtype=torch.int32, device=dev))
        st["nodes"][:, 0] = starts
        return st

    def grown(R, n, g):
        """R trees of exactly n nodes each, grown by the fused planner (K = 8, P = 8): a state with cap = n"""
        pl = plan_of(R, 8, 8, max(n, 2), g)
        st = blank(R, max(n, 2), pl.starts)
        far = pl.goals + 100.0   # no sample ever equals it: no goal node, every problem keeps running until it is full
        g0 = 0
        while bool((st["count"] < n).any()):
            smp = lo + (hi - lo) * torch.rand((64, R, 8, dof), generator=g, device=dev)
            st["status"].zero_()
            m.rrtstar_run(st, far, smp.contiguous(), g0, RANGE, STEP, 2 * RANGE, 8, pl.max_samples)
            g0 += 64
            if g0 > 1 << 16:
                raise SystemExit("the trees do not grow")
        return st, pl.max_samples, far

    def shape(R, P, K, n, g, st_n, max_samples, far):
        cap = n + T * P
        pl = plan_of(R, P, K, cap, g)
        init = blank(R, cap, st_n["nodes"][:, 0])
        for k in ("nodes", "parent", "elen", "cost"):
            init[k][:, :n] = st_n[k][:, :n]
        init["count"].fill_(n)
        solved = {k: v.clone() for k, v in init.items()}   # the informed leg's: the last node is the goal node
        solved["goal_node"].fill_(n - 1)
        reached = init["nodes"][:, n - 1].contiguous()
        st = {k: v.clone() for k, v in init.items()}

        def reset_to(src):
            def reset():
                for k in STATE:
                    st[k].copy_(src[k])
            return reset

        def host_fed():
            samples = pl.sampler(T, R, P).contiguous()
            m.rrtstar_run(st, far, samples, 0, RANGE, STEP, pl.radius, K, max_samples)

        def sampled(mode, goals):
            return lambda: m.rrtstar_run_sampled(st, goals, limits, 0, T, P, 0, RANGE, STEP, pl.radius, K, max_samples, mode=mode,
                                                 goal_bias=BIAS, tries=8)

        legs = [("host_fed", host_fed, reset_to(init))]
        if has_sampled:
            legs += [("sampled_uniform", sampled("uniform", far), reset_to(init)),
                     ("sampled_informed", sampled("informed", reached), reset_to(solved))]
        got = {name: ([], []) for name, _, _ in legs}
        for _ in range(3):
            for name, fn, reset in legs:
                ev, wall = timed(fn, reset, args.iters)
                got[name][0].append(ev / T)
                got[name][1].append(wall / T)
        med = lambda xs: sorted(xs)[1]   # noqa: E731
        res = dict(lib="baseline" if os.environ.get("DCX_LIB") else "this", R=R, P=P, K=K, tree=n, dof=dof, rounds=T, max_samples=max_samples)
        for name, (ev, wall) in got.items():
            res[name + "_us_per_round"] = round(med(ev), 1)
            res[name + "_x3"] = [round(x, 1) for x in ev]
            res[name + "_wall_us_per_round"] = round(med(wall), 1)
        if has_sampled:
            res["uniform_over_host_fed"] = round(res["sampled_uniform_us_per_round"] / res["host_fed_us_per_round"], 3)
            res["uniform_over_host_fed_wall"] = round(res["sampled_uniform_wall_us_per_round"] / res["host_fed_wall_us_per_round"], 3)
        emit(res)

    Rs, Ps, Ks = ((1, 32), (1, 4), (0, 8)) if args.quick else ((1, 32, 256), (1, 4, 8), (0, 8, 16))
    for n in args.trees:
        for R in Rs:
            g = torch.Generator(device=dev).manual_seed(n + R)
            st_n, ms, far = grown(R, n, g)
            for P in Ps:
                for K in Ks:
                    shape(R, P, K, n, g, st_n, ms, far)


def quality_leg(args, emit):
    import bench
    from diffco_amd import _lib, rrt, rrtstar, shortcut
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    w = bench.make_workload("headline", 1024, dev)
    m, lo, hi = w["model"], w["lo"].to(dev), w["hi"].to(dev)
    dof = len(lo)
    limits = torch.stack([lo, hi], dim=1)

    class Fused:   # the headline model as a checker the fused planners take
        def check_motions(self, a, b, max_step=None, wrap=None, max_samples=None, return_first=False):
            first, _ = m.check_motions(a, b, max_step=max_step, max_samples=max_samples, wrap=wrap)
            return first >= 0, first

        def _rrt_model(self, device=None):
            return m, 0.0

    g = torch.Generator(device=dev).manual_seed(7)
    q = lo + (hi - lo) * torch.rand((8 * args.problems, dof), generator=g, device=dev)
    q = q[m.check_motions(q, q, max_step=STEP, max_samples=2)[0] == -1]
    R = min(args.problems, len(q) // 2)
    starts, goals = q[:R], q[R:2 * R]
    plan = rrt.rrt_connect(Fused(), starts, goals, range=RANGE, max_step=STEP, slots=4, cap=1024, max_rounds=256, limits=limits, seed=0)
    path, count = plan.path_tensor()
    bent = count >= 3   # (a direct solve, two waypoints, is every method's fixed point)
    connect_rounds = int(plan.rounds[bent.cpu()].max()) if bool(bent.any()) else 0
    for N in ((16,) if args.quick else (16, 64, 256)):
        budget = 68 * N
        kw = dict(range=RANGE, max_step=STEP, radius=2 * RANGE, near=8, slots=4, cap=4 * N + 2, max_rounds=N, rounds_per_call=min(N, 64),
                  limits=limits, seed=0, goal_bias=BIAS)
        star = rrtstar.rrt_star(Fused(), starts, goals, **kw)
        reached = bent & (star.goal_node >= 0)
        res = dict(quality=True, problems=R, not_direct=int(bent.sum()), star_rounds=N, edges_per_problem=budget,
                   star_reached=int(reached.sum()), connect_rounds=connect_rounds)
        if bool(reached.any()):
            res["star_length"] = round(float(star.costs[reached].mean()), 4)
        for name, extra in (("informed", dict(sampling="informed")), ("informed_mix25", dict(sampling="informed", uniform_mix=0.25)),
                            ("device", dict(sampling="device"))):
            t0 = time.perf_counter()
            alt = rrtstar.rrt_star(Fused(), starts, goals, record_samples=(name == "informed"), **kw, **extra)
            torch.cuda.synchronize()
            got = bent & (alt.goal_node >= 0)
            both = got & reached
            res[name + "_reached"] = int(got.sum())
            res[name + "_seconds"] = round(time.perf_counter() - t0, 3)
            if bool(got.any()):
                res[name + "_length"] = round(float(alt.costs[got].mean()), 4)
            if bool(both.any()):   # the same problems under both samplers
                res[name + "_both"] = int(both.sum())
                res[name + "_length_both"] = round(float(alt.costs[both].mean()), 4)
                res["star_length_both_" + name] = round(float(star.costs[both].mean()), 4)
            if name == "informed":
                info = alt.sample_info[:, bent]
                drawn = int((info >= 0).sum())
                res["informed_share_of_draws"] = round(int((info >= 2).sum()) / max(drawn, 1), 4)
                res["informed_fell_back_share"] = round(int((info == 2 + 8).sum()) / max(int((info >= 2).sum()), 1), 4)
        rounds = (budget - 8 * connect_rounds) // 4
        if bool(reached.any()) and rounds >= 1:
            res["shortcut_rounds"] = rounds
            for name, skw in (("partial", dict(partial=True)), ("vertex", {})):
                out = shortcut.shortcut_paths(Fused(), path[reached].contiguous(), count[reached].contiguous(), max_step=STEP, slots=4,
                                              rounds=rounds, seed=1, **skw)
                res["connect_length"] = round(float(out.lengths_before.mean()), 4)
                res["connect_" + name + "_length"] = round(float(out.lengths.mean()), 4)
        emit(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4, help="rounds per timed chunk")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_rrtstar_informed.txt"))
    ap.add_argument("--quick", action="store_true", help="the small shapes only")
    ap.add_argument("--trees", type=lambda s: [int(v) for v in s.split(",")], default=[64, 4096], help="tree sizes of the timing leg")
    ap.add_argument("--problems", type=int, default=256, help="planning problems of the quality leg")
    ap.add_argument("--baseline-lib", default=None, help="the parent commit's libdcx.so: the timing leg's baseline")
    ap.add_argument("--leg", choices=("timing", "quality"), default=None, help="run this leg in this process and print its lines")
    ap.add_argument("--no-quality", action="store_true")
    args = ap.parse_args()

    def emit(res):
        print(json.dumps(res), flush=True)

    if args.leg:
        (timing_leg if args.leg == "timing" else quality_leg)(args, emit)
        return

    lines = []

    def child(leg, lib, trees=None):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--iters", str(args.iters), "--rounds", str(args.rounds),
               "--problems", str(args.problems)] + (["--quick"] if args.quick else []) + (["--trees", str(trees)] if trees else [])
        env = dict(os.environ)
        env.pop("DCX_LIB", None)
        if lib:
            env["DCX_LIB"] = os.path.abspath(lib)
        with subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True) as proc:
            for line in proc.stdout:   # (as they come)
                if line.startswith("{"):
                    print(line.rstrip(), flush=True)
                    lines.append(line.rstrip())
        if proc.returncode:
            raise SystemExit(f"the {leg} leg failed with exit status {proc.returncode}")

    for n in args.trees:   # the two libraries alternate, tree size by tree size
        if args.baseline_lib:
            child("timing", args.baseline_lib, n)
        child("timing", None, n)
    if not args.no_quality:
        child("quality", None)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/rrtstar_informed_bench.py (MI355X, headline model).  Timing lines: microseconds per round, medians of three\n"
                    "# interleaved rounds, HIP events and wall clock; lib: baseline = --baseline-lib, the parent commit's library (it\n"
                    "# measures host_fed alone), this = the tree's own.  Quality lines: mean path lengths at equal submitted edges per problem.\n"
                    + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
