"""Batched RRT*: the fused rounds (ScoreModel.rrtstar_run, dcx_rrtstar_run) against the host composition of the same contract
(rrtstar.host_rrt_star's round: roadmap.knn, torch arithmetic, one check_motions call per phase) on the same GPU, on the
headline model; one RRT-Connect round at the same R and slots from the same run as the yardstick; where a round's time goes;
and what the planner buys in path length.

    python tools/rrtstar_bench.py [--iters 10] [--rounds 4] [--out profiles/r23_rrtstar.txt] [--quick]
    python tools/rrtstar_bench.py --profile-shape 256,4,8,4096 --state FILE --grow-only
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/rrtstar_bench.py --profile-shape 256,4,8,4096 --state FILE
    python tools/rrtstar_bench.py --shares DIR [--append profiles/r23_rrtstar.txt]

Timing: R in {1, 32, 256} problems x P in {1, 4, 8} slots x K in {0, 8, 16} near nodes x trees of {64, 4096} nodes.  The
trees are grown by the fused planner itself (K = 8, P = 8, uniform samples) until every tree holds that many nodes, every
problem kept running (status 0, no goal), then copied into a state whose cap leaves room for every append of a timed chunk.
Microseconds per ROUND from HIP events around one chunk of --rounds rounds on an idle stream, every timed chunk starting from
the same state (restored outside the events); the legs interleaved in three rounds, the median of the three medians reported
with the three.  same_bits: the fused and the host leg leave the same state.

Shares (--profile-shape runs one shape's fused chunks alone, to be run under the profiler's kernel trace, on trees a run
with --grow-only has grown and left in --state, so that the trace holds the timed rounds alone; --shares reads the trace's
kernel statistics): the share of the kernels' time in the motion calls' kernels (the three sweeps with their prep), the
near search, the nearest + steer search, the refresh, and the rest of the tree logic.

Quality: the 256 problems of tools/shortcut_bench.py's outcome leg (accepted uniform configurations, seed 7).  On the problems
that are not direct motions, the mean path length of rrt_star after N rounds (slots 4, near 8: 4 * (1 + 2 * 8) = 68 edges per
problem and round) against rrt_connect + shortcut_paths in its vertex and its partial mode with the same number of submitted
edges per problem: rrt_connect's 8 edges per problem and round for the rounds its slowest problem took, the rest spent on
shortcut rounds of 4 edges per path.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STATE = ("nodes", "parent", "elen", "cost", "count", "status", "goal_node", "first_round")
RANGE, STEP = 1.0, 0.25


def timed(fn, reset, iters, warmup=1):
    for _ in range(warmup):
        reset()
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def same_state(a, b):
    return all(bool(torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                                b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k])) for k in STATE)


def shares(stats_dir):
    """the kernels' time of a rocprofv3 --kernel-trace --stats run, grouped"""
    files = glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {stats_dir}")
    groups = dict(motion_sweeps=0.0, near_search=0.0, nearest_steer=0.0, refresh=0.0, tree_logic=0.0, other=0.0)
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(next(v for k, v in row.items() if "TotalDuration" in k))
            key = ("near_search" if "rrtstar_near" in name else "refresh" if "rrtstar_refresh" in name else
                   "tree_logic" if "rrtstar_" in name else "nearest_steer" if "rrt_nearest" in name else
                   "motion_sweeps" if "motion" in name else "other")
            groups[key] += ns
    total = sum(groups.values())
    return dict(shares=True, shape_R_P_K_tree=os.path.basename(os.path.normpath(stats_dir)), total_ms=round(total / 1e6, 3),
                **{k: round(v / total, 4) for k, v in groups.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4, help="rounds per timed chunk")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_rrtstar.txt"))
    ap.add_argument("--quick", action="store_true", help="the small shapes only")
    ap.add_argument("--host-budget", type=float, default=1.5, help="seconds of host-route timing per round and shape")
    ap.add_argument("--problems", type=int, default=256, help="planning problems of the quality leg")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--profile-shape", default=None, help="R,P,K,tree: run this shape's fused chunks alone (for a kernel trace)")
    ap.add_argument("--state", default=None, help="with --profile-shape: the file that keeps the grown trees")
    ap.add_argument("--grow-only", action="store_true", help="with --profile-shape and --state: grow the trees, save them, stop")
    ap.add_argument("--shares", default=None, help="a kernel trace's output directory: print the grouped shares")
    ap.add_argument("--append", default=None, help="with --shares: append the line to this file")
    args = ap.parse_args()
    if args.shares:
        line = json.dumps(shares(args.shares))
        print(line)
        if args.append:
            with open(args.append, "a") as f:
                f.write(line + "\n")
        return
    import bench
    from diffco_amd import _lib, rrt, rrtstar, shortcut
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    w = bench.make_workload("headline", 1024, dev)
    m, lo, hi = w["model"], w["lo"].to(dev), w["hi"].to(dev)
    dof, T = len(lo), args.rounds
    limits = torch.stack([lo, hi], dim=1)
    lines = []

    class Checker:
        def check_motions(self, a, b, max_step=None, wrap=None, max_samples=None, return_first=False):
            first, _ = m.check_motions(a, b, max_step=max_step, max_samples=max_samples, wrap=wrap)
            return first >= 0, first

    class Fused(Checker):   # the headline model as a checker the fused planners take
        def _rrt_model(self, device=None):
            return m, 0.0

    ck = Checker()

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)

    def plan_of(R, P, K, cap, g):
        draw = lo + (hi - lo) * torch.rand((16 * R + 64, dof), generator=g, device=dev)
        draw = draw[m.check_motions(draw, draw, max_step=STEP, max_samples=2)[0] == -1]   # accepted configurations
        assert len(draw) >= 2 * R
        return rrtstar._StarPlan(ck, draw[:R], draw[R:2 * R], dev, RANGE, STEP, 2 * RANGE, K, None, P, cap, T, T, None, 0.0, limits, 0, None)

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
        return st, pl.max_samples

    def room(st, R, n, cap):
        big = blank(R, cap, st["nodes"][:, 0])
        for k in ("nodes", "parent", "elen", "cost"):
            big[k][:, :n] = st[k][:, :n]
        big["count"].fill_(n)
        return big

    def shape(R, P, K, n, g, st_n, max_samples, profile=False):
        cap = n + T * P
        pl = plan_of(R, P, K, cap, g)
        pl.max_samples = max_samples
        init = room(st_n, R, n, cap)
        samples = (lo + (hi - lo) * torch.rand((T, R, P, dof), generator=g, device=dev)).contiguous()
        st = {k: v.clone() for k, v in init.items()}
        edges = rrt._Edges(ck, STEP, max_samples, 0, 0.)

        def reset():
            for k in STATE:
                st[k].copy_(init[k])

        def fused():
            m.rrtstar_run(st, pl.goals, samples, 0, RANGE, STEP, pl.radius, K, max_samples)

        def host():
            for t in range(T):
                rrtstar._host_round(pl, edges, st, samples[t], t)

        if profile:
            for _ in range(50):
                reset()
                fused()
            torch.cuda.synchronize()
            return
        # the yardstick: RRT-Connect rounds at the same R and slots on two trees of these nodes
        cst = dict(nodes=torch.stack([init["nodes"], init["nodes"].flip(0)], dim=1).contiguous(),
                   parent=torch.stack([init["parent"].clamp(max=0)] * 2, dim=1).contiguous(),
                   count=torch.full((R, 2), n, dtype=torch.int32, device=dev), status=torch.zeros(R, dtype=torch.int32, device=dev),
                   link=torch.full((R, 2), -1, dtype=torch.int32, device=dev), solved_round=torch.full((R,), -1, dtype=torch.int32, device=dev))
        cinit = {k: v.clone() for k, v in cst.items()}

        def creset():
            for k in cst:
                cst[k].copy_(cinit[k])

        def connect():
            m.rrt_connect_run(cst, samples, 0, RANGE, STEP, max_samples, cap)

        reset()
        fused()
        after = {k: v.clone() for k, v in st.items()}
        reset()
        t0 = time.perf_counter()
        host()
        torch.cuda.synchronize()
        host_iters = max(2, min(args.iters, int(args.host_budget / max(time.perf_counter() - t0, 1e-4))))
        same = same_state(after, st)
        f3, h3, c3 = [], [], []
        for _ in range(3):
            f3.append(timed(fused, reset, args.iters) / T)
            c3.append(timed(connect, creset, args.iters) / T)
            h3.append(timed(host, reset, host_iters) / T)
        med = lambda xs: sorted(xs)[1]   # noqa: E731
        emit(dict(R=R, P=P, K=K, tree=n, cap=cap, dof=dof, rounds=T, range=RANGE, radius=pl.radius, max_step=STEP, max_samples=max_samples,
                  same_bits=same, appended=int((after["count"] - n).sum()),
                  reparented=int((after["parent"][:, :n] != init["parent"][:, :n]).sum()),
                  fused_us_per_round=round(med(f3), 1), fused_x3=[round(x, 1) for x in f3],
                  host_us_per_round=round(med(h3), 1), host_x3=[round(x, 1) for x in h3], host_iters=host_iters,
                  connect_us_per_round=round(med(c3), 1), connect_x3=[round(x, 1) for x in c3],
                  speedup=round(med(h3) / med(f3), 2), over_connect=round(med(f3) / med(c3), 2)))

    if args.profile_shape:
        R, P, K, n = (int(v) for v in args.profile_shape.split(","))
        g = torch.Generator(device=dev).manual_seed(n + R)
        if args.state and os.path.exists(args.state):
            st_n, ms = torch.load(args.state, map_location=dev)
        else:
            st_n, ms = grown(R, n, g)
            if args.state:
                torch.save((st_n, ms), args.state)
        if not args.grow_only:
            shape(R, P, K, n, g, st_n, ms, profile=True)
        return

    Rs, Ps, Ks, Ns = ((1, 32), (1, 4), (0, 8), (64,)) if args.quick else ((1, 32, 256), (1, 4, 8), (0, 8, 16), (64, 4096))
    for n in Ns:
        for R in Rs:
            g = torch.Generator(device=dev).manual_seed(n + R)
            st_n, ms = grown(R, n, g)
            for P in Ps:
                for K in Ks:
                    shape(R, P, K, n, g, st_n, ms)

    # ---- what it buys: path length at equal numbers of submitted edges per problem ---------------------------------------------
    if not args.no_quality:
        g = torch.Generator(device=dev).manual_seed(7)
        q = lo + (hi - lo) * torch.rand((8 * args.problems, dof), generator=g, device=dev)
        q = q[m.check_motions(q, q, max_step=STEP, max_samples=2)[0] == -1]
        R = min(args.problems, len(q) // 2)
        starts, goals = q[:R], q[R:2 * R]
        plan = rrt.rrt_connect(Fused(), starts, goals, range=RANGE, max_step=STEP, slots=4, cap=1024, max_rounds=256, limits=limits, seed=0)
        path, count = plan.path_tensor()
        bent = count >= 3   # (a direct solve, two waypoints, is every method's fixed point)
        connect_rounds = int(plan.rounds[bent.cpu()].max()) if bool(bent.any()) else 0
        for N in (16, 64, 256):
            budget = 68 * N
            star = rrtstar.rrt_star(Fused(), starts, goals, range=RANGE, max_step=STEP, radius=2 * RANGE, near=8, slots=4, cap=4 * N + 2,
                                    max_rounds=N, rounds_per_call=min(N, 64), limits=limits, seed=0, goal_bias=0.1)
            reached = bent & (star.goal_node >= 0)
            res = dict(quality=True, problems=R, not_direct=int(bent.sum()), star_rounds=N, edges_per_problem=budget,
                       star_reached=int(reached.sum()), connect_rounds=connect_rounds)
            rounds = (budget - 8 * connect_rounds) // 4
            if bool(reached.any()) and rounds >= 1:
                res["star_length"] = round(float(star.costs[reached].mean()), 4)
                res["shortcut_rounds"] = rounds
                for name, kw in (("partial", dict(partial=True)), ("vertex", {})):
                    out = shortcut.shortcut_paths(Fused(), path[reached].contiguous(), count[reached].contiguous(), max_step=STEP, slots=4,
                                                  rounds=rounds, seed=1, **kw)
                    res["connect_length"] = round(float(out.lengths_before.mean()), 4)
                    res["connect_" + name + "_length"] = round(float(out.lengths.mean()), 4)
            emit(res)

    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/rrtstar_bench.py: microseconds per round, medians of three interleaved rounds (MI355X, headline model);\n"
                    "# connect_*: one RRT-Connect round at the same R and slots; quality lines: mean path lengths at equal submitted edges\n"
                    + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
