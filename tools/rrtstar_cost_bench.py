"""Batched RRT* under clearance-weighted edge costs (ScoreModel.rrtstar_run_cost, dcx_rrtstar_run_cost) on the headline model:
what a clearance round costs against a length round (ScoreModel.rrtstar_run, whose code this objective leaves untouched) from
the same state in the same run, and what the objective buys: path length, peak score and clearance cost of the planners' paths,
all priced by rrtstar.clearance_cost_paths.

    python tools/rrtstar_cost_bench.py [--iters 10] [--rounds 4] [--out profiles/r26_rrtstar_clearance.txt] [--quick]

Timing: tools/rrtstar_bench.py's shapes and trees (grown by the length planner, K = 8, P = 8, until every tree holds `tree`
nodes, every problem kept running); microseconds per ROUND from HIP events around one chunk of --rounds rounds, every timed
chunk from the same state, the two legs interleaved in three rounds, the median of the three medians reported with the three.
gain0_same_bits: the clearance leg at gain 0 leaves the length leg's state.

Quality: the 256 problems of tools/rrtstar_bench.py's quality leg (accepted uniform configurations, seed 7), 256 rounds (slots
4, near 8).  The band is the median of -peak over the segments of the length planner's own paths, so about half of what that
planner considers a good edge is charged.  Routes: rrt_star under the length objective, under the clearance objective at two
gains, and rrt_connect + partial shortcuts at the same number of submitted edges per problem.  On the problems every route
solved with a bent path: the mean length, the mean peak of score - margin and the mean clearance cost at each gain.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from rrtstar_bench import RANGE, STATE, STEP, same_state, timed  # noqa: E402

GAINS = (1.0, 4.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4, help="rounds per timed chunk")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_rrtstar_clearance.txt"))
    ap.add_argument("--quick", action="store_true", help="the small shapes only")
    ap.add_argument("--problems", type=int, default=256, help="planning problems of the quality leg")
    ap.add_argument("--plan-rounds", type=int, default=256, help="rounds of the quality leg")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--no-timing", action="store_true")
    args = ap.parse_args()
    import bench
    from diffco_amd import _lib, rrt, rrtstar, shortcut
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    w = bench.make_workload("headline", 1024, dev)
    m, lo, hi = w["model"], w["lo"].to(dev), w["hi"].to(dev)
    dof, T = len(lo), args.rounds
    limits = torch.stack([lo, hi], dim=1)
    lines = []

    class Fused:   # the headline model as a checker the fused planners and the evaluator take
        def check_motions(self, a, b, max_step=None, wrap=None, max_samples=None, return_first=False):
            first, _ = m.check_motions(a, b, max_step=max_step, max_samples=max_samples, wrap=wrap)
            return first >= 0, first

        def motion_worst(self, a, b, max_step=None, wrap=None, max_samples=None):
            return m.motion_worst(a, b, max_step=max_step, max_samples=max_samples, wrap=wrap)

        def _rrt_model(self, device=None):
            return m, 0.0

    ck = Fused()

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)

    def accepted(n, g):
        q = lo + (hi - lo) * torch.rand((n, dof), generator=g, device=dev)
        return q[m.check_motions(q, q, max_step=STEP, max_samples=2)[0] == -1]

    def blank(R, cap, starts):
        st = dict(nodes=torch.zeros((R, cap, dof), device=dev), parent=torch.full((R, cap), -1, dtype=torch.int32, device=dev),
                  elen=torch.zeros((R, cap), device=dev), cost=torch.zeros((R, cap), device=dev),
                  count=torch.ones(R, dtype=torch.int32, device=dev), status=torch.zeros(R, dtype=torch.int32, device=dev),
                  goal_node=torch.full((R,), -1, dtype=torch.int32, device=dev),
                  first_round=torch.full((R,), -1, dtype=torch.int32, device=dev))
        st["nodes"][:, 0] = starts
        return st

    def shape(R, P, K, n, g, band):
        """trees of n nodes grown by the length planner, then T rounds of each objective from that state"""
        q = accepted(16 * R + 64, g)
        starts, far = q[:R], q[R:2 * R] + 100.0   # no sample ever equals a goal: every problem keeps running
        max_samples = rrtstar._StarPlan(ck, starts, q[R:2 * R], dev, RANGE, STEP, 2 * RANGE, K, None, P, 2, T, T, None, 0.0, limits, 0,
                                        None).max_samples
        cap = n + T * P
        full, g0 = blank(R, n, starts), 0   # cap = n: a tree stops at n nodes
        while bool((full["count"] < n).any()):
            smp = lo + (hi - lo) * torch.rand((64, R, 8, dof), generator=g, device=dev)
            full["status"].zero_()
            m.rrtstar_run(full, far, smp.contiguous(), g0, RANGE, STEP, 2 * RANGE, 8, max_samples)
            g0 += 64
            if g0 > 1 << 16:
                raise SystemExit("the trees do not grow")
        st = blank(R, cap, starts)   # ... and the timed chunks have room for every append
        for k in ("nodes", "parent", "elen", "cost"):
            st[k][:, :n] = full[k]
        st["count"].fill_(n)
        init = {k: v.clone() for k, v in st.items()}
        samples = (lo + (hi - lo) * torch.rand((T, R, P, dof), generator=g, device=dev)).contiguous()

        def reset():
            for k in STATE:
                st[k].copy_(init[k])

        def length():
            m.rrtstar_run(st, far, samples, 0, RANGE, STEP, 2 * RANGE, K, max_samples)

        def clearance(gain=GAINS[-1]):
            m.rrtstar_run_cost(st, far, samples, 0, RANGE, STEP, 2 * RANGE, K, max_samples, gain, band)

        reset()
        length()
        after = {k: v.clone() for k, v in st.items()}
        reset()
        clearance(0.0)
        same0 = same_state(after, st)
        reset()
        clearance()
        reparented = int((st["parent"][:, :n] != init["parent"][:, :n]).sum())
        l3, c3 = [], []
        for _ in range(3):
            l3.append(timed(length, reset, args.iters) / T)
            c3.append(timed(clearance, reset, args.iters) / T)
        med = lambda xs: sorted(xs)[1]   # noqa: E731
        emit(dict(R=R, P=P, K=K, tree=n, cap=cap, rounds=T, max_samples=max_samples, gain=GAINS[-1], band=band, gain0_same_bits=same0,
                  length_reparented=int((after["parent"][:, :n] != init["parent"][:, :n]).sum()), clearance_reparented=reparented,
                  length_us_per_round=round(med(l3), 1), length_x3=[round(x, 1) for x in l3],
                  clearance_us_per_round=round(med(c3), 1), clearance_x3=[round(x, 1) for x in c3], ratio=round(med(c3) / med(l3), 3)))

    # ---- the problems of the quality leg; the band from the length planner's own paths -----------------------------------------------
    g = torch.Generator(device=dev).manual_seed(7)
    q = accepted(8 * args.problems, g)
    R = min(args.problems, len(q) // 2)
    starts, goals = q[:R], q[R:2 * R]
    N = args.plan_rounds
    kw = dict(range=RANGE, max_step=STEP, radius=2 * RANGE, near=8, slots=4, cap=4 * N + 2, max_rounds=N, rounds_per_call=min(N, 64),
              limits=limits, seed=0, goal_bias=0.1)
    star = rrtstar.rrt_star(ck, starts, goals, **kw)
    path, count = star.path_tensor()
    seg = torch.arange(path.shape[1] - 1, device=dev)[None, :] + 1 < count[:, None]
    peaks = m.motion_worst(path[:, :-1][seg], path[:, 1:][seg], max_step=STEP)[0]
    band = round(float((-peaks).median()), 4)
    emit(dict(band=band, from_segments=int(seg.sum()), peak_min=round(float(peaks.min()), 4), peak_max=round(float(peaks.max()), 4)))

    if not args.no_timing:
        shapes = ((32, 4, 8, 64),) if args.quick else ((32, 4, 8, 64), (256, 4, 8, 64), (256, 8, 16, 64), (32, 4, 8, 4096), (256, 4, 8, 4096),
                                                       (256, 8, 16, 4096))
        for R_, P, K, n in shapes:
            shape(R_, P, K, n, torch.Generator(device=dev).manual_seed(n + R_), band)

    if not args.no_quality:
        routes = {"length": (path, count)}
        for gain in GAINS:
            routes[f"clearance_gain_{gain:g}"] = rrtstar.rrt_star(ck, starts, goals, objective="clearance", clearance_gain=gain,
                                                                  clearance_band=band, **kw).path_tensor()
        plan = rrt.rrt_connect(ck, starts, goals, range=RANGE, max_step=STEP, slots=4, cap=1024, max_rounds=256, limits=limits, seed=0)
        cpath, ccount = plan.path_tensor()
        bent = ccount >= 3
        connect_rounds = int(plan.rounds[bent.cpu()].max()) if bool(bent.any()) else 0
        rounds = max((68 * N - 8 * connect_rounds) // 4, 1)   # the same number of submitted edges per problem
        solved = ccount >= 2
        out = shortcut.shortcut_paths(ck, cpath[solved].contiguous(), ccount[solved].contiguous(), max_step=STEP, slots=4, rounds=rounds,
                                      seed=1, partial=True)
        spath = torch.zeros((R, out.path.shape[1], dof), device=dev)
        scount = torch.zeros(R, dtype=torch.int32, device=dev)
        spath[solved], scount[solved] = out.path, out.count.to(torch.int32)
        routes["connect_partial_shortcuts"] = (spath, scount)
        both = bent.clone()
        for p, c in routes.values():
            both &= c >= 2
        emit(dict(quality=True, problems=R, plan_rounds=N, compared=int(both.sum()), connect_rounds=connect_rounds, shortcut_rounds=rounds,
                  band=band))
        for name, (p, c) in routes.items():
            res = dict(route=name)
            for gain in GAINS:
                cost, length, peak = rrtstar.clearance_cost_paths(ck, p, c, max_step=STEP, gain=gain, band=band)
                res.update(mean_length=round(float(length[both].mean()), 4), mean_peak=round(float(peak[both].mean()), 4))
                res[f"mean_cost_gain_{gain:g}"] = round(float(cost[both].mean()), 4)
            emit(res)

    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/rrtstar_cost_bench.py (MI355X, headline model): microseconds per round of the length and the clearance objective,\n"
                    "# medians of three interleaved rounds; route lines: means over the problems every route solved, priced by clearance_cost_paths\n"
                    + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
