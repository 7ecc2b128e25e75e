"""Path shortcuts under the clearance objective (ScoreModel.shortcut_run(cost=, seg=); dcx_path_shortcut_run_cost and
dcx_path_shortcut_partial_run_cost) on the headline model: what a cost round takes against the length round of the same shape and
against the host composition of its own contract, and what the objective buys on planned paths.

    python tools/shortcut_clearance_bench.py [--iters 10] [--rounds 4] [--out profiles/r27_shortcut_clearance.txt] [--quick]
                                             [--reference-root DIR --reference-lib PATH]

Round time: tools/shortcut_bench.py's grid and paths - R in {1, 32, 256} paths x P in {1, 4, 8} slots x paths of {64, 512}
waypoints (W = waypoints + 16 in the partial mode), a straight motion between two uniform configurations, its waypoints shaken by
0.2 rad.  Microseconds per ROUND from HIP events around one chunk of --rounds rounds on an idle stream, every timed chunk from
the same state (restored outside the events); the legs - cost round, length round of the same mode, host composition of the cost
round - interleaved in three rounds, the median of the three medians reported with the three.  The cost round has no early exit
in its sweep (dcx_motion_worst visits every sample) and the partial one sweeps three edges per slot: over_length says what that
costs.  --reference-root / --reference-lib: a checkout of the reference commit (the parent of the change that added these
rounds) and its library (tools/build_variant.sh there, the headline width).  A second process with that package and that library
sets up the same shapes and times ITS length round whenever this process has timed its own legs - the same lease, interleaved
round by round - and the ratios are then taken against it: reference_length_us_per_round, over_reference, and
length_over_reference (this library's length round against the reference's: what sharing the pick and the compaction with the
cost kernels did to the length modes).  same_bits: the fused and the host leg leave the same path[:count], count, accepted and
seg[:count - 1].

Path quality: tools/rrtstar_cost_bench.py's 256 problems (accepted uniform configurations, seed 7) and its band (the median of
-peak over the segments of the length planner's own paths).  Routes: rrt_connect + partial length shortcuts (r26's row),
rrt_connect + partial clearance shortcuts at the same number of submitted edges (a third of the rounds: three edges per slot), the
clearance trees (rrt_star(objective="clearance"), gain 4; r26's row) and the clearance trees + partial clearance shortcuts.  On the
problems every route solved with a bent path: mean length, mean peak of score - margin and mean clearance cost at gain 4, all
priced by rrtstar.clearance_cost_paths."""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the reference's worker imports the reference's package and bench.py: its checkout goes in front of this one
_REF = sys.argv[sys.argv.index("--reference-root") + 1] if "--length-worker" in sys.argv and "--reference-root" in sys.argv else ROOT
sys.path.insert(0, _REF)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from rrtstar_bench import RANGE, STEP  # noqa: E402
from shortcut_bench import timed  # noqa: E402

GAIN = 4.0
STATE = ("path", "count", "accepted", "seg")


def same_state(a, b):
    if not (torch.equal(a["count"], b["count"]) and torch.equal(a["accepted"], b["accepted"])):
        return False
    bits = lambda t: t.contiguous().view(torch.int32)   # noqa: E731
    return all(bool(torch.equal(bits(a["path"][r, :n]), bits(b["path"][r, :n]))) and
               bool(torch.equal(bits(a["seg"][r, :max(n - 1, 0)]), bits(b["seg"][r, :max(n - 1, 0)])))
               for r, n in enumerate(a["count"].tolist()))


def grid(quick):
    return ((1, 32), (1, 4), (64,)) if quick else ((1, 32, 256), (1, 4, 8), (64, 512))


def shapes(quick):
    Rs, Ps, Ns = grid(quick)
    return [(partial, n, R, P) for partial in (False, True) for n in Ns for R in Rs for P in Ps]


def shape_inputs(lo, hi, n, R, P, T):
    """(waypoints [R, n, dof], counts, draws [T, R, P, 2]) of a shape: tools/shortcut_bench.py's paths, the same in every process"""
    dev, dof = lo.device, len(lo)
    gg = torch.Generator(device=dev).manual_seed(n + R + P)
    rand = lambda *shape: torch.rand(shape, generator=gg, device=dev)   # noqa: E731
    a, b = lo + (hi - lo) * rand(R, 1, dof), lo + (hi - lo) * rand(R, 1, dof)
    s = torch.linspace(0, 1, n, device=dev)[None, :, None]
    pts = (a + (b - a) * s + 0.2 * (2 * rand(R, n, dof) - 1)).contiguous()
    return pts, torch.full((R,), n, dtype=torch.int32, device=dev), rand(T, R, P, 2).contiguous()


def sampling(lo, hi):
    step = 0.25   # tools/shortcut_bench.py's stride and bound
    return step, int(torch.ceil(((hi - lo).norm() + 0.4 * len(lo) ** 0.5) / step)) + 2


def length_worker(args):
    """the reference's leg: per shape one line "ready <applied>" once its state stands, then one line of microseconds per round
    for every "t" read, anything else for the next shape"""
    sys.path.insert(0, os.path.abspath(args.reference_root))   # (in front of what the tools imported above put there)
    import bench
    from diffco_amd import _lib, shortcut
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    w = bench.make_workload("headline", 1024, dev)
    m, lo, hi = w["model"], w["lo"].to(dev), w["hi"].to(dev)
    T = args.rounds
    step, max_samples = sampling(lo, hi)

    class Checker:
        def check_motions(self, a, b, max_step=None, wrap=None, max_samples=None, return_first=False):
            first, _ = m.check_motions(a, b, max_step=max_step, max_samples=max_samples, wrap=wrap)
            return first >= 0, first

    for partial, n, R, P in shapes(args.quick):
        pts, cnt, draws = shape_inputs(lo, hi, n, R, P, T)
        pl = shortcut._Pass(Checker(), pts, cnt, dev, step, None, P, T, T, None, 0, max_samples, None, partial, None)
        init = {k: v.clone() for k, v in pl.st.items()}

        def reset():
            for k in STATE[:3]:
                pl.st[k].copy_(init[k])

        def length():
            m.shortcut_run(pl.st, draws, step, max_samples, partial=partial)

        reset()
        length()
        torch.cuda.synchronize()
        print("ready", int(pl.st["accepted"].sum()), flush=True)
        while True:
            line = sys.stdin.readline()
            if not line:
                return
            if line.strip() != "t":
                break
            print(timed(length, reset, args.iters) / T, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4, help="rounds per timed chunk")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_shortcut_clearance.txt"))
    ap.add_argument("--quick", action="store_true", help="the small shapes only")
    ap.add_argument("--problems", type=int, default=256, help="planning problems of the quality leg")
    ap.add_argument("--plan-rounds", type=int, default=256, help="rounds of the quality leg's trees")
    ap.add_argument("--host-budget", type=float, default=0.5, help="seconds of host-route timing per round and shape")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--reference-root", default=None, help="a checkout of the reference commit (its diffco_amd and bench.py)")
    ap.add_argument("--reference-lib", default=None, help="the reference commit's library")
    ap.add_argument("--length-worker", action="store_true", help="(internal) the reference's leg, driven over stdin / stdout")
    args = ap.parse_args()
    if args.length_worker:
        return length_worker(args)
    import bench
    from diffco_amd import _lib, rrt, rrtstar, shortcut
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    w = bench.make_workload("headline", 1024, dev)
    m, lo, hi = w["model"], w["lo"].to(dev), w["hi"].to(dev)
    dof, T = len(lo), args.rounds
    limits = torch.stack([lo, hi], dim=1)
    lines = []
    med = lambda xs: sorted(xs)[1]   # noqa: E731

    class Fused:   # the headline model as a checker the fused planners, the fused passes and the evaluator take
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
        if args.out:
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("# tools/shortcut_clearance_bench.py (MI355X, headline model): microseconds per round, medians of three interleaved\n"
                        "# rounds; route lines: means over the problems every route solved with a bent path, priced by clearance_cost_paths\n"
                        + ("# reference_*: the length round of the reference commit's library in a second process, timed between this\n"
                           "# process's legs; over_reference = cost round / reference length round\n" if args.reference_lib else
                           "# no reference library given: over_length is against this library's own length round\n")
                        + "\n".join(lines) + "\n")

    def accepted(n, g):
        q = lo + (hi - lo) * torch.rand((n, dof), generator=g, device=dev)
        return q[m.check_motions(q, q, max_step=STEP, max_samples=2)[0] == -1]

    # ---- the problems of the quality leg; the band from the length planner's own paths, as r26 takes it ---------------------------
    g = torch.Generator(device=dev).manual_seed(7)
    q = accepted(8 * args.problems, g)
    Rq = min(args.problems, len(q) // 2)
    starts, goals = q[:Rq], q[Rq:2 * Rq]
    N = args.plan_rounds
    kw = dict(range=RANGE, max_step=STEP, radius=2 * RANGE, near=8, slots=4, cap=4 * N + 2, max_rounds=N, rounds_per_call=min(N, 64),
              limits=limits, seed=0, goal_bias=0.1)
    star = rrtstar.rrt_star(ck, starts, goals, **kw)
    path, count = star.path_tensor()
    live = torch.arange(path.shape[1] - 1, device=dev)[None, :] + 1 < count[:, None]
    peaks = m.motion_worst(path[:, :-1][live], path[:, 1:][live], max_step=STEP)[0]
    band = round(float((-peaks).median()), 4)
    emit(dict(band=band, gain=GAIN, from_segments=int(live.sum()), peak_min=round(float(peaks.min()), 4),
              peak_max=round(float(peaks.max()), 4)))

    if not args.no_timing:
        step, max_samples = sampling(lo, hi)
        obj = rrtstar._objective("bench", "clearance", GAIN, band)
        ref = None
        if args.reference_lib:
            cmd = [sys.executable, os.path.abspath(__file__), "--length-worker", "--reference-root", os.path.abspath(args.reference_root),
                   "--iters", str(args.iters), "--rounds", str(T)] + (["--quick"] if args.quick else [])
            ref = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1,
                                   env=dict(os.environ, DCX_LIB=os.path.abspath(args.reference_lib)))

        def ask(word=None):
            if word is not None:
                ref.stdin.write(word + "\n")
                ref.stdin.flush()
            line = ref.stdout.readline()
            if not line:
                raise SystemExit("the reference's worker ended")
            return line.split()

        for at, (partial, n, R, P) in enumerate(shapes(args.quick)):
            pts, cnt, draws = shape_inputs(lo, hi, n, R, P, T)
            mk = lambda o: shortcut._Pass(ck, pts, cnt, dev, step, None, P, T, T, None, 0, max_samples, None, partial, None, o)   # noqa: E731
            pc, pl = mk(obj), mk(None)
            peaks_of = rrtstar._PeakEdges("bench", ck, step, max_samples, 0, 0.)
            pc.form_seg(rrtstar._FusedPeakEdges(m, step, max_samples, 0, 0.))
            init_c, init_l = {k: v.clone() for k, v in pc.st.items()}, {k: v.clone() for k, v in pl.st.items()}
            one_round = shortcut._host_round_partial_cost if partial else shortcut._host_round_cost

            def reset():
                for k in STATE:
                    pc.st[k].copy_(init_c[k])
                for k in STATE[:3]:
                    pl.st[k].copy_(init_l[k])

            def cost():
                m.shortcut_run({k: pc.st[k] for k in STATE[:3]}, draws, step, max_samples, partial=partial,
                               cost=(GAIN, band), seg=pc.st["seg"])

            def length():
                m.shortcut_run(pl.st, draws, step, max_samples, partial=partial)

            def host():
                for t in range(T):
                    one_round(pc, peaks_of, draws[t])

            reset()
            cost()
            after = {k: v.clone() for k, v in pc.st.items()}
            reset()
            host()
            torch.cuda.synchronize()
            same = same_state(after, pc.st)
            reset()
            length()
            applied_length = int(pl.st["accepted"].sum())
            reset()
            t0 = time.perf_counter()
            host()
            torch.cuda.synchronize()
            host_iters = max(2, min(args.iters, int(args.host_budget / max(time.perf_counter() - t0, 1e-4))))
            ref_applied = int(ask("n" if at else None)[1]) if ref else None   # (the worker's state of this shape stands)
            c3, l3, h3, r3 = [], [], [], []
            for _ in range(3):
                c3.append(timed(cost, reset, args.iters) / T)
                l3.append(timed(length, reset, args.iters) / T)
                h3.append(timed(host, reset, host_iters) / T)
                if ref:
                    r3.append(float(ask("t")[0]))
            res = dict(partial=partial, R=R, P=P, waypoints=n, W=int(pc.W), dof=dof, rounds=T, max_step=step,
                       max_samples=max_samples, same_bits=same, applied=int(after["accepted"].sum()),
                       applied_length=applied_length, unfree_segments=int(torch.isinf(init_c["seg"][:, :n - 1]).sum()),
                       cost_us_per_round=round(med(c3), 1), cost_x3=[round(x, 1) for x in c3],
                       length_us_per_round=round(med(l3), 1), length_x3=[round(x, 1) for x in l3],
                       host_us_per_round=round(med(h3), 1), host_x3=[round(x, 1) for x in h3], host_iters=host_iters,
                       over_length=round(med(c3) / med(l3), 2), speedup=round(med(h3) / med(c3), 2))
            if ref:
                res.update(reference_length_us_per_round=round(med(r3), 1), reference_length_x3=[round(x, 1) for x in r3],
                           reference_applied=ref_applied, over_reference=round(med(c3) / med(r3), 2),
                           length_over_reference=round(med(l3) / med(r3), 3))
            emit(res)
        if ref:
            ref.stdin.close()
            ref.wait(timeout=60)

    if not args.no_quality:
        plan = rrt.rrt_connect(ck, starts, goals, range=RANGE, max_step=STEP, slots=4, cap=1024, max_rounds=256, limits=limits, seed=0)
        cpath, ccount = plan.path_tensor()
        bent = ccount >= 3
        connect_rounds = int(plan.rounds[bent.cpu()].max()) if bool(bent.any()) else 0
        rounds = max((68 * N - 8 * connect_rounds) // 4, 1)   # r26's: the trees' number of submitted edges per problem
        trees = rrtstar.rrt_star(ck, starts, goals, objective="clearance", clearance_gain=GAIN, clearance_band=band, **kw)
        tpath, tcount = trees.path_tensor()
        cost_kw = dict(objective="clearance", clearance_gain=GAIN, clearance_band=band)

        def shortened(p, c, rounds, **more):
            ok = c >= 2
            out = shortcut.shortcut_paths(ck, p[ok].contiguous(), c[ok].contiguous(), max_step=STEP, slots=4, rounds=rounds, seed=1,
                                          partial=True, **more)
            sp = torch.zeros((len(p), out.path.shape[1], dof), device=dev)
            sc = torch.zeros(len(p), dtype=torch.int32, device=dev)
            sp[ok], sc[ok] = out.path, out.count.to(torch.int32)
            return sp, sc, out

        routes = {}
        routes["connect_partial_length_shortcuts"] = shortened(cpath, ccount, rounds)[:2]
        sp, sc, out = shortened(cpath, ccount, max(rounds // 3, 1), **cost_kw)
        routes["connect_partial_clearance_shortcuts"] = (sp, sc)
        emit(dict(clearance_shortcut_rounds=max(rounds // 3, 1), applied=int(out.accepted.sum()), route=out.route,
                  rows_with_an_unfree_segment=int(torch.isinf(out.costs).sum())))
        routes["clearance_trees"] = (tpath, tcount)
        sp, sc, out = shortened(tpath, tcount, max(rounds // 3, 1), **cost_kw)
        routes["clearance_trees_partial_clearance_shortcuts"] = (sp, sc)
        both = bent.clone()
        for p, c in routes.values():
            both &= c >= 2
        emit(dict(quality=True, problems=Rq, plan_rounds=N, compared=int(both.sum()), connect_rounds=connect_rounds,
                  length_shortcut_rounds=rounds, clearance_shortcut_rounds=max(rounds // 3, 1), band=band, gain=GAIN))
        for name, (p, c) in routes.items():
            cost, length, peak = rrtstar.clearance_cost_paths(ck, p, c, max_step=STEP, gain=GAIN, band=band)
            emit(dict(route=name, mean_length=round(float(length[both].mean()), 4), mean_peak=round(float(peak[both].mean()), 4),
                      mean_cost_gain_4=round(float(cost[both].mean()), 4), waypoints=round(float(c[both].float().mean()), 2)))


if __name__ == "__main__":
    main()
