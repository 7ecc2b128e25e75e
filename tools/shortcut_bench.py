"""Batched path shortcutting: the fused rounds (ScoreModel.shortcut_run, dcx_path_shortcut_run) against the host composition of
the same contract (shortcut.host_shortcut_paths' round: torch indexing, one check_motions call) on the same GPU, on the headline
model; and the device-side path extraction (dcx_rrt_extract_paths) against the host walk of the parents.

    python tools/shortcut_bench.py [--iters 10] [--rounds 4] [--out profiles/r17_shortcut.txt] [--quick]

Shapes: R in {1, 32, 256} paths x P in {1, 4, 8} slots x paths of {64, 512} waypoints (a straight motion between two uniform
configurations in the joint limits, its waypoints shaken by 0.2 rad).  Microseconds per ROUND from HIP events around one chunk
of --rounds rounds on an idle stream, every timed chunk starting from the same state (restored outside the events); the two
legs interleaved in three rounds, the median of the three medians reported with the three.  same_bits: the two legs leave the
same path[:count], count and accepted.  floor: ONE plain check_motions call on the R * P edges of the first round - what a round
cannot beat.  Extraction: 256 solved problems, two chains of --depth nodes each, one launch against the host walk (the parents
copied to the host, one int() per node, as RRTResult.paths).

    python tools/shortcut_bench.py --partial [--out profiles/r20_shortcut_partial.txt]

The partial mode (dcx_path_shortcut_partial_run) on the same grid, W = waypoints + 16: a fused partial round against the host
composition of its contract (shortcut._host_round_partial) and against a fused vertex round at the same shape; floor: ONE plain
check_motions call on the edges of the first partial round, and beside_sweep = 1 - floor / fused, the share of a round that the
pick and commit launches (and the call's host side) take beside the motion sweep.  Then what it buys: --problems planning
problems between accepted uniform configurations solved by rrt_connect, their paths shortened by shortcut_paths with
partial=True, partial=False and partial=False, subdivide=4 * max_step - 4 slots, the same seed, the mean length of the paths of
three waypoints or more (a direct solve is a fixed point of all three) after equal numbers of rounds, that is of submitted edges."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STATE = ("path", "count", "accepted")


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
    if not (torch.equal(a["count"], b["count"]) and torch.equal(a["accepted"], b["accepted"])):
        return False
    return all(bool(torch.equal(a["path"][r, :n].contiguous().view(torch.int32), b["path"][r, :n].contiguous().view(torch.int32)))
               for r, n in enumerate(a["count"].tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4, help="rounds per timed chunk")
    ap.add_argument("--depth", type=int, default=64, help="nodes per chain of the extraction's problems")
    ap.add_argument("--out", default=None, help="default: profiles/r17_shortcut.txt, with --partial profiles/r20_shortcut_partial.txt")
    ap.add_argument("--partial", action="store_true", help="the partial mode's legs instead of the vertex mode's")
    ap.add_argument("--problems", type=int, default=256, help="planning problems of the partial mode's outcome leg")
    ap.add_argument("--quick", action="store_true", help="the small shapes only")
    ap.add_argument("--host-budget", type=float, default=3.0, help="seconds of host-route timing per round and shape")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "r20_shortcut_partial.txt" if args.partial else "r17_shortcut.txt")
    import bench
    from diffco_amd import _lib, _ops, rrt, shortcut
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    w = bench.make_workload("headline", 1024, dev)
    m, lo, hi = w["model"], w["lo"].to(dev), w["hi"].to(dev)
    dof, T, step = len(lo), args.rounds, 0.25
    # no straight motion between two waypoints is longer than the box's diagonal plus the shake
    max_samples = int(torch.ceil(((hi - lo).norm() + 0.4 * dof ** 0.5) / step)) + 2
    lines = []

    class Checker:
        def check_motions(self, a, b, max_step=None, wrap=None, max_samples=None, return_first=False):
            first, _ = m.check_motions(a, b, max_step=max_step, max_samples=max_samples, wrap=wrap)
            return first >= 0, first

    ck = Checker()
    med = lambda xs: sorted(xs)[1]   # noqa: E731

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)

    Rs, Ps, Ns = ((1, 32), (1, 4), (64,)) if args.quick else ((1, 32, 256), (1, 4, 8), (64, 512))
    if args.partial:
        partial_legs(args, m, lo, hi, ck, max_samples, (Rs, Ps, Ns), emit)
        Ns = ()
    for n in Ns:
        for R in Rs:
            for P in Ps:
                g = torch.Generator(device=dev).manual_seed(n + R + P)
                rand = lambda *shape: torch.rand(shape, generator=g, device=dev)   # noqa: E731
                a, b = lo + (hi - lo) * rand(R, 1, dof), lo + (hi - lo) * rand(R, 1, dof)
                s = torch.linspace(0, 1, n, device=dev)[None, :, None]
                path = (a + (b - a) * s + 0.2 * (2 * rand(R, n, dof) - 1)).contiguous()
                init = dict(path=path, count=torch.full((R,), n, dtype=torch.int32, device=dev),
                            accepted=torch.zeros(R, dtype=torch.int32, device=dev))
                draws = rand(T, R, P, 2).contiguous()
                ps = shortcut._Pass(ck, path, init["count"], dev, step, None, P, T, T, None, 0, max_samples, None)
                st = ps.st
                edges = rrt._Edges(ck, step, max_samples, 0, 0.)
                i, j, live = shortcut._pick(init["count"], draws[0])
                rows = torch.arange(R, device=dev)[:, None]
                qa, qb = path[rows, i].reshape(-1, dof).contiguous(), path[rows, j].reshape(-1, dof).contiguous()

                def reset():
                    for k in STATE:
                        st[k].copy_(init[k])

                def fused():
                    m.shortcut_run(st, draws, step, max_samples)

                def host():
                    for t in range(T):
                        shortcut._host_round(ps, edges, draws[t])

                def floor():
                    m.check_motions(qa, qb, max_step=step, max_samples=max_samples)

                reset()
                fused()
                after = {k: v.clone() for k, v in st.items()}
                reset()
                host()
                torch.cuda.synchronize()
                same = same_state(after, st)
                reset()
                t0 = time.perf_counter()
                host()
                torch.cuda.synchronize()
                host_iters = max(2, min(args.iters, int(args.host_budget / max(time.perf_counter() - t0, 1e-4))))
                f3, h3, c3 = [], [], []
                for _ in range(3):
                    f3.append(timed(fused, reset, args.iters) / T)
                    h3.append(timed(host, reset, host_iters) / T)
                    c3.append(timed(floor, reset, args.iters))
                emit(dict(R=R, P=P, waypoints=n, dof=dof, rounds=T, max_step=step, max_samples=max_samples, same_bits=same,
                          applied=int(after["accepted"].sum()), removed=int((init["count"] - after["count"]).sum()),
                          fused_us_per_round=round(med(f3), 1), fused_x3=[round(x, 1) for x in f3],
                          host_us_per_round=round(med(h3), 1), host_x3=[round(x, 1) for x in h3], host_iters=host_iters,
                          floor_us=round(med(c3), 1), floor_x3=[round(x, 1) for x in c3],
                          speedup=round(med(h3) / med(f3), 2), over_floor=round(med(f3) / med(c3), 2)))

    if args.partial:
        write(args.out, lines)
        return

    # ---- the extraction: 256 solved problems, each tree one chain of `depth` nodes -------------------------------------------
    R, depth = 256, args.depth
    cap = depth + 8
    g = torch.Generator(device=dev).manual_seed(1)
    state = dict(nodes=torch.zeros((R, 2, cap, dof), device=dev), parent=torch.full((R, 2, cap), -1, dtype=torch.int32, device=dev),
                 count=torch.full((R, 2), depth, dtype=torch.int32, device=dev), status=torch.ones(R, dtype=torch.int32, device=dev),
                 link=torch.full((R, 2), depth - 1, dtype=torch.int32, device=dev),
                 solved_round=torch.zeros(R, dtype=torch.int32, device=dev))
    state["nodes"][:, :, :depth] = lo + (hi - lo) * torch.rand((R, 2, depth, dof), generator=g, device=dev)
    state["parent"][:, :, 1:depth] = torch.arange(depth - 1, dtype=torch.int32, device=dev)
    W = 2 * depth
    got = {}

    def device_walk():
        got["path"], got["count"] = _ops.rrt_extract_paths(state, W)

    def host_walk():
        parent, link = state["parent"].cpu(), state["link"].tolist()
        got["rows"] = [rrt._walk(state["nodes"], parent, link[r], r) for r in range(R)]

    device_walk()
    host_walk()
    torch.cuda.synchronize()
    same = got["count"].tolist() == [W] * R and all(bool(torch.equal(got["path"][r], got["rows"][r])) for r in range(R))
    d3, w3 = [], []
    for _ in range(3):
        d3.append(timed(device_walk, lambda: None, args.iters))
        t0 = time.perf_counter()
        host_walk()
        torch.cuda.synchronize()
        w3.append((time.perf_counter() - t0) * 1e6)
    emit(dict(extract=True, R=R, waypoints=W, dof=dof, same_bits=same, device_us=round(med(d3), 1), device_x3=[round(x, 1) for x in d3],
              host_walk_us=round(med(w3), 1), host_walk_x3=[round(x, 1) for x in w3], speedup=round(med(w3) / med(d3), 1)))
    write(args.out, lines)


def write(out, lines):
    if out:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            f.write("# tools/shortcut_bench.py: microseconds per round, medians of three interleaved rounds (MI355X, headline model)\n"
                    + "\n".join(lines) + "\n")


def partial_legs(args, m, lo, hi, ck, max_samples, grid, emit):
    from diffco_amd import rrt, shortcut
    dev, dof, T, step = lo.device, len(lo), args.rounds, 0.25
    med = lambda xs: sorted(xs)[1]   # noqa: E731

    class Keeping:   # the edges of the batches it is asked about
        def __init__(self):
            self.batches = []

        def check_motions(self, a, b, **kw):
            self.batches.append((a.clone(), b.clone()))
            return ck.check_motions(a, b, **kw)

    for n in grid[2]:
        for R in grid[0]:
            for P in grid[1]:
                g = torch.Generator(device=dev).manual_seed(n + R + P)
                rand = lambda *shape: torch.rand(shape, generator=g, device=dev)   # noqa: E731
                a, b = lo + (hi - lo) * rand(R, 1, dof), lo + (hi - lo) * rand(R, 1, dof)
                s = torch.linspace(0, 1, n, device=dev)[None, :, None]
                path = (a + (b - a) * s + 0.2 * (2 * rand(R, n, dof) - 1)).contiguous()
                count = torch.full((R,), n, dtype=torch.int32, device=dev)
                draws = rand(T, R, P, 2).contiguous()
                pv = shortcut._Pass(ck, path, count, dev, step, None, P, T, T, None, 0, max_samples, None)
                pp = shortcut._Pass(ck, path, count, dev, step, None, P, T, T, None, 0, max_samples, None, True, None)
                init_v, init_p = {k: v.clone() for k, v in pv.st.items()}, {k: v.clone() for k, v in pp.st.items()}
                edges = rrt._Edges(ck, step, max_samples, 0, 0.)
                kept = Keeping()
                shortcut._host_round_partial(pp, rrt._Edges(kept, step, max_samples, 0, 0.), draws[0])
                qa, qb = kept.batches[0]

                def reset():
                    for k in STATE:
                        pv.st[k].copy_(init_v[k])
                        pp.st[k].copy_(init_p[k])

                def fused():
                    m.shortcut_run(pp.st, draws, step, max_samples, partial=True)

                def vertex():
                    m.shortcut_run(pv.st, draws, step, max_samples)

                def host():
                    for t in range(T):
                        shortcut._host_round_partial(pp, edges, draws[t])

                def floor():
                    m.check_motions(qa, qb, max_step=step, max_samples=max_samples)

                reset()
                fused()
                after = {k: v.clone() for k, v in pp.st.items()}
                reset()
                host()
                torch.cuda.synchronize()
                same = same_state(after, pp.st)
                reset()
                t0 = time.perf_counter()
                host()
                torch.cuda.synchronize()
                host_iters = max(2, min(args.iters, int(args.host_budget / max(time.perf_counter() - t0, 1e-4))))
                f3, v3, h3, c3 = [], [], [], []
                for _ in range(3):
                    f3.append(timed(fused, reset, args.iters) / T)
                    v3.append(timed(vertex, reset, args.iters) / T)
                    h3.append(timed(host, reset, host_iters) / T)
                    c3.append(timed(floor, reset, args.iters))
                emit(dict(partial=True, R=R, P=P, waypoints=n, W=int(pp.W), dof=dof, rounds=T, max_step=step, max_samples=max_samples,
                          same_bits=same, applied=int(after["accepted"].sum()), count_change=int((after["count"] - init_p["count"]).sum()),
                          fused_us_per_round=round(med(f3), 1), fused_x3=[round(x, 1) for x in f3],
                          vertex_us_per_round=round(med(v3), 1), vertex_x3=[round(x, 1) for x in v3],
                          host_us_per_round=round(med(h3), 1), host_x3=[round(x, 1) for x in h3], host_iters=host_iters,
                          floor_us=round(med(c3), 1), floor_x3=[round(x, 1) for x in c3],
                          speedup=round(med(h3) / med(f3), 2), over_vertex=round(med(f3) / med(v3), 2),
                          beside_sweep=round(1 - med(c3) / med(f3), 3)))

    # ---- what it buys: planned paths, the three ways to shorten them, equal numbers of submitted edges -----------------------
    class Fused:   # the headline model as a checker the fused planner and the fused passes take
        check_motions = staticmethod(ck.check_motions)

        def _rrt_model(self, device=None):
            return m, 0.0

    g = torch.Generator(device=dev).manual_seed(7)
    q = lo + (hi - lo) * torch.rand((8 * args.problems, dof), generator=g, device=dev)
    q = q[m.check_motions(q, q, max_step=step, max_samples=2)[0] == -1]
    R = min(args.problems, len(q) // 2)
    plan = rrt.rrt_connect(Fused(), q[:R], q[R:2 * R], range=1.0, max_step=step, slots=4, cap=1024, max_rounds=256,
                           limits=torch.stack([lo, hi], dim=1), seed=0)
    path, count = plan.path_tensor()
    solved, bent = count >= 2, count >= 3   # (a direct solve, two waypoints, is a fixed point of all three)
    path, count = path[bent].contiguous(), count[bent].contiguous()
    for rounds in (4, 16, 64):
        res = dict(outcome=True, problems=R, solved=int(solved.sum()), direct=int((solved & ~bent).sum()), paths=len(count), slots=4,
                   rounds=rounds,
                   edges_per_path=4 * rounds, max_step=step, waypoints_before=round(float(count.float().mean()), 2))
        for name, kw in (("partial", dict(partial=True)), ("vertex", {}), ("vertex_subdivided", dict(subdivide=4 * step))):
            out = shortcut.shortcut_paths(Fused(), path, count, max_step=step, slots=4, rounds=rounds, seed=1, **kw)
            res["length_before"] = round(float(out.lengths_before.mean()), 4)
            res[name] = dict(route=out.route, length=round(float(out.lengths.mean()), 4), waypoints=round(float(out.count.float().mean()), 2),
                             applied=int(out.accepted.sum()), W=int(out.path.shape[1]))
        emit(res)


if __name__ == "__main__":
    main()
