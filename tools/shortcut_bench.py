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
copied to the host, one int() per node, as RRTResult.paths)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_shortcut.txt"))
    ap.add_argument("--quick", action="store_true", help="the small shapes only")
    ap.add_argument("--host-budget", type=float, default=3.0, help="seconds of host-route timing per round and shape")
    args = ap.parse_args()
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
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/shortcut_bench.py: microseconds per round, medians of three interleaved rounds (MI355X, headline model)\n"
                    + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
