"""Batched RRT-Connect: the fused rounds (ScoreModel.rrt_connect_run, dcx_rrt_connect_run) against the host composition of the
same contract (rrt.host_rrt_connect's round: roadmap.knn per tree, torch arithmetic, one check_motions call per phase) on the
same GPU, on the headline model.

    python tools/rrt_bench.py [--iters 10] [--rounds 4] [--out profiles/r16_rrt.txt] [--quick]

Shapes: R in {1, 32, 256} problems x P in {1, 4, 8} slots x pre-grown trees of {64, 1024, 4096} nodes (uniform configurations
in the joint limits, chained parents; cap leaves room for every append of a chunk).  Microseconds per ROUND from HIP events
around one chunk of --rounds rounds on an idle stream, every timed chunk starting from the same state (restored outside the
events); the two legs interleaved in three rounds, the median of the three medians reported with the three.  same_bits: the
two legs leave the same state.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STATE = ("nodes", "parent", "count", "status", "link", "solved_round")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4, help="rounds per timed chunk")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_rrt.txt"))
    ap.add_argument("--quick", action="store_true", help="the small shapes only")
    ap.add_argument("--host-budget", type=float, default=4.0, help="seconds of host-route timing per round and shape")
    args = ap.parse_args()
    import bench
    from diffco_amd import _lib, rrt
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    w = bench.make_workload("headline", 1024, dev)
    m, lo, hi = w["model"], w["lo"].to(dev), w["hi"].to(dev)
    dof, T, reach, step = len(lo), args.rounds, 1.0, 0.25
    limits = torch.stack([lo, hi], dim=1)
    lines = []

    class Checker:
        def check_motions(self, a, b, max_step=None, wrap=None, max_samples=None, return_first=False):
            first, _ = m.check_motions(a, b, max_step=max_step, max_samples=max_samples, wrap=wrap)
            return first >= 0, first

    ck = Checker()

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)

    Rs, Ps, Ns = ((1, 32), (1, 4), (64, 1024)) if args.quick else ((1, 32, 256), (1, 4, 8), (64, 1024, 4096))
    for n in Ns:
        for R in Rs:
            for P in Ps:
                cap = n + 2 * T * P
                g = torch.Generator(device=dev).manual_seed(n + R + P)
                draw = lambda *shape: lo + (hi - lo) * torch.rand(shape + (dof,), generator=g, device=dev)   # noqa: E731
                pl = rrt._Plan(ck, draw(R), draw(R), dev, reach, step, None, P, cap, T, T, None, limits, 0, None)
                init = dict(nodes=torch.zeros((R, 2, cap, dof), device=dev), parent=torch.full((R, 2, cap), -1, dtype=torch.int32, device=dev),
                            count=torch.full((R, 2), n, dtype=torch.int32, device=dev), status=torch.zeros(R, dtype=torch.int32, device=dev),
                            link=torch.full((R, 2), -1, dtype=torch.int32, device=dev),
                            solved_round=torch.full((R,), -1, dtype=torch.int32, device=dev))
                init["nodes"][:, :, :n] = draw(R, 2, n)
                init["parent"][:, :, 1:n] = torch.arange(n - 1, dtype=torch.int32, device=dev)
                samples = draw(T, R, P).contiguous()
                st = {k: v.clone() for k, v in init.items()}
                edges = rrt._Edges(ck, step, pl.max_samples, 0, 0.)

                def reset():
                    for k in STATE:
                        st[k].copy_(init[k])

                def fused():
                    m.rrt_connect_run(st, samples, 0, reach, step, pl.max_samples, cap)

                def host():
                    for t in range(T):
                        rrt._host_round(pl, edges, st, samples[t], t)

                reset()
                fused()
                after = {k: v.clone() for k, v in st.items()}
                reset()
                host()
                torch.cuda.synchronize()
                same = all(bool(torch.equal(after[k].view(torch.int32) if k == "nodes" else after[k],
                                            st[k].view(torch.int32) if k == "nodes" else st[k])) for k in STATE)
                reset()
                t0 = time.perf_counter()
                host()
                torch.cuda.synchronize()
                host_iters = max(2, min(args.iters, int(args.host_budget / max(time.perf_counter() - t0, 1e-4))))
                f3, h3 = [], []
                for _ in range(3):
                    f3.append(timed(fused, reset, args.iters) / T)
                    h3.append(timed(host, reset, host_iters) / T)
                med = lambda xs: sorted(xs)[1]   # noqa: E731
                emit(dict(R=R, P=P, tree=n, cap=cap, dof=dof, rounds=T, range=reach, max_step=step, max_samples=pl.max_samples,
                          same_bits=same, appended=int((after["count"] - n).sum()), solved=int((after["status"] == 1).sum()),
                          fused_us_per_round=round(med(f3), 1), fused_x3=[round(x, 1) for x in f3],
                          host_us_per_round=round(med(h3), 1), host_x3=[round(x, 1) for x in h3], host_iters=host_iters,
                          speedup=round(med(h3) / med(f3), 2)))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/rrt_bench.py: microseconds per round, medians of three interleaved rounds (MI355X, headline model)\n"
                    + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
