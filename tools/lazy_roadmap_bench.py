"""Lazy roadmaps on the headline model: Roadmap.build(lazy=True) + query_batch (the fused calls _ops.sssp_mark_routes and
_ops.graph_apply_checks between full relaxations) against the eager Roadmap.build + query_batch on the same nodes - the code path
lazy=False leaves as it was - with the plain fused checker and with a hybrid one whose ground truth is synthetic.

    python tools/lazy_roadmap_bench.py [--repeats 3] [--out profiles/r22_lazy_roadmap.txt] [--quick]

The roadmap: N = 65536 collision-free samples (4096 with --quick), k = 16, max_step 0.05, max_dist 1.0 - tools/sssp_bench.py's.
Q in {1, 64, 256} pairs of free configurations.  Times are wall clock around synchronised calls, microseconds, the median of
`repeats` runs, each lazy run from all-unknown edges (Roadmap.invalidate).  Per checker and Q:
  eager_build_us / eager_query_us   Roadmap.build (every candidate edge checked) with csr(), and query_batch on it
  lazy_build_us / lazy_query_us     Roadmap.build(lazy=True) (no edge checked) with csr() and its index arrays, and query_batch,
                                    its whole loop, uninstrumented.  Builds: the median of `repeats` after one uncounted round
  iters, checked, M                 relax-and-mark passes, edges handed to the checker, candidate edges
  per pass, from one more run with a synchronisation around every phase (so their sum exceeds what the pipelined run takes):
  relax_us, mark_us (mark + collect + the one read-back), check_us (check_motions), apply_us, and rounds per relaxation
  gt_eager / gt_lazy                (hybrid) samples inside the band on edges without a sure hit, build and queries: what a ground
                                    truth would be asked.  The synthetic ground truth is the proxy's own sign at those samples and
                                    costs nothing here; breakeven_us_per_sample = (lazy - eager time) / (gt_eager - gt_lazy) is the
                                    cost per ground-truth configuration above which the lazy roadmap is the faster one
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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_lazy_roadmap.txt"))
    ap.add_argument("--quick", action="store_true", help="a 4096-node roadmap")
    args = ap.parse_args()
    from diffco_amd import _lib, _ops
    from diffco_amd.roadmap import Roadmap
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    lines = []

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)

    import bench
    w = bench.make_workload("headline", 1024, dev)
    m, lo, hi = w["model"], w["lo"].to(dev), w["hi"].to(dev)

    class Plain:
        gt = 0

        def is_collision(self, q):
            return m.score_raw(q.contiguous())[:, 0] > 0

        def check_motions(self, a, b, max_step=None, wrap=None):
            return m.check_motions(a, b, max_step=max_step, wrap=wrap)[0] >= 0

    class Hybrid(Plain):
        """sure verdicts outside [-band, +band]; an edge without a sure hit and with samples inside the band takes the proxy's
        own sign (the synthetic ground truth) and counts those samples"""

        def __init__(self, band):
            self.band, self.gt = band, 0

        def check_motions(self, a, b, max_step=None, wrap=None):
            r = m.motion_band_raw(a, b, -self.band, self.band, max_step=max_step, wrap=wrap, want_q=False)
            unsure = r["verdict"] == 2
            self.gt += int(r["n_uncertain"][unsure].sum())
            return (r["verdict"] == 1) | (unsure & (m.check_motions(a, b, max_step=max_step, wrap=wrap)[0] >= 0))

    n_nodes, k, step = (4096 if args.quick else 65536), 16, 0.05
    g = torch.Generator(device=dev).manual_seed(5)
    plain = Plain()

    def free_configs(n):
        q = torch.rand((8 * n, len(lo)), generator=g, device=dev) * (hi - lo) + lo
        q = q[~plain.is_collision(q)]
        assert len(q) >= n, "too few free samples"
        return q[:n].contiguous()

    nodes = free_configs(n_nodes)
    ends = free_configs(2 * 256)
    band = float(m.score_raw(nodes)[:, 0].abs().median()) * 0.25
    phases = {}

    def phase(name, fn):
        def timed(*a, **kw):
            us, out = wall(lambda: fn(*a, **kw))
            phases.setdefault(name, []).append(us)
            return out
        return timed

    for label, ck in (("plain", plain), ("hybrid", Hybrid(band))):
        eb, lb = [], []
        for i in range(args.repeats + 1):                        # (the first round warms every call up and is not counted)
            ck.gt = 0
            us, eager = wall(lambda: (lambda rm: (rm.csr(), rm)[1])(Roadmap.build(ck, nodes, k, step, max_dist=1.0)))
            eb += [us] if i else []
            gt_build = ck.gt
            us, lazy = wall(lambda: (lambda rm: (rm.csr(), rm)[1])(Roadmap.build(ck, nodes, k, step, max_dist=1.0, lazy=True)))
            lb += [us] if i else []
        eager_build_us, lazy_build_us = median(eb), median(lb)
        M = len(lazy.edges)
        emit(dict(shape="roadmap", checker=label, band=round(band, 4) if label == "hybrid" else None, nodes=len(lazy.nodes), k=k,
                  candidates=M, free_edges=len(eager.edges), eager_build_us=round(eager_build_us, 1),
                  lazy_build_us=round(lazy_build_us, 1), gt_build=gt_build))
        for Q in (1, 64, 256):
            starts, goals = ends[:Q].contiguous(), ends[256:256 + Q].contiguous()
            eager.query_batch(starts, goals)
            eq, lq = [], []
            for _ in range(args.repeats):
                ck.gt = 0
                us, want = wall(lambda: eager.query_batch(starts, goals))
                eq.append(us)
                gt_queries = ck.gt
                lazy.invalidate()
                ck.gt = 0
                us, res = wall(lambda: lazy.query_batch(starts, goals))
                lq.append(us)
                gt_lazy = ck.gt
            same = all(torch.equal(a, b) for a, b in ((res.path, want.path), (res.count, want.count), (res.length, want.length)))
            # one more run, a synchronisation around every phase
            lazy.invalidate()
            phases.clear()
            keep = (_ops.sssp_run, _ops.sssp_mark_routes, _ops.graph_apply_checks, lazy.checker.motions)
            _ops.sssp_run = phase("relax", keep[0])

            def mark_and_read(*a, **kw):
                out = keep[1](*a, **kw)
                out[4].tolist()
                return out

            _ops.sssp_mark_routes = phase("mark", mark_and_read)
            _ops.graph_apply_checks = phase("apply", keep[2])
            lazy.checker.motions = phase("check", keep[3])
            try:
                split = lazy.query_batch(starts, goals)
            finally:
                _ops.sssp_run, _ops.sssp_mark_routes, _ops.graph_apply_checks, lazy.checker.motions = keep
            it = split.iters
            eager_us, lazy_us = eager_build_us + median(eq), lazy_build_us + median(lq)
            gt_eager = gt_build + gt_queries
            res_line = dict(shape="lazy_query", checker=label, Q=Q, M=M, iters=res.iters, checked=res.checked,
                            checked_share=round(res.checked / M, 5), routed=int((res.count > 2).sum()), same_bits_as_eager=same,
                            eager_query_us=round(median(eq), 1), lazy_query_us=round(median(lq), 1),
                            eager_total_us=round(eager_us, 1), lazy_total_us=round(lazy_us, 1),
                            rounds_per_relax=res.rounds, relax_us_per_pass=round(sum(phases["relax"]) / it, 1),
                            mark_us_per_pass=round(sum(phases["mark"]) / it, 1),
                            check_us_per_pass=round(sum(phases["check"][2:]) / max(it - 1, 1), 1),
                            apply_us_per_pass=round(sum(phases.get("apply", [0.0])) / max(it - 1, 1), 1),
                            prelude_check_us=round(sum(phases["check"][:2]), 1))
            if label == "hybrid":
                res_line.update(gt_eager=gt_eager, gt_lazy=gt_lazy,
                                breakeven_us_per_sample=round((lazy_us - eager_us) / max(gt_eager - gt_lazy, 1), 4))
            emit(res_line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# python tools/lazy_roadmap_bench.py" + (" --quick" if args.quick else "") + f" --repeats {args.repeats}: "
                    "microseconds, wall clock around synchronised calls, medians (MI355X)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
