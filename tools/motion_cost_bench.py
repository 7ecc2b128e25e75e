"""Differentiable motion costs (ScoreModel.motion_cost_raw) on the headline model (Baxter DH-7, Polyharmonic(1,1), S = 2000,
C = 1) and on cfg3's five-class model, with tools/motion_bench.py's edge sets: edges of 8 - 64 samples (max_step rule), all
free (a margin above every score) or cluttered (a margin at the 20th percentile of the sample scores).  Compared against
  (a) score_hinge_grad_raw on the same points already materialised (the sweep bound; no interpolation, no reduction),
  (b) the host composition (points built differentiably in torch, scored through autograd, index_add per edge, backward),
  (c) check_motions on the same edges and margins.
Every timing is the median of interleaved rounds (each a median over --iters calls, CUDA events on an idle stream).
--wrap: every joint masked as an angle on the circle (the edges are shorter than pi: the same sample sets, so the difference to
a plain run is the wrapped interpolation and the wrapped direction alone).

    python tools/motion_cost_bench.py [--edges 4096 65536] [--iters 30] [--models headline cfg3] [--wrap]

One JSON line per (model, E, set) on stdout.
"""
import argparse
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


def child(args):
    """--child E:margin[,margin ...] (--models: the one model): dcx_motion_cost on the library DCX_LIB names"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench
    from motion_bench import bench_edges
    from diffco_amd import _lib
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    w = bench.make_workload(args.models[0], 1024, dev)
    m = w["model"]
    E, margin = args.child.split(":")
    qa, qb, _ = bench_edges(int(E), w["lo"].to(dev), w["hi"].to(dev), dev, 0.05, m.dof)
    kw = dict(wrap=(1 << m.dof) - 1) if args.wrap else {}
    call = lambda: m.motion_cost_raw(qa, qb, max_step=0.05, margin=[float(x) for x in margin.split(",")], max_samples=64, **kw)  # noqa: E731
    print(json.dumps({"motion_cost_us": timed(call, args.iters)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--models", nargs="+", default=["headline", "cfg3"])
    ap.add_argument("--wrap", action="store_true", help="all joints masked: dcx_motion_cost_ex along the shortest arc")
    ap.add_argument("--parent-lib", default=None, help="another build of libdcx.so whose dcx_motion_cost is timed in child processes "
                                                       "(tools/motion_bench.py parent_round), interleaved with this library's rounds")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from motion_bench import add_parent_rounds, parent_round
    import bench
    from diffco_amd import _lib
    from diffco_amd._perceptron import host_motion_cost
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    step = 0.05
    for name in args.models:
        w = bench.make_workload(name, 1024, dev)
        m, lo, hi = w["model"], w["lo"].to(dev), w["hi"].to(dev)
        wrap = (1 << m.dof) - 1 if args.wrap else None
        kw = dict(wrap=wrap) if args.wrap else {}   # (a plain run passes nothing new: the call as it always was)
        for E in args.edges:
            g = torch.Generator(device=dev).manual_seed(E)
            qa = torch.rand((E, m.dof), generator=g, device=dev) * (hi - lo) + lo
            dirn = torch.randn((E, m.dof), generator=g, device=dev)
            dirn = dirn / dirn.norm(dim=1, keepdim=True)
            n_want = torch.randint(8, 65, (E, 1), generator=g, device=dev).float()
            qb = qa + dirn * step * (n_want - 1.5)        # ceil(L / step) + 1 = n_want samples
            d = qb - qa
            L = d.norm(dim=1)
            nn = torch.ceil(L * (1.0 / step)).long() + 1
            edge = torch.repeat_interleave(torch.arange(E, device=dev), nn)
            k = torch.arange(len(edge), device=dev) - (torch.cumsum(nn, 0) - nn)[edge]
            pts = (qa[edge] + k.float()[:, None] * (d[edge] * (step / L)[edge, None])).contiguous()
            last = k == nn[edge] - 1
            if args.wrap:
                from diffco_amd.utils import wrap2pi
                pts = wrap2pi(pts)
            pts = torch.where(last[:, None], qb[edge], pts).contiguous()
            scores = m.score_raw(pts)
            total = int(nn.sum())
            free = (scores.max(dim=0).values + 1.0).tolist()
            clut = torch.quantile(scores[:1 << 20], 0.2, dim=0).tolist()
            for label, margin in (("free", free), ("cluttered", clut)):
                cost, ga, gb, n = m.motion_cost_raw(qa, qb, max_step=step, margin=margin, max_samples=64, **kw)
                assert int(torch.isnan(cost).sum()) == 0
                res = dict(model=name, C=m.C, E=E, set=label, wrap=bool(args.wrap), samples=total,
                           costly_edges=int((cost > 0).sum()))
                qa_g, qb_g = qa.clone().requires_grad_(True), qb.clone().requires_grad_(True)
                mg_t = torch.tensor(margin, device=dev)

                def host():
                    c = host_motion_cost(lambda p: m.score(p), qa_g, qb_g, max_step=step, margin=mg_t, max_samples=64,
                                         wrap=wrap or 0)
                    return torch.autograd.grad(c.sum(), (qa_g, qb_g))

                calls = {
                    "motion_cost_us": lambda: m.motion_cost_raw(qa, qb, max_step=step, margin=margin, max_samples=64, **kw),
                    "hinge_grad_materialised_us": lambda: m.score_hinge_grad_raw(pts, margin, 1.0),
                    "check_motions_us": lambda: m.check_motions(qa, qb, max_step=step, margin=margin, max_samples=64, **kw),
                }
                rounds = {k: [] for k in list(calls) + ["host_composition_us"]}
                parent = []
                for _ in range(args.rounds):   # interleaved
                    if args.parent_lib:
                        parent.append(parent_round(__file__, args.parent_lib, f"{E}:{','.join(repr(float(x)) for x in margin)}",
                                                   ["--iters", str(args.iters), "--models", name] + (["--wrap"] if args.wrap else [])))
                    for k, fn in calls.items():
                        rounds[k].append(timed(fn, args.iters))
                    rounds["host_composition_us"].append(timed(host, max(3, args.iters // 5)))
                for k, v in rounds.items():
                    res[k] = round(sorted(v)[len(v) // 2], 1)
                res["motion_cost_us_x3"] = [round(x, 1) for x in rounds["motion_cost_us"]]
                add_parent_rounds(res, parent)
                hc = host_motion_cost(lambda p: m.score(p), qa, qb, max_step=step, margin=mg_t, max_samples=64, wrap=wrap or 0)
                res["host_cost_max_rel_diff"] = float((hc - cost).abs().max() / cost.abs().max().clamp(min=1e-30))
                res["ratio_vs_hinge_grad"] = round(res["motion_cost_us"] / res["hinge_grad_materialised_us"], 3)
                res["ratio_vs_check_motions"] = round(res["motion_cost_us"] / res["check_motions_us"], 3)
                res["speedup_vs_host"] = round(res["host_composition_us"] / res["motion_cost_us"], 2)
                print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
