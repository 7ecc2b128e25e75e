"""Worst-sample motion queries on the headline model (Baxter DH-7, Polyharmonic(1,1), S = 2000): ScoreModel.motion_worst_raw
without and with gradients against dcx_check_motions with the early exit switched off (knob motion_early_exit = 0: the same
sweep work on the check's kernel) and against the host composition (host_motion_worst over ScoreModel.score: the points built
in torch, one score launch, a segment arg-max; with gradients, autograd through it).  tools/motion_bench.py's edges: 8 - 64
samples (max_step rule, max_samples = 64), two sets: free (a margin above every score) and cluttered (a margin at the 20th
percentile of the sample scores).

    python tools/motion_worst_bench.py [--edges 4096 65536] [--iters 50] [--parent-lib devlibs/libdcx_parent.so]

One JSON line per (E, set) on stdout: microseconds per call (CUDA events around each call on an idle stream), the fused legs
interleaved three times (median of the three medians; the three medians of the check are printed as its run-to-run spread).
--parent-lib: another build of the library times dcx_motion_worst without and with gradients in a fresh child process per round
(tools/motion_bench.py parent_round), interleaved with this library's rounds.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def child(args):
    """--child E:margin: dcx_motion_worst without and with gradients on the library DCX_LIB names"""
    import bench
    from motion_bench import bench_edges, timed
    from diffco_amd import _lib
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    w = bench.make_workload("headline", 1024, dev)
    E, margin = args.child.split(":")
    qa, qb, _ = bench_edges(int(E), w["lo"].to(dev), w["hi"].to(dev), dev, 0.05)
    kw = dict(max_step=0.05, margin=float(margin), max_samples=64)
    print(json.dumps({"motion_worst_us": timed(lambda: w["model"].motion_worst_raw(qa, qb, **kw), args.iters),
                      "motion_worst_grad_us": timed(lambda: w["model"].motion_worst_raw(qa, qb, grad=True, **kw), args.iters)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--parent-lib", default=None, help="another build of libdcx.so whose dcx_motion_worst is timed in child processes")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import bench
    from motion_bench import add_parent_rounds, bench_edges, parent_round, timed
    from diffco_amd import _lib
    from diffco_amd._perceptron import host_motion_worst
    lib = _lib.require_gpu()
    dev = torch.device("cuda", 0)
    w = bench.make_workload("headline", 1024, dev)
    m, lo, hi = w["model"], w["lo"].to(dev), w["hi"].to(dev)
    step = 0.05
    for E in args.edges:
        qa, qb, g = bench_edges(E, lo, hi, dev, step)
        worst0, _, _, n = m.motion_worst_raw(qa, qb, max_step=step, max_samples=64)
        assert int(torch.isnan(worst0).sum()) == 0
        # the sample scores' range from the worst scores and a sample of the points' scores (the sets of tools/motion_bench.py)
        pts = (qa + (qb - qa) * torch.rand((E, 1), generator=g, device=dev))
        scores = m.score_raw(pts.contiguous())[:, 0]
        for label, margin in (("free", float(worst0.max()) + 1.0), ("cluttered", float(torch.quantile(scores[:1 << 20], 0.2)))):
            kw = dict(max_step=step, margin=margin, max_samples=64)
            f, _ = m.check_motions(qa, qb, **kw)
            wv, wi, wc, _ = m.motion_worst_raw(qa, qb, **kw)
            assert torch.equal(wv > 0, f >= 0)
            res = dict(E=E, set=label, samples=int(n.sum()), hit_edges=int((f >= 0).sum()))
            check, worst, worst_g, parent = [], [], [], []
            for _ in range(3):
                if args.parent_lib:
                    parent.append(parent_round(__file__, args.parent_lib, f"{E}:{margin}", ["--iters", str(args.iters)]))
                lib.dcx_debug_set(b"motion_early_exit", 0)
                check.append(timed(lambda: m.check_motions(qa, qb, **kw), args.iters))
                lib.dcx_debug_set(b"motion_early_exit", -1)
                worst.append(timed(lambda: m.motion_worst_raw(qa, qb, **kw), args.iters))
                worst_g.append(timed(lambda: m.motion_worst_raw(qa, qb, grad=True, **kw), args.iters))
            res["check_no_early_exit_us_x3"] = [round(x, 1) for x in check]
            res["check_no_early_exit_us"] = round(sorted(check)[1], 1)
            res["check_spread"] = round((max(check) - min(check)) / min(check), 4)
            res["motion_worst_us"] = round(sorted(worst)[1], 1)
            res["motion_worst_us_x3"] = [round(x, 1) for x in worst]
            res["motion_worst_grad_us"] = round(sorted(worst_g)[1], 1)
            res["motion_worst_grad_us_x3"] = [round(x, 1) for x in worst_g]
            add_parent_rounds(res, parent)
            res["score_grad_E_points_us"] = round(timed(lambda: m.score_grad_raw(qa), args.iters), 1)
            host = lambda a, b: host_motion_worst(lambda p: m.score(p), a, b, **dict(kw, wrap=0))  # noqa: E731
            res["host_composition_us"] = round(timed(lambda: host(qa, qb), max(5, args.iters // 5)), 1)

            def host_grad():
                a, b = qa.clone().requires_grad_(True), qb.clone().requires_grad_(True)
                torch.autograd.grad(host(a, b)[0].sum(), (a, b))
            res["host_composition_grad_us"] = round(timed(host_grad, max(5, args.iters // 5)), 1)
            hw, hi_, _, _ = host(qa, qb)
            res["host_idx_agrees"] = float((hi_ == wi).float().mean())
            res["host_value_max_rel_diff"] = float((hw - wv).abs().max() / wv.abs().max())
            res["ratio_vs_check"] = round(res["motion_worst_us"] / res["check_no_early_exit_us"], 3)
            res["grad_over_plain"] = round(res["motion_worst_grad_us"] / res["motion_worst_us"], 3)
            res["speedup_vs_host"] = round(res["host_composition_us"] / res["motion_worst_us"], 2)
            res["speedup_vs_host_grad"] = round(res["host_composition_grad_us"] / res["motion_worst_grad_us"], 2)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
