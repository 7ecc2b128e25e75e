"""Batched motion checks on the headline model (Baxter DH-7, Polyharmonic(1,1), S = 2000): ScoreModel.check_motions against
dcx_score on the same points already materialised (the bound without early exit) and against the host composition
(the points built in torch, one score launch, the first hit per edge).  Edges of 8 - 64 samples (max_step rule), two sets:
all free (a margin above every score) and cluttered (a margin at the 20th percentile of the sample scores: most edges hit
within their first quarter).  check_motions runs with max_samples = 64 (the edges' own bound), with the default bound
(max_samples=None: the longest edge's count, one read-back) and with a loose bound (10000), and with the early exit switched
off (knob motion_early_exit = 0).  --wrap: every joint masked as an angle on the circle (the edges are shorter than pi, so the
sample sets are the same and the difference to a plain run is the wrapped interpolation alone).

    python tools/motion_bench.py [--edges 4096 65536] [--iters 50] [--wrap] [--parent-lib devlibs/libdcx_parent.so]

One JSON line per (E, set) on stdout: median microseconds per call (CUDA events around each call on an idle stream).
--parent-lib (tools/motion_band_bench.py's mechanism): another build of the library - the parent commit's,
tools/build_variant.sh - runs the early-exit legs in a fresh child process per round, interleaved with this library's rounds.
"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warmup=5):
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


def bench_edges(E, lo, hi, dev, step, dof=7):
    """the benchmarks' edges of 8 - 64 samples under max_step = step, and the generator behind them"""
    g = torch.Generator(device=dev).manual_seed(E)
    qa = torch.rand((E, dof), generator=g, device=dev) * (hi - lo) + lo
    dirn = torch.randn((E, dof), generator=g, device=dev)
    dirn = dirn / dirn.norm(dim=1, keepdim=True)
    n_want = torch.randint(8, 65, (E, 1), generator=g, device=dev).float()
    return qa, qa + dirn * step * (n_want - 1.5), g        # ceil(L / step) + 1 = n_want samples


def parent_round(script, parent_lib, spec, extra=()):
    """one round of `script --child spec` on the library `parent_lib` (DCX_LIB) in a fresh process - this one keeps its own
    library: the child's JSON line, {leg: median microseconds}"""
    env = dict(os.environ, DCX_LIB=os.path.abspath(parent_lib))
    p = subprocess.run([sys.executable, os.path.abspath(script), "--child", spec, *extra], env=env, capture_output=True,
                       text=True, check=True)
    return json.loads(p.stdout.strip().splitlines()[-1])


def add_parent_rounds(res, rounds):
    """the parent's three round medians per leg, their median, and its run-to-run spread (max - min) / min"""
    for leg in rounds[0] if rounds else ():
        xs = [r[leg] for r in rounds]
        res[f"parent_{leg}_x3"] = [round(x, 1) for x in xs]
        res[f"parent_{leg}"] = round(sorted(xs)[len(xs) // 2], 1)
        res[f"parent_{leg}_spread"] = round((max(xs) - min(xs)) / min(xs), 4)


def child(args):
    """--child E:margin: the early-exit legs of main() on the library DCX_LIB names"""
    import bench
    from diffco_amd import _lib
    lib = _lib.require_gpu()
    dev = torch.device("cuda", 0)
    w = bench.make_workload("headline", 1024, dev)
    E, margin = args.child.split(":")
    qa, qb, _ = bench_edges(int(E), w["lo"].to(dev), w["hi"].to(dev), dev, 0.05)
    kw = dict(wrap=(1 << 7) - 1) if args.wrap else {}
    call = lambda: w["model"].check_motions(qa, qb, max_step=0.05, margin=float(margin), max_samples=64, **kw)  # noqa: E731
    out = {"check_motions_us": timed(call, args.iters)}
    lib.dcx_debug_set(b"motion_early_exit", 0)
    out["check_motions_no_early_exit_us"] = timed(call, args.iters)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--wrap", action="store_true", help="all joints masked: dcx_check_motions_ex along the shortest arc")
    ap.add_argument("--parent-lib", default=None, help="another build of libdcx.so whose early-exit legs are timed in child processes")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import bench
    from diffco_amd import _lib
    from diffco_amd._perceptron import host_motions
    lib = _lib.require_gpu()
    dev = torch.device("cuda", 0)
    w = bench.make_workload("headline", 1024, dev)
    m, lo, hi = w["model"], w["lo"].to(dev), w["hi"].to(dev)
    step = 0.05
    wrap = (1 << 7) - 1 if args.wrap else None
    kw = dict(wrap=wrap) if args.wrap else {}   # (a plain run passes nothing new: the call as it always was)
    for E in args.edges:
        qa, qb, _ = bench_edges(E, lo, hi, dev, step)
        first, n = m.check_motions(qa, qb, max_step=step, max_samples=64, **kw)
        assert int((first == -2).sum()) == 0
        # the materialised points (built once, outside the timing of the bound)
        d = qb - qa
        L = d.norm(dim=1)
        nn = torch.ceil(L * (1.0 / step)).long() + 1
        edge = torch.repeat_interleave(torch.arange(E, device=dev), nn)
        k = torch.arange(len(edge), device=dev) - (torch.cumsum(nn, 0) - nn)[edge]
        pts = (qa[edge] + k.float()[:, None] * (d[edge] * (step / L)[edge, None])).contiguous()
        if args.wrap:
            from diffco_amd.utils import wrap2pi
            pts = wrap2pi(pts).contiguous()
        scores = m.score_raw(pts)[:, 0]
        total = int(nn.sum())
        for label, margin in (("free", float(scores.max()) + 1.0), ("cluttered", float(torch.quantile(scores[:1 << 20], 0.2)))):
            f, _ = m.check_motions(qa, qb, max_step=step, margin=margin, max_samples=64, **kw)
            hit = f >= 0
            swept_hint = float(((f.float() + 1) / n.float()).where(hit, torch.ones_like(f, dtype=torch.float32)).mean())
            res = dict(E=E, set=label, wrap=bool(args.wrap), samples=total, hit_edges=int(hit.sum()),
                       mean_first_frac=round(swept_hint, 3))
            call = lambda ms: (lambda: m.check_motions(qa, qb, max_step=step, margin=margin, max_samples=ms, **kw))  # noqa: E731
            # early exit on / off, interleaved three times (median of the three medians each)
            on, off, parent = [], [], []
            for _ in range(3):
                if args.parent_lib:
                    parent.append(parent_round(__file__, args.parent_lib, f"{E}:{margin}",
                                               ["--iters", str(args.iters)] + (["--wrap"] if args.wrap else [])))
                on.append(timed(call(64), args.iters))
                lib.dcx_debug_set(b"motion_early_exit", 0)
                off.append(timed(call(64), args.iters))
                lib.dcx_debug_set(b"motion_early_exit", -1)
            res["check_motions_us"] = sorted(on)[1]
            res["check_motions_us_x3"] = [round(x, 1) for x in on]
            res["check_motions_no_early_exit_us"] = sorted(off)[1]
            res["check_motions_no_early_exit_us_x3"] = [round(x, 1) for x in off]
            add_parent_rounds(res, parent)
            # the default bound (max_samples=None: derived from the longest edge, one read-back) and a loose one (10000)
            res["check_motions_default_bound_us"] = timed(call(None), args.iters)
            res["check_motions_bound_10000_us"] = timed(call(10000), max(3, args.iters // 5))
            res["dcx_score_materialised_us"] = timed(lambda: m.score_raw(pts), args.iters)
            res["host_composition_us"] = timed(lambda: host_motions(lambda p: m.score_raw(p), qa, qb, max_step=step,
                                                                    margin=margin, max_samples=64, wrap=wrap or 0),
                                               max(5, args.iters // 5))
            hf, _ = host_motions(lambda p: m.score_raw(p), qa, qb, max_step=step, margin=margin, max_samples=64, wrap=wrap or 0)
            res["host_agrees"] = float((hf == f).float().mean())
            res["ratio_vs_score"] = round(res["check_motions_us"] / res["dcx_score_materialised_us"], 3)
            res["speedup_vs_host"] = round(res["host_composition_us"] / res["check_motions_us"], 1)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
