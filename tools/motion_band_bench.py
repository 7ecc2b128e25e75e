"""Hybrid motion checks on the headline model (Baxter DH-7, Polyharmonic(1,1), S = 2000): ScoreModel.motion_band_raw (a fixed
list capacity: nothing read back) against dcx_motion_worst without gradients - the same sweep work on the same plan, with the
other answer step - from this library; with --parent-lib, both calls also from another build of the library (the parent
commit's, tools/build_variant.sh), timed in a fresh child process per round (tools/motion_bench.py parent_round; a build
that predates dcx_motion_band times dcx_motion_worst alone); against dcx_check_motions with the early exit switched off;
and against the host composition (host_motion_band over ScoreModel.score_raw: the points built in torch, one score launch, the
masks, a segment reduction and `nonzero`).  tools/motion_bench.py's edges: 8 - 64 samples (max_step rule, max_samples = 64),
two sets: free (a band above every score: nothing listed) and cluttered (lo / hi at the 20th / 40th percentile of the sample
scores).

    python tools/motion_band_bench.py [--edges 4096 65536] [--iters 50] [--parent-lib devlibs/libdcx_parent.so]

One JSON line per (E, set) on stdout: microseconds per call (CUDA events around each call on an idle stream), the legs
interleaved three times (median of the three medians; the three medians of motion_worst are printed as its run-to-run spread).
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEP = 0.05


def edges(E, lo, hi, dev):
    g = torch.Generator(device=dev).manual_seed(E)
    qa = torch.rand((E, 7), generator=g, device=dev) * (hi - lo) + lo
    dirn = torch.randn((E, 7), generator=g, device=dev)
    dirn = dirn / dirn.norm(dim=1, keepdim=True)
    n_want = torch.randint(8, 65, (E, 1), generator=g, device=dev).float()
    qb = qa + dirn * STEP * (n_want - 1.5)        # ceil(L / step) + 1 = n_want samples
    pts = (qa + (qb - qa) * torch.rand((E, 1), generator=g, device=dev))
    return qa, qb, pts


def child(args):
    """--child E:lo:hi: one round of dcx_motion_worst without gradients (margin lo) and of dcx_motion_band on the library DCX_LIB
    names: a JSON line {leg: median microseconds}"""
    import bench
    from motion_bench import timed
    from diffco_amd import _lib
    has_band = hasattr(ctypes.CDLL(_lib.LIB_PATH), "dcx_motion_band")
    if not has_band:   # (the other build predates the call)
        for name in [k for k in _lib.SYMBOLS if k.startswith("dcx_motion_band")]:
            del _lib.SYMBOLS[name]
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    w = bench.make_workload("headline", 1024, dev)
    m = w["model"]
    E, b_lo, b_hi = args.child.split(":")
    qa, qb, _ = edges(int(E), w["lo"].to(dev), w["hi"].to(dev), dev)
    kw = dict(max_step=STEP, max_samples=64)
    out = {"motion_worst_us": timed(lambda: m.motion_worst_raw(qa, qb, margin=float(b_lo), **kw), args.iters)}
    if has_band:
        cap = int(m.motion_worst_raw(qa, qb, **kw)[3].sum())
        out["motion_band_us"] = timed(lambda: m.motion_band_raw(qa, qb, float(b_lo), float(b_hi), unc_cap=cap, **kw), args.iters)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--parent-lib", default=None, help="another build of libdcx.so whose dcx_motion_worst and dcx_motion_band are timed in child processes")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import bench
    from motion_bench import add_parent_rounds, parent_round, timed
    from diffco_amd import _lib
    from diffco_amd._perceptron import host_motion_band
    lib = _lib.require_gpu()
    dev = torch.device("cuda", 0)
    w = bench.make_workload("headline", 1024, dev)
    m, lo, hi = w["model"], w["lo"].to(dev), w["hi"].to(dev)
    for E in args.edges:
        qa, qb, pts = edges(E, lo, hi, dev)
        worst0, _, _, n = m.motion_worst_raw(qa, qb, max_step=STEP, max_samples=64)
        assert int(torch.isnan(worst0).sum()) == 0
        scores = m.score_raw(pts.contiguous())[:, 0]
        top = float(worst0.max())
        q20, q40 = (float(torch.quantile(scores[:1 << 20], p)) for p in (0.2, 0.4))
        for label, b_lo, b_hi in (("free", top + 1.0, top + 2.0), ("cluttered", q20, q40)):
            kw = dict(max_step=STEP, max_samples=64)
            cap = int(n.sum())
            r = m.motion_band_raw(qa, qb, b_lo, b_hi, unc_cap=cap, **kw)
            f, _ = m.check_motions(qa, qb, margin=b_hi, **kw)
            assert torch.equal(r["first_hit"], f)
            res = dict(E=E, set=label, samples=cap, listed=int(r["unc_total"]),
                       verdicts=[int((r["verdict"] == v).sum()) for v in (0, 1, 2)])
            band, band_noq, worst, check, parent = [], [], [], [], []
            for _ in range(3):
                if args.parent_lib:
                    parent.append(parent_round(__file__, args.parent_lib, f"{E}:{b_lo}:{b_hi}", ["--iters", str(args.iters)]))
                worst.append(timed(lambda: m.motion_worst_raw(qa, qb, margin=b_lo, **kw), args.iters))
                band.append(timed(lambda: m.motion_band_raw(qa, qb, b_lo, b_hi, unc_cap=cap, **kw), args.iters))
                band_noq.append(timed(lambda: m.motion_band_raw(qa, qb, b_lo, b_hi, unc_cap=cap, want_q=False, **kw), args.iters))
                lib.dcx_debug_set(b"motion_early_exit", 0)
                check.append(timed(lambda: m.check_motions(qa, qb, margin=b_hi, **kw), args.iters))
                lib.dcx_debug_set(b"motion_early_exit", -1)
            med = lambda xs: round(sorted(xs)[1], 1)  # noqa: E731
            res["motion_worst_us_x3"] = [round(x, 1) for x in worst]
            res["motion_worst_us"] = med(worst)
            res["motion_worst_spread"] = round((max(worst) - min(worst)) / min(worst), 4)
            add_parent_rounds(res, parent)
            res["motion_band_us_x3"] = [round(x, 1) for x in band]
            res["motion_band_us"] = med(band)
            res["motion_band_no_q_us"] = med(band_noq)
            res["check_no_early_exit_us"] = med(check)
            host = lambda: host_motion_band(m.score_raw, qa, qb, b_lo, b_hi, **dict(kw, wrap=0))  # noqa: E731
            res["host_composition_us"] = round(timed(host, max(5, args.iters // 5)), 1)
            hv = host()
            res["host_verdict_agrees"] = float((hv[0] == r["verdict"]).float().mean())
            res["ratio_vs_motion_worst"] = round(res["motion_band_us"] / res["motion_worst_us"], 3)
            if parent:
                res["ratio_vs_parent_motion_worst"] = round(res["motion_band_us"] / res["parent_motion_worst_us"], 3)
                if "parent_motion_band_us" in res:
                    res["ratio_vs_parent_motion_band"] = round(res["motion_band_us"] / res["parent_motion_band_us"], 3)
            res["speedup_vs_host"] = round(res["host_composition_us"] / res["motion_band_us"], 2)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
