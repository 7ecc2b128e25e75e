"""k-nearest neighbours under the motion metric: the fused call (_ops.knn, dcx_knn) against the torch composition with the same
contract and the same bits (roadmap.host_knn) on the same GPU; the fused call against an instruction bound; and Roadmap.build on
the headline model split into its parts.

    python tools/knn_bench.py [--iters 20] [--out profiles/r15_knn.txt] [--quick]

Shapes: self-kNN (an exclude_self call, N = Q in {4096, 65536}, dof 7, k in {1, 16, 64}, no mask / every coordinate masked) and
an RRT's query (Q in {1, 64} against N in {1e5, 1e6}, k = 1).  Microseconds per call from HIP events around each call on an idle
stream; the two legs interleaved in three rounds, the median of the three medians reported with the three (the run-to-run
spread).  The host route's chunk is tuned per shape over CHUNKS first and the winner recorded.
The bound: VALU_PER_PAIR wave instructions per (query, point) pair - counted in the search kernel's inner loop for dof 7 in the
ISA - times Q * N pairs, over the chip's 256 CUs x 4 SIMDs x 16 lanes per clock at the shader clock
dcx_debug_clock_probe measures during the run.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CHUNKS = (1024, 2048, 4096, 8192)
VALU_PER_PAIR = {(7, False): 18}     # dof 7, no mask: 1 + 3 packed subtracts, 1 + 3 packed multiplies, 6 adds, 4 for the admission tests
LANES_PER_CLOCK = 256 * 4 * 16


def timed(fn, iters, warmup=2):
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


def shader_mhz(lib, dev, fn):
    """the shader clock WHILE fn's launches run: dcx_debug_clock_probe on a side stream (one wave: shader ticks against the
    fixed-rate wall clock over ~5 ms) beside a loop of fn on the current stream"""
    out = torch.zeros(4, dtype=torch.int64, device=dev)
    khz = ctypes.c_int32(0)
    side = torch.cuda.Stream(dev)
    fn()
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    rc = lib.dcx_debug_clock_probe(dev.index, ctypes.c_void_p(out.data_ptr()), 500000, ctypes.byref(khz), ctypes.c_void_p(side.cuda_stream))
    done.record(side)
    t0 = time.perf_counter()
    while not done.query() and time.perf_counter() - t0 < 5.0:
        fn()
    torch.cuda.synchronize()
    if rc != 0 or khz.value <= 0:
        return None
    s0, s1, w0, w1 = out.tolist()
    return (s1 - s0) / (w1 - w0) * khz.value / 1e3 if w1 > w0 else None


def cloud(n, dof, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.rand((n, dof), generator=g, device=dev) * 2 - 1) * 3.14159


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_knn.txt"))
    ap.add_argument("--quick", action="store_true", help="the small shapes only")
    ap.add_argument("--host-budget", type=float, default=6.0, help="seconds of host-route timing per round and shape")
    args = ap.parse_args()
    from diffco_amd import _lib, _ops
    from diffco_amd.roadmap import Roadmap, host_knn, knn_edges
    lib = _lib.require_gpu()
    dev = torch.device("cuda", 0)
    lines = []

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)

    dof = 7
    shapes = [("self", n, n, k, m) for n in ((4096,) if args.quick else (4096, 65536)) for k in (1, 16, 64) for m in (0, (1 << dof) - 1)]
    shapes += [("rrt", q, n, 1, 0) for n in ((100000,) if args.quick else (100000, 1000000)) for q in (1, 64)]
    for kind, Q, N, k, mask in shapes:
        p = cloud(N, dof, dev, N)
        q = p if kind == "self" else cloud(Q, dof, dev, Q + 1)
        kw = dict(wrap=mask, exclude_self=(kind == "self"))
        fused = lambda: _ops.knn(q, p, k, **kw)   # noqa: E731
        a = fused()
        # the host route's best chunk: one call each, after a warm-up call
        best = None
        for c in CHUNKS:
            host_knn(q[:min(Q, c)], p[:min(N, 4 * c)], k, wrap=mask, chunk=c)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b = host_knn(q, p, k, chunk=c, **kw)
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            if best is None or t < best[1]:
                best = (c, t)
        chunk = best[0]
        host = lambda: host_knn(q, p, k, chunk=chunk, **kw)   # noqa: E731
        b = host()
        same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
        host_iters = max(2, min(args.iters, int(args.host_budget / max(best[1], 1e-4))))
        f3, h3 = [], []
        for _ in range(3):
            f3.append(timed(fused, args.iters))
            h3.append(timed(host, host_iters, warmup=1))
        mhz = shader_mhz(lib, dev, fused)
        med = lambda xs: sorted(xs)[1]   # noqa: E731
        res = dict(shape=kind, Q=Q, N=N, dof=dof, k=k, mask=mask, same_bits=same, fused_us=round(med(f3), 1),
                   fused_us_x3=[round(x, 1) for x in f3], host_us=round(med(h3), 1), host_us_x3=[round(x, 1) for x in h3],
                   host_chunk=chunk, host_iters=host_iters, speedup=round(med(h3) / med(f3), 2), shader_mhz=mhz and round(mhz))
        valu = VALU_PER_PAIR.get((dof, bool(mask)))
        if valu and mhz:
            bound = valu * Q * N / (LANES_PER_CLOCK * mhz)      # microseconds
            res.update(valu_per_pair=valu, bound_us=round(bound, 1), bound_ratio=round(med(f3) / bound, 2))
        emit(res)

    # Roadmap.build on the headline model, and its parts timed on their own
    import bench
    w = bench.make_workload("headline", 1024, dev)
    m, lo, hi = w["model"], w["lo"].to(dev), w["hi"].to(dev)

    class Checker:
        def is_collision(self, q):
            return m.score_raw(q.contiguous())[:, 0] > 0

        def check_motions(self, a, b, max_step=None, wrap=None):
            return m.check_motions(a, b, max_step=max_step, wrap=wrap)[0] >= 0

    n_nodes, k, step = (4096 if args.quick else 65536), 16, 0.05
    g = torch.Generator(device=dev).manual_seed(5)
    nodes = torch.rand((n_nodes, len(lo)), generator=g, device=dev) * (hi - lo) + lo
    ck = Checker()
    rm = Roadmap.build(ck, nodes, k, step, max_dist=1.0)
    kept = rm.nodes
    its = max(3, args.iters // 4)
    t_point = timed(lambda: ck.is_collision(nodes), its)
    t_knn = timed(lambda: _ops.knn(kept, kept, k, max_dist=1.0, exclude_self=True), its)
    t_edges = timed(lambda: knn_edges(kept, k, max_dist=1.0), its)
    cand = knn_edges(kept, k, max_dist=1.0)
    qa, qb = kept[cand[:, 0]], kept[cand[:, 1]]
    t_check = timed(lambda: ck.check_motions(qa, qb, max_step=step), its)
    t_build = timed(lambda: Roadmap.build(ck, nodes, k, step, max_dist=1.0), its)
    emit(dict(shape="roadmap_build", nodes=n_nodes, kept=len(kept), k=k, max_step=step, max_dist=1.0, candidates=len(cand),
              edges=len(rm.edges), point_check_us=round(t_point, 1), knn_us=round(t_knn, 1), edge_forming_us=round(t_edges - t_knn, 1),
              check_motions_us=round(t_check, 1), build_us=round(t_build, 1),
              rest_us=round(t_build - t_point - t_edges - t_check, 1)))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/knn_bench.py: microseconds per call, medians of three interleaved rounds (MI355X)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
