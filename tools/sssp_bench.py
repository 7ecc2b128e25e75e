"""Batched roadmap queries on the headline model: Roadmap.query_batch (the fused calls _ops.sssp_run and
_ops.sssp_extract_paths) against Roadmap.query called once per pair (scipy's Dijkstra on the host, the yardstick) and against
roadmap.host_sssp (the same contract in torch ops) on the same GPU.

    python tools/sssp_bench.py [--iters 5] [--out profiles/r18_sssp.txt] [--quick]

The roadmap: N = 65536 collision-free samples (4096 with --quick), k = 16, max_step 0.05, max_dist 1.0 - tools/knn_bench.py's.
Q in {1, 64, 256} pairs of free configurations.  Per Q, in microseconds (HIP events around each call on an idle stream, medians):
  round_us        one relaxation round (_ops.sssp_run, round0 = 1, n_rounds = 1: the first round of a call never returns early,
                  and a round's work does not depend on the state)
  round_bytes     what a round moves: nnz * Q * 4 gathered from dist_old + N * Q * 4 read + N * Q * 4 written + the CSR (8 bytes
                  an entry, 4 a row) once per block of 64 queries; pred's stores, which follow the state, are left out.
                  round_tbps is round_bytes over round_us
  routed / direct / none: how many of the Q pairs went over the roadmap, had a free direct motion, had no path.  Roadmap.query
                  returns before its graph search for a direct pair, so query_us is mostly the routed pairs' searches
  batch_us        the whole query_batch, its three checker calls and its read-backs included; rounds: what it ran
  relax_us        all its relaxation rounds as one sssp_run call, extract_us the sizing and the writing extraction
  query_us        Roadmap.query called for each of the Q pairs (wall clock, once)
  host_sssp_us    roadmap.host_sssp to the fixed point from the same links (wall clock, once)
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


def timed(fn, iters, warmup=1):
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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_sssp.txt"))
    ap.add_argument("--quick", action="store_true", help="a 4096-node roadmap")
    args = ap.parse_args()
    from diffco_amd import _lib, _ops
    from diffco_amd.roadmap import Roadmap, host_sssp, knn
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

    class Checker:
        def is_collision(self, q):
            return m.score_raw(q.contiguous())[:, 0] > 0

        def check_motions(self, a, b, max_step=None, wrap=None):
            return m.check_motions(a, b, max_step=max_step, wrap=wrap)[0] >= 0

    ck = Checker()
    n_nodes, k, step = (4096 if args.quick else 65536), 16, 0.05
    g = torch.Generator(device=dev).manual_seed(5)

    def free_configs(n):
        q = torch.rand((8 * n, len(lo)), generator=g, device=dev) * (hi - lo) + lo
        q = q[~ck.is_collision(q)]
        assert len(q) >= n, "too few free samples"
        return q[:n].contiguous()

    nodes = free_configs(n_nodes)
    build_us, rm = wall(lambda: Roadmap.build(ck, nodes, k, step, max_dist=1.0))
    assert len(rm.nodes) == n_nodes
    csr_us, (rowptr, col, weight) = wall(rm.csr)
    N, nnz = n_nodes, len(col)
    deg = rowptr[1:] - rowptr[:-1]
    emit(dict(shape="roadmap", nodes=N, k=k, max_step=step, max_dist=1.0, edges=len(rm.edges), nnz=nnz, degree_mean=round(nnz / N, 2),
              degree_max=int(deg.max()), build_us=round(build_us, 1), csr_us=round(csr_us, 1)))
    ends = free_configs(2 * 256)
    for Q in (1, 64, 256):
        starts, goals = ends[:Q].contiguous(), ends[256:256 + Q].contiguous()
        res = rm.query_batch(starts, goals)
        batch_us = timed(lambda: rm.query_batch(starts, goals), args.iters)
        # the relaxation on its own, from every start's k nearest nodes taken as free links
        idx, d2 = knn(starts, rm.nodes, k)
        si, sl = idx.contiguous(), d2.sqrt().contiguous()
        dist = torch.empty((2, N, Q), dtype=torch.float32, device=dev)
        pred = torch.empty((N, Q), dtype=torch.int32, device=dev)
        rounds, done = None, 0
        while rounds is None and done < N:
            flags = _ops.sssp_run(rowptr, col, weight, si, sl, dist, pred, done, 8).tolist()
            rounds = done + flags.index(0) + 1 if 0 in flags else None
            done += 8
        rounds = N if rounds is None else rounds
        relax_us = timed(lambda: _ops.sssp_run(rowptr, col, weight, si, sl, dist, pred, 0, rounds), args.iters)
        round_us = timed(lambda: _ops.sssp_run(rowptr, col, weight, si, sl, dist, pred, 1, 1), 4 * args.iters)
        _ops.sssp_run(rowptr, col, weight, si, sl, dist, pred, 0, rounds)
        mode = torch.full((Q,), 2, dtype=torch.int32, device=dev)
        gi, gd2 = knn(goals, rm.nodes, k)
        ex = (rowptr, col, weight, rm.nodes, dist, pred, rounds, mode, starts, goals, gi.contiguous(), gd2.sqrt().contiguous(),
              torch.zeros(Q, device=dev))

        def extract():
            W = max(-int(_ops.sssp_extract_paths(*ex, 0)[1].min()), 2)
            return _ops.sssp_extract_paths(*ex, W)

        extract_us = timed(extract, args.iters)
        host_us, (hd, hp, hf) = wall(lambda: host_sssp(rowptr, col, weight, si, sl))
        same = bool(torch.equal(hd.view(torch.int32), dist[(rounds - 1) & 1].view(torch.int32)) and torch.equal(hp, pred))
        print(f"# Q={Q}: fused and host_sssp timed, {Q} Roadmap.query calls next", flush=True)
        t0 = time.perf_counter()
        single, routed_s, routed_n = [], 0.0, 0
        for q in range(Q):
            t1 = time.perf_counter()
            single.append(rm.query(starts[q], goals[q]))   # (returns floats: it has synchronised)
            if single[-1] is not None and len(single[-1][0]) > 2:
                routed_s, routed_n = routed_s + time.perf_counter() - t1, routed_n + 1
            if q % 32 == 31:
                print(f"#   {q + 1} / {Q} after {time.perf_counter() - t0:.1f} s", flush=True)
        torch.cuda.synchronize()
        query_us = (time.perf_counter() - t0) * 1e6
        agree = all((s is None) == (n == 0) for s, n in zip(single, res.count.tolist()))
        worst = max([abs(float(res.length[q]) - s[1]) / s[1] for q, s in enumerate(single) if s is not None] + [0.0])
        moved = nnz * Q * 4 + 2 * N * Q * 4 + ((Q + 63) // 64) * (nnz * 8 + N * 4)
        emit(dict(shape="query_batch", Q=Q, N=N, k=k, rounds_batch=res.rounds, rounds_relax=rounds, routed=int((res.count > 2).sum()),
                  direct=int((res.count == 2).sum()), none=int((res.count == 0).sum()), waypoints_max=int(res.count.max()),
                  round_us=round(round_us, 1), round_bytes=moved, round_tbps=round(moved / round_us / 1e6, 3), relax_us=round(relax_us, 1), extract_us=round(extract_us, 1),
                  batch_us=round(batch_us, 1), query_us=round(query_us, 1), query_us_per_pair=round(query_us / Q, 1),
                  query_us_per_routed_pair=round(routed_s * 1e6 / routed_n, 1) if routed_n else None,
                  host_sssp_us=round(host_us, 1), host_same_bits=same, same_none_cases_as_query=agree, worst_rel_length_gap=worst,
                  batch_vs_query=round(query_us / batch_us, 2), relax_vs_host_sssp=round(host_us / relax_us, 2)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/sssp_bench.py: microseconds, medians of HIP-event timings; query_us and host_sssp_us wall clock, once (MI355X)\n"
                    + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
