"""GPU: batched path resampling (dcx_path_resample, _ops.path_resample, resample.resample_paths) against its referee
resample.host_resample_paths - the same contract in torch ops on the CPU - bit for bit on path, count and lengths: batches of 67
paths with counts of every kind mixed (no path, one waypoint, below, at and above one chunk, more than a block's LDS holds, more
chunks than a block has threads, NaN and infinite waypoints, coincident waypoints), dof 1, 2 and 7, without and with a mixed
wrap mask, up to more output waypoints than a block has threads.  Then untouched rows, untouched inputs, graph capture,
repeatability, routing, and the chain plan -> shortcut -> resample -> optimise on test_gpu_rrt's small Baxter problem."""
import functools

import numpy as np
import pytest
import torch

from helpers import CASE_ROBOT, make_robot, relerr
from resample_helpers import DOFS, MIXED, NS, TS, bits, random_path
from test_gpu_rrt import B, _baxter   # (_baxter's checker is a ModelChecker over the fixture's ScoreModel)

pytestmark = pytest.mark.gpu

R = 67
# the host file's shapes, 32 * 64 + 1 (past the LDS cut-over: the workspace form) and 32 * 256 + 5 (more chunks than threads)
COUNTS = NS + (32 * 64 + 1, 32 * 256 + 5)
T_ALL = TS + (1025,)   # ... and more output waypoints than a block has threads


@functools.lru_cache(maxsize=None)
def mixed_batch(dof, mask):
    """(path [67, W, dof] on the CPU, rows beyond each count NaN; count [67] int32): COUNTS in turn, and among them a row
    without a path, one with a single waypoint, one with a NaN and one with an infinite waypoint, one of coincident waypoints"""
    g = np.random.default_rng(77 + dof)
    special = {5: "none", 11: "one", 17: "nan", 23: "inf", 29: "same"}
    rows = []
    for r in range(R):
        kind = special.get(r)
        p = random_path(g, 1 if kind == "one" else COUNTS[r % len(COUNTS)], dof, mask)
        if kind == "none":
            p = p[:0]
        elif kind == "nan":
            p[1, 0] = float("nan")
        elif kind == "inf":
            p[len(p) - 1, dof - 1] = float("inf")
        elif kind == "same":
            p[:] = p[0]
        rows.append(p)
    W = max(len(p) for p in rows)
    path = torch.full((R, W, dof), float("nan"))
    for r, p in enumerate(rows):
        path[r, :len(p)] = p
    count = torch.tensor([len(p) for p in rows], dtype=torch.int32)
    assert W == COUNTS[-1] and {0, 1, 32, 33, 34, 2049, COUNTS[-1]} <= set(count.tolist())
    return path, count


@functools.lru_cache(maxsize=None)
def both(dof, masked, T):
    from diffco_amd.resample import host_resample_paths, resample_paths
    mask = MIXED[dof] if masked else 0
    path, count = mixed_batch(dof, mask)
    host = host_resample_paths(path, count, n_waypoints=T, wrap=mask)
    dpath, dcount = path.cuda(), count.cuda()
    keep = dpath.clone(), dcount.clone()
    fused = resample_paths(dpath, dcount, n_waypoints=T, wrap=mask)
    torch.cuda.synchronize()
    return host, fused, (dpath, dcount), keep, mask


def _assert_same(a, b):
    assert torch.equal(a.count.cpu(), b.count.cpu()), (a.count.tolist(), b.count.tolist())
    la, lb = bits(a.lengths.cpu()), bits(b.lengths.cpu())
    assert torch.equal(la, lb), torch.nonzero(la != lb).reshape(-1).tolist()
    pa, pb = bits(a.path.cpu()), bits(b.path.cpu())
    assert torch.equal(pa, pb), torch.nonzero((pa != pb).any(dim=2).any(dim=1)).reshape(-1).tolist()


@pytest.mark.parametrize("T", T_ALL)
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "mixed-mask"])
@pytest.mark.parametrize("dof", DOFS)
def test_fused_equals_host_bit_for_bit(dof, masked, T):
    host, fused, (dpath, dcount), keep, mask = both(dof, masked, T)
    assert fused.route == "fused" and host.route == "host" and fused.path.shape == (R, T, dof)
    _assert_same(fused, host)
    got = fused.count.tolist()
    assert got.count(0) == 4 and set(got) == {0, T} and [r for r, c in enumerate(got) if c == 0] == [5, 11, 17, 23]
    ln = fused.lengths.tolist()
    # (an infinite step on a masked coordinate wraps to NaN, on a plain one the length is +inf)
    assert ln[5] != ln[5] and ln[11] != ln[11] and ln[17] != ln[17] and not ln[23] < float("inf") and ln[29] == 0.0
    assert (masked and dof != 7) or ln[23] == float("inf")
    # the inputs are as they were
    assert torch.equal(bits(dpath), bits(keep[0])) and torch.equal(dcount, keep[1])


def test_rows_without_a_result_are_not_written_and_calls_repeat():
    from diffco_amd import _ops
    host, fused, (dpath, dcount), keep, mask = both(7, True, 65)
    out = torch.full((R, 65, 7), -7.0, device="cuda")
    got, n, ln = _ops.path_resample(dpath, dcount, 65, mask, out=out)
    assert got is out and torch.equal(n, fused.count) and torch.equal(bits(ln), bits(fused.lengths))
    dead = n == 0
    assert int(dead.sum()) == 4 and bool((out[dead] == -7.0).all())
    assert torch.equal(bits(out[~dead]), bits(fused.path[~dead]))
    # a second eager call gives the same bits
    again, n2, ln2 = _ops.path_resample(dpath, dcount, 65, mask)
    assert torch.equal(bits(again), bits(fused.path)) and torch.equal(n2, n) and torch.equal(bits(ln2), bits(ln))
    assert torch.equal(bits(dpath), bits(keep[0])) and torch.equal(dcount, keep[1])


def test_a_captured_call_replays_to_the_eager_result():
    """a single stream, no parallel branches: the call is one launch"""
    from diffco_amd import _ops
    host, fused, (dpath, dcount), keep, mask = both(7, True, 65)
    out = torch.full((R, 65, 7), -7.0, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        _, n, ln = _ops.path_resample(dpath, dcount, 65, mask, out=out)
    dead = fused.count == 0
    for _ in range(2):
        out.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(n, fused.count) and torch.equal(bits(ln), bits(fused.lengths))
        assert torch.equal(bits(out[~dead]), bits(fused.path[~dead])) and bool((out[dead] == -7.0).all())


def test_routing_cpu_tensors_take_the_host_route_to_the_same_result():
    from diffco_amd import resample_paths
    host, fused, (dpath, dcount), keep, mask = both(2, True, 64)
    cpu = resample_paths(dpath.cpu(), dcount.cpu(), n_waypoints=64, wrap=mask)
    assert cpu.route == "host" and cpu.path.device.type == "cpu" and fused.route == "fused" and fused.path.device.type == "cuda"
    _assert_same(cpu, fused)
    # a list of paths on the GPU: the fused route, the same rows
    rows = [dpath[r, :n] if n else None for r, n in enumerate(dcount.tolist())]
    lst = resample_paths(rows, n_waypoints=64, wrap=[bool((mask >> j) & 1) for j in range(2)])
    assert lst.route == "fused"
    _assert_same(lst, fused)


# ---- the chain: plan -> shortcut -> resample -> optimise ------------------------------------------------------------------------
T_CHAIN = 16
# tests/test_gpu_traj_dense.py::test_step_matches_float64_restatement's bar on a path after three steps: relerr(path) < 2e-5
PATH_RELERR = 2e-5


@functools.lru_cache(maxsize=None)
def chain():
    from diffco_amd.resample import resample_paths
    from diffco_amd.rrt import rrt_connect
    from diffco_amd.shortcut import shortcut_paths
    ck, starts, goals, lim = _baxter("cfg2_baxter_rq")
    plan = rrt_connect(ck, starts, goals, range=B["range"], max_step=B["max_step"], slots=B["P"], cap=B["cap"], max_rounds=B["rounds"],
                       rounds_per_call=B["chunk"], limits=lim, seed=11)
    path, count = plan.path_tensor()
    sc = shortcut_paths(ck, path, count, max_step=B["max_step"], slots=2, rounds=8, seed=0)
    assert plan.route == sc.route == "fused"
    solved = [r for r, n in enumerate(sc.count.tolist()) if n >= 2]
    assert len(solved) >= 2, sc.count.tolist()
    count = sc.count.clone()
    count[solved[0]] = 0           # one problem made unsolvable
    res = resample_paths(sc.path, count, n_waypoints=T_CHAIN)
    return ck, starts, goals, sc, count, res, solved


def test_chain_resampled_rows_keep_the_problems_endpoints():
    ck, starts, goals, sc, count, res, solved = chain()
    assert res.route == "fused" and res.path.shape == (B["R"], T_CHAIN, 7)
    want = [T_CHAIN if n >= 2 else 0 for n in count.tolist()]
    assert res.count.tolist() == want and want.count(T_CHAIN) >= 1 and want[solved[0]] == 0
    for r, n in enumerate(want):
        if n:
            assert torch.equal(bits(res.path[r, 0]), bits(starts[r])) and torch.equal(bits(res.path[r, -1]), bits(goals[r])), r
            # resampling does not lengthen: the chords of a polyline are no longer than its arcs
            assert float(res.lengths[r]) <= float(sc.lengths[r]) * (1 + 1e-5)
        else:
            assert bool((res.path[r] == 0).all())


def test_chain_optimize_paths_agrees_with_one_run_per_path():
    from diffco_amd import fused_adam_traj_optimize, optimize_paths
    ck, starts, goals, sc, count, res, solved = chain()
    rob = make_robot(CASE_ROBOT["cfg2_baxter_rq"])
    opts = {"MAXITER": 3, "max_speed": 0.3, "safety_margin": float(ck.margin), "extra_optimizer_options": {"lr": 0.05},
            "dense_max_samples": 64}
    recs = optimize_paths(rob, ck.model, sc.path, count, n_waypoints=T_CHAIN, options=dict(opts))
    assert len(recs) == B["R"] and [rec is None for rec in recs] == [n == 0 for n in res.count.tolist()]
    assert recs[solved[0]] is None and sum(rec is not None for rec in recs) >= 1
    for r, rec in enumerate(recs):
        if rec is None:
            continue
        assert set(rec) == {"success", "cost", "solution", "steps", "cnt_check", "frozen_on_bound"}
        sol = rec["solution"]
        assert sol.shape == (T_CHAIN, 7) and sol.device.type == "cuda" and rec["steps"] == 3 and rec["cnt_check"] > 0
        assert not rec["frozen_on_bound"]
        assert torch.equal(bits(sol[0]), bits(starts[r])) and torch.equal(bits(sol[-1]), bits(goals[r])), r
        one = fused_adam_traj_optimize(rob, ck.model, starts[r].cpu(), goals[r].cpu(),
                                       dict(opts, NUM_RE_TRIALS=1, N_WAYPOINTS=T_CHAIN, seed=0, init_solution=res.path[r].cpu(),
                                            dense_check=True))
        err = relerr(sol.cpu().numpy(), np.array(one["solution"]))
        print(f"problem {r}: success {rec['success']} / {one['success']}, cost {rec['cost']:.6g} / {one['cost']:.6g}, relerr {err:.2e}")
        assert rec["success"] == one["success"]
        assert err < PATH_RELERR, (r, err)   # (kept even where the bits agree: batch composition is not promised to keep them)
    # another robot's fkine is refused as fused_adam_traj_optimize refuses it
    with pytest.raises(ValueError, match="not this robot's fkine"):
        optimize_paths(make_robot("panda"), ck.model, sc.path, count, n_waypoints=T_CHAIN, options=dict(opts))
