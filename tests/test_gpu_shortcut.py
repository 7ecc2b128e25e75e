"""GPU: batched path shortcutting (dcx_path_shortcut_run, ScoreModel.shortcut_run, shortcut.shortcut_paths) against its referee
shortcut.host_shortcut_paths - the same contract composed of torch indexing and the checker's check_motions - bit for bit on
path[:count], count and accepted for identical draws: the paths rrt_connect returns on the 2-DoF planar arm with both joints on
the circle, random polylines on a 7-DoF Baxter fixture without a mask, and on a five-class one with per-class margins and the
slot maximum.  Then every final segment's provenance, the lengths round by round, one call of T rounds against T calls of one,
graph capture, the device-side path extraction of an RRT state (dcx_rrt_extract_paths) and the routing of shortcut_paths."""
import functools

import numpy as np
import pytest
import torch

from motion_wrap_helpers import fixture_model, mixed_margin
from test_gpu_rrt import A, B, Recorder, _baxter, _pairs, _t, case_a   # (case_a plans problem_a; _baxter's checker is a ModelChecker)

pytestmark = pytest.mark.gpu

# chosen on the GPU against host_shortcut_paths so that the coverage conditions of _covers hold
SEED_A, SEED_B, SEED_C = 9, 0, 0
ROUNDS = 24
CASE_B = dict(name="cfg2_baxter_rq", R=4, P=2, n=12)
CASE_C = dict(name="cfg3_baxter_rq_c5", R=3, P=16, n=16)


def _fixed(draws):
    at = [0]

    def sampler(T, R, P):
        out = draws[at[0]:at[0] + T]
        at[0] += T
        return out
    return sampler


def draws_for(seed, R, P, spoil):
    """[ROUNDS, R, P, 2] uniform draws; `spoil` puts a NaN, a 1.0 and a negative draw in: each idles its slot"""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(ROUNDS, R, P, 2, generator=g)
    if spoil:
        u[1, 0, 0, 0] = float("nan")
        u[2, R - 1, P - 1, 1] = 1.0
        u[3, 0, P - 1, 0] = -0.5
    return u.cuda()


def _recording():
    seen = dict(applied=0, blocked=0, lost=0, idle=0, two=0)

    def hook(live, first, free, applied):
        seen["applied"] += int(applied.sum())
        seen["blocked"] += int((live & (first != -1)).sum())
        seen["lost"] += int((free & ~applied).sum())
        seen["idle"] += int((~live).sum())
        seen["two"] += int((applied.sum(dim=1) >= 2).sum())
    return seen, hook


def run_both(ck, path, count, draws, P, max_step, wrap, fused=True):
    """(host result, its Recorder, its coverage record, fused result or None) for the same draws"""
    from diffco_amd.shortcut import host_shortcut_paths, shortcut_paths
    rec = Recorder(ck)
    seen, hook = _recording()
    kw = dict(max_step=max_step, wrap=wrap, slots=P, rounds=len(draws), rounds_per_call=5)
    host = host_shortcut_paths(rec, path, count, sampler=_fixed(draws), _record=hook, **kw)
    return host, rec, seen, shortcut_paths(ck, path, count, sampler=_fixed(draws), **kw) if fused else None


def _covers(seen, two=False):
    return min(seen["applied"], seen["blocked"], seen["lost"], seen["idle"]) >= 1 and (not two or seen["two"] >= 1)


def _assert_same(a, b):
    assert torch.equal(a.count, b.count), (a.count.tolist(), b.count.tolist())
    assert torch.equal(a.accepted, b.accepted), (a.accepted.tolist(), b.accepted.tolist())
    for r, n in enumerate(a.count.tolist()):
        assert torch.equal(a.path[r, :n].contiguous().view(torch.int32), b.path[r, :n].contiguous().view(torch.int32)), r


@functools.lru_cache(maxsize=None)
def input_a():
    """(checker, wrap mask, the planner's result, path [6, W, 2], count): the paths rrt_connect returns for problem_a, the
    unsolved problems as count = 0 rows, the direct one as 2 points, W = the longest path"""
    d, dc, starts, goals, samples, kw, host, rec, fused = case_a()
    path, count = fused.path_tensor()
    assert path.shape[1] == int(count.max()) and count.tolist().count(0) >= 2 and 2 in count.tolist()
    return dc, kw["wrap"], fused, path, count


@functools.lru_cache(maxsize=None)
def polylines(name, R, n, seed=5):
    """(checker, R random n-waypoint polylines of configurations the checker accepts); path 0 runs between the nearest pair of a
    sample whose direct motion the checker accepts (test_gpu_rrt's _pairs, hard=False).  A segment may collide: the contract
    only checks new edges."""
    ck = _baxter(name)[0]
    d = fixture_model(name)[0]
    q = _t(d["q"])
    free = q[((ck.model.score_raw(q) - _t(mixed_margin(d))[None]) <= 0).all(dim=1)]
    check = lambda a, b: ck.check_motions(a, b, max_step=B["max_step"], max_samples=200)[0]   # noqa: E731
    i, j = _pairs(check, free, 1, hard=False)[0]
    g = np.random.default_rng(seed)
    paths = []
    for r in range(R):
        p = free[torch.as_tensor(g.choice(len(free), n, replace=False), device="cuda")].clone()
        if r == 0:
            p[0], p[-1] = free[i], free[j]
        paths.append(p)
    return ck, paths


@functools.lru_cache(maxsize=None)
def run_a(seed=SEED_A, fused=True):
    dc, wrap, _, path, count = input_a()
    return run_both(dc, path, count, draws_for(seed, A["R"], 3, False), 3, A["max_step"], wrap, fused)


@functools.lru_cache(maxsize=None)
def run_baxter(which, seed, fused=True):
    c = CASE_B if which == "b" else CASE_C
    ck, paths = polylines(c["name"], c["R"], c["n"])
    return run_both(ck, list(paths), None, draws_for(seed, c["R"], c["P"], True), c["P"], B["max_step"], None, fused)


def test_case_a_fused_equals_host_bit_for_bit():
    host, rec, seen, fused = run_a()
    print("case a:", seen, "counts", host.count.tolist(), "accepted", host.accepted.tolist())
    assert fused.route == "fused" and host.route == "host"
    _assert_same(fused, host)
    assert _covers(seen, two=True), seen
    before = input_a()[4].tolist()
    assert [n for n, b in zip(host.count.tolist(), before) if b < 3] == [b for b in before if b < 3]   # nothing to cut there


@pytest.mark.parametrize("which,seed", [("b", SEED_B), ("c", SEED_C)])
def test_baxter_fused_equals_host_bit_for_bit(which, seed):
    """cases (b) and (c): 7 DoF, no mask, one class with a margin; five classes with a margin each, 16 slots, W = 16"""
    host, rec, seen, fused = run_baxter(which, seed)
    print("case", which, seen, "counts", host.count.tolist(), "accepted", host.accepted.tolist())
    assert fused.route == "fused" and host.route == "host"
    assert fused.path.shape[1] == (CASE_B if which == "b" else CASE_C)["n"]
    _assert_same(fused, host)
    assert _covers(seen), seen


def test_long_paths_compact_over_several_chunks():
    """case (b)'s polylines with a waypoint every 0.05 along their segments (subdivide): hundreds of waypoints of 7 floats, so the
    commit kernel's in-place compaction runs over several of its 1024-float chunks, with up to 8 disjoint cuts in one round"""
    from diffco_amd.shortcut import host_shortcut_paths, shortcut_paths
    ck, paths = polylines(CASE_B["name"], CASE_B["R"], CASE_B["n"])
    R, P, T = CASE_B["R"], 8, 12
    u = torch.rand(T, R, P, 2, generator=torch.Generator().manual_seed(1)).cuda()
    seen, hook = _recording()
    kw = dict(max_step=B["max_step"], slots=P, rounds=T, rounds_per_call=4, subdivide=0.05)
    host = host_shortcut_paths(Recorder(ck), list(paths), sampler=_fixed(u), _record=hook, **kw)
    fused = shortcut_paths(ck, list(paths), sampler=_fixed(u), **kw)
    print("long paths:", seen, "W", fused.path.shape[1], "counts", host.count.tolist(), "accepted", host.accepted.tolist())
    assert fused.route == "fused" and host.route == "host"
    assert fused.path.shape[1] * 7 > 3 * 1024          # more than three chunks of floats in a row
    _assert_same(fused, host)
    assert seen["applied"] >= 1 and seen["two"] >= 1 and int(fused.count.max()) < fused.path.shape[1]
    for r, p in enumerate(paths):
        assert torch.equal(fused.paths[r][0], p[0]) and torch.equal(fused.paths[r][-1], p[-1])
    # (float32 sums of up to ~1000 segment lengths: 1000 * 2^-24 = 6e-5 at the worst)
    assert all(b <= a * (1 + 1e-4) for a, b in zip(fused.lengths_before.tolist(), fused.lengths.tolist()))


def _rows(t):
    return [bytes(x) for x in np.ascontiguousarray(t.detach().cpu().numpy(), np.float32).view(np.uint8).reshape(len(t), -1)]


@pytest.mark.parametrize("which", ["a", "b", "c"])
def test_provenance(which):
    """every round submitted exactly R * P edges; every segment of a final path is a segment of the input path or an edge some
    recorded batch answered -1; the endpoints are the input's, bit for bit"""
    if which == "a":
        host, rec, seen, fused = run_a()
        _, _, _, path, count = input_a()
        before = [path[r, :n] for r, n in enumerate(count.tolist())]
        R, P = A["R"], 3
    else:
        c = CASE_B if which == "b" else CASE_C
        host, rec, seen, fused = run_baxter(which, SEED_B if which == "b" else SEED_C)
        before = polylines(c["name"], c["R"], c["n"])[1]
        R, P = c["R"], c["P"]
    assert len(rec.calls) == ROUNDS and {len(qa) for qa, _, _ in rec.calls} == {R * P}
    answered = set()
    for qa, qb, first in rec.calls:
        ok = (first == -1).cpu().numpy()
        answered.update(a + b for a, b, f in zip(_rows(qa), _rows(qb), ok) if f)
    shortened = 0
    for r in range(R):
        n = int(fused.count[r])
        assert n == len(before[r]) or 2 <= n < len(before[r])
        if n == 0:
            continue
        got, was = _rows(fused.path[r, :n]), _rows(before[r])
        assert got[0] == was[0] and got[-1] == was[-1]
        given = {a + b for a, b in zip(was[:-1], was[1:])}
        for a, b in zip(got[:-1], got[1:]):
            assert a + b in given or a + b in answered, (r, "a segment nobody checked")
        shortened += n < len(was)
    assert shortened >= 1


def _len64(p, on):
    p = p.astype(np.float64)
    d = p[1:] - p[:-1]
    d = np.where(on[None], (d + np.pi) % (2 * np.pi) - np.pi, d)
    return float(np.linalg.norm(d, axis=1).sum())


def _raw_a():
    """case (a)'s model, margin, initial state, draws and the raw call"""
    dc, wrap, _, path, count = input_a()
    model, margin = dc._rrt_model(torch.device("cuda"))
    init = dict(path=path.clone(), count=count.clone(), accepted=torch.zeros_like(count))
    longest = float(run_a()[0].lengths_before.nan_to_num(0.0).max())
    ms = int(np.ceil(longest / A["max_step"])) + 2
    run = lambda st, u: model.shortcut_run(st, u, A["max_step"], ms, margin=margin, wrap=wrap)   # noqa: E731
    return init, draws_for(SEED_A, A["R"], 3, False), run


def test_no_round_lengthens_a_path():
    """float64 lengths of the fp32 waypoints, the wrapped delta on the masked joints: the triangle inequality of the metric; the
    1e-9 covers the float64 summation only"""
    init, draws, run = _raw_a()
    st = {k: v.clone() for k, v in init.items()}
    on = np.array([True, True])
    length = lambda: [_len64(st["path"][r, :n].cpu().numpy(), on) for r, n in enumerate(st["count"].tolist())]   # noqa: E731
    was, cuts = length(), 0
    for t in range(ROUNDS):
        run(st, draws[t:t + 1].contiguous())
        now = length()
        for r, (a, b) in enumerate(zip(was, now)):
            assert b <= a * (1 + 1e-9), (t, r, a, b)
            cuts += b < a
        was = now
    print("case a: lengths", length(), "rounds that shortened a path", cuts)
    assert cuts >= 1
    # the rounds one by one end where shortcut_paths ended
    fused = run_a()[3]
    assert torch.equal(st["count"], fused.count) and torch.equal(st["accepted"], fused.accepted)
    for r, n in enumerate(fused.count.tolist()):
        assert torch.equal(st["path"][r, :n], fused.path[r, :n])


def _same_state(a, b):
    assert torch.equal(a["count"], b["count"]) and torch.equal(a["accepted"], b["accepted"])
    for r, n in enumerate(a["count"].tolist()):
        assert torch.equal(a["path"][r, :n], b["path"][r, :n]), r


def test_one_call_of_eight_rounds_equals_eight_calls_of_one():
    init, draws, run = _raw_a()
    one = {k: v.clone() for k, v in init.items()}
    run(one, draws[:8].contiguous())
    many = {k: v.clone() for k, v in init.items()}
    for t in range(8):
        run(many, draws[t:t + 1].contiguous())
    again = {k: v.clone() for k, v in init.items()}
    run(again, draws[:8].contiguous())
    torch.cuda.synchronize()
    _same_state(one, many)
    _same_state(one, again)
    assert int(one["accepted"].sum()) >= 1 and int(one["count"].sum()) < int(init["count"].sum())
    # T = 0 launches nothing and changes nothing
    run(one, draws[:0].contiguous())
    _same_state(one, again)


def test_a_captured_call_replays_to_the_eager_result():
    init, draws, run = _raw_a()
    u = draws[:4].contiguous()
    want = {k: v.clone() for k, v in init.items()}
    run(want, u)
    st = {k: v.clone() for k, v in init.items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(st, u)
    torch.cuda.current_stream().wait_stream(s)
    _same_state(st, want)
    for k in st:
        st[k].copy_(init[k])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run(st, u)
    for _ in range(2):
        for k in st:
            st[k].copy_(init[k])
        g.replay()
        torch.cuda.synchronize()
        _same_state(st, want)
    assert int(want["accepted"].sum()) >= 1


# ---- dcx_rrt_extract_paths -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _baxter_plan():
    from diffco_amd.rrt import rrt_connect
    ck, starts, goals, lim = _baxter("cfg2_baxter_rq")
    return rrt_connect(ck, starts, goals, range=B["range"], max_step=B["max_step"], slots=B["P"], cap=B["cap"], max_rounds=B["rounds"],
                       rounds_per_call=B["chunk"], limits=lim, seed=11)


@pytest.mark.parametrize("which", ["a", "b"])
def test_path_tensor_rows_equal_paths(which):
    from diffco_amd import _ops
    res = case_a()[-1] if which == "a" else _baxter_plan()
    assert res.route == "fused"
    path, count = res.path_tensor()
    sizes = [0 if p is None else len(p) for p in res.paths]
    print("case", which, "status", res.status.tolist(), "waypoints", sizes)
    assert count.dtype == torch.int32 and count.tolist() == sizes and path.shape == (len(sizes), max(sizes), res.nodes.shape[3])
    assert max(sizes) > 2
    for r, p in enumerate(res.paths):
        if p is not None:
            assert torch.equal(path[r, :len(p)].view(torch.int32), p.contiguous().view(torch.int32)), r
        assert bool((path[r, sizes[r]:] == 0).all())
    if which == "a":   # unsolved (full) and blocked problems give 0
        assert {s for s, n in zip(res.status.tolist(), sizes) if n == 0} >= {2, 3}
    # the size query: W = 0, no path buffer
    empty, n0 = _ops.rrt_extract_paths(res.state(), 0)
    assert empty.numel() == 0 and n0.tolist() == [-n for n in sizes]
    # one row short of the longest path: that row is left as it was, the others are written
    W = max(sizes) - 1
    out = torch.full((len(sizes), W, res.nodes.shape[3]), -7.0, device="cuda")
    got, n1 = _ops.rrt_extract_paths(res.state(), W, out=out)
    assert got is out and n1.tolist() == [n if n <= W else -n for n in sizes]
    for r, p in enumerate(res.paths):
        if sizes[r] > W:
            assert bool((out[r] == -7.0).all())
        elif p is not None:
            assert torch.equal(out[r, :len(p)], p) and bool((out[r, len(p):] == -7.0).all())
        else:
            assert bool((out[r] == -7.0).all())
    # the CPU state is walked on the host to the same rows
    from diffco_amd.rrt import RRTResult
    cpu = RRTResult("host", {k: v.cpu() for k, v in res.state().items()}, None, None, None)
    hp, hc = cpu.path_tensor()
    assert torch.equal(hc, count.cpu()) and torch.equal(hp, path.cpu())
    assert cpu.path_tensor(W)[1].tolist() == n1.tolist()


def test_extraction_bounds_every_walk():
    """a chain that does not reach -1 within cap hops, or leaves the tree, gives count 0; the other problems are not disturbed"""
    from diffco_amd import _ops
    res = case_a()[-1]
    sizes = [0 if p is None else len(p) for p in res.paths]
    solved = [r for r, n in enumerate(sizes) if n > 2]
    assert len(solved) >= 2
    st = {k: v.clone() for k, v in res.state().items()}
    r0, r1 = solved[0], solved[1]
    i0 = int(st["link"][r0, 0])
    st["parent"][r0, 0, i0] = i0                    # a cycle
    st["link"][r1, 1] = A["cap"] + 5                # a link beyond the tree
    path, count = _ops.rrt_extract_paths(st, max(sizes))
    want = [0 if r in (r0, r1) else n for r, n in enumerate(sizes)]
    assert count.tolist() == want
    assert bool((path[r0] == 0).all()) and bool((path[r1] == 0).all())
    st["link"][r1, 1] = -1                          # a solved problem without a link node
    st["parent"][r0, 0, i0] = -5                    # a parent that is neither a node nor -1
    assert _ops.rrt_extract_paths(st, max(sizes))[1].tolist() == want


# ---- routing ---------------------------------------------------------------------------------------------------------------------
def test_routing_cpu_tensors_take_the_host_route_to_the_same_result():
    from diffco_amd.shortcut import shortcut_paths
    dc, wrap, _, path, count = input_a()
    host, rec, seen, fused = run_a()
    draws = draws_for(SEED_A, A["R"], 3, False)
    cpu = shortcut_paths(dc, path.cpu(), count.cpu(), max_step=A["max_step"], wrap=wrap, slots=3, rounds=ROUNDS, rounds_per_call=5,
                         sampler=_fixed(draws.cpu()))
    assert cpu.route == "host" and cpu.path.device.type == "cpu" and fused.route == "fused"
    assert torch.equal(cpu.count, fused.count.cpu()) and torch.equal(cpu.accepted, fused.accepted.cpu())
    for r, n in enumerate(cpu.count.tolist()):
        assert torch.equal(cpu.path[r, :n], fused.path[r, :n].cpu())
    # the default sampler and max_samples: a seeded run repeats itself, whatever the chunking
    a = shortcut_paths(dc, path, count, max_step=A["max_step"], wrap=wrap, slots=3, rounds=12, rounds_per_call=12, seed=3)
    b = shortcut_paths(dc, path, count, max_step=A["max_step"], wrap=wrap, slots=3, rounds=12, rounds_per_call=5, seed=3)
    assert a.route == "fused"
    _assert_same(a, b)
    assert all((x <= y * (1 + 1e-6)) or (x != x) for x, y in zip(a.lengths.tolist(), a.lengths_before.tolist()))


def test_routing_of_the_facades():
    """ForwardKinematicsDiffCo shortcuts fused; the hybrid facade goes through its own check_motions; with a zero band it
    answers as the plain one on the same perceptron, so the results are equal"""
    from diffco_amd import kernel
    from diffco_amd.collision_checkers import ForwardKinematicsDiffCo, HybridForwardKinematicsDiffCo
    from diffco_amd.shortcut import shortcut_paths
    from helpers import load, urdf_robot
    rob = urdf_robot("urdf_panda_nogripper")
    d = load("cfg2_panda_rq")
    w = torch.as_tensor(d["weights"][:300, 0], dtype=torch.float32)

    def facade(cls, **extra):
        ck = cls(robot=rob, gamma=10, **extra)
        p = ck.perceptron
        p.support_points = torch.as_tensor(d["sup_q"][:300], dtype=torch.float32).cuda()
        p.support_transformed = rob.fkine(p.support_points)
        p.rbf_kernel = kernel.Polyharmonic(1, 1.0)
        p.rbf_nodes = (w - w.mean()).cuda()
        ck.safety_bias = 0.0
        return ck

    plain = facade(ForwardKinematicsDiffCo)
    hybrid = facade(HybridForwardKinematicsDiffCo, gt_check_func=lambda q: torch.as_tensor(q).reshape(-1, 7)[:, 0] > 0)
    torch.manual_seed(6)
    q = rob.rand_configs(400).cuda()
    free = q[~plain.collision(q).reshape(len(q), -1).any(dim=1)]
    assert len(free) >= 40
    g = np.random.default_rng(2)
    paths = [free[torch.as_tensor(g.choice(len(free), 8, replace=False), device="cuda")].clone() for _ in range(3)]
    out = {}
    for name, ck in (("plain", plain), ("hybrid", hybrid)):
        out[name] = shortcut_paths(ck, paths, max_step=0.25, slots=4, rounds=8, rounds_per_call=4, seed=4)
    print("facades: counts", out["plain"].count.tolist(), "accepted", out["plain"].accepted.tolist())
    assert out["plain"].route == "fused" and out["hybrid"].route == "host"
    _assert_same(out["plain"], out["hybrid"])
    assert int(out["plain"].accepted.sum()) >= 1 and hybrid.last_gt_checks == 0
