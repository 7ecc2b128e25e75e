"""GPU: partial path shortcuts (dcx_path_shortcut_partial_run, ScoreModel.shortcut_run(partial=True),
shortcut.shortcut_paths(partial=True)) against their referee shortcut.host_shortcut_paths(partial=True) - the same contract in
torch ops and the checker's check_motions - bit for bit on path[:count], count and accepted for identical draws: the paths
rrt_connect returns on the 2-DoF planar arm with both joints on the circle, random polylines on a 7-DoF Baxter fixture without a
mask, and on a five-class one with per-class margins, the slot maximum, a mask on some joints and no room to grow.  Then a path
longer than the pick block's LDS table, the lengths round by round, one call of T rounds against T calls of one, graph capture
and the routing of shortcut_paths."""
import functools

import numpy as np
import pytest
import torch

from motion_wrap_helpers import fixture_model, mixed_margin
from test_gpu_rrt import A, B, Recorder, _t
from test_gpu_shortcut import CASE_B, CASE_C, ROUNDS, _assert_same, _fixed, _len64, _same_state, input_a, polylines

pytestmark = pytest.mark.gpu

# chosen by running the host route (host_shortcut_paths(partial=True)) alone over seeds 0 .. 7, so that the coverage conditions
# of EVENTS hold in every case ("capacity" in case (c), whose capacity is the longest count)
SEED_A, SEED_B, SEED_C = 6, 4, 1
MASK_C = 0b0100101   # joints 0, 2 and 5 of 7 on the circle
EVENTS = ("applied", "two", "lost", "blocked", "idle_draw", "idle_same", "grew")


def draws_for(seed, R, P, row, rounds=ROUNDS):
    """[rounds, R, P, 2] uniform draws with a NaN, a 1.0 and a negative draw on path `row` (one with three waypoints or more):
    each idles its slot"""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(rounds, R, P, 2, generator=g)
    u[1, row, 0, 0] = float("nan")
    u[2, row, P - 1, 1] = 1.0
    u[3, row, P - 1, 0] = -0.5
    return u.cuda()


def _recording():
    seen = dict.fromkeys(EVENTS + ("capacity",), 0)

    def hook(live, first, free, applied, more):
        grew = applied & (more["eb"] == more["ea"] + 1)
        seen["applied"] += int(applied.sum())
        seen["two"] += int((applied.sum(dim=1) >= 2).sum())
        seen["lost"] += int((free & ~more["apart"]).sum())
        seen["blocked"] += int((live & (first != -1)).sum())
        seen["idle_draw"] += int((more["has"][:, None] & ~more["drawn"]).sum())
        seen["idle_same"] += int((more["drawn"] & ~live).sum())
        seen["grew"] += int(grew.sum())
        seen["capacity"] += int((more["apart"] & ~applied).sum())
    return seen, hook


def run_both(ck, path, count, draws, P, max_step, wrap, capacity=None, fused=True):
    """(host result, its Recorder, its coverage record, fused result or None) for the same draws"""
    from diffco_amd.shortcut import host_shortcut_paths, shortcut_paths
    rec = Recorder(ck)
    seen, hook = _recording()
    kw = dict(max_step=max_step, wrap=wrap, slots=P, rounds=len(draws), rounds_per_call=5, partial=True, capacity=capacity)
    host = host_shortcut_paths(rec, path, count, sampler=_fixed(draws), _record=hook, **kw)
    return host, rec, seen, shortcut_paths(ck, path, count, sampler=_fixed(draws), **kw) if fused else None


def _covers(seen, capacity=False):
    return all(seen[what] >= 1 for what in EVENTS + (("capacity",) if capacity else ()))


@functools.lru_cache(maxsize=None)
def run_a(seed=SEED_A, fused=True):
    dc, wrap, _, path, count = input_a()
    row = next(r for r, n in enumerate(count.tolist()) if n >= 3)
    return run_both(dc, path, count, draws_for(seed, A["R"], 3, row), 3, A["max_step"], wrap, None, fused)


@functools.lru_cache(maxsize=None)
def run_baxter(which, seed, fused=True):
    c = CASE_B if which == "b" else CASE_C
    ck, paths = polylines(c["name"], c["R"], c["n"])
    # case (c): a mask on some but not all joints, and capacity = the longest count, so that the capacity rule decides something
    wrap, capacity = (None, None) if which == "b" else (MASK_C, c["n"])
    return run_both(ck, list(paths), None, draws_for(seed, c["R"], c["P"], 0), c["P"], B["max_step"], wrap, capacity, fused)


def test_case_a_fused_equals_host_bit_for_bit():
    host, rec, seen, fused = run_a()
    before = input_a()[4].tolist()
    print("case a:", seen, "counts", before, "->", host.count.tolist(), "accepted", host.accepted.tolist())
    assert fused.route == "fused" and host.route == "host"
    assert fused.path.shape[1] == max(before) + 16   # the default capacity: the longest count + the slot maximum
    _assert_same(fused, host)
    assert _covers(seen), seen
    assert before.count(0) >= 2 and 2 in before
    assert [n for n, b in zip(host.count.tolist(), before) if b < 3] == [b for b in before if b < 3]   # nothing to cut there
    assert len(rec.calls) == ROUNDS and {len(qa) for qa, _, _ in rec.calls} == {A["R"] * 3}           # the fixed batch


@pytest.mark.parametrize("which,seed", [("b", SEED_B), ("c", SEED_C)])
def test_baxter_fused_equals_host_bit_for_bit(which, seed):
    """cases (b) and (c): 7 DoF, no mask, one class with a margin; five classes with a margin each, 16 slots, three joints on the
    circle, W = 16 = the longest count"""
    c = CASE_B if which == "b" else CASE_C
    host, rec, seen, fused = run_baxter(which, seed)
    print("case", which, seen, "counts", host.count.tolist(), "accepted", host.accepted.tolist())
    assert fused.route == "fused" and host.route == "host"
    assert fused.path.shape[1] == (c["n"] + 16 if which == "b" else c["n"])
    _assert_same(fused, host)
    assert _covers(seen, capacity=which == "c"), seen
    assert int(fused.count.max()) <= fused.path.shape[1]
    assert len(rec.calls) == ROUNDS and {len(qa) for qa, _, _ in rec.calls} == {c["R"] * c["P"]}
    for r, p in enumerate(polylines(c["name"], c["R"], c["n"])[1]):
        assert torch.equal(fused.paths[r][0], p[0]) and torch.equal(fused.paths[r][-1], p[-1])


def test_a_path_longer_than_the_lds_table():
    """2100 waypoints: c and len of that row live in the workspace, not in the pick block's LDS (2048 waypoints).  The row is a
    random walk inside the accepted set; half of the slots draw two positions close together, so that some chord is free"""
    from diffco_amd.shortcut import host_shortcut_paths, shortcut_paths
    name = CASE_B["name"]
    ck, short = polylines(name, CASE_B["R"], CASE_B["n"])
    mg = _t(mixed_margin(fixture_model(name)[0]))[None]
    g = torch.Generator(device="cuda").manual_seed(4)
    walk = [short[0][0]]
    while len(walk) < 2100:
        cand = walk[-1][None] + torch.cumsum(0.03 * torch.randn(32, 7, generator=g, device="cuda"), dim=0)
        ok = ((ck.model.score_raw(cand) - mg) <= 0).all(dim=1)
        walk.extend(cand[:int(ok.to(torch.int32).cumprod(dim=0).sum())])   # (the steps up to the first refused one)
    walk = torch.stack(walk[:2100])
    R, P, T, W = 2, 4, 3, 2104
    u = torch.rand(T, R, P, 2, generator=torch.Generator().manual_seed(2))
    u[:, :, :2, 1] = (u[:, :, :2, 0] + 0.004 * torch.rand(T, R, 2)).clamp(max=0.999)
    u = u.cuda()
    seen, hook = _recording()
    kw = dict(max_step=B["max_step"], slots=P, rounds=T, rounds_per_call=2, partial=True, capacity=W)
    host = host_shortcut_paths(Recorder(ck), [walk, short[1]], sampler=_fixed(u), _record=hook, **kw)
    fused = shortcut_paths(ck, [walk, short[1]], sampler=_fixed(u), **kw)
    print("long path:", seen, "counts", host.count.tolist(), "accepted", host.accepted.tolist())
    assert fused.route == "fused" and host.route == "host" and fused.path.shape[1] == W > 2048
    _assert_same(fused, host)
    assert int(host.accepted[0]) >= 1 and seen["applied"] >= 1
    assert torch.equal(fused.paths[0][0], walk[0]) and torch.equal(fused.paths[0][-1], walk[-1])


def _raw_a():
    """case (a)'s model, margin, initial state (W = the default capacity), draws and the raw call"""
    dc, wrap, _, path, count = input_a()
    model, margin = dc._rrt_model(torch.device("cuda"))
    host = run_a()[0]
    W = host.path.shape[1]
    grown = torch.zeros((len(path), W, 2), device="cuda")
    grown[:, :path.shape[1]] = path
    init = dict(path=grown, count=count.clone(), accepted=torch.zeros_like(count))
    longest = float(host.lengths_before.nan_to_num(0.0).max())
    ms = int(np.ceil(longest / A["max_step"])) + 2
    run = lambda st, u: model.shortcut_run(st, u, A["max_step"], ms, margin=margin, wrap=wrap, partial=True)   # noqa: E731
    row = next(r for r, n in enumerate(count.tolist()) if n >= 3)
    return init, draws_for(SEED_A, A["R"], 3, row), run


def test_no_round_lengthens_a_path():
    """float64 lengths of the fp32 waypoints, the wrapped delta on the masked joints, under test_gpu_shortcut's tolerance; the
    endpoints keep their bits and count never exceeds W, round by round"""
    init, draws, run = _raw_a()
    st = {k: v.clone() for k, v in init.items()}
    W = st["path"].shape[1]
    on = np.array([True, True])
    length = lambda: [_len64(st["path"][r, :n].cpu().numpy(), on) for r, n in enumerate(st["count"].tolist())]   # noqa: E731
    ends = lambda: [(st["path"][r, 0].clone(), st["path"][r, max(n - 1, 0)].clone()) for r, n in enumerate(st["count"].tolist())]   # noqa: E731
    was, first, cuts, worst = length(), ends(), 0, 0.0
    for t in range(ROUNDS):
        run(st, draws[t:t + 1].contiguous())
        now = length()
        assert int(st["count"].max()) <= W
        for r, (a, b) in enumerate(zip(was, now)):
            worst = max(worst, (b - a) / a if a > 0 else 0.0)
            cuts += b < a
        for (a0, a1), (b0, b1) in zip(first, ends()):
            assert torch.equal(a0.view(torch.int32), b0.view(torch.int32)) and torch.equal(a1.view(torch.int32), b1.view(torch.int32))
        was = now
    print("case a: lengths", length(), "rounds that shortened a path", cuts, "largest relative growth of a round", worst)
    assert worst <= 1e-9, worst
    assert cuts >= 1
    # the rounds one by one end where shortcut_paths ended
    fused = run_a()[3]
    assert torch.equal(st["count"], fused.count) and torch.equal(st["accepted"], fused.accepted)
    for r, n in enumerate(fused.count.tolist()):
        assert torch.equal(st["path"][r, :n], fused.path[r, :n])


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
    assert int(one["accepted"].sum()) >= 1
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


# ---- routing ---------------------------------------------------------------------------------------------------------------------
def test_routing_cpu_tensors_and_unfused_checkers_take_the_host_route_to_the_same_result():
    from diffco_amd.shortcut import shortcut_paths
    dc, wrap, _, path, count = input_a()
    host, rec, seen, fused = run_a()
    row = next(r for r, n in enumerate(count.tolist()) if n >= 3)
    draws = draws_for(SEED_A, A["R"], 3, row)
    kw = dict(max_step=A["max_step"], wrap=wrap, slots=3, rounds=ROUNDS, rounds_per_call=5, partial=True)
    cpu = shortcut_paths(dc, path.cpu(), count.cpu(), sampler=_fixed(draws.cpu()), **kw)
    assert cpu.route == "host" and cpu.path.device.type == "cpu" and fused.route == "fused"
    assert torch.equal(cpu.count, fused.count.cpu()) and torch.equal(cpu.accepted, fused.accepted.cpu())
    for r, n in enumerate(cpu.count.tolist()):
        assert torch.equal(cpu.path[r, :n], fused.path[r, :n].cpu())
    plain = shortcut_paths(Recorder(dc), path, count, sampler=_fixed(draws), **kw)   # a checker without a fused model
    assert plain.route == "host"
    _assert_same(plain, fused)


def test_partial_false_is_todays_shortcut_paths():
    from diffco_amd.shortcut import shortcut_paths
    from test_gpu_shortcut import SEED_A as VERTEX_SEED, draws_for as vertex_draws, run_a as vertex_run_a
    dc, wrap, _, path, count = input_a()
    today = vertex_run_a()[3]
    draws = vertex_draws(VERTEX_SEED, A["R"], 3, False)
    same = shortcut_paths(dc, path, count, max_step=A["max_step"], wrap=wrap, slots=3, rounds=ROUNDS, rounds_per_call=5,
                          sampler=_fixed(draws), partial=False)
    assert same.route == "fused" and same.path.shape == today.path.shape
    _assert_same(same, today)
    assert int(today.accepted.sum()) >= 1
