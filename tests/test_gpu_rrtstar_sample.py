"""GPU: RRT*'s samples drawn on the device (dcx_rrtstar_sample, dcx_rrtstar_run_sampled, rrt_star(sampling=...)) against the
referee rrtstar.host_device_samples.  The raw draw on hand-made states mixing running, direct, blocked, solved and unsolved
problems at R in {3, 256}, P in {1, 16}, dof in {2, 7, 32}: uniform mode bit for bit; informed mode against the referee's float64
candidate of the try the kernel names, to the project's parity bar, every accepted sample inside the informed set; 65 536 draws
of one geometry mapped back to the unit ball and held to its moments.  Then the run call on test_gpu_rrtstar.py's planar case S
and Baxter problems: the recorded samples replayed through host_rrt_star and through the fused planner leave the same state bit
for bit, the samples agree with the referee round by round on the traced states, one call of eight rounds equals eight calls
of one, a captured call replays to the eager result, seeds reproduce and differ, and the routing of rrt_star."""
import functools
import math

import pytest
import torch

from rrtstar_helpers import STATE, Recorder, assert_same_state, fixed
from rrtstar_sample_helpers import (BAXTER_MASK, GOAL_BIAS, TRIES, assert_in_informed_set, assert_matches_referee, make_state)
from test_gpu_rrtstar import B, G, _baxter, kwargs_s, problem_s

pytestmark = pytest.mark.gpu

SEED_S = 3   # case S: chosen on the GPU so that a hard problem reaches its goal early and draws informed rounds after it
SHAPES = [(R, P, dof) for R in (3, 256) for P in (1, 16) for dof in (2, 7, 32)]


def _cuda(st):
    return {k: v.cuda() for k, v in st.items()}


@pytest.mark.parametrize("R,P,dof", SHAPES)
def test_uniform_mode_is_the_referees_bit_for_bit(R, P, dof):
    from diffco_amd import _ops
    from diffco_amd.rrtstar import host_device_samples
    st, goals, lim = make_state(R, dof, 0, seed=R + P + dof)
    smp, info = _ops.rrtstar_sample(_cuda(st), goals.cuda(), lim.cuda(), 1234567 + (9 << 32), 5, P, mode="uniform", goal_bias=GOAL_BIAS)
    want, winfo, _ = host_device_samples(st, goals, lim, 1234567 + (9 << 32), 5, P, "uniform", GOAL_BIAS, 0., TRIES, 0)
    assert torch.equal(info.cpu(), winfo)
    assert torch.equal(smp.cpu().view(torch.int32), want.view(torch.int32))
    kinds = set(winfo.reshape(-1).tolist())
    assert kinds <= {-1, 0, 1} and 0 in kinds and (R * P < 64 or kinds == {-1, 0, 1})


@pytest.mark.parametrize("wrapped", [False, True])
@pytest.mark.parametrize("R,P,dof", SHAPES)
def test_informed_mode_against_fp64(R, P, dof, wrapped):
    from diffco_amd import _ops
    mask = 0 if not wrapped else (3 if dof == 2 else BAXTER_MASK)
    st, goals, lim = make_state(R, dof, mask, seed=R + P + dof)
    seed, g = 99 + (3 << 32), 7
    smp, info = _ops.rrtstar_sample(_cuda(st), goals.cuda(), lim.cuda(), seed, g, P, mode="informed", goal_bias=GOAL_BIAS,
                                    uniform_mix=0.125, tries=TRIES, wrap=mask)
    counts = assert_matches_referee(smp, info, st, goals, lim, seed, g, "informed", mask, uniform_mix=0.125)
    accepted = assert_in_informed_set(smp, info, st, goals, mask)
    print(R, P, dof, mask, "info", counts)
    assert accepted >= 1 and bool(((lim[:, 0] <= smp.cpu()) & (smp.cpu() < lim[:, 1]))[info.cpu() != -1].all())
    if R == 256 and P == 16 and mask != (1 << dof) - 1:   # the corner problem's ellipsoid pokes out of the limits: 16 draws of it
        assert any(k > 2 for k in counts)


def test_uniform_in_the_ball():
    """one geometry on 256 problems x 16 slots x 16 rounds, limits wide enough that every draw is try 0 (rejection would
    truncate the distribution): mapped back to the unit ball in float64, |u|^dof is uniform on [0, 1] and every coordinate has
    the ball's mean 0 and mean square 1 / (dof + 2), each within six standard errors of the uniform ball's own moments"""
    from diffco_amd import _ops
    R, P, T, dof = 256, 16, 16, 7
    lim = torch.tensor([[-8.0, 8.0]] * dof)
    start = torch.tensor([0.3, -0.2, 0.5, 0.1, -0.4, 0.2, 0.0])
    goal = torch.tensor([-0.9, 0.7, 1.1, -0.6, 0.3, -0.8, 0.9])
    st, goals, _ = make_state(R, dof, 0, limits=lim)
    st["nodes"][:, 0] = start
    goals = goal[None].repeat(R, 1)
    a = (goal - start).to(torch.float64)
    cmin = float(a.norm())
    c = torch.tensor(1.5 * cmin, dtype=torch.float32)
    st["status"][:], st["goal_node"][:], st["cost"][:, 2] = 0, 2, c
    dst, dgoals, dlim = _cuda(st), goals.cuda(), lim.cuda()
    draws = [_ops.rrtstar_sample(dst, dgoals, dlim, 2024, g, P, mode="informed", goal_bias=GOAL_BIAS, tries=TRIES) for g in range(T)]
    info = torch.stack([d[1] for d in draws]).cpu()
    assert bool((info == 2).all())
    x = torch.stack([d[0] for d in draws]).cpu().to(torch.float64).reshape(-1, dof)
    N = len(x)
    assert N == 65536
    # H is its own inverse: y = H (x - centre), u = y / radii
    ah = a / cmin
    v = ah.clone()
    v[0] += -1.0 if ah[0] < 0 else 1.0
    d = x - (start.to(torch.float64) + a / 2)
    y = d - 2.0 * v[None] * (d @ v)[:, None] / (v @ v)
    c64 = float(c)
    radii = torch.full((dof,), math.sqrt(c64 * c64 - cmin * cmin) / 2, dtype=torch.float64)
    radii[0] = c64 / 2
    u = y / radii
    rad = u.norm(dim=1)
    assert float(rad.max()) <= 1 + 1e-5
    assert abs(float((rad ** dof).mean()) - 0.5) <= 6 * math.sqrt(1 / 12 / N)
    m2 = 1 / (dof + 2)
    assert float(u.mean(dim=0).abs().max()) <= 6 * math.sqrt(m2 / N)
    m4 = 3 / ((dof + 2) * (dof + 4))
    assert float(((u * u).mean(dim=0) - m2).abs().max()) <= 6 * math.sqrt((m4 - m2 * m2) / N)


def _referee_rounds(res, init, trace, goals, lim, seed, mask, **kw):
    """res.samples / sample_info against the referee round by round on the states the host replay traced; info's counts summed"""
    total = {}
    for g in range(res.rounds):
        before = init if g == 0 else trace[g - 1]["state"]
        before = {k: v.cpu() for k, v in before.items()}
        for k, n in assert_matches_referee(res.samples[g], res.sample_info[g], before, goals.cpu(), lim.cpu(), seed, g, "informed", mask,
                                           **kw).items():
            total[k] = total.get(k, 0) + n
        assert_in_informed_set(res.samples[g], res.sample_info[g], before, goals.cpu(), mask)
    return total


@functools.lru_cache(maxsize=None)
def case_s_informed():
    from diffco_amd.rrtstar import host_rrt_star, rrt_star
    dc, rob, starts, goals, _ = problem_s()
    kw = kwargs_s(rob)
    res = rrt_star(dc, starts, goals, sampling="informed", goal_bias=GOAL_BIAS, seed=SEED_S, record_samples=True, **kw)
    init = rrt_star(dc, starts, goals, sampling="informed", goal_bias=GOAL_BIAS, seed=SEED_S, **dict(kw, max_rounds=0)).state()
    trace = []
    host = host_rrt_star(dc, starts, goals, sampler=fixed(res.samples), _trace=trace, **kw)
    return dc, rob, starts, goals, kw, res, init, host, trace


def test_case_s_informed_run():
    from diffco_amd.rrtstar import rrt_star
    dc, rob, starts, goals, kw, res, init, host, trace = case_s_informed()
    assert res.route == "fused" and host.route == "host" and res.rounds == host.rounds == G["rounds"]
    assert res.samples.shape == (G["rounds"], G["R"], G["P"], 2) and res.sample_info.shape == (G["rounds"], G["R"], G["P"])
    assert res.samples.is_cuda and res.sample_info.dtype == torch.int32
    assert_same_state(res, host)
    again = rrt_star(dc, starts, goals, sampler=fixed(res.samples), **kw)
    assert again.route == "fused"
    assert_same_state(res, again)
    lim = torch.tensor([[-math.pi, math.pi]] * 2)
    total = _referee_rounds(res, init, trace, goals, lim, SEED_S, rob.wrap_mask)
    print("case S informed: status", res.status.tolist(), "first_round", res.first_round.tolist(), "costs", res.costs.tolist(), "info", total)
    assert res.status.tolist()[:2] == [3, 1]
    assert any(k >= 2 for k in total) and total.get(1, 0) >= 1 and total.get(0, 0) >= 1   # informed rounds, goal rows, uniform ones
    # a second run with the seed: the same bits; another seed: other samples
    twin = rrt_star(dc, starts, goals, sampling="informed", goal_bias=GOAL_BIAS, seed=SEED_S, record_samples=True, **kw)
    assert_same_state(res, twin)
    assert torch.equal(res.samples, twin.samples) and torch.equal(res.sample_info, twin.sample_info)
    other = rrt_star(dc, starts, goals, sampling="informed", goal_bias=GOAL_BIAS, seed=SEED_S + 1, record_samples=True,
                     **dict(kw, max_rounds=4))
    assert not torch.equal(other.samples, res.samples[:4])


@pytest.mark.parametrize("K", [0, 16])
@pytest.mark.parametrize("P", [1, 16])
@pytest.mark.parametrize("name", ["cfg2_baxter_rq", "cfg3_baxter_rq_c5"])
def test_baxter_informed_run(name, P, K):
    from diffco_amd.rrtstar import host_rrt_star, rrt_star
    ck, starts, goals, lim = _baxter(name)
    kw = dict(range=B["range"], max_step=B["max_step"], radius=B["radius"], near=K, wrap=B["mask"], slots=P, cap=B["cap"],
              max_rounds=B["rounds"], rounds_per_call=B["chunk"], limits=lim)
    res = rrt_star(ck, starts, goals, sampling="informed", goal_bias=GOAL_BIAS, seed=21, record_samples=True, **kw)
    init = rrt_star(ck, starts, goals, sampling="informed", seed=21, **dict(kw, max_rounds=0)).state()
    trace = []
    host = host_rrt_star(ck, starts, goals, sampler=fixed(res.samples), _trace=trace, **kw)
    again = rrt_star(ck, starts, goals, sampler=fixed(res.samples), **kw)
    assert res.route == again.route == "fused" and host.route == "host" and res.rounds == host.rounds
    assert_same_state(res, host)
    assert_same_state(res, again)
    total = _referee_rounds(res, init, trace, goals, lim, 21, B["mask"])
    print(name, P, K, "status", res.status.tolist(), "first_round", res.first_round.tolist(), "info", total)
    assert int(res.count.sum()) > B["R"]


def _raw_setup():
    """case S's model, margin, initial state and the raw sampled call"""
    dc, rob, starts, goals, kw, res, init, host, trace = case_s_informed()
    model, margin = dc._rrt_model(torch.device("cuda"))
    goals = goals.contiguous()
    lim = torch.tensor([[-math.pi, math.pi]] * 2, device="cuda")

    def run(st, T, g0, samples_out=None, info_out=None):
        model.rrtstar_run_sampled(st, goals, lim, SEED_S, T, G["P"], g0, G["range"], G["max_step"], G["radius"], G["K"], 47,
                                  mode="informed", goal_bias=GOAL_BIAS, tries=8, margin=margin, wrap=rob.wrap_mask,
                                  samples_out=samples_out, info_out=info_out)
    return init, run, res, trace


def test_one_call_of_eight_rounds_equals_eight_calls_of_one():
    init, run, res, trace = _raw_setup()
    one = {k: v.clone() for k, v in init.items()}
    smp = torch.zeros((8, G["R"], G["P"], 2), device="cuda")
    info = torch.zeros((8, G["R"], G["P"]), dtype=torch.int32, device="cuda")
    run(one, 8, 0, smp, info)
    many = {k: v.clone() for k, v in init.items()}
    for t in range(8):
        run(many, 1, t)   # (the samples stay in the work slot)
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(one[k], many[k]), k
    assert int(one["count"].sum()) > G["R"] + 8
    # the first eight rounds of the planner's run, which took them in chunks of four
    assert_same_state(one, trace[7]["state"])
    assert torch.equal(smp, res.samples[:8]) and torch.equal(info, res.sample_info[:8])
    run(one, 0, 8)   # T = 0 launches nothing
    for k in STATE:
        assert torch.equal(one[k], many[k]), k


def test_a_captured_call_replays_to_the_eager_result():
    """one stream, no parallel branches"""
    init, run, res, trace = _raw_setup()
    want = {k: v.clone() for k, v in init.items()}
    run(want, 4, 0)
    st = {k: v.clone() for k, v in init.items()}
    smp = torch.zeros((4, G["R"], G["P"], 2), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(st, 4, 0, smp)   # (warm-up on the side stream)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for k in STATE:
        st[k].copy_(init[k])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run(st, 4, 0, smp)
    for _ in range(2):
        for k in STATE:
            st[k].copy_(init[k])
        smp.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in STATE:
            assert torch.equal(st[k], want[k]), k
        assert torch.equal(smp, res.samples[:4])


def test_near_0_and_near_8_grow_the_same_nodes_until_a_goal_node():
    """the draw reads a problem's cost only once it has a goal node: until then the set of nodes does not depend on the parents"""
    from diffco_amd.rrtstar import rrt_star
    dc, rob, starts, goals, kw, res, *_ = case_s_informed()
    first = [f for f, s in zip(res.first_round.tolist(), res.status.tolist()) if f >= 0 and s != 1]
    rounds = min(first) + 1 if first else G["rounds"]   # through the round that first reaches a goal
    run = lambda K: rrt_star(dc, starts, goals, sampling="informed", goal_bias=GOAL_BIAS, seed=SEED_S, record_samples=True,   # noqa: E731
                             **dict(kw, near=K, max_rounds=rounds, rounds_per_call=1))
    a, b = run(0), run(8)
    assert a.rounds == b.rounds == rounds and rounds >= 2
    assert torch.equal(a.samples, b.samples) and torch.equal(a.samples, res.samples[:rounds])
    assert torch.equal(a.nodes.view(torch.int32), b.nodes.view(torch.int32)) and torch.equal(a.count, b.count)
    assert torch.equal(a.goal_node, b.goal_node)


def test_routing():
    from diffco_amd.rrtstar import rrt_star
    dc, rob, starts, goals, kw, res, *_ = case_s_informed()
    rec = Recorder(dc)   # no fused model: the host route, drawing from the referee
    via = rrt_star(rec, starts, goals, sampling="informed", goal_bias=GOAL_BIAS, seed=SEED_S, record_samples=True, **dict(kw, max_rounds=4))
    E = G["R"] * G["P"]
    assert via.route == "host" and rec.sizes == [3 * G["R"]] + [E, E * G["K"], E * G["K"]] * 4
    informed = (res.sample_info >= 2).reshape(G["rounds"], -1).any(dim=1).tolist()
    m = min(4, (informed.index(True) if True in informed else G["rounds"]) + 1)   # the states agree bit for bit up to there
    assert torch.equal(via.sample_info[:m], res.sample_info[:m])
    plain = res.sample_info[:m] < 2
    assert torch.equal(via.samples[:m][plain].view(torch.int32), res.samples[:m][plain].view(torch.int32))
    with pytest.raises(ValueError, match="sampler"):
        rrt_star(dc, starts, goals, sampling="informed", sampler=fixed(res.samples), **kw)
