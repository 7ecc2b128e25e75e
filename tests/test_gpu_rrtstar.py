"""GPU: batched RRT* (dcx_rrtstar_run, ScoreModel.rrtstar_run, rrtstar.rrt_star) against its referee rrtstar.host_rrt_star - the
same contract composed of roadmap.knn, torch arithmetic and the checker's check_motions - bit for bit on every state tensor for
identical samples: case S on the DiffCo of the 2-DoF planar arm with both joints on the circle (a blocked endpoint, a free
direct motion, two hard problems of which one fills its tree; P = 4, K = 8), and the 7-DoF Baxter fixtures with a wrap mask on
two joints, one class and five classes with a margin each, at P in {1, 16} and K in {0, 1, 16}.  Then one call of T rounds against
T calls of one, graph capture, the device's path extraction against the host walk, and the routing of rrt_star."""
import functools

import numpy as np
import pytest
import torch

from rrtstar_helpers import (STATE, ModelChecker, Recorder, assert_same_state, far_refused_pairs, fixed, host_walk,
                             near_accepted_pair, planar_checker, with_goal_rows)

pytestmark = pytest.mark.gpu

# case S: the samples' seed and the cap were chosen against host_rrt_star on the GPU so that its trace shows the events
# test_case_s_fused_equals_host_bit_for_bit asks for
SEED_S = 19
G = dict(R=4, P=4, K=8, cap=48, range=0.5, radius=1.0, max_step=0.1, rounds=24, chunk=4)
B = dict(R=3, cap=64, range=1.5, radius=3.0, max_step=0.25, rounds=12, chunk=4, mask=(1 << 4) | (1 << 6))


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")


@functools.lru_cache(maxsize=None)
def problem_s():
    """(checker, robot, starts [4, 2], goals, samples): a colliding start; the nearest pair whose direct motion is free; the two
    farthest pairs whose direct motion the checker refuses"""
    d, dc, rob = planar_checker()
    g = torch.Generator().manual_seed(3)
    nodes = ((torch.rand(512, 2, generator=g) * 2 - 1) * np.pi).float().cuda()
    hit = dc.is_collision(nodes).reshape(-1)
    free = nodes[~hit]
    assert int(hit.sum()) >= 1 and len(free) >= 40
    check = lambda a, b: torch.as_tensor(dc.check_motions(a, b, max_step=G["max_step"], wrap=True)).cuda()   # noqa: E731
    easy = near_accepted_pair(check, free)
    hard = far_refused_pairs(check, free, 2)
    starts = torch.stack([nodes[hit][0], free[easy[0]]] + [free[i] for i, _ in hard])
    goals = torch.stack([free[0], free[easy[1]]] + [free[j] for _, j in hard])
    gs = torch.Generator().manual_seed(SEED_S)
    samples = ((torch.rand(G["rounds"], G["R"], G["P"], 2, generator=gs) * 2 - 1) * np.pi).float().cuda()
    return dc, rob, starts, goals, with_goal_rows(samples, goals)


def kwargs_s(rob, **over):
    kw = dict(range=G["range"], max_step=G["max_step"], radius=G["radius"], near=G["K"], wrap=rob.wrap_mask, slots=G["P"], cap=G["cap"],
              max_rounds=G["rounds"], rounds_per_call=G["chunk"], limits=[[-np.pi, np.pi]] * 2)
    kw.update(over)
    return kw


@functools.lru_cache(maxsize=None)
def case_s():
    """(checker, robot, starts, goals, samples, host result, its trace, recorder, fused result)"""
    from diffco_amd.rrtstar import host_rrt_star, rrt_star
    dc, rob, starts, goals, samples = problem_s()
    rec, trace = Recorder(dc), []
    host = host_rrt_star(rec, starts, goals, sampler=fixed(samples), _trace=trace, **kwargs_s(rob))
    fused = rrt_star(dc, starts, goals, sampler=fixed(samples), **kwargs_s(rob))
    return dc, rob, starts, goals, samples, host, trace, rec, fused


def test_case_s_fused_equals_host_bit_for_bit():
    *_, host, trace, rec, fused = case_s()
    assert fused.route == "fused" and host.route == "host"
    total = {k: sum(ev[k] for ev in trace) for k in ("chose_other", "rewires", "contested", "lowered_descendants", "short_near", "dropped")}
    print("case S: status", fused.status.tolist(), "count", fused.count.tolist(), "first_round", fused.first_round.tolist(),
          "costs", fused.costs.tolist(), "events", total)
    assert_same_state(fused, host)
    assert fused.rounds == host.rounds == G["rounds"]
    for p, q in zip(fused.paths, host.paths):
        assert (p is None) == (q is None) and (p is None or torch.equal(p, q))
    assert torch.equal(fused.costs.view(torch.int32), host.costs.view(torch.int32))
    assert fused.status.tolist()[:2] == [3, 1] and 2 in fused.status.tolist() and int(fused.count[2:].sum()) > 20
    # what the kernels met on the way: parents other than near, rewires (one contested by two slots), refreshed descendants,
    # short near lists, a dropped append, a goal
    assert all(total[k] >= 1 for k in total), total
    assert int((fused.first_round >= 0).sum()) >= 1
    # the tree the kernels left: a tree, its costs the fixed point, nothing past count touched
    st = fused.state()
    assert (fused.parent[:, 0] == -1).all()
    n = fused.count.tolist()
    for r in range(G["R"]):
        par, cost, elen = fused.parent[r, :n[r]].long(), fused.cost[r, :n[r]], fused.elen[r, :n[r]]
        assert bool((par[1:] >= 0).all()) and bool((par[1:] < n[r]).all())
        assert torch.equal(cost[1:].view(torch.int32), (cost[par[1:]] + elen[1:]).view(torch.int32))
        assert not bool(fused.nodes[r, n[r]:].any()) and bool((fused.parent[r, n[r]:] == -1).all())
    assert all(host_walk(st, r) is not None or int(fused.goal_node[r]) == -1 for r in range(G["R"]))


def test_case_s_same_nodes_as_plain_rrt():
    from diffco_amd.rrtstar import rrt_star
    dc, rob, starts, goals, samples, host, trace, rec, fused = case_s()
    plain = rrt_star(dc, starts, goals, sampler=fixed(samples), **kwargs_s(rob, near=0))
    assert plain.route == "fused"
    assert torch.equal(plain.nodes.view(torch.int32), fused.nodes.view(torch.int32)) and torch.equal(plain.count, fused.count)
    live = torch.arange(G["cap"], device="cuda")[None, :] < fused.count[:, None]
    assert bool((fused.cost[live] <= plain.cost[live]).all())


@functools.lru_cache(maxsize=None)
def _baxter(name):
    from diffco_amd import _lib, _ops
    from helpers import CASE_ROBOT, make_robot
    from motion_wrap_helpers import fixture_model, mixed_margin
    _lib.require_gpu()
    d, desc, kern, sup, W = fixture_model(name)
    m = _ops.ScoreModel(desc, kern[0], kern[1], kern[2], _t(sup), _t(W))
    mg = mixed_margin(d)
    ck = ModelChecker(m, mg if W.shape[1] > 1 else mg[0])
    q = _t(d["q"])
    free = q[((m.score_raw(q) - _t(mg)[None]) <= 0).all(dim=1)]
    assert len(free) >= 40
    check = lambda a, b: ck.check_motions(a, b, max_step=B["max_step"], max_samples=200, wrap=B["mask"])[0]   # noqa: E731
    pairs = far_refused_pairs(check, free, B["R"])
    starts, goals = torch.stack([free[i] for i, _ in pairs]), torch.stack([free[j] for _, j in pairs])
    return ck, starts, goals, torch.as_tensor(make_robot(CASE_ROBOT[name]).limits, dtype=torch.float32)


@pytest.mark.parametrize("K", [0, 1, 16])
@pytest.mark.parametrize("P", [1, 16])
@pytest.mark.parametrize("name", ["cfg2_baxter_rq", "cfg3_baxter_rq_c5"])
def test_baxter_fused_equals_host_bit_for_bit(name, P, K):
    """7 DoF (the nearest kernel's register path), two joints on the circle, one class with a margin and five classes with a
    margin each; one slot and the most, no near set, one near node and the most"""
    from diffco_amd.rrtstar import host_rrt_star, rrt_star
    ck, starts, goals, lim = _baxter(name)
    g = torch.Generator().manual_seed(11)
    lo, span = lim[:, 0], lim[:, 1] - lim[:, 0]
    samples = with_goal_rows((lo + span * torch.rand(B["rounds"], B["R"], P, 7, generator=g)).float().cuda(), goals, every=2)
    kw = dict(range=B["range"], max_step=B["max_step"], radius=B["radius"], near=K, wrap=B["mask"], slots=P, cap=B["cap"],
              max_rounds=B["rounds"], rounds_per_call=B["chunk"], limits=lim)
    rec, trace = Recorder(ck), []
    host = host_rrt_star(rec, starts, goals, sampler=fixed(samples), _trace=trace, **kw)
    fused = rrt_star(ck, starts, goals, sampler=fixed(samples), **kw)
    assert fused.route == "fused" and host.route == "host"
    total = {k: sum(ev[k] for ev in trace) for k in ("chose_other", "rewires", "contested", "lowered_descendants", "short_near", "dropped")}
    print(name, P, K, "status", fused.status.tolist(), "counts", fused.count.tolist(), "first_round", fused.first_round.tolist(), total)
    assert_same_state(fused, host)
    E = B["R"] * P
    assert rec.sizes == [3 * B["R"]] + ([E, E * K, E * K] if K else [E]) * host.rounds
    assert int(fused.count.sum()) > B["R"]
    for r, p in enumerate(fused.paths):
        if p is not None:
            assert torch.equal(p[0], starts[r]) and torch.equal(p[-1], goals[r])


def _raw_setup():
    """case S's model, margin, initial state and samples for the raw call"""
    from diffco_amd.rrtstar import rrt_star
    dc, rob, starts, goals, samples, *_ = case_s()
    init = rrt_star(dc, starts, goals, sampler=fixed(samples), **kwargs_s(rob, max_rounds=0))
    assert init.status.tolist()[:2] == [3, 1] and init.count.tolist() == [1, 2, 1, 1] and init.rounds == 0
    model, margin = dc._rrt_model(torch.device("cuda"))
    goals = goals.contiguous()
    run = lambda st, smp, g0: model.rrtstar_run(st, goals, smp, g0, G["range"], G["max_step"], G["radius"], G["K"], 47,   # noqa: E731
                                                margin=margin, wrap=rob.wrap_mask)
    return init.state(), samples, run


def test_one_call_of_eight_rounds_equals_eight_calls_of_one():
    init, samples, run = _raw_setup()
    one = {k: v.clone() for k, v in init.items()}
    run(one, samples[:8].contiguous(), 0)
    many = {k: v.clone() for k, v in init.items()}
    for t in range(8):
        run(many, samples[t:t + 1].contiguous(), t)
    again = {k: v.clone() for k, v in init.items()}
    run(again, samples[:8].contiguous(), 0)
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(one[k], many[k]) and torch.equal(one[k], again[k]), k
    assert int(one["count"].sum()) > G["R"] + 8
    # the first eight rounds of case S's fused run, which took them in chunks of four
    *_, trace, _, _ = case_s()
    assert_same_state(one, trace[7]["state"])
    # T = 0 launches nothing and changes nothing
    run(one, samples[:0].contiguous(), 8)
    for k in STATE:
        assert torch.equal(one[k], again[k]), k


def test_a_captured_call_replays_to_the_eager_result():
    """one stream, no parallel branches"""
    init, samples, run = _raw_setup()
    smp = samples[:4].contiguous()
    want = {k: v.clone() for k, v in init.items()}
    run(want, smp, 0)
    st = {k: v.clone() for k, v in init.items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(st, smp, 0)
    torch.cuda.current_stream().wait_stream(s)
    for k in STATE:
        assert torch.equal(st[k], want[k]), k
    for k in STATE:
        st[k].copy_(init[k])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run(st, smp, 0)
    for _ in range(2):
        for k in STATE:
            st[k].copy_(init[k])
        g.replay()
        torch.cuda.synchronize()
        for k in STATE:
            assert torch.equal(st[k], want[k]), k


def test_path_tensor_on_the_device_equals_the_host_walk():
    *_, fused = case_s()
    st = fused.state()
    walks = [host_walk(st, r) for r in range(G["R"])]
    assert walks[0] is None and walks[1] is not None and len(walks[1]) == 2
    path, count = fused.path_tensor()
    assert path.is_cuda and count.tolist() == [0 if w is None else len(w) for w in walks]
    assert path.shape[1] == max(len(w) for w in walks if w is not None)
    for r, w in enumerate(walks):
        if w is None:
            assert not bool(path[r].any())
        else:
            assert torch.equal(path[r, :len(w)], w) and not bool(path[r, len(w):].any())
    # W too small for the longer paths: -n and an untouched row; W = 0 is the size query
    small, c2 = fused.path_tensor(W=2)
    assert c2.tolist() == [0 if w is None else (len(w) if len(w) <= 2 else -len(w)) for w in walks]
    for r, w in enumerate(walks):
        assert torch.equal(small[r], w) if (w is not None and len(w) <= 2) else not bool(small[r].any())
    from diffco_amd import _ops
    assert _ops.rrtstar_extract_paths(st, 0)[1].tolist() == [0 if w is None else -len(w) for w in walks]


def test_routing():
    """a checker with a fused model plans fused; a recorder around it has none and plans on the host, through the fixed batches"""
    dc, rob, starts, goals, samples, host, trace, rec, fused = case_s()
    assert fused.route == "fused" and host.route == "host"
    E = G["R"] * G["P"]
    assert rec.sizes == [3 * G["R"]] + [E, E * G["K"], E * G["K"]] * G["rounds"]
    from diffco_amd.rrtstar import rrt_star
    rec2 = Recorder(dc)
    via = rrt_star(rec2, starts, goals, sampler=fixed(samples), **kwargs_s(rob, max_rounds=4))
    assert via.route == "host" and rec2.sizes == [3 * G["R"]] + [E, E * G["K"], E * G["K"]] * 4
    assert_same_state(via, trace[3]["state"])
    # stop_on_first on the fused route: the loop ends at the chunk after which every running problem has a goal node
    early = rrt_star(dc, starts, goals, sampler=fixed(samples), stop_on_first=True, **kwargs_s(rob, rounds_per_call=2))

    def done(state):
        running = state["status"] == 0
        return bool((state["goal_node"][running] >= 0).all())
    want = next((g for g in range(2, G["rounds"] + 1, 2) if done(trace[g - 1]["state"])), G["rounds"])
    assert early.route == "fused" and early.rounds == want
    assert_same_state(early, trace[want - 1]["state"])
