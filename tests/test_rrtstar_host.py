"""host_rrt_star (diffco_amd/rrtstar.py), the referee of the fused RRT*, on CPU tensors with a fake 2-D checker of discs: case S
(rrtstar_helpers.py: a blocked endpoint, a free direct motion, a problem that fills its tree, a hard one; P = 4, K = 8,
radius = 2 range, 24 rounds, fixed samples with goal rows).  After every round the state's invariants restated in numpy float32;
the K = 0 run grows the same nodes at costs that are nowhere lower; the referee's own trace shows every event of the contract;
the returned paths, path_tensor, the fixed batches and stop_on_first.  No GPU."""
import numpy as np
import torch

from rrtstar_helpers import (GOALS_S, S, STARTS_S, Discs, bits, check_state, fixed, host_walk, kwargs_s, samples_s, traced_s)


def test_invariants_after_every_round():
    res, trace, ck = traced_s()
    assert len(trace) == S["rounds"] and res.rounds == S["rounds"] and res.route == "host"
    prev = None
    for ev in trace:
        check_state(ev["state"], prev, Discs(), S["max_step"])
        prev = ev["state"]
    # the last trace entry is the returned state
    for k, v in res.state().items():
        assert torch.equal(v, trace[-1]["state"][k]), k


def test_outcomes_of_case_s():
    res, trace, _ = traced_s()
    print("case S: status", res.status.tolist(), "count", res.count.tolist(), "first_round", res.first_round.tolist(),
          "costs", res.costs.tolist())
    assert res.status.tolist() == [3, 1, 2, 0]
    assert res.count.tolist()[:3] == [1, 2, S["cap"]] and 1 < int(res.count[3]) < S["cap"]
    # the blocked problem: untouched;  the direct one: node 1 is the goal at the motion's own length, no round reached it
    assert res.paths[0] is None and np.isnan(float(res.costs[0])) and int(res.goal_node[0]) == -1
    assert torch.equal(res.paths[1], torch.stack([STARTS_S[1], GOALS_S[1]])) and int(res.first_round[1]) == -1
    assert float(res.costs[1]) == float(res.elen[1, 1]) == float(np.float32(np.sqrt(np.float32(np.float32(1.8) * np.float32(1.8)))))
    for r in (2, 3):
        p = res.paths[r]
        assert torch.equal(p[0], STARTS_S[r]) and torch.equal(p[-1], GOALS_S[r]) and len(p) > 2
        assert int(res.first_round[r]) >= 0 and int(res.goal_node[r]) > 0
        # the goal node holds the goal's bits and was appended in the round first_round names
        g = int(res.first_round[r])
        before = trace[g - 1]["state"] if g else None
        assert before is None or int(before["goal_node"][r]) == -1
        assert int(trace[g]["state"]["goal_node"][r]) == int(res.goal_node[r]) >= (int(before["count"][r]) if g else 1)
        # the cost of the goal is the path's length summed from the root in float32
        c = np.float32(0)
        for a, b in zip(p[:-1].numpy(), p[1:].numpy()):
            d = (b - a).astype(np.float32)
            c = np.float32(c + np.float32(np.sqrt(np.float32(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])))))
        assert bits(c) == bits(res.costs[r].numpy())


def test_same_nodes_better_costs_than_plain_rrt():
    res, _, _ = traced_s()
    plain, trace0, _ = traced_s(near=0)
    assert torch.equal(res.nodes.view(torch.int32), plain.nodes.view(torch.int32)) and torch.equal(res.count, plain.count)
    assert torch.equal(res.status, plain.status) and torch.equal(res.goal_node, plain.goal_node)
    assert torch.equal(res.first_round, plain.first_round)
    live = torch.arange(S["cap"])[None, :] < res.count[:, None]
    assert bool((res.cost[live] <= plain.cost[live]).all())
    assert bool((res.cost[live] < plain.cost[live]).any())
    # plain RRT never changes a parent: every node keeps the near node, at a lower index
    assert all(ev["chose_other"] == 0 and ev["rewires"] == 0 for ev in trace0)
    assert bool((plain.parent[live] < torch.arange(S["cap"])[None, :].expand_as(live)[live]).all())


def test_case_s_covers_the_contract():
    """asserted on the referee's own trace: every event below happens in case S"""
    res, trace, _ = traced_s()
    plain, _, _ = traced_s(near=0)
    total = {k: sum(ev[k] for ev in trace) for k in ("chose_other", "rewires", "contested", "lowered_descendants", "short_near", "dropped")}
    print("case S events:", total)
    assert total["chose_other"] >= 1      # a chosen parent that is not near
    assert total["rewires"] >= 1          # a rewire
    assert total["contested"] >= 1        # ... contested by two slots of one round
    assert total["lowered_descendants"] >= 1   # a refresh that lowers a descendant of a rewired node
    assert total["short_near"] >= 1       # a near list shorter than K
    assert total["dropped"] >= 1          # a dropped append: FULL
    improved = strictly_better = 0
    for r in (2, 3):
        seq = [float(ev["state"]["cost"][r, int(ev["state"]["goal_node"][r])]) for ev in trace if int(ev["state"]["goal_node"][r]) >= 0]
        assert all(b <= a for a, b in zip(seq, seq[1:]))
        improved += seq[-1] < seq[0]
        strictly_better += float(res.costs[r]) < float(plain.costs[r])
        assert float(res.costs[r]) <= float(plain.costs[r])
    assert improved >= 1 and strictly_better >= 1   # a goal reached and improved later; better than K = 0 at the goal


def test_path_tensor_on_the_cpu_equals_the_host_walk():
    res, _, _ = traced_s()
    st = res.state()
    path, count = res.path_tensor()
    walks = [host_walk(st, r) for r in range(S["R"])]
    assert walks[0] is None and count.tolist() == [0 if w is None else len(w) for w in walks]
    assert path.shape == (S["R"], max(len(w) for w in walks if w is not None), 2)
    for r, w in enumerate(walks):
        if w is not None:
            assert torch.equal(path[r, :len(w)], w) and torch.equal(res.paths[r], w) and not bool(path[r, len(w):].any())
    # W too small: -n and an untouched row
    small, c2 = res.path_tensor(W=2)
    assert c2.tolist() == [0, 2] + [-len(walks[r]) for r in (2, 3)] and not bool(small[2:].any()) and torch.equal(small[1], walks[1])


def test_fixed_batches():
    ck = Discs()
    from diffco_amd.rrtstar import host_rrt_star
    host_rrt_star(ck, STARTS_S, GOALS_S, sampler=fixed(samples_s()), **kwargs_s(max_rounds=6))
    E = S["R"] * S["P"]
    assert ck.batches == [3 * S["R"]] + [E, E * S["K"], E * S["K"]] * 6
    ck = Discs()
    host_rrt_star(ck, STARTS_S, GOALS_S, sampler=fixed(samples_s()), **kwargs_s(max_rounds=6, near=0))
    assert ck.batches == [3 * S["R"]] + [E] * 6


def test_chunking_and_stop_on_first():
    from diffco_amd.rrtstar import host_rrt_star
    res, trace, _ = traced_s()
    # the chunking does not change the result
    other = host_rrt_star(Discs(), STARTS_S, GOALS_S, sampler=fixed(samples_s()), **kwargs_s(rounds_per_call=7))
    for k, v in res.state().items():
        assert torch.equal(v, other.state()[k]), k
    # stop_on_first: the loop ends at the first chunk boundary at which every running problem has a goal node
    chunk = 2

    def done(st):
        running = st["status"] == 0
        return bool((st["goal_node"][running] >= 0).all())
    want = next(g for g in range(chunk, S["rounds"] + 1, chunk) if done(trace[g - 1]["state"]))
    assert chunk < want < S["rounds"]
    early = host_rrt_star(Discs(), STARTS_S, GOALS_S, sampler=fixed(samples_s()), stop_on_first=True, **kwargs_s(rounds_per_call=chunk))
    assert early.rounds == want
    for k, v in early.state().items():
        assert torch.equal(v, trace[want - 1]["state"][k]), k


def test_default_sampler_goal_bias_and_seed():
    from diffco_amd.rrtstar import host_rrt_star
    kw = kwargs_s(max_rounds=8)
    a = host_rrt_star(Discs(), STARTS_S, GOALS_S, seed=5, goal_bias=0.5, **kw)
    b = host_rrt_star(Discs(), STARTS_S, GOALS_S, seed=5, goal_bias=0.5, **dict(kw, rounds_per_call=3))
    c = host_rrt_star(Discs(), STARTS_S, GOALS_S, seed=6, goal_bias=0.5, **kw)
    for k, v in a.state().items():
        assert torch.equal(v, b.state()[k]), k
    assert not torch.equal(a.nodes, c.nodes)
    check_state(a.state(), None, Discs(), S["max_step"])
