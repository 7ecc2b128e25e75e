"""host_rrt_star under objective="clearance" (diffco_amd/rrtstar.py), the referee of dcx_rrtstar_run_cost, on CPU tensors with a
fake 2-D checker of discs that has a score (rrtstar_cost_helpers.SoftDiscs), on rrtstar_helpers' case S: gain 0 is the length
planner bit for bit; with a gain the invariants hold after every round with every edge's cost recomputed in numpy float32; the
nodes are the length run's; submitting every near place instead of those the lower bounds let through ends in the same state;
the referee's own trace shows every event of the contract; a penalised direct motion is improved on; clearance_cost_paths
prices the planner's own paths to the goal nodes' costs; the argument errors.  No GPU."""
import numpy as np
import pytest
import torch

from rrtstar_cost_helpers import BAND_C, EVENTS, GAIN_C, SoftDiscs, check_state_cost, cost32, kwargs_c, traced_c
from rrtstar_helpers import (GOALS_S, S, STARTS_S, Discs, assert_same_state, bits, fixed, kwargs_s, length32, samples_s, traced_s)


def test_gain_zero_is_the_length_planner_bit_for_bit():
    want, trace_l, _ = traced_s()
    got, trace_c, _ = traced_c(gain=0.0)
    assert got.route == "host" and got.rounds == want.rounds
    assert_same_state(got, want)
    for a, b in zip(trace_c, trace_l):
        assert_same_state(a["state"], b["state"])
        assert a["pruned_after"] == a["rewire_rejected_after"] == 0   # (pen > 0 still counts as penalised: the gain is what is 0)
        assert all(a[k] == b[k] for k in ("chose_other", "rewires", "contested", "lowered_descendants", "short_near", "dropped"))
    assert torch.equal(got.costs.view(torch.int32), want.costs.view(torch.int32))


def test_invariants_after_every_round_and_no_cost_rises():
    res, trace, _ = traced_c()
    assert len(trace) == S["rounds"] and res.rounds == S["rounds"] and res.route == "host"
    prev = None
    for ev in trace:
        check_state_cost(ev["state"], prev, SoftDiscs(), S["max_step"], GAIN_C, BAND_C)
        prev = ev["state"]
    for k, v in res.state().items():
        assert torch.equal(v, trace[-1]["state"][k]), k
    # the objective is at work: some edge of the final trees costs more than its length
    nodes, parent, elen, count = (res.state()[k].numpy() for k in ("nodes", "parent", "elen", "count"))
    dearer = sum(elen[r, i] > length32(nodes[r, parent[r, i]], nodes[r, i]) for r in range(S["R"]) for i in range(1, count[r]))
    assert dearer >= 1


def test_the_node_set_is_the_length_run_s():
    res, _, _ = traced_c()
    plain, _, _ = traced_s()
    assert torch.equal(res.nodes.view(torch.int32), plain.nodes.view(torch.int32)) and torch.equal(res.count, plain.count)
    assert torch.equal(res.status, plain.status) and torch.equal(res.goal_node, plain.goal_node)
    assert torch.equal(res.first_round, plain.first_round)
    # ... at costs that are nowhere below the lengths the length planner found, and with other parents somewhere
    live = torch.arange(S["cap"])[None, :] < res.count[:, None]
    assert bool((res.cost[live] >= plain.cost[live]).all()) and not torch.equal(res.parent, plain.parent)


def test_submitting_every_near_place_ends_in_the_same_state():
    """the pruning by the lower bounds is exact: what it leaves out could not have won"""
    res, trace, ck = traced_c()
    full, trace_all, ck_all = traced_c(submit_all=True)
    for a, b in zip(trace, trace_all):
        assert_same_state(a["state"], b["state"])
    assert_same_state(res, full)
    assert ck.batches == ck_all.batches   # the batches are fixed either way
    assert sum(ev["pruned_after"] for ev in trace_all) > sum(ev["pruned_after"] for ev in trace)


def test_case_s_covers_the_contract():
    """asserted on the referee's own trace: every event below happens in case S under the objective"""
    res, trace, ck = traced_c()
    total = {k: sum(ev[k] for ev in trace) for k in EVENTS}
    print("case S under the objective:", total, "status", res.status.tolist(), "costs", res.costs.tolist())
    assert all(total[k] >= 1 for k in EVENTS), total
    E = S["R"] * S["P"]
    assert ck.batches == [3 * S["R"]] + [E, E * S["K"], E * S["K"]] * S["rounds"]
    assert res.status.tolist() == [3, 1, 2, 0]
    # a goal's cost never rises
    for r in (2, 3):
        seq = [float(ev["state"]["cost"][r, int(ev["state"]["goal_node"][r])]) for ev in trace if int(ev["state"]["goal_node"][r]) >= 0]
        assert len(seq) >= 1 and all(b <= a for a, b in zip(seq, seq[1:]))


def test_a_penalised_direct_motion_keeps_running_and_is_improved_on():
    """problem 1 of case S passes a disc at a distance of 0.23: free, and under a band of 0.3 penalised"""
    from diffco_amd.rrtstar import host_rrt_star
    band, gain = 0.3, 4.0
    ck = SoftDiscs()
    w = ck.motion_worst(STARTS_S[1:2], GOALS_S[1:2], max_step=S["max_step"], max_samples=1 << 20)[0].numpy()[0]
    L = length32(STARTS_S[1].numpy(), GOALS_S[1].numpy())
    C = cost32(L, w, gain, band)
    assert w <= 0 and C > L
    init = host_rrt_star(ck, STARTS_S, GOALS_S, sampler=fixed(samples_s()), **kwargs_c(clearance_gain=gain, clearance_band=band, max_rounds=0))
    assert init.status.tolist() == [3, 0, 0, 0] and init.count.tolist() == [1, 2, 1, 1] and init.goal_node.tolist() == [-1, 1, -1, -1]
    assert bits(init.cost[1, 1].numpy()) == bits(init.elen[1, 1].numpy()) == bits(C) and int(init.parent[1, 1]) == 0
    trace = []
    res = host_rrt_star(ck, STARTS_S, GOALS_S, sampler=fixed(samples_s()), _trace=trace,
                        **kwargs_c(clearance_gain=gain, clearance_band=band))
    assert int(res.goal_node[1]) == 1 and int(res.first_round[1]) == -1 and int(res.count[1]) > 2
    assert float(res.costs[1]) <= float(C)
    prev = None
    for ev in trace:
        check_state_cost(ev["state"], prev, SoftDiscs(), S["max_step"], gain, band)
        prev = ev["state"]
    # under the band of the other tests the same motion is not penalised: final at its length
    assert traced_c()[0].status.tolist()[1] == 1 and bits(traced_c()[0].costs[1].numpy()) == bits(L)


def test_clearance_cost_paths_prices_the_referee_s_paths_to_their_costs():
    from diffco_amd import clearance_cost_paths
    res, _, _ = traced_c()
    path, count = res.path_tensor()
    assert count.tolist()[0] == 0 and min(count.tolist()[1:]) >= 2
    cost, length, peak = clearance_cost_paths(SoftDiscs(), path, count, max_step=S["max_step"], gain=GAIN_C, band=BAND_C)
    has = count > 0
    assert torch.equal(cost[has].view(torch.int32), res.costs[has].view(torch.int32))
    assert float(cost[0]) == 0 and float(length[0]) == 0 and np.isnan(float(peak[0]))
    assert bool((peak[has] <= 0).all()) and bool((cost[has] >= length[has]).all()) and bool((cost[has] > length[has]).any())
    # the length is the path's own, summed from the root in float32
    for r in (1, 2, 3):
        p, c = res.paths[r].numpy(), np.float32(0)
        for a, b in zip(p[:-1], p[1:]):
            c = np.float32(c + length32(a, b))
        assert bits(c) == bits(length[r].numpy())
    # a path of the length planner is priced too: never below its length, which is that planner's cost
    plain = traced_s()[0]
    path, count = plain.path_tensor()
    cost, length, peak = clearance_cost_paths(SoftDiscs(), path, count, max_step=S["max_step"], gain=GAIN_C, band=BAND_C)
    has = count > 0
    assert torch.equal(length[has].view(torch.int32), plain.costs[has].view(torch.int32)) and bool((cost[has] >= length[has]).all())


def test_argument_errors_and_routing():
    from diffco_amd import clearance_cost_paths
    from diffco_amd.rrtstar import host_rrt_star, rrt_star
    args = (STARTS_S, GOALS_S)
    for fn in (host_rrt_star, rrt_star):
        with pytest.raises(ValueError, match="clearance_band"):
            fn(SoftDiscs(), *args, sampler=fixed(samples_s()), **kwargs_s(objective="clearance"))
        with pytest.raises(ValueError, match="clearance_band"):
            fn(SoftDiscs(), *args, sampler=fixed(samples_s()), **kwargs_s(objective="clearance", clearance_band=0.0))
        with pytest.raises(ValueError, match="clearance_gain"):
            fn(SoftDiscs(), *args, sampler=fixed(samples_s()), **kwargs_s(objective="clearance", clearance_band=0.1, clearance_gain=-1.0))
        with pytest.raises(ValueError, match="objective"):
            fn(SoftDiscs(), *args, sampler=fixed(samples_s()), **kwargs_s(objective="integral"))
        # a checker without motion_worst cannot be planned for under the objective
        with pytest.raises(TypeError, match="motion_worst"):
            fn(Discs(), *args, sampler=fixed(samples_s()), **kwargs_c())
    with pytest.raises(TypeError, match="motion_worst"):
        clearance_cost_paths(Discs(), torch.zeros(1, 2, 2), torch.tensor([2]), max_step=0.1, band=0.1)
    with pytest.raises(ValueError, match="clearance_band"):
        clearance_cost_paths(SoftDiscs(), torch.zeros(1, 2, 2), torch.tensor([2]), max_step=0.1, band=0.0)
    # rrt_star hands a checker without a fused model to the referee, the objective with it; the default is the length planner
    via = rrt_star(SoftDiscs(), *args, sampler=fixed(samples_s()), **kwargs_c())
    assert via.route == "host"
    assert_same_state(via, traced_c()[0])
    assert_same_state(rrt_star(SoftDiscs(), *args, sampler=fixed(samples_s()), **kwargs_s()), traced_s()[0])
