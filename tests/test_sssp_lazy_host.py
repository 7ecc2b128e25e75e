"""CPU: the host route of the lazy roadmap queries.  host_mark_routes and host_apply_checks against the numpy referee bit for
bit (one pass on partly known edges, and whole relax - mark - check - apply loops at capacities 1, 2 and M); the loop's fixed
point on a fake 2-D checker (a wall with a gap) against an eager roadmap on the same nodes; and what the laziness saves under a
verdict rule that needs no model, pinned on the referee."""
import copy
import math

import numpy as np
import pytest
import torch

from sssp_helpers import case, same_bits
from sssp_lazy_helpers import LAZY_GRAPHS, apply_ref, lazy_graph, loop_case, mark_ref, verdicts

ONE_PASS = [("pair", 3), ("chain40", 65), ("grid12", 65), ("hub", 65), ("two_components", 130), ("duplicates300", 3),
            ("duplicates300", 65), ("knn300", 65)]


def _t(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]


def _caps(M):
    return sorted({1, 2, M})


@pytest.mark.parametrize("name,Q", ONE_PASS)
def test_host_mark_and_apply_equal_the_referee(name, Q):
    from diffco_amd.roadmap import host_apply_checks, host_mark_routes
    c, g = case(name, Q), lazy_graph(name)                       # every mode, the relaxation's fixed point
    state = np.array([1 if m % 5 == 3 else 0 for m in range(g["M"])], np.uint8)
    marked = 0
    for cap in _caps(g["M"]):
        want = mark_ref(g, state, c["nodes"], c["dist"], c["pred"], c["mode"], c["goal_idx"], c["goal_len"], cap)
        got = host_mark_routes(*_t(g["rowptr"], g["col"], g["eid"], g["ends"], state, c["nodes"], c["dist"], c["pred"], c["mode"],
                                   c["goal_idx"], c["goal_len"]), cap)
        assert all(same_bits(a.numpy(), b) for a, b in zip(got, want)), cap
        total, n = want[4]
        assert n == min(total, cap) and (np.diff(want[1][:n]) > 0).all() and (state[want[1][:n]] == 0).all()
        marked = max(marked, int(total))
        hit = verdicts(want[1][:n])
        w_want, s_want, any_want = apply_ref(g, g["weight"], state, want[1], want[4], hit)
        w, s = _t(g["weight"].copy(), state.copy())
        flag = host_apply_checks(w, _t(g["ent"])[0], s, got[1], got[4], torch.from_numpy(hit))
        assert same_bits(w.numpy(), w_want) and same_bits(s.numpy(), s_want) and same_bits(flag.numpy(), any_want)
        assert (s_want != state).sum() == n                      # the listed edges are settled, the rest stay as they were
    if g["M"] > 1 and Q >= 64:
        assert marked > 2                                        # (the capacities 1 and 2 did truncate)


def _host_loop(name, Q, cap, all_modes=False):
    """the loop of Roadmap.query_batch's host route on the referee's graph, the verdict rule in the checker's place"""
    from diffco_amd.roadmap import host_apply_checks, host_extract_paths, host_mark_routes, host_sssp
    c, g = loop_case(name, Q, all_modes, None if cap == lazy_graph(name)["M"] else cap), lazy_graph(name)
    rowptr, col, eid, ent, ends, nodes = _t(g["rowptr"], g["col"], g["eid"], g["ent"], g["ends"], c["nodes"])
    weight, state = _t(g["weight"].copy(), np.zeros(g["M"], np.uint8))
    si, sl, gi, gl, mode = _t(c["start_idx"], c["start_len"], c["goal_idx"], c["goal_len"], c["mode"])
    iters = checked = 0
    while True:
        d, p, _ = host_sssp(rowptr, col, weight, si, sl)
        pending, lst, qa, qb, n_out = host_mark_routes(rowptr, col, eid, ends, state, nodes, d, p, mode, gi, gl, cap)
        want = c["passes"][iters]
        assert same_bits(pending.numpy(), want[0]) and same_bits(lst.numpy(), want[1]) and same_bits(n_out.numpy(), want[2])
        iters += 1
        if int(n_out[0]) == 0:
            break
        n = int(n_out[1])
        host_apply_checks(weight, ent, state, lst, n_out, torch.from_numpy(verdicts(lst[:n].tolist())))
        checked += n
    got = host_extract_paths(nodes, d, p, mode, *_t(c["starts"], c["goals"]), gi, gl, _t(c["direct_len"])[0], c["W"])
    assert iters == c["iters"] and checked == c["checked"]
    assert same_bits(weight.numpy(), c["weight"]) and same_bits(state.numpy(), c["state"])
    assert all(same_bits(a.numpy(), b) for a, b in zip(got, (c["path"], c["count"], c["length"])))
    return c


@pytest.mark.parametrize("name", LAZY_GRAPHS)
def test_whole_host_loops_equal_the_referee(name):
    M = lazy_graph(name)["M"]
    _host_loop(name, 65, M)
    if name in ("knn300", "two_components", "hub"):              # (queries with a colliding endpoint or a free direct motion mark nothing)
        _host_loop(name, 65, M, all_modes=True)
    if M <= 300:                                                 # (a pass per edge: the small graphs)
        for cap in (1, 2):
            c = _host_loop(name, 3, cap)
            assert c["iters"] >= c["checked"] / cap


def test_what_the_laziness_saves_is_pinned_on_the_referee():
    # the verdict rule blocks a quarter of the edges; three routes touch a few dozen of the ~1000 candidates
    for name, Q, M, checked, iters in (("knn300", 3, 1073, 12, 3), ("duplicates300", 3, 1042, 38, 10), ("knn300", 65, 1073, 293, 7),
                                       ("duplicates300", 65, 1042, 286, 7)):
        c = loop_case(name, Q)
        assert (c["g"]["M"], c["checked"], c["iters"]) == (M, checked, iters)
        assert bool(c["settled"].all()) and (c["state"][c["weight"][c["g"]["ent"][:, 0]] == np.inf] == 2).all()
        if Q == 3:
            assert c["checked"] <= M // 4
    # a chain has one route: every edge is checked, a quarter of them fall, and nothing reaches the far end any more
    c = loop_case("chain40", 65)
    assert (c["g"]["M"], c["checked"], c["blocked"], c["iters"]) == (39, 39, 10, 2)
    assert np.isinf(c["dist"][39]).all() and int((c["count"] > 0).sum()) == 4


# ------------------------------------------------------------------------------------------------ Roadmap
class _Wall:
    """a 2-D point robot and a wall at x = 0.5 of half-thickness 0.02 with a gap for |y - gap_y| < 0.1: exact geometry, the
    motion check sampled under the max_step rule as the library samples (both endpoints included)"""

    def __init__(self, gap_y=0.5):
        self.gap_y = gap_y
        self.motion_calls = self.edges_checked = 0

    def is_collision(self, q):
        q = torch.as_tensor(q).reshape(-1, 2)
        return ((q[:, 0] - 0.5).abs() <= 0.02) & ((q[:, 1] - self.gap_y).abs() >= 0.1)

    def check_motions(self, starts, targets, max_step=None, wrap=None):
        assert wrap is None and max_step is not None
        self.motion_calls += 1
        self.edges_checked += len(starts)
        out = []
        for a, b in zip(torch.as_tensor(starts), torch.as_tensor(targets)):
            n = int(math.ceil(float((b - a).norm()) / max_step)) + 1
            t = torch.linspace(0, 1, max(n, 2), dtype=a.dtype)[:, None]
            out.append(bool(self.is_collision(a + t * (b - a)).any()))
        return torch.tensor(out, dtype=torch.bool)


STEP, K = 0.01, 8


def _nodes(n=150):
    """nodes away from the wall's strip, so that moving the gap changes no node's validity (the candidate graph stays)"""
    q = torch.rand(2 * n, 2, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    return q[(q[:, 0] - 0.5).abs() > 0.03][:n]


def _pairs():
    g = torch.Generator().manual_seed(1)
    starts, goals = torch.rand(12, 2, generator=g, dtype=torch.float64), torch.rand(12, 2, generator=g, dtype=torch.float64)
    starts[:, 0] = starts[:, 0] * 0.4                            # left of the wall
    goals[:8, 0] = 0.6 + goals[:8, 0] * 0.4                      # eight across it, four on the same side
    goals[8:, 0] = goals[8:, 0] * 0.4
    return starts, goals


def _same_paths(a, b):
    return all(torch.equal(x, y) and x.dtype == y.dtype for x, y in ((a.path, b.path), (a.count, b.count), (a.length, b.length)))


def _route_edges(rm, res):
    """the edge ids the routes of a result walk over"""
    ids = {tuple(e): m for m, e in enumerate(rm.edges.tolist())}
    out = []
    for p in res.paths():
        if p is not None and len(p) > 2:
            inner = [int((rm.nodes == w).all(dim=1).nonzero()[0, 0]) for w in p[1:-1]]
            out += [ids[(min(a, b), max(a, b))] for a, b in zip(inner, inner[1:])]
    return out


def _states_agree_with_the_checker(rm, ck):
    known = (rm.edge_state != 0).nonzero().reshape(-1)
    hit = ck.check_motions(rm.nodes[rm.edges[known, 0]], rm.nodes[rm.edges[known, 1]], max_step=STEP)
    return torch.equal(rm.edge_state[known] == 2, hit)


def test_lazy_roadmap_reaches_the_eager_one_on_a_fake_checker():
    from diffco_amd.roadmap import Roadmap, knn_edges
    ck, nodes = _Wall(), _nodes()
    starts, goals = _pairs()
    lazy = Roadmap.build(ck, nodes, K, STEP, lazy=True)
    assert ck.motion_calls == 0 and lazy.lazy and lazy.edge_state.dtype == torch.uint8 and not lazy.edge_state.any()
    M = len(lazy.edges)
    assert torch.equal(lazy.edges, knn_edges(nodes, K)) and lazy.lengths.shape == (M,)
    # the index arrays: entry ent[m, 0] lies in row i and names j, ent[m, 1] the other way round, and eid leads back
    rowptr, col, weight = lazy.csr()
    eid, ent, ends, state = lazy.lazy_arrays()
    assert state is lazy.edge_state and torch.equal(ends.long(), lazy.edges)
    for side in (0, 1):
        e = ent[:, side].long()
        assert torch.equal(eid[e].long(), torch.arange(M)) and torch.equal(col[e].long(), lazy.edges[:, 1 - side])
        assert bool((rowptr[lazy.edges[:, side]] <= e).all()) and bool((e < rowptr[lazy.edges[:, side] + 1]).all())
        assert torch.equal(weight[e], lazy.lengths.float())
    eager = Roadmap.build(_Wall(), nodes, K, STEP)
    assert not eager.lazy and 0 < len(eager.edges) < M
    want = eager.query_batch(starts, goals)
    assert bool(want.settled.all()) and (want.iters, want.checked) == (1, 0)

    res = lazy.query_batch(starts, goals)
    assert res.route == "host" and res.iters > 1 and bool(res.settled.all())
    assert 0 < res.checked == int((lazy.edge_state != 0).sum()) < M // 2 and ck.edges_checked == res.checked + 12 + 2 * 12 * K
    full = copy.deepcopy(lazy)
    assert full.validate() == M - res.checked and not bool((full.edge_state == 0).any())
    assert torch.equal(full.edges[full.edge_state == 1], eager.edges)
    after = full.query_batch(starts, goals)
    assert torch.equal(res.length.view(torch.int32), after.length.view(torch.int32))           # (i)
    assert _same_paths(after, want) and (after.iters, after.checked) == (1, 0)                   # (ii)
    assert _same_paths(res, want)                               # (the routes themselves are the eager ones)
    used = _route_edges(lazy, res)
    assert len(used) > 20 and bool((lazy.edge_state[used] == 1).all())                           # (iii)
    assert _states_agree_with_the_checker(lazy, ck) and bool((lazy.edge_state == 2).any())       # (iv)
    assert int((res.count > 2).sum()) >= 6
    # what the roadmap learnt stays: the same queries again check nothing, and `query` is query_batch with one pair
    again = lazy.query_batch(starts, goals)
    assert (again.iters, again.checked) == (1, 0) and _same_paths(again, res)
    path, length = lazy.query(starts[0], goals[0])
    assert torch.equal(path, res.path[0, :int(res.count[0])]) and length == float(res.length[0])
    assert lazy.query(torch.tensor([0.5, 0.9], dtype=torch.float64), goals[0]) is None

    # (v) the gap moves: invalidate, and the routes are those of an eager roadmap built on the new wall
    ck.gap_y = 0.2
    checked_before = ck.edges_checked
    lazy.invalidate()
    assert not lazy.edge_state.any() and torch.equal(lazy.csr()[2][ent[:, 0].long()], lazy.lengths.float())
    moved = lazy.query_batch(starts, goals)
    want2 = Roadmap.build(_Wall(0.2), nodes, K, STEP).query_batch(starts, goals)
    assert _same_paths(moved, want2) and not _same_paths(moved, res)
    assert moved.checked > 0 and ck.edges_checked == checked_before + moved.checked + 12 + 2 * 12 * K
    assert _states_agree_with_the_checker(lazy, ck)
    # ... and edge by edge: forgetting the blocked edges alone re-checks them alone
    was_blocked = (lazy.edge_state == 2).nonzero().reshape(-1)
    unknown_before = int((lazy.edge_state == 0).sum())
    lazy.invalidate(was_blocked)
    assert int((lazy.edge_state == 0).sum()) == unknown_before + len(was_blocked) > unknown_before
    assert not bool(torch.isinf(lazy.csr()[2]).any())
    once_more = lazy.query_batch(starts, goals)
    assert _same_paths(once_more, want2) and once_more.checked > 0


def test_max_iters_cuts_the_loop_and_says_so():
    from diffco_amd.roadmap import Roadmap
    ck, nodes = _Wall(), _nodes()
    starts, goals = _pairs()
    full = Roadmap.build(ck, nodes, K, STEP, lazy=True).query_batch(starts, goals)
    rm = Roadmap.build(ck, nodes, K, STEP, lazy=True)
    cut = rm.query_batch(starts, goals, max_iters=1)
    assert cut.iters == 1 and 0 < cut.checked < full.checked
    out = ~cut.settled
    assert bool(out.any()) and not bool(out.all())                                               # (vi)
    assert not cut.count[out].any() and bool(torch.isinf(cut.length[out]).all()) and bool((cut.mode[out] == 2).all())
    # a settled query's route is final
    keep = cut.settled
    assert torch.equal(cut.count[keep], full.count[keep]) and torch.equal(cut.length[keep], full.length[keep])
    # a small capacity only takes more passes: the same routes, and never more checks than the passes allow
    small = Roadmap.build(ck, nodes, K, STEP, lazy=True).query_batch(starts, goals, check_capacity=4)
    assert _same_paths(small, full) and small.iters > full.iters and small.checked <= 4 * small.iters
    with pytest.raises(ValueError, match="max_iters"):
        rm.query_batch(starts, goals, max_iters=0)
    with pytest.raises(ValueError, match="check_capacity"):
        rm.query_batch(starts, goals, check_capacity=0)
    with pytest.raises(ValueError, match="lazy=False"):
        Roadmap.build(_Wall(), nodes, K, STEP).lazy_arrays()
