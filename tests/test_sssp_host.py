"""CPU checks of the roadmap queries: the numpy referee against a heap Dijkstra in float32 (bit for bit) and scipy's in float64
(within the roundings of the adds), roadmap.host_sssp and roadmap.host_extract_paths against the referee bit for bit, and
Roadmap.query_batch against Roadmap.query on a fake checker (a 2-D point robot and a wall with a gap) - no GPU, no native call."""
import math

import numpy as np
import pytest
import torch

from sssp_helpers import F, GRAPHS, case, dijkstra32, extract_ref, graph, same_bits, sssp_ref

U = 2.0 ** -23   # a rounded float32 add or cast is off by at most half of this, relatively


def _t(c, *names):
    return [torch.from_numpy(c[n]) for n in names]


# ------------------------------------------------------------------------------------------------ the referee itself
@pytest.mark.parametrize("name", GRAPHS)
def test_referee_equals_float32_dijkstra_and_its_walks_end(name):
    c = case(name, 5, all_modes=False)
    n, dist, pred = c["n"], c["dist"], c["pred"]
    assert c["changed"][-1] == 0 and (c["changed"][:-1] == 1).all() or c["rounds"] == 1
    for q in range(5):
        src = [(int(v), c["start_len"][q, s]) for s, v in enumerate(c["start_idx"][q]) if v >= 0]
        assert same_bits(dist[:, q], dijkstra32(c["rowptr"], c["col"], c["weight"], src)), (name, q)
        linked = {v for v, _ in src}
        for v in range(n):
            u, steps = v, 0
            while pred[u, q] >= 0:
                u, steps = int(pred[u, q]), steps + 1
                assert steps <= n, ("cycle", name, q, v)
            assert not np.isfinite(dist[v, q]) or u in linked
    if name == "chain40":      # one source at the end of the chain: a round per hop, and one more that changes nothing
        assert c["rounds"] == 41
    if name == "two_components":
        assert np.isinf(dist).any() and np.isfinite(dist).any()
    if name == "extremes70":   # no +inf edge was adopted
        rp, col, w = c["rowptr"], c["col"], c["weight"]
        for q in range(5):
            for v in np.flatnonzero(pred[:, q] >= 0):
                e = rp[v] + list(col[rp[v]:rp[v + 1]]).index(pred[v, q])
                assert np.isfinite(w[e])


@pytest.mark.parametrize("name", ["chain40", "grid12", "knn300", "hub"])
def test_referee_against_scipy_float64(name):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    c = case(name, 5, all_modes=False)
    n, rp, col, w = c["n"], c["rowptr"], c["col"], c["weight"]
    assert (w > 0).all()                      # (scipy reads a stored zero as no edge)
    rows = np.repeat(np.arange(n), np.diff(rp))
    for q in range(5):
        real = c["start_idx"][q] >= 0
        li, ll = c["start_idx"][q][real], c["start_len"][q][real]
        g = csr_matrix((np.concatenate([w.astype(np.float64), ll.astype(np.float64)]),
                        (np.concatenate([rows, np.full(len(li), n)]), np.concatenate([col, li]))), shape=(n + 1, n + 1))
        d64, p64 = dijkstra(g, directed=True, indices=n, return_predecessors=True)
        d64 = d64[:n]
        assert np.array_equal(np.isfinite(d64), np.isfinite(c["dist"][:, q]))
        for v in np.flatnonzero(np.isfinite(d64)):
            # the adds on the route each side took: its edges and its link
            h32, u = 1, v
            while c["pred"][u, q] >= 0:
                u, h32 = int(c["pred"][u, q]), h32 + 1
            h64, u = 0, v
            while u != n:
                u, h64 = int(p64[u]), h64 + 1
            hops = max(h32, h64)
            assert hops <= n and (hops + 1) * U < 1e-3
            assert abs(float(c["dist"][v, q]) - d64[v]) <= (hops + 1) * U * d64[v], (name, q, v)


# ------------------------------------------------------------------------------------------------ host_sssp == referee
@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("Q", [3, 65])
def test_host_sssp_and_extraction_equal_the_referee(name, Q):
    from diffco_amd.roadmap import host_extract_paths, host_sssp
    c = case(name, Q)
    g = _t(c, "rowptr", "col", "weight")
    si, sl = _t(c, "start_idx", "start_len")
    dist, pred, changed = host_sssp(*g, si, sl)
    assert len(changed) == c["n"] + 1 and changed[c["rounds"]:].sum() == 0
    assert same_bits(dist.numpy(), c["dist"]) and same_bits(pred.numpy(), c["pred"])
    assert np.array_equal(changed[:c["rounds"]].numpy(), c["changed"])
    # a fixed number of rounds short of the fixed point, in small chunks of queries
    few = max(c["rounds"] // 2, 1)
    want = sssp_ref(c["rowptr"], c["col"], c["weight"], c["start_idx"], c["start_len"], few)
    got = host_sssp(*g, si, sl, rounds=few, state_bytes=1)
    assert all(same_bits(a.numpy(), b) for a, b in zip(got, want))
    # extraction: the sizes, the paths, a W that is too small for some
    ex = _t(c, "nodes") + [dist, pred] + _t(c, "mode", "starts", "goals", "goal_idx", "goal_len", "direct_len")
    path, count, length = host_extract_paths(*ex)
    assert path.shape[1] == c["W"]
    assert same_bits(path.numpy(), c["path"]) and same_bits(count.numpy(), c["count"]) and same_bits(length.numpy(), c["length"])
    assert same_bits(host_extract_paths(*ex, W=0)[1].numpy(), c["sizes"])
    small = max(c["W"] - 1, 1)
    want = extract_ref(c["nodes"], c["dist"], c["pred"], c["mode"], c["starts"], c["goals"], c["goal_idx"], c["goal_len"],
                       c["direct_len"], small)
    got = host_extract_paths(*ex, W=small)
    assert all(same_bits(a.numpy(), b) for a, b in zip(got, want))
    if Q == 65:
        assert set(c["mode"].tolist()) == {0, 1, 2}
        if c["n"] > 2:
            assert (want[1] < 0).any() or c["W"] == 2


def test_cases_hold_what_they_are_for():
    c = case("grid12", 65)
    # equal weights: among equal candidates the lowest neighbour is the predecessor (rows are sorted by col)
    rp, col, w = c["rowptr"], c["col"], c["weight"]
    ties = 0
    for q in range(65):
        for v in np.flatnonzero(c["pred"][:, q] >= 0):
            nb = col[rp[v]:rp[v + 1]]
            reach = [int(u) for u in nb if F(c["dist"][u, q] + F(1.0)) == c["dist"][v, q]]
            ties += len(reach) > 1
    assert ties > 100
    c = case("two_components", 65)
    assert ((c["mode"] == 2) & (c["count"] == 0)).any() and np.isinf(c["length"][(c["mode"] == 2) & (c["count"] == 0)]).all()
    c = case("duplicates300", 65)
    assert (c["weight"] == 0).sum() > 20 and (c["count"] > 3).any()
    c = case("hub", 65)
    assert np.diff(c["rowptr"]).max() == 100 and (np.diff(c["rowptr"]) == 0).sum() == 29


def test_no_start_link_at_all():
    from diffco_amd.roadmap import host_extract_paths, host_sssp
    c = case("knn300", 3)
    none = torch.full((3, 4), -1, dtype=torch.int32)
    dist, pred, changed = host_sssp(*_t(c, "rowptr", "col", "weight"), none, torch.from_numpy(c["start_len"]), rounds=6)
    assert changed.tolist() == [0] * 6 and torch.isinf(dist).all() and (pred == -1).all()
    ex = _t(c, "nodes") + [dist, pred] + [torch.full((3,), 2, dtype=torch.int32)] + _t(c, "starts", "goals", "goal_idx", "goal_len",
                                                                                      "direct_len")
    path, count, length = host_extract_paths(*ex)
    assert count.tolist() == [0, 0, 0] and torch.isinf(length).all() and path.shape == (3, 2, 3) and not path.any()


# ------------------------------------------------------------------------------------------------ Roadmap.query_batch
class _Wall:
    """a 2-D point robot and a wall at x = 0.5 of half-thickness 0.02 with a gap for |y - 0.5| < 0.1: exact geometry, the
    motion check sampled under the max_step rule as the library samples (both endpoints included)"""

    def __init__(self, gap=True):
        self.gap = gap
        self.motion_calls = 0
        self.point_calls = 0

    def is_collision(self, q):
        self.point_calls += 1
        return self._hit(torch.as_tensor(q).reshape(-1, 2))

    def _hit(self, q):
        hit = (q[:, 0] - 0.5).abs() <= 0.02
        if self.gap:
            hit &= (q[:, 1] - 0.5).abs() >= 0.1
        return hit

    def check_motions(self, starts, targets, max_step=None, wrap=None, max_samples=None, return_first=False):
        assert wrap is None and max_step is not None
        self.motion_calls += 1
        out, first = [], []
        for a, b in zip(torch.as_tensor(starts), torch.as_tensor(targets)):
            n = int(math.ceil(float((b - a).norm()) / max_step)) + 1
            t = torch.linspace(0, 1, max(n, 2), dtype=a.dtype)[:, None]
            hit = self._hit(a + t * (b - a))
            out.append(bool(hit.any()))
            first.append(int(hit.nonzero()[0, 0]) if out[-1] else -1)
        out = torch.tensor(out, dtype=torch.bool)
        return (out, torch.tensor(first, dtype=torch.int32)) if return_first else out


def _nodes(seed=0, n=150):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 2, generator=g, dtype=torch.float64)


def _pairs():
    t = lambda *v: torch.tensor(v, dtype=torch.float64)   # noqa: E731
    g = torch.Generator().manual_seed(7)
    left = torch.rand(6, 2, generator=g, dtype=torch.float64) * torch.tensor([0.4, 1.0], dtype=torch.float64) + 0.02
    right = left.flip(0) + torch.tensor([0.55, 0.0], dtype=torch.float64)
    starts = torch.cat([torch.stack([t(0.1, 0.9), t(0.1, 0.2), t(0.5, 0.9), t(0.1, 0.9)]), left])
    goals = torch.cat([torch.stack([t(0.9, 0.85), t(0.4, 0.8), t(0.9, 0.85), t(0.51, 0.1)]), right])
    return starts, goals


@pytest.mark.parametrize("gap", [True, False], ids=["gap", "walled_off"])
def test_query_batch_on_a_fake_checker(gap):
    from diffco_amd.roadmap import Roadmap, RoadmapPaths, knn
    from diffco_amd.shortcut import host_shortcut_paths
    ck = _Wall(gap)
    step, k = 0.01, 8
    rm = Roadmap.build(ck, _nodes(0 if gap else 1), k, step)
    starts, goals = _pairs()
    Q = len(starts)
    single = [rm.query(a, b) for a, b in zip(starts, goals)]
    ck.motion_calls = ck.point_calls = 0
    res = rm.query_batch(starts, goals)
    assert isinstance(res, RoadmapPaths) and res.route == "host"
    assert ck.point_calls == 1 and ck.motion_calls == 2                     # the checker is asked three times, whatever Q is
    assert res.path.shape[0] == Q and res.path.shape[2] == 2 and res.count.dtype == torch.int32 and res.length.dtype == torch.float32
    assert res.mode.tolist()[:4] == [2, 1, 0, 0] and 1 <= res.rounds <= len(rm.nodes)
    paths = res.paths()
    # the links the test itself finds free
    ends = torch.cat([starts, goals])
    idx, _ = knn(ends, rm.nodes, k)
    free = ~ck.check_motions(ends.repeat_interleave(k, dim=0), rm.nodes[idx.long().reshape(-1)], max_step=step).reshape(2 * Q, k)
    have = {tuple(e) for e in rm.edges.tolist()}
    routed = 0
    for q in range(Q):
        if single[q] is None:                                               # a colliding endpoint, a walled-off goal
            assert paths[q] is None and int(res.count[q]) == 0 and math.isinf(float(res.length[q])), q
            continue
        p1, l1 = single[q]
        p = paths[q]
        assert p is not None and len(p) == int(res.count[q]) and p.dtype == rm.nodes.dtype
        assert torch.equal(p[0], starts[q]) and torch.equal(p[-1], goals[q])
        assert not ck.check_motions(p[:-1], p[1:], max_step=step).any()
        if len(p1) == 2:                                                    # a free direct motion: the two-point path
            assert len(p) == 2 and int(res.mode[q]) == 1
        hops = max(len(p), len(p1)) - 1
        assert hops < 64
        assert abs(float(res.length[q]) - l1) <= (hops + 1) * U * l1, (q, float(res.length[q]), l1)
        assert abs(float(res.length[q]) - float((p[1:] - p[:-1]).norm(dim=1).sum())) <= (hops + 1) * U * l1
        if len(p) > 2:
            routed += 1
            inner = [int((rm.nodes == w).all(dim=1).nonzero()[0, 0]) for w in p[1:-1]]
            assert all((min(a, b), max(a, b)) in have for a, b in zip(inner, inner[1:]))
            assert inner[0] in idx[q][free[q]].tolist() and inner[-1] in idx[Q + q][free[Q + q]].tolist()
    assert [s is None for s in single][:4] == [not gap, False, True, True]
    assert routed >= (3 if gap else 0) and any(s is None for s in single)
    # the result goes into the shortcutter as it is (two-point paths alone leave it nothing to pick from)
    if res.path.shape[1] > 2:
        short = host_shortcut_paths(ck, res.path, res.count, max_step=step, rounds=4)
        assert all(n <= c for n, c in zip(short.count.tolist(), res.count.tolist()))
        for q in range(Q):
            if int(res.count[q]) >= 2:
                assert float(short.lengths[q]) <= float(res.length[q]) * (1 + 1e-5)
    else:
        assert not gap
    # a W that some routes do not fit: -n, and their rows stay zero
    if routed:
        tight = rm.query_batch(starts, goals, max_waypoints=2)
        assert tight.path.shape[1] == 2 and (tight.count < 0).sum() == routed
        assert torch.equal(tight.count.abs(), res.count) and torch.equal(tight.length, res.length)
        assert not tight.path[tight.count < 0].any()
    # the chunking of the queries does not change anything
    old = Roadmap.STATE_BUDGET
    try:
        Roadmap.STATE_BUDGET = 12 * len(rm.nodes) * 3
        parts = rm.query_batch(starts, goals, rounds_per_call=1)
    finally:
        Roadmap.STATE_BUDGET = old
    assert torch.equal(parts.path, res.path) and torch.equal(parts.count, res.count) and torch.equal(parts.length, res.length)
    assert parts.rounds == res.rounds


def test_csr_is_the_symmetric_graph():
    from diffco_amd.roadmap import Roadmap
    rm = Roadmap.build(_Wall(), _nodes(), 8, 0.01)
    rowptr, col, weight = rm.csr()
    n = len(rm.nodes)
    assert rowptr.dtype == torch.int32 and col.dtype == torch.int32 and weight.dtype == torch.float32
    g = rm.graph.tocsr()
    g.sort_indices()
    assert rowptr.tolist() == g.indptr.tolist() and col.tolist() == g.indices.tolist() and len(rowptr) == n + 1
    assert np.array_equal(weight.numpy(), g.data.astype(np.float32))
    assert rm.csr()[0] is rowptr


def test_python_layer_rejects_bad_arguments_without_a_device():
    from diffco_amd.roadmap import Roadmap, host_sssp
    rm = Roadmap.build(_Wall(), _nodes(), 8, 0.01)
    with pytest.raises(ValueError, match="starts and"):
        rm.query_batch(torch.zeros(2, 2), torch.zeros(3, 2))
    with pytest.raises(ValueError, match="route"):
        rm.query_batch(torch.zeros(2, 2), torch.zeros(2, 2), route="fused")
    with pytest.raises(ValueError, match="rounds_per_call"):
        rm.query_batch(torch.zeros(2, 2), torch.zeros(2, 2), rounds_per_call=0)
    n, rp, col, w = graph("pair")
    with pytest.raises(ValueError, match="link_idx"):
        host_sssp(torch.from_numpy(rp), torch.from_numpy(col), torch.from_numpy(w), torch.zeros(3, 2, dtype=torch.int32),
                  torch.zeros(3, 1))
    empty = rm.query_batch(torch.zeros(0, 2), torch.zeros(0, 2))
    assert empty.path.shape == (0, 2, 2) and empty.paths() == [] and empty.rounds == 0
