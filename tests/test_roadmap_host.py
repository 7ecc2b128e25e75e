"""CPU checks of the roadmap layer: the numpy referee of dcx_knn against an fp64 brute force, roadmap.host_knn against the
referee bit for bit, knn_edges against a set built in pure Python, and Roadmap on a fake checker (a 2-D point robot and a
wall with a gap) - no GPU, no native call."""
import math

import numpy as np
import pytest
import torch

from knn_helpers import cloud, knn_ref, same, where_differs
from motion_wrap_helpers import F


# ------------------------------------------------------------------------------------------------ the referee itself
def _brute64(q, p, mask):
    d = p[None].astype(np.float64) - q[:, None].astype(np.float64)
    on = np.array([bool((mask >> j) & 1) for j in range(q.shape[1])])
    d[..., on] = (d[..., on] + np.pi) % (2 * np.pi) - np.pi
    return (d * d).sum(-1)


@pytest.mark.parametrize("dof,mask", [(2, 0), (2, 0b11), (7, 0), (7, 0b0100101)])
def test_referee_agrees_with_fp64_where_the_gap_is_clear(dof, mask):
    k = 5
    x = cloud(11 + dof, 200, dof, mask)
    idx, _ = knn_ref(x, x, k, mask, self_offset=0)
    d64 = _brute64(x, x, mask)
    np.fill_diagonal(d64, np.inf)
    order = np.argsort(d64, axis=1, kind="stable")
    srt = np.take_along_axis(d64, order, axis=1)
    clear = (srt[:, k] - srt[:, k - 1]) > 1e-5 * srt[:, k]
    assert clear.mean() >= 0.95
    for i in np.flatnonzero(clear):
        assert set(idx[i].tolist()) == set(order[i, :k].tolist()), i


def test_referee_measures_along_the_shortest_arc():
    p = np.array([[3.0, 0.0], [0.0, 0.0], [-3.0, 0.0], [1.5, 0.0]], F)
    idx, d2 = knn_ref(p[:1], p, 1, mask=0b01, self_offset=0)
    assert idx[0, 0] == 2 and abs(math.sqrt(d2[0, 0]) - (2 * math.pi - 6.0)) < 1e-5
    idx, d2 = knn_ref(p[:1], p, 3, mask=0, self_offset=0)
    assert idx[0].tolist() == [3, 1, 2] and abs(d2[0, 2] - 36.0) < 1e-4


# ------------------------------------------------------------------------------------------------ host_knn == referee
def _tricky(seed, n, dof, mask):
    """a cloud with a fifth of its points duplicated (ties go by index) and one row holding a NaN"""
    x = cloud(seed, n, dof, mask)
    g = np.random.default_rng(seed + 1)
    dup = g.choice(n, n // 5, replace=False)
    x[dup] = x[g.integers(0, n, len(dup))]
    x[n // 2, dof - 1] = np.nan
    return x


@pytest.mark.parametrize("chunk", [7, 64, 1000])
@pytest.mark.parametrize("dof,mask", [(2, 0b10), (7, 0), (7, 0b1111111)])
def test_host_knn_equals_the_referee(dof, mask, chunk):
    from diffco_amd.roadmap import host_knn
    p = _tricky(3, 151, dof, mask)
    q = np.concatenate([cloud(4, 40, dof, mask), p[:9]])
    q[5, 0] = np.nan                                                # a NaN query: its row is all -1 / +inf
    for k in (1, 5, 16):
        got = host_knn(torch.from_numpy(q), torch.from_numpy(p), k, wrap=mask, chunk=chunk)
        want = knn_ref(q, p, k, mask)
        assert same(got, want), (k, where_differs(got, want))
        assert (want[0][5] == -1).all() and np.isinf(want[1][5]).all()
    # a radius that is one of the referee's own distances: the boundary itself is admitted
    want5 = knn_ref(q, p, 5, mask)
    r2 = want5[1][0, 2]
    got = host_knn(torch.from_numpy(q), torch.from_numpy(p), 5, wrap=mask, max_dist=math.sqrt(float(r2)), chunk=chunk)
    r2_host = F(math.sqrt(float(r2))) * F(math.sqrt(float(r2)))      # what the host squares in float32
    want = knn_ref(q, p, 5, mask, max_dist2=r2_host)
    assert same(got, want), where_differs(got, want)
    assert (want[0] == -1).any() and (want[0][:, 0] >= 0).any()
    # the queries are the points / a slice of them
    got = host_knn(torch.from_numpy(p), torch.from_numpy(p), 5, wrap=mask, exclude_self=True, chunk=chunk)
    want = knn_ref(p, p, 5, mask, self_offset=0)
    assert same(got, want), where_differs(got, want)
    assert not (want[0] == np.arange(len(p))[:, None]).any()
    got = host_knn(torch.from_numpy(p[30:50]), torch.from_numpy(p), 5, wrap=mask, self_offset=30, chunk=chunk)
    want = knn_ref(p[30:50], p, 5, mask, self_offset=30)
    assert same(got, want), where_differs(got, want)
    # fewer points than k, none at all, no query
    got = host_knn(torch.from_numpy(q), torch.from_numpy(p[:4]), 16, wrap=mask, chunk=chunk)
    assert same(got, knn_ref(q, p[:4], 16, mask))
    got = host_knn(torch.from_numpy(q), torch.from_numpy(p[:0]), 3, wrap=mask, chunk=chunk)
    assert same(got, knn_ref(q, p[:0], 3, mask))
    got = host_knn(torch.from_numpy(q[:0]), torch.from_numpy(p), 3, wrap=mask, chunk=chunk)
    assert got[0].shape == (0, 3) and got[1].shape == (0, 3)


def test_host_knn_breaks_ties_by_index():
    from diffco_amd.roadmap import host_knn
    p = np.zeros((10, 3), F)
    p[7] = 1.0
    idx, d2 = host_knn(torch.from_numpy(p[:1]), torch.from_numpy(p), 4, chunk=3)
    assert idx[0].tolist() == [0, 1, 2, 3] and d2[0].tolist() == [0.0] * 4
    idx, _ = host_knn(torch.from_numpy(p), torch.from_numpy(p), 9, exclude_self=True, chunk=4)
    assert idx[3].tolist() == [0, 1, 2, 4, 5, 6, 8, 9, 7]


# ------------------------------------------------------------------------------------------------ knn_edges
@pytest.mark.parametrize("mask", [0, 0b11])
def test_knn_edges_is_the_sorted_undirected_union(mask):
    from diffco_amd.roadmap import knn_edges
    x = cloud(8, 120, 2, mask)
    for k, r in ((1, None), (6, None), (6, 0.6)):
        e = knn_edges(torch.from_numpy(x), k, wrap=mask, max_dist=r).numpy()
        idx, _ = knn_ref(x, x, k, mask, self_offset=0, max_dist2=None if r is None else F(r) * F(r))
        want = sorted({(min(i, int(j)), max(i, int(j))) for i in range(len(x)) for j in idx[i] if j >= 0})
        assert e.dtype == np.int64 and e.shape == (len(want), 2)
        assert [tuple(r_) for r_ in e.tolist()] == want
        assert (e[:, 0] < e[:, 1]).all()
    assert knn_edges(torch.from_numpy(x[:1]), 3).shape == (0, 2)


# ------------------------------------------------------------------------------------------------ Roadmap
class _Wall:
    """a 2-D point robot and a wall at x = 0.5 of half-thickness 0.02 with a gap for |y - 0.5| < 0.1: exact geometry, the
    motion check sampled under the max_step rule as the library samples (both endpoints included)"""

    def __init__(self, gap=True):
        self.gap = gap
        self.motion_calls = 0

    def is_collision(self, q):
        q = torch.as_tensor(q).reshape(-1, 2)
        hit = (q[:, 0] - 0.5).abs() <= 0.02
        if self.gap:
            hit &= (q[:, 1] - 0.5).abs() >= 0.1
        return hit

    def check_motions(self, starts, targets, max_step=None, wrap=None):
        assert wrap is None and max_step is not None
        self.motion_calls += 1
        out = []
        for a, b in zip(torch.as_tensor(starts), torch.as_tensor(targets)):
            n = int(math.ceil(float((b - a).norm()) / max_step)) + 1
            t = torch.linspace(0, 1, max(n, 2), dtype=a.dtype)[:, None]
            out.append(bool(self.is_collision(a + t * (b - a)).any()))
        return torch.tensor(out, dtype=torch.bool)


def _nodes(seed=0, n=150):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 2, generator=g, dtype=torch.float64)


def _own_dijkstra(n, edges, lengths, extra):
    """the shortest start -> goal distance over (edges, lengths) plus extra = [(end, node, length)], end 0 = start, 1 = goal"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    i = [int(a) for a, _ in edges] + [n + e for e, _, _ in extra]
    j = [int(b) for _, b in edges] + [v for _, v, _ in extra]
    w = [float(x) for x in lengths] + [x for _, _, x in extra]
    g = csr_matrix((w, (i, j)), shape=(n + 2, n + 2))
    return float(dijkstra(g, directed=False, indices=n)[n + 1])


def test_roadmap_on_a_fake_checker():
    from diffco_amd.roadmap import Roadmap, knn_edges
    ck = _Wall()
    nodes = _nodes()
    step, k = 0.01, 8
    rm = Roadmap.build(ck, nodes, k, step)
    assert ck.motion_calls == 1
    # the kept nodes are the free ones, the kept edges exactly those the checker frees
    free = ~ck.is_collision(nodes)
    assert rm.kept.tolist() == free.nonzero().reshape(-1).tolist() and torch.equal(rm.nodes, nodes[free])
    cand = knn_edges(nodes[free], k)
    hit = ck.check_motions(nodes[free][cand[:, 0]], nodes[free][cand[:, 1]], max_step=step)
    assert 0 < int(hit.sum()) < len(cand)
    assert torch.equal(rm.edges, cand[~hit])
    want_len = (nodes[free][rm.edges[:, 1]] - nodes[free][rm.edges[:, 0]]).norm(dim=1)
    assert torch.allclose(rm.lengths, want_len, rtol=0, atol=1e-12)
    g = rm.graph.toarray()
    assert g.shape == (len(rm.nodes),) * 2 and np.array_equal(g, g.T) and (g > 0).sum() == 2 * len(rm.edges)
    assert np.allclose(g[rm.edges[:, 0].numpy(), rm.edges[:, 1].numpy()], rm.lengths.numpy(), rtol=0, atol=0)

    # through the gap: every segment free, the length that of the test's own Dijkstra
    start, goal = torch.tensor([0.1, 0.9], dtype=torch.float64), torch.tensor([0.9, 0.85], dtype=torch.float64)
    assert bool(ck.check_motions(start[None], goal[None], max_step=step)[0])       # the direct motion hits the wall
    ck.motion_calls = 0
    path, length = rm.query(start, goal)
    assert ck.motion_calls == 2                                                    # the direct motion, then the 2k candidates
    assert torch.equal(path[0], start) and torch.equal(path[-1], goal) and len(path) > 2
    assert not ck.check_motions(path[:-1], path[1:], max_step=step).any()
    assert length == pytest.approx(float((path[1:] - path[:-1]).norm(dim=1).sum()), rel=1e-12)
    ends = torch.stack([start, goal])
    d = (rm.nodes[None] - ends[:, None]).norm(dim=2)
    extra = []
    for e in range(2):
        for v in torch.argsort(d[e], stable=True)[:k].tolist():
            if not bool(ck.check_motions(ends[e][None], rm.nodes[v][None], max_step=step)[0]):
                extra.append((e, v, float(d[e, v])))
    assert length == pytest.approx(_own_dijkstra(len(rm.nodes), rm.edges.tolist(), rm.lengths.tolist(), extra), rel=1e-12)
    # the inner waypoints are roadmap nodes joined by roadmap edges
    inner = [int((rm.nodes == p).all(dim=1).nonzero()[0, 0]) for p in path[1:-1]]
    have = {tuple(e) for e in rm.edges.tolist()}
    assert all((min(a, b), max(a, b)) in have for a, b in zip(inner, inner[1:]))

    # a free direct motion: the two-point path; a colliding endpoint: nothing
    a, b = torch.tensor([0.1, 0.2], dtype=torch.float64), torch.tensor([0.4, 0.8], dtype=torch.float64)
    path, length = rm.query(a, b)
    assert path.shape == (2, 2) and torch.equal(path, torch.stack([a, b])) and length == pytest.approx(float((b - a).norm()), rel=1e-12)
    assert rm.query(torch.tensor([0.5, 0.9], dtype=torch.float64), goal) is None
    assert rm.query(start, torch.tensor([0.51, 0.1], dtype=torch.float64)) is None
    # the RRT's query
    i, d2 = rm.nearest(torch.stack([start, goal]))
    assert i.tolist() == d.argmin(dim=1).tolist() and d2.dtype == torch.float32


def test_roadmap_reports_a_walled_off_goal():
    from diffco_amd.roadmap import Roadmap
    ck = _Wall(gap=False)
    rm = Roadmap.build(ck, _nodes(1), 8, 0.01)
    assert len(rm.edges) > 0
    assert rm.query(torch.tensor([0.1, 0.9], dtype=torch.float64), torch.tensor([0.9, 0.1], dtype=torch.float64)) is None
    both_left = rm.query(torch.tensor([0.1, 0.9], dtype=torch.float64), torch.tensor([0.3, 0.1], dtype=torch.float64))
    assert both_left is not None
