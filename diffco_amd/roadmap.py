"""From samples to a path: which configurations to connect, under the metric the motion calls walk.

`knn` (the fused HIP call, _ops.knn) and `host_knn` (the same contract as a chunked torch composition: CPU tensors, and the
baseline the fused call is measured against) return, for every query, its k nearest points ordered by (dist2, index), where
dist2 is bit for bit the squared edge length `check_motions(query, point, wrap=...)` samples.  `knn_edges` turns the lists of
a node set into the undirected edge list of a PRM, and `Roadmap` chains it with a checker's `check_motions` and scipy's
Dijkstra.  The checker is any object with `is_collision(q)` (or `collision(q)`) and `check_motions(starts, targets,
max_step=..., wrap=...)`: DiffCo, the collision_checkers facades, HybridForwardKinematicsDiffCo.
"""
import numpy as np
import torch

from . import _ops

__all__ = ["knn", "host_knn", "knn_edges", "Roadmap"]

_EMPTY = torch.iinfo(torch.int64).max   # the key of an unfilled slot: above every real key (bits(dist2) << 32 | index)


def _knn_args(queries, points, k, exclude_self, self_offset):
    queries, points = torch.as_tensor(queries), torch.as_tensor(points)
    if points.dim() != 2 or queries.dim() != 2 or queries.shape[1] != points.shape[1]:
        raise ValueError(f"knn: queries {tuple(queries.shape)} and points {tuple(points.shape)} must be [Q, dof] and [N, dof]")
    if not 1 <= int(k) <= 64:
        raise ValueError(f"knn: k must be in [1, 64], got {k}")
    if exclude_self:
        if self_offset not in (None, 0):
            raise ValueError("knn: exclude_self means self_offset = 0")
        if queries is not points and queries.shape != points.shape:
            raise ValueError("knn: exclude_self needs the queries to be the points")
        self_offset = 0
    if self_offset is not None and int(self_offset) < 0:
        raise ValueError("knn: self_offset must be >= 0")
    return queries, points, int(k), self_offset


def host_knn(queries, points, k, wrap=None, max_dist=None, exclude_self=False, self_offset=None, transform=None, chunk=4096):
    """_ops.knn's contract and results in plain torch ops, on the tensors' own device: wrapped deltas, the squared sum in
    coordinate order (one rounded operation at a time), keys bits(dist2) << 32 | index, a sort.  At most a chunk x chunk block
    of the Q x N matrix exists at a time."""
    queries, points, k, self_offset = _knn_args(queries, points, k, exclude_self, self_offset)
    dev = points.device
    dof = points.shape[1]
    mask = _ops.wrap_mask(wrap, dof, transform)
    p32 = points.detach().to(torch.float32)
    q32 = queries.detach().to(device=dev, dtype=torch.float32)
    Q, N = len(q32), len(p32)
    chunk = max(int(chunk), 1)
    max_d2 = None if max_dist is None else torch.tensor(float(max_dist), dtype=torch.float32).square().to(dev)
    idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
    dist2 = torch.empty((Q, k), dtype=torch.float32, device=dev)
    from .utils import wrap2pi
    for q0 in range(0, Q, chunk):
        qs = q32[q0:q0 + chunk]
        best = torch.full((len(qs), k), _EMPTY, dtype=torch.int64, device=dev)
        rows = torch.arange(q0, q0 + len(qs), device=dev)
        for p0 in range(0, N, chunk):
            ps = p32[p0:p0 + chunk]
            l2 = torch.zeros((len(qs), len(ps)), dtype=torch.float32, device=dev)
            for j in range(dof):
                d = ps[None, :, j] - qs[:, None, j]
                if (mask >> j) & 1:
                    d = wrap2pi(d)
                l2 = l2 + d * d
            cols = torch.arange(p0, p0 + len(ps), device=dev)
            ok = ~torch.isnan(l2)
            if max_d2 is not None:
                ok &= l2 <= max_d2
            if self_offset is not None:
                ok &= cols[None, :] != (rows[:, None] + int(self_offset))
            keys = (l2.view(torch.int32).to(torch.int64) << 32) | cols[None, :]
            keys = torch.where(ok, keys, torch.full_like(keys, _EMPTY))
            best = torch.sort(torch.cat([best, keys], dim=1), dim=1).values[:, :k]
        empty = best == _EMPTY
        idx[q0:q0 + len(qs)] = torch.where(empty, torch.full_like(best, -1), best & 0xFFFFFFFF).to(torch.int32)
        d2 = (best >> 32).to(torch.int32).view(torch.float32)
        dist2[q0:q0 + len(qs)] = torch.where(empty, torch.full_like(d2, float("inf")), d2)
    return idx, dist2


def knn(queries, points, k, wrap=None, max_dist=None, exclude_self=False, self_offset=None, transform=None):
    """(idx int32 [Q, k], dist2 float32 [Q, k]): the fused call for device tensors (_ops.knn), host_knn for CPU tensors"""
    points = torch.as_tensor(points)
    fn = _ops.knn if points.device.type == "cuda" else host_knn
    return fn(queries, points, k, wrap=wrap, max_dist=max_dist, exclude_self=exclude_self, self_offset=self_offset,
              transform=transform)


def knn_edges(nodes, k, wrap=None, max_dist=None, transform=None):
    """[M, 2] int64: the undirected union of every node's k-nearest list, each pair once as (i, j) with i < j, sorted by (i, j)"""
    nodes = torch.as_tensor(nodes)
    N = len(nodes)
    idx, _ = knn(nodes, nodes, min(int(k), 64), wrap=wrap, max_dist=max_dist, exclude_self=True, transform=transform)
    j = idx.to(torch.int64)
    i = torch.arange(N, device=j.device)[:, None].expand_as(j)
    found = j >= 0
    i, j = i[found], j[found]
    keys = torch.unique_consecutive(torch.sort(torch.minimum(i, j) * N + torch.maximum(i, j)).values)
    return torch.stack([torch.div(keys, max(N, 1), rounding_mode="floor"), keys % max(N, 1)], dim=1)


class _Checker:
    """the two calls a roadmap needs, whatever the checker calls them: `is_collision` (DiffCo) or `collision` (the facades,
    whose scores keep a trailing class axis), and `check_motions`"""

    def __init__(self, checker):
        self.checker = checker
        self.point = getattr(checker, "is_collision", None) or getattr(checker, "collision")
        self.transform = getattr(checker, "transform", None) or getattr(getattr(checker, "perceptron", None), "transform", None)

    def collides(self, q):
        hit = torch.as_tensor(self.point(q)).to(torch.bool).reshape(len(q), -1)
        return hit.any(dim=1)

    def motions(self, qa, qb, max_step, mask, **kw):
        if len(qa) == 0:
            return torch.zeros(0, dtype=torch.bool, device=qa.device)
        hit = self.checker.check_motions(qa, qb, max_step=max_step, wrap=mask if mask else None, **kw)
        return torch.as_tensor(hit).to(device=qa.device, dtype=torch.bool).reshape(-1)


class Roadmap:
    """A probabilistic roadmap over `nodes`: `build` keeps the collision-free nodes, connects each to its k nearest under the
    motion metric and keeps the edges one `check_motions` call frees; `query` connects two configurations to it and returns
    the shortest route.  Attributes: nodes [n, dof] (the kept ones), kept [n] (their indices into the given nodes), edges
    [M, 2] int64 (i < j, into `nodes`), lengths [M], graph (symmetric scipy.sparse.csr_matrix of the lengths)."""

    def __init__(self, checker, nodes, kept, edges, lengths, k, max_step, mask, check_kw):
        from scipy.sparse import csr_matrix
        self.checker = checker if isinstance(checker, _Checker) else _Checker(checker)
        self.nodes, self.kept, self.edges, self.lengths = nodes, kept, edges, lengths
        self.k, self.max_step, self.wrap_mask, self.check_kw = k, max_step, mask, dict(check_kw)
        n = len(nodes)
        e = edges.cpu().numpy()
        w = lengths.detach().cpu().numpy().astype(np.float64)
        self.graph = csr_matrix((np.concatenate([w, w]), (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))),
                                shape=(n, n))

    @classmethod
    def build(cls, checker, nodes, k, max_step, wrap=None, max_dist=None, **check_kw):
        ck = _Checker(checker)
        nodes = torch.as_tensor(nodes).detach()
        mask = _ops.wrap_mask(wrap, nodes.shape[1], ck.transform)
        kept = (~ck.collides(nodes)).to(nodes.device).nonzero().reshape(-1)
        nodes = nodes[kept]
        cand = knn_edges(nodes, k, wrap=mask, max_dist=max_dist)
        qa, qb = nodes[cand[:, 0]], nodes[cand[:, 1]]
        free = ~ck.motions(qa, qb, max_step, mask, **check_kw)
        edges = cand[free]
        lengths = _ops.wrapped_delta(qa[free], qb[free], mask).norm(dim=1)
        return cls(ck, nodes, kept, edges, lengths, int(k), max_step, mask, check_kw)

    def nearest(self, q):
        """(idx [Q], dist2 [Q]) of the kept node nearest to each q [Q, dof] (an RRT's query)"""
        q = torch.as_tensor(q).reshape(-1, self.nodes.shape[1])
        idx, d2 = knn(q, self.nodes, 1, wrap=self.wrap_mask)
        return idx[:, 0], d2[:, 0]

    def query(self, start, goal, k=None):
        """(waypoints [W, dof], length) of the shortest route start -> goal over the roadmap, or None where an endpoint
        collides or no route exists.  A free direct motion is returned as the two-point path."""
        from scipy.sparse import coo_matrix, vstack, hstack, csr_matrix
        from scipy.sparse.csgraph import dijkstra
        nodes, mask = self.nodes, self.wrap_mask
        dof = nodes.shape[1]
        ends = torch.stack([torch.as_tensor(start).reshape(dof), torch.as_tensor(goal).reshape(dof)]).to(device=nodes.device, dtype=nodes.dtype)
        if bool(self.checker.collides(ends).any()):
            return None
        if not bool(self.checker.motions(ends[:1], ends[1:], self.max_step, mask, **self.check_kw)[0]):
            return ends, float(_ops.wrapped_delta(ends[:1], ends[1:], mask).norm(dim=1)[0])
        n = len(nodes)
        if n == 0:
            return None
        idx, _ = knn(ends, nodes, min(int(self.k if k is None else k), 64), wrap=mask)
        j = idx.to(torch.int64).reshape(-1)
        e = torch.arange(2, device=j.device).repeat_interleave(idx.shape[1])
        e, j = e[j >= 0], j[j >= 0]
        qa, qb = ends[e], nodes[j]
        free = ~self.checker.motions(qa, qb, self.max_step, mask, **self.check_kw)
        e, j = e[free].cpu().numpy(), j[free].cpu().numpy()
        w = _ops.wrapped_delta(qa[free], qb[free], mask).norm(dim=1).detach().cpu().numpy().astype(np.float64)
        link = coo_matrix((w, (e, j)), shape=(2, n)).tocsr()   # rows: start, goal
        g = vstack([hstack([self.graph, link.T]), hstack([link, csr_matrix((2, 2))])]).tocsr()
        dist, pred = dijkstra(g, directed=False, indices=n, return_predecessors=True)
        if not np.isfinite(dist[n + 1]):
            return None
        route = [n + 1]
        while route[-1] != n:
            route.append(int(pred[route[-1]]))
        inner = torch.as_tensor(route[-2:0:-1], dtype=torch.int64, device=nodes.device)
        return torch.cat([ends[:1], nodes[inner], ends[1:]]), float(dist[n + 1])
