"""From samples to a path: which configurations to connect, under the metric the motion calls walk.

`knn` (the fused HIP call, _ops.knn) and `host_knn` (the same contract as a chunked torch composition: CPU tensors, and the
baseline the fused call is measured against) return, for every query, its k nearest points ordered by (dist2, index), where
dist2 is bit for bit the squared edge length `check_motions(query, point, wrap=...)` samples.  `knn_edges` turns the lists of
a node set into the undirected edge list of a PRM, and `Roadmap` chains it with a checker's `check_motions` and scipy's
Dijkstra.  The checker is any object with `is_collision(q)` (or `collision(q)`) and `check_motions(starts, targets,
max_step=..., wrap=...)`: DiffCo, the collision_checkers facades, HybridForwardKinematicsDiffCo.

`Roadmap.query_batch` is the multi-query half: Q start/goal pairs answered by synchronous min-plus relaxation over the roadmap's
CSR (the fused HIP calls _ops.sssp_run and _ops.sssp_extract_paths; `host_sssp` and `host_extract_paths` state the same contract
in torch ops: CPU tensors, the referee and the baseline), the routes in one [Q, W, dof] tensor (`RoadmapPaths`).

`Roadmap.build(..., lazy=True)` is the lazy PRM: no edge is checked until a shortest route uses it.  `query_batch` then loops
relax - mark - check - apply (the fused HIP calls _ops.sssp_mark_routes and _ops.graph_apply_checks; `host_mark_routes` and
`host_apply_checks` are their contract in torch ops) until every route stands on checked edges: for a checker whose motion
checks are expensive (the hybrid one's ground truth) or whose model changes (`invalidate` after `checker.update`).
"""
import numpy as np
import torch

from . import _ops

__all__ = ["knn", "host_knn", "knn_edges", "Roadmap", "RoadmapPaths", "host_sssp", "host_extract_paths", "host_mark_routes",
           "host_apply_checks"]

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


def _bits_key(cand, slot):
    """int64 keys bits(cand) << 32 | slot: among non-negative floats the order of the keys is that of (value, slot), +inf last"""
    return (cand.contiguous().view(torch.int32).to(torch.int64) << 32) | slot


def host_sssp(rowptr, col, weight, link_idx, link_len, rounds=None, state_bytes=1 << 28):
    """dcx_sssp_run's contract (include/dcx.h, "roadmap queries") in plain torch ops on the tensors' own device: Jacobi rounds
    of the min-plus relaxation over the symmetric CSR (rowptr [N + 1], col, weight [nnz]) for the Q queries whose start
    links are link_idx / link_len [Q, k] (-1 = no link).  Every candidate is one rounded float32 add, the first minimum in
    row order wins (keys bits(cand) << 32 | slot and a min), and dist / pred change on a strict decrease only.
    Returns (dist [N, Q] float32, pred [N, Q] int32, changed int32 [rounds]): the state after `rounds` rounds, round 0 (the
    links) included; rounds=None runs until a round changes nothing, that round included (at most N + 1).
    The rows are padded to the largest degree and the queries taken in chunks, so that a chunk's keys stay under
    `state_bytes`."""
    rowptr, col, weight = torch.as_tensor(rowptr), torch.as_tensor(col), torch.as_tensor(weight)
    link_idx, link_len = torch.as_tensor(link_idx), torch.as_tensor(link_len)
    dev = rowptr.device
    N, Q = len(rowptr) - 1, len(link_idx)
    if rowptr.dim() != 1 or N < 0 or col.shape != weight.shape or col.dim() != 1 or link_idx.dim() != 2 or link_idx.shape != link_len.shape:
        raise ValueError("host_sssp: rowptr [N + 1], col and weight [nnz], link_idx and link_len [Q, k]")
    cap = N + 1 if rounds is None else int(rounds)
    if cap < 0:
        raise ValueError("host_sssp: rounds must be >= 0")
    rp = rowptr.to(torch.int64)
    nnz = len(col)
    deg = rp[1:] - rp[:-1]
    D = int(deg.max()) if N > 0 else 0
    slot = torch.arange(D, device=dev)
    valid = slot[None, :] < deg[:, None]                                             # [N, D]
    ent = (rp[:-1, None] + slot[None, :]).clamp(max=max(nnz - 1, 0))
    nb = col.to(torch.int64)[ent] if nnz else torch.zeros((N, D), dtype=torch.int64, device=dev)
    valid = valid & (nb >= 0) & (nb < N)
    nb = nb.clamp(0, max(N - 1, 0))
    w = weight.to(torch.float32)[ent] if nnz else torch.zeros((N, D), dtype=torch.float32, device=dev)
    li = link_idx.to(torch.int64)
    real = (li >= 0) & (li < N)
    dist = torch.full((N, Q), float("inf"), dtype=torch.float32, device=dev)
    pred = torch.full((N, Q), -1, dtype=torch.int32, device=dev)
    changed = torch.zeros(cap, dtype=torch.int32, device=dev)
    if cap == 0 or Q == 0:
        return dist, pred, changed
    qq = torch.arange(Q, device=dev)[:, None].expand_as(li)
    dist[li[real], qq[real]] = link_len.to(torch.float32)[real]
    changed[0] = int(bool(real.any()))
    if N == 0:
        return dist, pred, changed
    qc = max(1, int(state_bytes) // max(8 * N * max(D, 1), 1))
    for t in range(1, cap):
        if int(changed[t - 1]) == 0:
            break   # (the rounds left change nothing either: their flags stay 0)
        new = dist.clone()
        any_change = False
        for q0 in range(0, Q, qc):
            old = dist[:, q0:q0 + qc]                                               # [N, Qc]
            if D == 0:
                continue
            cand = old[nb] + w[:, :, None]                                          # [N, D, Qc]: one rounded add each
            keys = torch.where(valid[:, :, None], _bits_key(cand, slot[None, :, None]), torch.full((), _EMPTY, dtype=torch.int64, device=dev))
            best = keys.min(dim=1).values                                           # [N, Qc]
            bc = torch.where(best == _EMPTY, torch.full_like(old, float("inf")), (best >> 32).to(torch.int32).view(torch.float32))
            bu = torch.gather(nb, 1, (best & 0xFFFFFFFF).clamp(max=max(D - 1, 0)))
            win = bc < old
            new[:, q0:q0 + qc] = torch.where(win, bc, old)
            pred[:, q0:q0 + qc] = torch.where(win, bu.to(torch.int32), pred[:, q0:q0 + qc])
            any_change = any_change or bool(win.any())
        dist = new
        changed[t] = int(any_change)
    return dist, pred, changed


def host_extract_paths(nodes, dist, pred, mode, starts, goals, goal_idx, goal_len, direct_len, W=None):
    """dcx_sssp_extract_paths' contract in plain torch ops on the tensors' own device: (path [Q, W, dof] in the nodes' dtype,
    count [Q] int32, length [Q] float32) from the state (dist, pred [N, Q]) of host_sssp.  mode 0: no path; mode 1: (start,
    goal) and direct_len; mode 2: the first goal slot, in slot order, with the least dist[goal_idx][q] + goal_len (one rounded
    float32 add), then pred walked back to -1.  count[q] = n where the n waypoints fit in W and were written, -n where they
    do not (the row stays zero), 0 without a route.  W=None: the longest route's size (at least 2)."""
    nodes = torch.as_tensor(nodes)
    dev = nodes.device
    N, dof = nodes.shape
    Q = len(goal_idx)
    mode = torch.as_tensor(mode).to(device=dev, dtype=torch.int64)
    length, routed, chain = _walk_routes(N, dist, pred, mode, goal_idx, goal_len)
    inf = torch.full((Q,), float("inf"), dtype=torch.float32, device=dev)
    depth = (chain >= 0).sum(dim=0) * routed
    length = torch.where(mode == 1, torch.as_tensor(direct_len).to(device=dev, dtype=torch.float32), torch.where(routed, length, inf))
    n = torch.where(mode == 1, torch.full_like(depth, 2), torch.where(routed, depth + 2, torch.zeros_like(depth)))
    if W is None:
        W = max(int(n.max()) if Q else 0, 2)
    W = int(W)
    fits = (n > 0) & (n <= W)
    count = torch.where(fits, n, -n).to(torch.int32)
    path = torch.zeros((Q, W, dof), dtype=nodes.dtype, device=dev)
    qf = fits.nonzero().reshape(-1)
    if len(qf):
        path[qf, 0] = torch.as_tensor(starts).to(device=dev, dtype=nodes.dtype)[qf]
        path[qf, n[qf] - 1] = torch.as_tensor(goals).to(device=dev, dtype=nodes.dtype)[qf]
    on = (chain >= 0) & (fits & routed & (mode == 2))[None, :]
    h, q = on.nonzero(as_tuple=True)
    if len(h):
        path[q, depth[q] - h] = nodes[chain[h, q]]
    return path, count, length


def _walk_routes(N, dist, pred, mode, goal_idx, goal_len):
    """the goal slot and the predecessor walk host_extract_paths and host_mark_routes share, for mode int64 [Q] on the state's
    device: (length [Q] float32, +inf without a route; routed [Q] bool; chain [H, Q] int64, chain[h, q] the node h hops
    before the goal link's, -1 past the walk's end)"""
    dev = dist.device
    Q, k = goal_idx.shape
    gi = goal_idx.to(torch.int64)
    real = (gi >= 0) & (gi < N) & (mode == 2)[:, None]
    qq = torch.arange(Q, device=dev)
    slot = torch.arange(k, device=dev)[None, :]
    if N > 0:
        cand = dist[gi.clamp(0, N - 1), qq[:, None]] + goal_len.to(torch.float32)
    else:
        cand = torch.full((Q, k), float("inf"), dtype=torch.float32, device=dev)
    keys = torch.where(real, _bits_key(cand, slot), torch.full((), _EMPTY, dtype=torch.int64, device=dev))
    best = keys.min(dim=1).values if k > 0 else torch.full((Q,), _EMPTY, dtype=torch.int64, device=dev)
    inf = torch.full((Q,), float("inf"), dtype=torch.float32, device=dev)
    length = torch.where(best == _EMPTY, inf, (best >> 32).to(torch.int32).view(torch.float32))
    routed = length < inf                                                            # (an inf or NaN sum is no route)
    last = torch.where(routed, torch.gather(gi, 1, (best & 0xFFFFFFFF).clamp(max=max(k - 1, 0))[:, None])[:, 0], torch.full_like(best, -1))
    # the walks, goal side first: chain[h, q] is the node h hops before the goal link's, -1 past the walk's end
    chain = []
    cur = last
    while bool((cur >= 0).any()):
        if len(chain) >= N:                                                          # a walk that has not ended after N nodes
            routed = routed & (cur < 0)
            break
        chain.append(cur)
        cur = torch.where(cur >= 0, pred[cur.clamp(min=0), qq].to(torch.int64), cur)
    chain = torch.stack(chain) if chain else torch.zeros((0, Q), dtype=torch.int64, device=dev)
    return length, routed, chain


def host_mark_routes(rowptr, col, eid, ends, edge_state, nodes, dist, pred, mode, goal_idx, goal_len, capacity):
    """dcx_sssp_mark_routes' contract (include/dcx.h, "lazy roadmap queries") in plain torch ops on the tensors' own device: the
    still unknown edges (edge_state [M] uint8 == 0) on the routes the state (dist, pred [N, Q]) of host_sssp holds for the
    mode-2 queries, found as host_extract_paths finds them.  A hop (v, u = pred[v][q]) is the first entry of row v whose col
    is u, its edge eid[entry]; a hop without an entry or with an edge id outside 0 .. M - 1 is skipped.
    Returns (pending [Q] int32: the unknown edges on query q's route; list [capacity] int32; qa, qb [capacity, dof] in the
    nodes' dtype; n_out [2] int32 = (total, n = min(total, capacity))): list[:n] holds the n smallest marked edge ids in
    ascending order, qa[:n] = nodes[ends[list[:n], 0]] and qb[:n] = nodes[ends[list[:n], 1]], the rest zeros."""
    nodes = torch.as_tensor(nodes)
    dev = nodes.device
    N, dof = nodes.shape
    Q, M, nnz, capacity = len(goal_idx), len(edge_state), len(col), int(capacity)
    if capacity < 0:
        raise ValueError("host_mark_routes: capacity must be >= 0")
    mode = torch.as_tensor(mode).to(device=dev, dtype=torch.int64)
    _, routed, chain = _walk_routes(N, dist, pred, mode, goal_idx, goal_len)
    mark = torch.zeros(M, dtype=torch.bool, device=dev)
    pending = torch.zeros(Q, dtype=torch.int32, device=dev)
    if len(chain) > 1 and nnz and M:
        on = (chain[1:] >= 0) & routed[None, :]
        h, q = on.nonzero(as_tuple=True)
        v, u = chain[:-1][h, q], chain[1:][h, q]
        rp = rowptr.to(torch.int64)
        beg, end = rp[v].clamp(min=0), rp[v + 1].clamp(max=nnz)
        D = int((end - beg).max()) if len(v) else 0
        if D > 0:
            slot = torch.arange(D, device=dev)[None, :]
            at = beg[:, None] + slot                                                 # [hops, D]
            match = (at < end[:, None]) & (col.to(torch.int64)[at.clamp(max=nnz - 1)] == u[:, None])
            first = torch.where(match, slot, torch.full_like(at, D)).min(dim=1).values
            m = eid.to(torch.int64)[(beg + first).clamp(max=nnz - 1)]
            unknown = (first < D) & (m >= 0) & (m < M)
            unknown &= edge_state[m.clamp(0, M - 1)] == 0
            mark[m[unknown]] = True
            pending.index_add_(0, q[unknown], torch.ones_like(q[unknown], dtype=torch.int32))
    ids = mark.nonzero().reshape(-1)
    total = len(ids)
    n = min(total, capacity)
    lst = torch.zeros(capacity, dtype=torch.int32, device=dev)
    qa, qb = torch.zeros((capacity, dof), dtype=nodes.dtype, device=dev), torch.zeros((capacity, dof), dtype=nodes.dtype, device=dev)
    lst[:n] = ids[:n].to(torch.int32)
    e = ends.to(torch.int64)[ids[:n]]
    qa[:n], qb[:n] = nodes[e[:, 0]], nodes[e[:, 1]]
    return pending, lst, qa, qb, torch.tensor([total, n], dtype=torch.int32, device=dev)


def host_apply_checks(weight, ent, edge_state, lst, n_out, hit):
    """dcx_graph_apply_checks' contract in plain torch ops, IN PLACE on weight [nnz] float32 and edge_state [M] uint8: for
    i < n_out[1] the state of edge lst[i] becomes 2 where hit[i] else 1, and both CSR entries ent[lst[i]] of an edge that hit
    get the weight +inf.  Returns any_blocked int32 [1]."""
    n = int(n_out[1])
    ids = lst[:n].to(torch.int64)
    hit = torch.as_tensor(hit).to(device=ids.device).reshape(-1)[:n] != 0
    edge_state[ids] = torch.where(hit, 2, 1).to(torch.uint8)
    weight[ent.to(torch.int64)[ids[hit]].reshape(-1)] = float("inf")
    return hit.any().to(torch.int32).reshape(1)


class RoadmapPaths:
    """What Roadmap.query_batch returns: path [Q, W, dof], count [Q] int32 (n where query q's n waypoints are in path[q, :n],
    0 where there is no route, -n where n > W), length [Q] float32 (+inf without a route), mode [Q] int32 (0 an endpoint
    collides, 1 the direct motion is free, 2 over the roadmap), rounds (relaxation rounds run, round 0 included) and route
    ('fused' or 'host').  `path, count` go into shortcut_paths as they are.
    A lazy roadmap's loop adds settled [Q] bool (false only where `max_iters` cut the loop while the query's route still stood on
    unchecked edges: such a query has count 0 and length +inf), iters (relax-and-mark passes, the largest of the query chunks')
    and checked (edges handed to the checker, over all chunks); an eager roadmap reports all-true, 1 and 0."""

    def __init__(self, path, count, length, mode, rounds, route, settled=None, iters=1, checked=0):
        self.path, self.count, self.length, self.mode, self.rounds, self.route = path, count, length, mode, rounds, route
        self.settled = torch.ones(len(count), dtype=torch.bool, device=count.device) if settled is None else settled
        self.iters, self.checked = iters, checked

    def paths(self):
        """a list with, per query, its waypoints [n, dof] or None"""
        return [self.path[q, :n] if n > 0 else None for q, n in enumerate(self.count.tolist())]


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
    [M, 2] int64 (i < j, into `nodes`), lengths [M], graph (symmetric scipy.sparse.csr_matrix of the lengths).
    `build(..., lazy=True)` checks no edge: `edges` are then ALL the k-nearest candidates, in knn_edges' order (ascending
    i * n + j: the position is the edge id), `edge_state` [M] uint8 on the nodes' device says what is known of each (0 unknown,
    1 free, 2 blocked) and `lazy` is True.  `query_batch` checks the edges its shortest routes use and no others, and what it
    learns stays: states persist across calls.  `validate` checks whatever is still unknown, `invalidate` forgets (the call
    after the checker's model changed).  `graph` is the candidate graph at build time and is NOT kept up to date."""

    def __init__(self, checker, nodes, kept, edges, lengths, k, max_step, mask, check_kw, lazy=False):
        from scipy.sparse import csr_matrix
        self.checker = checker if isinstance(checker, _Checker) else _Checker(checker)
        self.nodes, self.kept, self.edges, self.lengths = nodes, kept, edges, lengths
        self.k, self.max_step, self.wrap_mask, self.check_kw = k, max_step, mask, dict(check_kw)
        n = len(nodes)
        e = edges.cpu().numpy()
        w = lengths.detach().cpu().numpy().astype(np.float64)
        self.graph = csr_matrix((np.concatenate([w, w]), (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))),
                                shape=(n, n))
        self._csr = None
        self.lazy = bool(lazy)
        if self.lazy:
            self.edge_state = torch.zeros(len(edges), dtype=torch.uint8, device=nodes.device)
            self._lazy = None

    @classmethod
    def build(cls, checker, nodes, k, max_step, wrap=None, max_dist=None, lazy=False, **check_kw):
        ck = _Checker(checker)
        nodes = torch.as_tensor(nodes).detach()
        mask = _ops.wrap_mask(wrap, nodes.shape[1], ck.transform)
        kept = (~ck.collides(nodes)).to(nodes.device).nonzero().reshape(-1)
        nodes = nodes[kept]
        cand = knn_edges(nodes, k, wrap=mask, max_dist=max_dist)
        qa, qb = nodes[cand[:, 0]], nodes[cand[:, 1]]
        if lazy:
            return cls(ck, nodes, kept, cand, _ops.wrapped_delta(qa, qb, mask).norm(dim=1), int(k), max_step, mask, check_kw, lazy=True)
        free = ~ck.motions(qa, qb, max_step, mask, **check_kw)
        edges = cand[free]
        lengths = _ops.wrapped_delta(qa[free], qb[free], mask).norm(dim=1)
        return cls(ck, nodes, kept, edges, lengths, int(k), max_step, mask, check_kw)

    def nearest(self, q):
        """(idx [Q], dist2 [Q]) of the kept node nearest to each q [Q, dof] (an RRT's query)"""
        q = torch.as_tensor(q).reshape(-1, self.nodes.shape[1])
        idx, d2 = knn(q, self.nodes, 1, wrap=self.wrap_mask)
        return idx[:, 0], d2[:, 0]

    def csr(self):
        """(rowptr int32 [n + 1], col int32 [nnz], weight float32 [nnz]) on the nodes' device: the roadmap as the symmetric CSR
        dcx_sssp_run reads (every edge in both rows, each row sorted by col).  Built once from `edges` and `lengths`.
        On a lazy roadmap `weight` is a buffer the roadmap changes: an entry holds its edge's length while the edge is unknown
        or free and +inf once it is blocked."""
        if self._csr is None:
            n, dev = len(self.nodes), self.nodes.device
            e = self.edges.to(dev)
            w = self.lengths.detach().to(device=dev, dtype=torch.float32)
            i, j = torch.cat([e[:, 0], e[:, 1]]), torch.cat([e[:, 1], e[:, 0]])
            order = torch.sort(i * max(n, 1) + j).indices      # (i, j) pairs are distinct: no tie to break
            rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            rowptr[1:] = torch.cumsum(torch.bincount(i, minlength=n), dim=0)
            self._csr = (rowptr.to(torch.int32), j[order].to(torch.int32).contiguous(), torch.cat([w, w])[order].contiguous())
            if self.lazy:
                # entry p of the unsorted list belongs to edge p % M: p < M in row i, else in row j
                M = len(e)
                inv = torch.empty_like(order)
                inv[order] = torch.arange(2 * M, device=dev)
                self._lazy = ((order % max(M, 1)).to(torch.int32).contiguous(), torch.stack([inv[:M], inv[M:]], dim=1).to(torch.int32).contiguous(),
                              e.to(torch.int32).contiguous())
        return self._csr

    def lazy_arrays(self):
        """(eid int32 [nnz]: CSR entry -> edge id; ent int32 [M, 2]: edge id -> its two CSR entries; ends int32 [M, 2]; edge_state):
        what dcx_sssp_mark_routes and dcx_graph_apply_checks read beside csr() (include/dcx.h, "lazy roadmap queries")"""
        if not self.lazy:
            raise ValueError("lazy_arrays: the roadmap was built with lazy=False")
        self.csr()
        return self._lazy + (self.edge_state,)

    def validate(self):
        """checks every still unknown edge in one check_motions call: afterwards the roadmap holds exactly the information of
        one built with lazy=False.  Returns the number of edges checked."""
        _, _, weight = self.csr()
        _, ent, _, state = self.lazy_arrays()
        ids = (state == 0).nonzero().reshape(-1)
        hit = self.checker.motions(self.nodes[self.edges[ids, 0]], self.nodes[self.edges[ids, 1]], self.max_step, self.wrap_mask, **self.check_kw)
        host_apply_checks(weight, ent, state, ids, (len(ids), len(ids)), hit)
        return len(ids)

    def invalidate(self, edge_ids=None):
        """sets the given edges (default: all) back to unknown and their weights back to their lengths: the call after the
        checker changed (`checker.update(...)`).  The nodes' validity is NOT asked again: an edge check samples its endpoints,
        so the edges of a node that now collides fall one by one as routes try them."""
        _, _, weight = self.csr()
        _, ent, _, state = self.lazy_arrays()
        ids = torch.arange(len(state), device=state.device) if edge_ids is None else torch.as_tensor(edge_ids, device=state.device).to(torch.int64).reshape(-1)
        state[ids] = 0
        w = self.lengths.detach().to(device=weight.device, dtype=torch.float32)[ids]
        e = ent.to(torch.int64)[ids]
        weight[e[:, 0]], weight[e[:, 1]] = w, w

    STATE_BUDGET = 1 << 28   # bytes of relaxation state query_batch holds at a time: 12 bytes per (node, query)

    def query_batch(self, starts, goals, k=None, rounds_per_call=8, max_rounds=None, max_waypoints=None, route=None, max_iters=None,
                    check_capacity=None):
        """`query` for Q start/goal pairs at once, as a RoadmapPaths: the shortest routes over the roadmap in one
        [Q, W, dof] tensor that goes into shortcut_paths as it is.  The checker is called three times whatever Q is (the 2Q
        endpoints, the Q direct motions, the 2Qk links to each endpoint's k nearest nodes); the shortest paths are the fixed
        point of synchronous min-plus relaxation in float32 (include/dcx.h, "roadmap queries"), so a length is the float32 sum
        of its route's segments in path order, where `query` sums in float64.
        Device tensors take the fused calls (_ops.sssp_run in chunks of `rounds_per_call` rounds, one flag slice read back
        per chunk, until a round changes nothing or `max_rounds`, default the number of nodes, have run; then
        _ops.sssp_extract_paths), CPU tensors host_sssp and host_extract_paths; `route` ('fused' / 'host') forces one.
        `max_waypoints`: W; None sizes it by the longest route (one more number read back).  The queries are taken in chunks
        of Q such that the relaxation state (two float32 distance buffers and an int32 predecessor per node and query) stays
        within STATE_BUDGET = 256 MiB.
        On a lazy roadmap each chunk of queries loops: relax from round 0 to the fixed point over the current weights; mark the
        still unknown edges of the routes found (_ops.sssp_mark_routes / host_mark_routes; their number is the one value read
        back per pass, 0 ends the loop); check the first `check_capacity` (default: all M) of them, in edge-id order, in one
        check_motions call; write the verdicts into the graph (_ops.graph_apply_checks / host_apply_checks), +inf for a blocked
        edge.  The relaxation starts over each time, since distances only grow when edges go.  Every pass that marks anything
        settles at least one edge, so the loop ends within M passes; `max_iters` cuts it earlier, and a query whose route still
        stands on unknown edges then is reported unsettled, without a path.  The routes are those of the eager roadmap, bit
        for bit, for the edges checked on the way; the states stay with the roadmap."""
        nodes, mask = self.nodes, self.wrap_mask
        dev, dof, n = nodes.device, nodes.shape[1], len(nodes)
        starts = torch.as_tensor(starts).reshape(-1, dof).to(device=dev, dtype=nodes.dtype)
        goals = torch.as_tensor(goals).reshape(-1, dof).to(device=dev, dtype=nodes.dtype)
        Q = len(starts)
        if len(goals) != Q:
            raise ValueError(f"query_batch: {Q} starts and {len(goals)} goals")
        if route is None:
            route = "fused" if dev.type == "cuda" else "host"
        if route not in ("fused", "host") or (route == "fused" and dev.type != "cuda"):
            raise ValueError("query_batch: route is 'fused' (a roadmap on a GPU) or 'host'")
        kk = min(int(self.k if k is None else k), 64)
        if kk < 1 or int(rounds_per_call) < 1:
            raise ValueError("query_batch: k and rounds_per_call must be >= 1")
        # 1, 2: the endpoints and the direct motions
        ends = torch.cat([starts, goals])
        if Q:
            hit = self.checker.collides(ends).to(dev)
            bad = hit[:Q] | hit[Q:]
        else:
            bad = torch.zeros(0, dtype=torch.bool, device=dev)
        blocked = self.checker.motions(starts, goals, self.max_step, mask, **self.check_kw)
        direct_len = _ops.wrapped_delta(starts, goals, mask).norm(dim=1).to(torch.float32)
        two = torch.full((Q,), 2, dtype=torch.int32, device=dev)
        mode = torch.where(bad, torch.zeros_like(two), torch.where(blocked, two, torch.ones_like(two)))
        # 3: every endpoint's links to its k nearest nodes, one fixed-shape batch (an unfilled slot checks a node against itself)
        if Q and n:
            idx, _ = knn(ends, nodes, kk, wrap=mask)
            qa = ends.repeat_interleave(kk, dim=0)
            qb = nodes[idx.to(torch.int64).clamp(min=0).reshape(-1)]
            free = ~self.checker.motions(qa, qb, self.max_step, mask, **self.check_kw).reshape(2 * Q, kk)
            link_idx = torch.where(free & (idx >= 0), idx, torch.full_like(idx, -1))
            link_len = _ops.wrapped_delta(qa, qb, mask).norm(dim=1).to(torch.float32).reshape(2 * Q, kk)
        else:
            link_idx = torch.full((2 * Q, kk), -1, dtype=torch.int32, device=dev)
            link_len = torch.zeros((2 * Q, kk), dtype=torch.float32, device=dev)
        # (only the queries that go over the roadmap keep their start links: the others would only hold the rounds up)
        start_idx = torch.where((mode == 2)[:, None], link_idx[:Q], torch.full_like(link_idx[:Q], -1)).contiguous()
        start_len, goal_idx, goal_len = link_len[:Q].contiguous(), link_idx[Q:].contiguous(), link_len[Q:].contiguous()
        # 4, 5: relaxation and extraction, a chunk of queries at a time
        rowptr, col, weight = self.csr()
        cap = max(1, int(n if max_rounds is None else max_rounds))
        rpc = int(rounds_per_call)
        qchunk = max(1, self.STATE_BUDGET // (12 * max(n, 1)))
        qchunk -= qchunk % 64 if qchunk >= 64 else 0
        fused = route == "fused"
        if max_iters is not None and int(max_iters) < 1:
            raise ValueError("query_batch: max_iters must be >= 1")
        lazy = self.lazy and len(self.edges) > 0
        settled, iters, checked = torch.ones(Q, dtype=torch.bool, device=dev), 1, 0
        if lazy:
            M = len(self.edges)
            eid, ent, ends_, state = self.lazy_arrays()
            capn = M if check_capacity is None else min(int(check_capacity), M)
            if capn < 1:
                raise ValueError("query_batch: check_capacity must be >= 1")
            if fused:
                lz = (eid, ent, ends_, state)
                # (list, qa, qb, n_out): written by every mark pass, read by the checker and the apply call
                mark_out = (torch.zeros(capn, dtype=torch.int32, device=dev), torch.zeros((capn, dof), device=dev),
                            torch.zeros((capn, dof), device=dev), torch.zeros(2, dtype=torch.int32, device=dev))
                hitbuf = torch.zeros(capn, dtype=torch.uint8, device=dev)
                flag = torch.zeros(1, dtype=torch.int32, device=dev)
        if fused:
            nodes32, starts32, goals32 = (t.to(torch.float32).contiguous() for t in (nodes, starts, goals))
        W = None if max_waypoints is None else int(max_waypoints)
        parts, rounds = [], 0
        for q0 in range(0, Q, qchunk):
            s = slice(q0, q0 + qchunk)
            Qc = len(mode[s])
            mode_c, it = mode[s], 0
            if fused:
                dist = torch.empty((2, n, Qc), dtype=torch.float32, device=dev)
                pred = torch.empty((n, Qc), dtype=torch.int32, device=dev)
                pending = torch.zeros(Qc, dtype=torch.int32, device=dev)
                while True:
                    done, took = 0, None
                    while done < cap and took is None:
                        m = min(rpc, cap - done)
                        flags = _ops.sssp_run(rowptr, col, weight, start_idx[s], start_len[s], dist, pred, done, m).tolist()
                        if 0 in flags:
                            took = done + flags.index(0) + 1
                        done += m
                    it += 1
                    if not lazy:
                        break
                    _, lst, ea, eb, n_out = _ops.sssp_mark_routes(rowptr, col, weight, lz, nodes32, dist, pred, done, mode_c, goal_idx[s],
                                                                  goal_len[s], capn, out=(pending,) + mark_out)
                    total, nn = n_out.tolist()
                    if total == 0:
                        break
                    if nodes.dtype != torch.float32:   # (the checker sees the nodes' own bits, as an eager build's does)
                        ids = lst[:nn].to(torch.int64)
                        ea, eb = nodes[self.edges[ids, 0]], nodes[self.edges[ids, 1]]
                    hitbuf[:nn] = self.checker.motions(ea[:nn], eb[:nn], self.max_step, mask, **self.check_kw)
                    _ops.graph_apply_checks(rowptr, col, weight, lz, lst, n_out, hitbuf, any_blocked=flag)
                    checked += nn
                    if max_iters is not None and it >= int(max_iters):
                        settled[s] = pending == 0
                        mode_c = torch.where(pending == 0, mode_c, torch.zeros_like(mode_c))
                        break
                args = (rowptr, col, weight, nodes32, dist, pred, done, mode_c, starts32[s], goals32[s], goal_idx[s], goal_len[s],
                        direct_len[s])
                Wc = W
                if Wc is None:
                    Wc = max(-int(_ops.sssp_extract_paths(*args, 0)[1].min()), 2)
                part = _ops.sssp_extract_paths(*args, Wc)
            else:
                while True:
                    d, p, flags = host_sssp(rowptr, col, weight, start_idx[s], start_len[s], rounds=cap)
                    flags = flags.tolist()
                    took = flags.index(0) + 1 if 0 in flags else None
                    it += 1
                    if not lazy:
                        break
                    pending, lst, ea, eb, n_out = host_mark_routes(rowptr, col, eid, ends_, state, nodes, d, p, mode_c, goal_idx[s],
                                                                   goal_len[s], capn)
                    total, nn = n_out.tolist()
                    if total == 0:
                        break
                    hit = self.checker.motions(ea[:nn], eb[:nn], self.max_step, mask, **self.check_kw)
                    host_apply_checks(weight, ent, state, lst, n_out, hit)
                    checked += nn
                    if max_iters is not None and it >= int(max_iters):
                        settled[s] = pending == 0
                        mode_c = torch.where(pending == 0, mode_c, torch.zeros_like(mode_c))
                        break
                part = host_extract_paths(nodes, d, p, mode_c, starts[s], goals[s], goal_idx[s], goal_len[s], direct_len[s], W)
            rounds = max(rounds, cap if took is None else took)
            iters = max(iters, it)
            parts.append(part)
        if len(parts) == 1:
            path, count, length = parts[0]
        else:
            Wmax = max([p[0].shape[1] for p in parts] + [2 if W is None else W])
            path = torch.zeros((Q, Wmax, dof), dtype=torch.float32 if fused else nodes.dtype, device=dev)
            q0 = 0
            for p in parts:
                path[q0:q0 + len(p[0]), :p[0].shape[1]] = p[0]
                q0 += len(p[0])
            count = torch.cat([p[1] for p in parts]) if parts else torch.zeros(0, dtype=torch.int32, device=dev)
            length = torch.cat([p[2] for p in parts]) if parts else torch.zeros(0, dtype=torch.float32, device=dev)
        return RoadmapPaths(path, count, length, mode, rounds, route, settled, iters, checked)

    def query(self, start, goal, k=None):
        """(waypoints [W, dof], length) of the shortest route start -> goal over the roadmap, or None where an endpoint
        collides or no route exists.  A free direct motion is returned as the two-point path.  On a lazy roadmap this is
        `query_batch` with one pair (its float32 relaxation, its lazy checks), the waypoints in the dtype query_batch returns."""
        if self.lazy:
            res = self.query_batch(torch.as_tensor(start).reshape(1, -1), torch.as_tensor(goal).reshape(1, -1), k=k)
            n = int(res.count[0])
            return (res.path[0, :n], float(res.length[0])) if n > 0 else None
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
