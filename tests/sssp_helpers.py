"""The referee of the roadmap queries (include/dcx.h, "roadmap queries") in numpy float32, written with plain loops over the
nodes, the rows' entries and the slots - the queries alone are taken as a vector, every operation on them rounded alone - and
a heap Dijkstra that accumulates in float32; the graphs and the query sets the CPU and GPU tests share."""
import functools
import heapq

import numpy as np

F = np.float32
INF = F(np.inf)


# ------------------------------------------------------------------------------------------------ graphs
def csr_of(n, edges):
    """the symmetric CSR (rowptr int32 [n + 1], col int32, weight float32) of undirected edges {(i, j): w}, rows sorted by col"""
    adj = [[] for _ in range(n)]
    for (i, j), w in edges.items():
        assert i != j and (j, i) not in edges
        adj[i].append((j, F(w)))
        adj[j].append((i, F(w)))
    rowptr, col, weight = [0], [], []
    for v in range(n):
        for j, w in sorted(adj[v]):
            col.append(j)
            weight.append(w)
        rowptr.append(len(col))
    return np.array(rowptr, np.int32), np.array(col, np.int32), np.array(weight, F)


def _knn_edges(x, k, keep=1.0, rng=None):
    d = ((x[:, None].astype(np.float64) - x[None]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    e = {}
    for i in range(len(x)):
        for j in np.argsort(d[i], kind="stable")[:k]:
            key = (min(i, int(j)), max(i, int(j)))
            if key not in e and (rng is None or rng.random() < keep):
                e[key] = F(np.sqrt(d[i, j]))
    return e


def _chain(n=40):
    rng = np.random.default_rng(1)
    return n, {(i, i + 1): F(0.5 + rng.random()) for i in range(n - 1)}


def _grid(m=12):
    e = {}
    for r in range(m):
        for c in range(m):
            if c + 1 < m:
                e[(r * m + c, r * m + c + 1)] = F(1.0)
            if r + 1 < m:
                e[(r * m + c, (r + 1) * m + c)] = F(1.0)
    return m * m, e


def _hub():
    """node 0 has degree 100, nodes 1 .. 100 a ring of their own, nodes 101 .. 129 no edge at all (empty rows)"""
    rng = np.random.default_rng(2)
    e = {(0, j): F(0.2 + rng.random()) for j in range(1, 101)}
    e.update({(j, j + 1): F(0.05 + 0.1 * rng.random()) for j in range(1, 100)})
    return 130, e


def _two_components():
    rng = np.random.default_rng(3)
    x = rng.random((70, 2)).astype(F)
    e = _knn_edges(x[:40], 4)
    e.update({(40 + i, 40 + j): w for (i, j), w in _knn_edges(x[40:], 4).items()})
    return 70, e


def _duplicates(n=300):
    """a kNN graph with a quarter of its nodes duplicated: zero-length edges"""
    rng = np.random.default_rng(4)
    x = rng.random((n, 2)).astype(F)
    dup = rng.choice(n, n // 4, replace=False)
    x[dup] = x[rng.integers(0, n, len(dup))]
    e = _knn_edges(x, 6, keep=0.9, rng=rng)
    assert sum(1 for w in e.values() if w == 0) > 10
    return n, e


def _extremes():
    """weights of 3e7 beside 1e-3 (the small ones are absorbed by rounding), and +inf edges that nothing may adopt"""
    rng = np.random.default_rng(5)
    x = rng.random((70, 3)).astype(F)
    e = _knn_edges(x, 5)
    for n_, key in enumerate(sorted(e)):
        e[key] = (F(3e7), F(1e-3), INF, e[key])[n_ % 7 if n_ % 7 < 3 else 3]
    assert sum(1 for w in e.values() if np.isinf(w)) > 3
    return 70, e


def _knn300():
    rng = np.random.default_rng(6)
    return 300, _knn_edges(rng.random((300, 2)).astype(F), 6)


_GRAPHS = {
    "single": lambda: (1, {}),
    "pair": lambda: (2, {(0, 1): F(0.75)}),
    "chain40": _chain,
    "grid12": _grid,
    "hub": _hub,
    "two_components": _two_components,
    "duplicates300": _duplicates,
    "extremes70": _extremes,
    "knn300": _knn300,
}
GRAPHS = tuple(_GRAPHS)


@functools.lru_cache(maxsize=None)
def graph(name):
    """(n, rowptr, col, weight) of a named graph"""
    n, e = _GRAPHS[name]()
    return (n,) + csr_of(n, e)


def queries(name, Q, k=4, dof=3, seed=0, all_modes=True):
    """a query set on a named graph: start and goal links [Q, k] (distinct nodes per query, some slots -1), mode, starts,
    goals, direct_len, nodes [n, dof] - all numpy, float32 / int32"""
    n = graph(name)[0]
    rng = np.random.default_rng(1000 + seed + 17 * Q)
    out = {}
    for side in ("start", "goal"):
        idx = np.full((Q, k), -1, np.int32)
        for q in range(Q):
            m = min(n, k)
            idx[q, :m] = rng.choice(n, m, replace=False)
            idx[q, rng.random(k) < 0.25] = -1
        out[side + "_idx"] = idx
        out[side + "_len"] = (0.05 + 0.1 * rng.random((Q, k))).astype(F)
    if name == "chain40":          # one source at the chain's end: the rounds are the hops
        out["start_idx"][:] = -1
        out["start_idx"][:, 0] = 0
        out["goal_idx"][:, 0] = n - 1
    mode = np.full(Q, 2, np.int32)
    if all_modes:
        mode[rng.random(Q) < 0.15] = 0
        mode[rng.random(Q) < 0.15] = 1
        if Q >= 3:
            mode[:3] = (2, 0, 1)
    out["mode"] = mode
    out["nodes"] = rng.random((n, dof)).astype(F)
    out["starts"] = rng.random((Q, dof)).astype(F) - F(2)
    out["goals"] = rng.random((Q, dof)).astype(F) + F(2)
    out["direct_len"] = rng.random(Q).astype(F)
    return out


# ------------------------------------------------------------------------------------------------ the referee
def sssp_ref(rowptr, col, weight, link_idx, link_len, rounds):
    """(dist [N, Q], pred [N, Q], changed [rounds]) after `rounds` Jacobi rounds, round 0 (the links) included; rounds=None:
    up to and including the first round that changes nothing"""
    N, (Q, k) = len(rowptr) - 1, link_idx.shape
    dist = np.full((N, Q), INF, F)
    pred = np.full((N, Q), -1, np.int32)
    until_quiet = rounds is None
    rounds = N + 2 if until_quiet else rounds
    changed = np.zeros(rounds, np.int32)
    if rounds == 0:
        return dist, pred, changed
    for q in range(Q):
        for s in range(k):
            v = int(link_idx[q, s])
            if 0 <= v < N:
                dist[v, q] = link_len[q, s]
                changed[0] = 1
    for t in range(1, rounds):
        if until_quiet and changed[t - 1] == 0:
            return dist, pred, changed[:t]
        new = dist.copy()
        for v in range(N):
            best = np.full(Q, INF, F)
            bu = np.full(Q, -1, np.int32)
            for e in range(rowptr[v], rowptr[v + 1]):
                u = int(col[e])
                c = dist[u] + weight[e]                  # float32 + float32: one rounded add per query
                first = c < best                         # strict: an earlier entry keeps a tie; inf and NaN never win
                best = np.where(first, c, best)
                bu = np.where(first, np.int32(u), bu)
            win = best < dist[v]
            new[v] = np.where(win, best, dist[v])
            pred[v] = np.where(win, bu, pred[v])
            if win.any():
                changed[t] = 1
        dist = new
    return dist, pred, changed


def extract_ref(nodes, dist, pred, mode, starts, goals, goal_idx, goal_len, direct_len, W, path=None):
    """(path [Q, W, dof], count [Q], length [Q]); `path`: the rows as they stand before the call (zeros by default)"""
    N, dof = nodes.shape
    Q, k = goal_idx.shape
    path = np.zeros((Q, W, dof), F) if path is None else path.copy()
    count = np.zeros(Q, np.int32)
    length = np.full(Q, INF, F)
    for q in range(Q):
        if mode[q] == 1:
            length[q] = direct_len[q]
            count[q] = 2 if W >= 2 else -2
            if W >= 2:
                path[q, 0], path[q, 1] = starts[q], goals[q]
            continue
        if mode[q] != 2:
            continue
        best, last = INF, -1
        for s in range(k):
            v = int(goal_idx[q, s])
            if not 0 <= v < N:
                continue
            c = F(dist[v, q] + goal_len[q, s])
            if c < best:
                best, last = c, v
        if last < 0:
            continue
        walk, i = [], last
        while i != -1 and len(walk) <= N:
            walk.append(i)
            i = int(pred[i, q])
        if len(walk) > N:
            continue
        n = len(walk) + 2
        length[q] = best
        if n > W:
            count[q] = -n
            continue
        count[q] = n
        path[q, 0], path[q, n - 1] = starts[q], goals[q]
        for h, v in enumerate(walk):
            path[q, n - 2 - h] = nodes[v]
    return path, count, length


def dijkstra32(rowptr, col, weight, sources):
    """[N] float32: a textbook heap Dijkstra from sources = [(node, length)] that accumulates in float32 from the start"""
    N = len(rowptr) - 1
    d = np.full(N, INF, F)
    heap = []
    for v, w in sources:
        if F(w) < d[v]:
            d[v] = F(w)
            heapq.heappush(heap, (float(w), v))
    while heap:
        x, v = heapq.heappop(heap)
        if x > d[v]:
            continue
        for e in range(rowptr[v], rowptr[v + 1]):
            c = F(d[v] + weight[e])
            if c < d[col[e]]:
                d[col[e]] = c
                heapq.heappush(heap, (float(c), int(col[e])))
    return d


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint32) if a.dtype == F else a, b.view(np.uint32) if b.dtype == F else b)


@functools.lru_cache(maxsize=None)
def case(name, Q, all_modes=True):
    """a graph, a query set and the referee's answers at the fixed point: shared by the tests, never changed"""
    n, rowptr, col, weight = graph(name)
    qs = queries(name, Q, all_modes=all_modes)
    dist, pred, changed = sssp_ref(rowptr, col, weight, qs["start_idx"], qs["start_len"], None)
    rounds = len(changed)
    assert changed[-1] == 0 and rounds <= n + 1
    sizes = extract_ref(qs["nodes"], dist, pred, qs["mode"], qs["starts"], qs["goals"], qs["goal_idx"], qs["goal_len"],
                        qs["direct_len"], 0)
    W = max(int(-sizes[1].min()), 2)
    path, count, length = extract_ref(qs["nodes"], dist, pred, qs["mode"], qs["starts"], qs["goals"], qs["goal_idx"],
                                      qs["goal_len"], qs["direct_len"], W)
    return dict(qs, n=n, rowptr=rowptr, col=col, weight=weight, rounds=rounds, dist=dist, pred=pred, changed=changed, W=W,
                sizes=sizes[1], path=path, count=count, length=length)
