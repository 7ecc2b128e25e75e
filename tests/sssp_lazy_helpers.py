"""The referee of the lazy roadmap queries (include/dcx.h, "lazy roadmap queries") in numpy, written with plain loops over the
queries, the hops of a walk, a row's entries and the edges, on the graphs and query sets of sssp_helpers; a verdict that needs
no model (edge m is blocked iff ((m * 2654435761) >> 7) % 4 == 0); and whole relax - mark - check - apply loops on it."""
import functools

import numpy as np

from sssp_helpers import F, INF, extract_ref, graph, queries, sssp_ref

LAZY_GRAPHS = ("pair", "chain40", "grid12", "hub", "two_components", "duplicates300", "knn300")


def blocked(m):
    """the deterministic verdict of edge m (python ints: the product does not wrap)"""
    return ((int(m) * 2654435761) >> 7) % 4 == 0


def verdicts(ids):
    return np.array([blocked(m) for m in ids], np.uint8)


@functools.lru_cache(maxsize=None)
def lazy_graph(name):
    """a named graph with its edges numbered in ascending (i, j), i < j: eid [nnz], ent [M, 2], ends [M, 2] (int32), lengths [M]"""
    n, rowptr, col, weight = graph(name)
    ends, lengths, index = [], [], {}
    for v in range(n):
        for e in range(rowptr[v], rowptr[v + 1]):
            if col[e] > v:                               # rows are sorted by col: (v, col) ascends
                index[(v, int(col[e]))] = len(ends)
                ends.append((v, int(col[e])))
                lengths.append(weight[e])
    M = len(ends)
    eid = np.zeros(len(col), np.int32)
    ent = np.full((M, 2), -1, np.int32)
    for v in range(n):
        for e in range(rowptr[v], rowptr[v + 1]):
            u = int(col[e])
            m = index[(min(v, u), max(v, u))]
            eid[e] = m
            ent[m, 0 if v < u else 1] = e
    assert (ent >= 0).all() and 2 * M == len(col)
    return dict(n=n, rowptr=rowptr, col=col, weight=weight, M=M, eid=eid, ent=ent, ends=np.array(ends, np.int32).reshape(M, 2),
                lengths=np.array(lengths, F))


def mark_ref(g, state, nodes, dist, pred, mode, goal_idx, goal_len, capacity, before=None):
    """(pending [Q], list [capacity], qa, qb [capacity, dof], n_out [2]); `before`: (list, qa, qb) as they stand before the call
    (zeros by default): the entries from n_out[1] on stay as they are"""
    N, M = g["n"], g["M"]
    rowptr, col, eid = g["rowptr"], g["col"], g["eid"]
    Q, k = goal_idx.shape
    dof = nodes.shape[1]
    mark = np.zeros(M, np.uint8)
    pending = np.zeros(Q, np.int32)
    for q in range(Q):
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
        while i != -1 and len(walk) < N and 0 <= i < N:
            walk.append(i)
            i = int(pred[i, q])
        if i != -1:                                      # the walk did not end within N nodes, or left 0 .. N - 1
            continue
        for v, u in zip(walk, walk[1:]):
            for e in range(max(int(rowptr[v]), 0), min(int(rowptr[v + 1]), len(col))):
                if col[e] == u:
                    m = int(eid[e])
                    if 0 <= m < M and state[m] == 0:
                        mark[m] = 1
                        pending[q] += 1
                    break
    ids = [m for m in range(M) if mark[m]]
    total, n = len(ids), min(len(ids), capacity)
    if before is None:
        lst, qa, qb = np.zeros(capacity, np.int32), np.zeros((capacity, dof), F), np.zeros((capacity, dof), F)
    else:
        lst, qa, qb = (x.copy() for x in before)
    for i in range(n):
        lst[i] = ids[i]
        qa[i], qb[i] = nodes[g["ends"][ids[i], 0]], nodes[g["ends"][ids[i], 1]]
    return pending, lst, qa, qb, np.array([total, n], np.int32)


def apply_ref(g, weight, state, lst, n_out, hit):
    """(weight, state, any_blocked [1]) after the verdicts hit[i] of the edges lst[i], i < n_out[1]"""
    weight, state = weight.copy(), state.copy()
    any_blocked = np.zeros(1, np.int32)
    for i in range(int(n_out[1])):
        m = int(lst[i])
        state[m] = 2 if hit[i] else 1
        if hit[i]:
            weight[g["ent"][m, 0]] = weight[g["ent"][m, 1]] = INF
            any_blocked[0] = 1
    return weight, state, any_blocked


def loop_case(name, Q, all_modes=False, capacity=None, max_iters=None):
    """shared by the tests, never changed: see _loop_case"""
    return _loop_case(name, Q, all_modes, capacity, max_iters)


@functools.lru_cache(maxsize=None)
def _loop_case(name, Q, all_modes, capacity, max_iters):
    """a whole relax - mark - check - apply loop of the referee from all-unknown edges under the verdict rule: the final weight
    and state, iters, checked, settled, the routes at the end (path, count, length, W) and every pass's (pending, list, n_out)"""
    g = lazy_graph(name)
    qs = queries(name, Q, all_modes=all_modes)
    cap = g["M"] if capacity is None else capacity
    weight, state = g["weight"].copy(), np.zeros(g["M"], np.uint8)
    passes, checked = [], 0
    settled = np.ones(Q, bool)
    mode = qs["mode"]
    while True:
        dist, pred, changed = sssp_ref(g["rowptr"], g["col"], weight, qs["start_idx"], qs["start_len"], None)
        pending, lst, qa, qb, n_out = mark_ref(g, state, qs["nodes"], dist, pred, qs["mode"], qs["goal_idx"], qs["goal_len"], cap)
        passes.append((pending, lst, n_out))
        if n_out[0] == 0:
            break
        weight, state, _ = apply_ref(g, weight, state, lst, n_out, verdicts(lst[:n_out[1]]))
        checked += int(n_out[1])
        if max_iters is not None and len(passes) >= max_iters:
            settled = pending == 0
            mode = np.where(settled, mode, 0).astype(np.int32)
            break
    ex = (qs["nodes"], dist, pred, mode, qs["starts"], qs["goals"], qs["goal_idx"], qs["goal_len"], qs["direct_len"])
    W = max(int(-extract_ref(*ex, 0)[1].min()), 2)
    path, count, length = extract_ref(*ex, W)
    return dict(qs, g=g, weight=weight, state=state, iters=len(passes), checked=checked, settled=settled, passes=passes, dist=dist,
                pred=pred, rounds=len(changed), W=W, path=path, count=count, length=length, blocked=int((state == 2).sum()))
