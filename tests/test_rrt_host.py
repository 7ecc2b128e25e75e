"""host_rrt_connect (diffco_amd/rrt.py) on CPU tensors with a fake 2-D checker - a wall with a gap whose check_motions answers
with return_first - against a plain list-and-loop restatement of include/dcx.h's contract written here: equal nodes (bits),
parents, counts, status, link and solved_round; and the planner's outcomes (solved through the gap with free segments, full
without it, a colliding start, a free direct motion, chunking).  No GPU."""
import numpy as np
import pytest
import torch

from motion_band_helpers import listed_points32

F = np.float32
LIMITS = [[-1.0, 1.0], [-1.0, 1.0]]


class Wall:
    """collides inside |x| < 0.1 except where lo < y < hi (the gap; None: a solid wall).  check_motions samples an edge on its own
    fp64 restatement of the max_step rule - the planner only ever sees its verdicts."""

    def __init__(self, gap=(-0.25, 0.25)):
        self.gap, self.calls, self.batches = gap, 0, set()

    def hit(self, p):
        inside = np.abs(p[:, 0]) < 0.1
        if self.gap is not None:
            inside &= ~((p[:, 1] > self.gap[0]) & (p[:, 1] < self.gap[1]))
        return inside

    def check_motions(self, qa, qb, max_step=None, wrap=None, max_samples=None, return_first=False):
        assert wrap is None and return_first
        qa, qb = np.asarray(qa, np.float64), np.asarray(qb, np.float64)
        self.calls += 1
        self.batches.add(len(qa))
        first = np.full(len(qa), -1, np.int32)
        for e, (a, b) in enumerate(zip(qa, qb)):
            L = float(np.linalg.norm(b - a))
            n = int(np.ceil(L / max_step))
            assert n + 1 <= max_samples
            pts = np.concatenate([a[None] + (np.arange(n)[:, None] * max_step / L) * (b - a)[None] if n else np.zeros((0, 2)), b[None]])
            at = np.nonzero(self.hit(pts))[0]
            if len(at):
                first[e] = at[0]
        return torch.from_numpy(first >= 0), torch.from_numpy(first)


def _samples(seed, T, R, P):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1, 1, (T, R, P, 2)).astype(F))


def _fixed(samples):
    """a sampler that hands out the rows of `samples` in order, whatever the chunking"""
    at = [0]

    def sampler(T, R, P):
        out = samples[at[0]:at[0] + T]
        at[0] += T
        return out
    return sampler


# ---- the contract in lists and loops, numpy float32 one operation at a time --------------------------------------------------
def _dist2(q, node):
    l2 = F(0)
    for j in range(len(q)):
        d = F(node[j] - q[j])
        l2 = F(l2 + F(d * d))
    return l2


def _nearest(q, nodes):
    best = None
    for i, node in enumerate(nodes):
        l2 = _dist2(q, node)
        if np.isnan(l2):
            continue
        key = (int(np.float32(l2).view(np.uint32)) << 32) | i
        if best is None or key < best:
            best = key
    return -1 if best is None else best & 0xFFFFFFFF


def _steer(near, s, rng):
    d = [F(s[j] - near[j]) for j in range(len(s))]
    l2 = F(0)
    for v in d:
        l2 = F(l2 + F(v * v))
    L = F(np.sqrt(l2))
    if not L > 0:
        return None
    if L <= F(rng):
        return np.array(s, F)
    f = F(F(rng) / L)
    return np.array([F(near[j] + F(d[j] * f)) for j in range(len(s))], F)


def restated(checker, starts, goals, samples, rng, max_step, max_samples, P, cap):
    R = len(starts)
    trees = [[[np.array(starts[r], F)], [np.array(goals[r], F)]] for r in range(R)]
    parents = [[[-1], [-1]] for _ in range(R)]
    status, link, solved_round = [0] * R, [[-1, -1] for _ in range(R)], [-1] * R
    seen = dict(partial=0, rejected=0)

    def check(edges):   # the fixed batch: idle slots take the start node's zero-length edge
        qa = np.array([e[0] if e else trees[r][0][0] for r, row in enumerate(edges) for e in row], F)
        qb = np.array([e[1] if e else trees[r][0][0] for r, row in enumerate(edges) for e in row], F)
        first = checker.check_motions(torch.from_numpy(qa), torch.from_numpy(qb), max_step=max_step, wrap=None,
                                      max_samples=max_samples, return_first=True)[1].numpy().reshape(R, P)
        return qa.reshape(R, P, -1), qb.reshape(R, P, -1), first

    # the initial checks: one batch of the zero-length edges on starts and goals and the direct motions
    S, G = np.asarray(starts, F), np.asarray(goals, F)
    first = checker.check_motions(torch.from_numpy(np.concatenate([S, G, S])), torch.from_numpy(np.concatenate([S, G, G])),
                                  max_step=max_step, wrap=None, max_samples=max_samples, return_first=True)[1].numpy()
    for r in range(R):
        if first[r] != -1 or first[R + r] != -1:
            status[r] = 3
        elif first[2 * R + r] == -1:
            status[r], link[r] = 1, [0, 0]

    for g in range(len(samples)):
        a, b = g & 1, 1 - (g & 1)
        run = [st == 0 for st in status]
        snap = [[len(trees[r][0]), len(trees[r][1])] for r in range(R)]
        full = [False] * R
        edges, near = [[None] * P for _ in range(R)], [[-1] * P for _ in range(R)]
        for r in range(R):
            for p in range(P):
                if not run[r]:
                    continue
                s = samples[g][r][p]
                i = _nearest(s, trees[r][a][:snap[r][a]])
                qb = None if i < 0 else _steer(trees[r][a][i], s, rng)
                if qb is not None:
                    edges[r][p], near[r][p] = (trees[r][a][i], qb), i
        _, _, first = check(edges)
        added = [[-1] * P for _ in range(R)]
        for r in range(R):
            for p in range(P):
                seen["rejected"] += bool(edges[r][p]) and first[r][p] != -1
                if edges[r][p] and first[r][p] == -1:
                    if len(trees[r][a]) < cap:
                        added[r][p] = len(trees[r][a])
                        trees[r][a].append(edges[r][p][1])
                        parents[r][a].append(near[r][p])
                    else:
                        full[r] = True
        edges, nb = [[None] * P for _ in range(R)], [[-1] * P for _ in range(R)]
        for r in range(R):
            for p in range(P):
                if added[r][p] >= 0:
                    x = trees[r][a][added[r][p]]
                    i = _nearest(x, trees[r][b][:snap[r][b]])
                    if i >= 0:
                        edges[r][p], nb[r][p] = (trees[r][b][i], x), i
        qa, qb, first = check(edges)
        for r in range(R):
            joined = None
            for p in range(P):
                if not edges[r][p]:
                    continue
                h = first[r][p]
                if h == -1 and joined is None:
                    joined = p
                if h >= 2:
                    seen["partial"] += 1
                    if len(trees[r][b]) < cap:
                        trees[r][b].append(listed_points32(qa[r, p][None], qb[r, p][None], 0, [0], [h - 1], None, max_step)[0])
                        parents[r][b].append(nb[r][p])
                    else:
                        full[r] = True
            if joined is not None:
                status[r], solved_round[r] = 1, g
                link[r][a], link[r][b] = added[r][joined], nb[r][joined]
            elif run[r] and full[r]:
                status[r] = 2
    return trees, parents, status, link, solved_round, seen


def _assert_equal_state(res, ref, cap):
    trees, parents, status, link, solved_round, _ = ref
    assert res.status.tolist() == status and res.link.tolist() == link and res.solved_round.tolist() == solved_round
    assert res.count.tolist() == [[len(t[0]), len(t[1])] for t in trees]
    for r, t in enumerate(trees):
        for k in (0, 1):
            got = res.nodes[r, k, :len(t[k])].numpy()
            assert (got.view(np.uint32) == np.array(t[k], F).view(np.uint32)).all(), (r, k)
            assert res.parent[r, k, :len(t[k])].tolist() == parents[r][k]
            assert (res.parent[r, k, len(t[k]):] == -1).all() and (res.nodes[r, k, len(t[k]):] == 0).all()


KW = dict(range=0.4, max_step=0.05, limits=LIMITS, max_samples=64)
STARTS = [[-0.8, 0.7], [-0.6, -0.8], [-0.9, 0.6], [-0.5, 0.9]]
GOALS = [[0.8, 0.7], [0.7, -0.6], [0.9, 0.9], [0.6, 0.5]]     # every direct motion runs into the wall


def test_equals_the_restated_contract():
    from diffco_amd.rrt import host_rrt_connect
    T, R, P, cap = 24, 4, 3, 24
    samples = _samples(3, T, R, P)
    wall = Wall()
    res = host_rrt_connect(wall, torch.tensor(STARTS), torch.tensor(GOALS), slots=P, cap=cap, max_rounds=T, rounds_per_call=T,
                           sampler=_fixed(samples), **KW)
    assert res.route == "host" and wall.batches == {3 * R, R * P}       # the initial batch, then the fixed batch and nothing else
    ref = restated(Wall(), STARTS, GOALS, samples.numpy(), KW["range"], KW["max_step"], KW["max_samples"], P, cap)
    _assert_equal_state(res, ref, cap)
    # the case is not a trivial one: somebody got through, some tree took a partial advance, some edge was rejected
    assert 1 in ref[2] and max(ref[4]) > 0 and ref[5]["partial"] > 0 and ref[5]["rejected"] > 0, (ref[2], ref[4], ref[5])


def test_solves_through_the_gap_with_free_segments():
    from diffco_amd.rrt import host_rrt_connect
    wall = Wall()
    res = host_rrt_connect(wall, torch.tensor(STARTS), torch.tensor(GOALS), slots=4, cap=256, max_rounds=200, seed=1, **KW)
    assert res.status.tolist() == [1] * len(STARTS)
    for r, p in enumerate(res.paths):
        assert len(p) > 2 and torch.equal(p[0], torch.tensor(STARTS[r])) and torch.equal(p[-1], torch.tensor(GOALS[r]))
        hit, _ = wall.check_motions(p[:-1], p[1:], max_step=KW["max_step"], max_samples=10 ** 6, return_first=True)
        assert not bool(hit.any())
        assert np.isfinite(float(res.lengths[r])) and float(res.lengths[r]) >= float((p[-1] - p[0]).norm()) - 1e-5
        assert int(res.rounds[r]) == int(res.solved_round[r]) + 1
        # consecutive waypoints are parent-linked: tree 0 down from the link node, tree 1 up from its link node
        i, j = res.link[r].tolist()
        n0 = 1
        while int(res.parent[r, 0, i]) >= 0:
            i, n0 = int(res.parent[r, 0, i]), n0 + 1
        n1 = 1
        while int(res.parent[r, 1, j]) >= 0:
            j, n1 = int(res.parent[r, 1, j]), n1 + 1
        assert n0 + n1 == len(p)


def test_a_solid_wall_fills_the_trees_and_never_solves():
    from diffco_amd.rrt import host_rrt_connect
    res = host_rrt_connect(Wall(gap=None), torch.tensor(STARTS[:2]), torch.tensor(GOALS[:2]), slots=4, cap=12, max_rounds=100, seed=2, **KW)
    assert res.status.tolist() == [2, 2] and res.paths == [None, None]
    assert int(res.count.max()) == 12 and bool(torch.isnan(res.lengths).all())
    assert (res.link == -1).all() and (res.solved_round == -1).all()


def test_a_colliding_start_and_a_free_direct_motion():
    from diffco_amd.rrt import host_rrt_connect
    starts = torch.tensor([[0.05, 0.9], [-0.8, 0.1], [-0.8, 0.6]])
    goals = torch.tensor([[0.8, 0.0], [0.8, -0.1], [-0.3, -0.6]])
    res = host_rrt_connect(Wall(), starts, goals, slots=2, cap=16, max_rounds=0, **KW)
    assert res.status.tolist() == [3, 1, 1]
    assert res.paths[0] is None
    for r in (1, 2):
        assert torch.equal(res.paths[r], torch.stack([starts[r], goals[r]]))
        assert int(res.solved_round[r]) == -1 and res.link[r].tolist() == [0, 0] and int(res.rounds[r]) == 0
    assert res.count.tolist() == [[1, 1]] * 3
    # a blocked problem stays blocked, and idles, while the others' rounds run
    starts[1], goals[1] = torch.tensor(STARTS[0]), torch.tensor(GOALS[0])
    res = host_rrt_connect(Wall(), starts, goals, slots=2, cap=64, max_rounds=60, seed=5, **KW)
    assert res.status.tolist()[0] == 3 and res.status.tolist()[2] == 1 and res.count[0].tolist() == [1, 1]
    assert res.count[1].sum() > 2


def test_chunking_does_not_change_the_state():
    from diffco_amd.rrt import host_rrt_connect
    out = []
    for chunk in (1, 8):
        out.append(host_rrt_connect(Wall(), torch.tensor(STARTS), torch.tensor(GOALS), slots=3, cap=32, max_rounds=16,
                                    rounds_per_call=chunk, seed=7, **KW))
    a, b = out
    # (chunks of 8 run on after the last problem stopped; stopped problems idle, so the state is the same)
    for name in ("nodes", "parent", "count", "status", "link", "solved_round"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.status.tolist().count(0) < len(STARTS)


def test_rejects_bad_arguments():
    from diffco_amd.rrt import host_rrt_connect
    s, g = torch.tensor(STARTS), torch.tensor(GOALS)
    with pytest.raises(ValueError, match="slots"):
        host_rrt_connect(Wall(), s, g, slots=17, **KW)
    with pytest.raises(ValueError, match="range and max_step"):
        host_rrt_connect(Wall(), s, g, range=0.0, max_step=0.05, limits=LIMITS)
    with pytest.raises(ValueError, match="limits"):
        host_rrt_connect(Wall(), s, g, range=0.4, max_step=0.05)
