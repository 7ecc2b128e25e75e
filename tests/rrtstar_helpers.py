"""What the RRT* tests share: a deterministic CPU checker of discs in the plane, fixed samplers with goal rows, case S (four
problems: a blocked endpoint, a free direct motion, one that fills its tree, one hard), the traced run of the referee
host_rrt_star with its invariants restated in numpy float32, and - for the GPU tests - the planar DiffCo, a ScoreModel as a
checker and a recorder of the batches a planner submits."""
import functools

import numpy as np
import torch

F = np.float32
STATE = ("nodes", "parent", "elen", "cost", "count", "status", "goal_node", "first_round")
LIMITS = [[-1.0, 1.0], [-1.0, 1.0]]
# case S: range, radius ~ 2 range, the stride, P, K, the rounds and the cap that the third problem fills
S = dict(R=4, P=4, K=8, range=0.25, radius=0.5, max_step=0.05, rounds=24, cap=64, chunk=4)
SEED_S = 30   # chosen on the CPU so that the referee's own trace shows every event test_rrtstar_host.py asks for


class Discs:
    """collides inside any of the discs (cx, cy, radius).  check_motions samples an edge on its own fp64 restatement of the
    closed max_step rule - the planner only ever sees its verdicts."""

    def __init__(self, discs=((0.0, 0.0, 0.4), (0.0, 0.8, 0.15), (0.0, -0.55, 0.12))):
        self.discs, self.batches = np.asarray(discs, np.float64), []

    def hit(self, p):
        return (((p[:, None, :] - self.discs[None, :, :2]) ** 2).sum(axis=2) < self.discs[None, :, 2] ** 2).any(axis=1)

    def check_motions(self, qa, qb, max_step=None, wrap=None, max_samples=None, return_first=False):
        assert wrap is None and return_first
        qa, qb = np.asarray(qa, np.float64), np.asarray(qb, np.float64)
        self.batches.append(len(qa))
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


def fixed(samples):
    """a sampler that hands out the rows of `samples` in order, whatever the chunking"""
    at = [0]

    def sampler(T, R, P):
        out = samples[at[0]:at[0] + T]
        at[0] += T
        return out
    return sampler


def with_goal_rows(samples, goals, every=3):
    """`samples` [T, R, P, dof] with the last slot of every `every`-th round replaced by the problem's goal row, bit for bit"""
    samples = samples.clone()
    samples[::every, :, -1, :] = goals[None].to(samples)
    return samples


# ---- case S on the CPU -------------------------------------------------------------------------------------------------------
STARTS_S = torch.tensor([[0.1, 0.1], [-0.9, -0.9], [-0.9, 0.8], [-0.8, 0.0]])   # (the first lies inside the large disc)
GOALS_S = torch.tensor([[0.9, 0.9], [0.9, -0.9], [0.9, 0.8], [0.8, 0.05]])


def samples_s(seed=SEED_S):
    """fixed samples of case S: uniform in the square, goal rows every third round; the hard problem spends its last slot on its
    own start (a zero-length extension: an idle slot) outside the goal rounds and its third slot always, so that its tree cannot
    fill"""
    rng = np.random.default_rng(seed)
    smp = torch.from_numpy(rng.uniform(-1, 1, (S["rounds"], S["R"], S["P"], 2)).astype(F))
    smp[:, 3, 2:, :] = STARTS_S[3]
    return with_goal_rows(smp, GOALS_S)


def kwargs_s(**over):
    kw = dict(range=S["range"], max_step=S["max_step"], radius=S["radius"], near=S["K"], slots=S["P"], cap=S["cap"],
              max_rounds=S["rounds"], rounds_per_call=S["chunk"], limits=LIMITS)
    kw.update(over)
    return kw


@functools.lru_cache(maxsize=None)
def traced_s(near=S["K"], seed=SEED_S):
    """(result, trace, checker) of the referee on case S: trace[g] holds the round's events and the state after it"""
    from diffco_amd.rrtstar import host_rrt_star
    ck, trace = Discs(), []
    res = host_rrt_star(ck, STARTS_S, GOALS_S, sampler=fixed(samples_s(seed)), _trace=trace, **kwargs_s(near=near))
    return res, trace, ck


# ---- the invariants of a state, numpy float32 one operation at a time --------------------------------------------------------
def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def length32(a, b):
    """the motion calls' length of the directed edge a -> b without a wrap mask"""
    l2 = F(0)
    for j in range(len(a)):
        d = F(b[j] - a[j])
        l2 = F(l2 + F(d * d))
    return F(np.sqrt(l2))


def check_state(st, prev=None, checker=None, max_step=None):
    """the parent graph is a tree on count nodes rooted at node 0; elen[i] holds the length bits of the directed edge
    parent -> i (d = node_i - node_parent: the motion calls' L of a chosen parent's edge and sqrt(dist2) of a rewirer's edge are
    that same expression); cost[i] == fl32(cost[parent[i]] + elen[i]); no cost rose since `prev`; every tree edge is free under
    `checker` in its checked direction parent -> child; rows past count are as initialised"""
    nodes, parent, elen, cost, count = (st[k].cpu().numpy() for k in ("nodes", "parent", "elen", "cost", "count"))
    for r in range(len(count)):
        n = int(count[r])
        assert n >= 1 and parent[r, 0] == -1 and bits(cost[r, 0]) == 0 and bits(elen[r, 0]) == 0
        for i in range(1, n):
            p = int(parent[r, i])
            assert 0 <= p < n and p != i, (r, i, p)
            assert bits(elen[r, i]) == bits(length32(nodes[r, p], nodes[r, i])), (r, i)
            assert bits(cost[r, i]) == bits(F(cost[r, p] + elen[r, i])), (r, i)
            hops, j = 0, i
            while j != 0:
                j, hops = int(parent[r, j]), hops + 1
                assert hops < n, (r, i, "no path to the root")
        assert (parent[r, n:] == -1).all() and (nodes[r, n:] == 0).all() and (cost[r, n:] == 0).all() and (elen[r, n:] == 0).all()
        if prev is not None:
            m = int(prev["count"][r])
            assert m <= n and (cost[r, :m] <= prev["cost"][r, :m].cpu().numpy()).all(), r
            assert (bits(nodes[r, :m]) == bits(prev["nodes"][r, :m].cpu().numpy())).all(), r
        if checker is not None and n > 1:
            qa = torch.from_numpy(nodes[r, parent[r, 1:n]])
            qb = torch.from_numpy(nodes[r, 1:n])
            assert not bool(checker.check_motions(qa, qb, max_step=max_step, max_samples=1 << 20, return_first=True)[0].any()), r


def host_walk(st, r):
    """the path root .. goal node of problem r walked from `parent` in plain Python, None without a goal node"""
    i = int(st["goal_node"][r])
    if i < 0:
        return None
    parent, walk = st["parent"].cpu(), []
    while i >= 0:
        walk.append(i)
        i = int(parent[r, i])
    return st["nodes"][r][torch.tensor(walk[::-1], device=st["nodes"].device)]


def assert_same_state(a, b):
    for name in STATE:
        x, y = getattr(a, name) if not isinstance(a, dict) else a[name], getattr(b, name) if not isinstance(b, dict) else b[name]
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), (name, int((x != y).sum()))


# ---- for the GPU tests -------------------------------------------------------------------------------------------------------
class Recorder:
    """a checker's check_motions with every batch's size kept: what the planner asked"""

    def __init__(self, checker):
        self.checker, self.sizes = checker, []

    def check_motions(self, qa, qb, **kw):
        self.sizes.append(len(qa))
        return self.checker.check_motions(qa, qb, **kw)


class ModelChecker:
    """a ScoreModel with per-class margins as a checker: check_motions for the host planner, _rrt_model for the fused one"""

    def __init__(self, model, margin):
        self.model, self.margin = model, margin

    def check_motions(self, qa, qb, max_step=None, wrap=None, max_samples=None, return_first=False):
        first, _ = self.model.check_motions(qa, qb, max_step=max_step, margin=self.margin, max_samples=max_samples, wrap=wrap)
        return first >= 0, first

    def _rrt_model(self, device=None):
        return self.model, self.margin


def far_refused_pairs(check, nodes, n, seed=0):
    """of 40 sampled nodes, the n farthest pairs whose direct motion `check` refuses"""
    pick = torch.as_tensor(np.random.default_rng(seed).choice(len(nodes), 40, replace=False), device=nodes.device)
    a, b = torch.triu_indices(40, 40, 1, device=nodes.device)
    hit = torch.as_tensor(check(nodes[pick[a]], nodes[pick[b]])).to(nodes.device)
    dist = (nodes[pick[a]] - nodes[pick[b]]).norm(dim=1)
    assert int(hit.sum()) >= n
    order = torch.argsort(dist * hit, descending=True)[:n].tolist()
    return [(int(pick[a[i]]), int(pick[b[i]])) for i in order]


def near_accepted_pair(check, nodes, seed=0):
    """of 40 sampled nodes, the nearest pair whose direct motion `check` accepts"""
    pick = torch.as_tensor(np.random.default_rng(seed).choice(len(nodes), 40, replace=False), device=nodes.device)
    a, b = torch.triu_indices(40, 40, 1, device=nodes.device)
    hit = torch.as_tensor(check(nodes[pick[a]], nodes[pick[b]])).to(nodes.device)
    dist = (nodes[pick[a]] - nodes[pick[b]]).norm(dim=1)
    i = int(torch.where(hit, torch.full_like(dist, float("inf")), dist).argmin())
    assert not bool(hit[i])
    return int(pick[a[i]]), int(pick[b[i]])


def planar_checker():
    """the DiffCo of the 2-DoF planar arm fixture, both joints on the circle: (fixture, checker, robot)"""
    from diffco_amd import _lib, kernel
    from diffco_amd.kernel_perceptrons import DiffCo
    from helpers import CASE_ROBOT, case_kernel, load, make_robot
    _lib.require_gpu()
    name = "cfg1_planar2_rq"
    d = load(name)
    kind, p0, p1 = case_kernel(d)
    rob = make_robot(CASE_ROBOT[name])
    dc = DiffCo(kernel_func=kernel.RQKernel(p0, p1), transform=rob.fkine)
    dc.support_points = torch.as_tensor(np.asarray(d["sup_q"]), dtype=torch.float32, device="cuda")
    dc.support_transformed = rob.fkine(dc.support_points)
    dc.gains = torch.as_tensor(np.asarray(d["weights"][:, 0]), dtype=torch.float32, device="cuda")
    return d, dc, rob
