"""What the tests of RRT*'s device-side sampling share: hand-made states that mix running, direct, blocked, solved and unsolved
problems with a chosen best cost each, the informed set's bound restated in float64 under the torus metric, and the comparison
of a draw (the kernel's, or the planner's recorded one) with the referee rrtstar.host_device_samples in the two senses of the
contract: bit for bit where it is float32 one operation at a time, to the project's parity bar where it is float64."""
import math

import numpy as np
import torch

BAXTER_MASK = (1 << 4) | (1 << 6)
GOAL_BIAS = 0.25
TRIES = 8


def box(dof, half=math.pi):
    return torch.tensor([[-half, half]] * dof, dtype=torch.float32)


def wrapped(d, mask):
    """the float64 delta d with the masked coordinates along the shortest arc"""
    on = torch.tensor([bool((mask >> j) & 1) for j in range(d.shape[-1])])
    return torch.where(on, torch.remainder(d + math.pi, 2 * math.pi) - math.pi, d)


def dist64(a, b, mask):
    return wrapped(b.to(torch.float64) - a.to(torch.float64), mask).norm(dim=-1)


UNSOLVED, DIRECT, BLOCKED, SOLVED = 0, 1, 2, 3


def kinds(R):
    """[R]: what make_state makes of problem r, by r % 6 (three problems already hold an unsolved, a solved and a direct one)"""
    return torch.tensor([UNSOLVED, SOLVED, DIRECT, SOLVED, BLOCKED, SOLVED])[torch.arange(R) % 6]


def make_state(R, dof, mask=0, cap=8, seed=0, limits=None):
    """(state, goals, limits) on the CPU.  Problem r by kinds(R): running without a goal node; the direct motion is free
    (status 1, goal node 1); an endpoint collides (status 3); running with a goal node whose cost runs from c_min (the first
    of them, exactly) to 2 c_min over the problems.  The last solved problem sits in a corner of the limits (with c = 2 c_min
    where it is not also the first): its ellipsoid pokes out of them."""
    g = torch.Generator().manual_seed(seed)
    lim = box(dof) if limits is None else limits
    lo, span = lim[:, 0], lim[:, 1] - lim[:, 0]
    starts = lo + span * (0.25 + 0.5 * torch.rand(R, dof, generator=g))
    goals = lo + span * (0.25 + 0.5 * torch.rand(R, dof, generator=g))
    kind = kinds(R)
    solved = torch.nonzero(kind == SOLVED).reshape(-1)
    if len(solved):   # the corner problem
        r = int(solved[-1])
        starts[r] = lo + span * 0.02
        goals[r] = lo + span * 0.10
    st = dict(nodes=torch.zeros(R, cap, dof), parent=torch.full((R, cap), -1, dtype=torch.int32), elen=torch.zeros(R, cap),
              cost=torch.zeros(R, cap), count=torch.ones(R, dtype=torch.int32), status=torch.zeros(R, dtype=torch.int32),
              goal_node=torch.full((R,), -1, dtype=torch.int32), first_round=torch.full((R,), -1, dtype=torch.int32))
    st["nodes"][:, 0] = starts
    st["status"][kind == DIRECT] = 1
    st["goal_node"][kind == DIRECT] = 1
    st["status"][kind == BLOCKED] = 3
    from diffco_amd import _ops
    from diffco_amd.rrt import _length
    cmin = _length(_ops.wrapped_delta(starts, goals, mask))
    for n, r in enumerate(solved.tolist()):
        frac = n / max(len(solved) - 1, 1)   # 0 .. 1; the first is c_min itself, the last (the corner) 2 c_min
        node = 2 + r % (cap - 2)
        st["goal_node"][r] = node
        st["cost"][r, node] = cmin[r] * torch.tensor(1.0 + frac, dtype=torch.float32)
        st["count"][r] = node + 1
    st["cost"][kind == DIRECT, 1] = cmin[kind == DIRECT]
    return st, goals.contiguous(), lim.contiguous()


def best_cost(st):
    """[R] float64: the goal nodes' cost, nan without one"""
    gn = st["goal_node"].cpu().to(torch.int64)
    c = st["cost"].cpu().gather(1, gn.clamp(min=0)[:, None])[:, 0].to(torch.float64)
    return torch.where(gn >= 0, c, torch.full_like(c, float("nan")))


def assert_in_informed_set(samples, info, st, goals, mask, tries=TRIES):
    """every accepted informed sample x (info 2 .. 1 + tries; a fallback is a uniform point) of a problem with best cost c:
    d(start, x) + d(x, goal) <= c (1 + 1e-5) in float64 under the torus metric.  Returns how many there were."""
    samples, info = samples.cpu(), info.cpu()
    start, goals, c = st["nodes"].cpu()[:, 0][:, None, :], goals.cpu()[:, None, :], best_cost(st)[:, None]
    total = dist64(start, samples, mask) + dist64(samples, goals, mask)
    sel = (info >= 2) & (info < 2 + tries)
    assert bool((total[sel] <= (c.expand_as(total)[sel]) * (1 + 1e-5)).all()), float((total / c)[sel].max())
    return int(sel.sum())


def tolerance(st, goals, mask):
    """[R] float64: 1e-5 * max(1, c / 2 + max |centre|), the parity bar against the float64 referee at the draw's own scale"""
    start = st["nodes"].cpu()[:, 0].to(torch.float64)
    centre = start + wrapped(goals.cpu().to(torch.float64) - start, mask) / 2
    c = torch.nan_to_num(best_cost(st), nan=0.0)
    return 1e-5 * torch.clamp(c / 2 + centre.abs().max(dim=1).values, min=1.0)


def assert_matches_referee(samples, info, st, goals, limits, seed, g, mode, mask, uniform_mix=0., goal_bias=GOAL_BIAS, tries=TRIES):
    """a draw against host_device_samples on the same state.  Rows that are not informed (not running, goal, uniform): the
    referee's bits, and its info word.  Informed rows: the draw names its try t (or the fallback); the sample equals the
    referee's float64 candidate of try t within tolerance() under the wrapped difference (a fallback: the referee's uniform
    point, bit for bit); every earlier candidate lies outside the limits in float64 or within the tolerance of a bound.
    Returns info's counts {word: n}."""
    from diffco_amd.rrtstar import host_device_samples
    R, P, dof = samples.shape
    want, winfo, cand = host_device_samples(st, goals, limits, seed, g, P, mode, goal_bias, uniform_mix, tries, mask)
    uni = host_device_samples(st, goals, limits, seed, g, P, "uniform", 0.0, uniform_mix, tries, mask)[0]   # step 2's point of every slot
    samples, info = samples.cpu(), info.cpu()
    plain = winfo < 2
    assert torch.equal(info < 2, plain), "which rows are informed depends on float32 comparisons alone"
    assert torch.equal(info[plain], winfo[plain])
    assert torch.equal(samples[plain].view(torch.int32), want[plain].view(torch.int32))
    tol = tolerance(st, goals, mask)[:, None].expand(R, P)
    lo, hi = limits.cpu()[:, 0].to(torch.float64), limits.cpu()[:, 1].to(torch.float64)
    for r, p in torch.nonzero(~plain).tolist():
        t = int(info[r, p]) - 2
        assert 0 <= t <= tries
        if t == tries:
            assert torch.equal(samples[r, p].view(torch.int32), uni[r, p].view(torch.int32)), (r, p)
        else:
            err = wrapped(samples[r, p].to(torch.float64) - cand[t, r, p], mask).abs().max()
            assert float(err) <= float(tol[r, p]), (r, p, t, float(err), float(tol[r, p]))
            assert bool(((lo <= samples[r, p]) & (samples[r, p] < hi)).all()), (r, p)
        for e in range(t):   # an earlier try was refused: outside in float64, or within the tolerance of a bound
            x = cand[e, r, p]
            assert bool(((x < lo + tol[r, p]) | (x >= hi - tol[r, p])).any()), (r, p, e)
    return {int(k): int(n) for k, n in zip(*np.unique(info.numpy(), return_counts=True))}
