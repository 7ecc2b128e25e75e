"""What the tests of RRT* under clearance-weighted edge costs share (include/dcx.h, "batched RRT*: clearance-weighted edge
costs"): rrtstar_helpers' discs with a score field, case S under the objective traced through the referee host_rrt_star, and the
invariants of a state with the edges' costs restated in numpy float32."""
import functools

import numpy as np
import torch

from rrtstar_helpers import F, GOALS_S, S, STARTS_S, Discs, bits, fixed, kwargs_s, length32, samples_s

# case S under the objective: the samples' seed, the gain and the band were chosen on the CPU against the referee's own trace so
# that it shows every event test_rrtstar_cost_host.py asks for.  The discs' score is a signed distance (radius - distance), so a
# band of 0.15 charges every motion that passes within 0.15 of a disc
SEED_C = 30
GAIN_C = 4.0
BAND_C = 0.15
EVENTS = ("penalised", "pruned_after", "rewire_rejected_after", "chose_other", "rewires", "lowered_descendants")


class SoftDiscs(Discs):
    """Discs with a score: max over the discs of (radius - distance), positive inside one.  motion_worst samples an edge on
    check_motions' own fp64 restatement of the closed max_step rule, edge by edge: an edge's answer does not depend on the batch
    it travels in.  A point collides where its float32 score is positive, so both calls give one verdict."""

    def score(self, p):
        d = np.sqrt(((p[:, None, :] - self.discs[None, :, :2]) ** 2).sum(axis=2))
        return (self.discs[None, :, 2] - d).max(axis=1).astype(F)

    def hit(self, p):
        return self.score(p) > 0

    def motion_worst(self, qa, qb, max_step=None, wrap=None, max_samples=None):
        assert wrap is None
        qa, qb = np.asarray(qa, np.float64), np.asarray(qb, np.float64)
        self.batches.append(len(qa))
        worst, idx = np.zeros(len(qa), F), np.zeros(len(qa), np.int32)
        for e, (a, b) in enumerate(zip(qa, qb)):
            L = float(np.linalg.norm(b - a))
            n = int(np.ceil(L / max_step))
            assert n + 1 <= max_samples
            pts = np.concatenate([a[None] + (np.arange(n)[:, None] * max_step / L) * (b - a)[None] if n else np.zeros((0, 2)), b[None]])
            s = self.score(pts)
            idx[e] = int(s.argmax())
            worst[e] = s[idx[e]]
        return torch.from_numpy(worst), torch.from_numpy(idx), torch.zeros(len(qa), dtype=torch.int32)


def cost32(L, w, gain, band):
    """C = L * (1 + gain * max(w + band, 0)) in numpy float32, one rounded operation at a time"""
    pen = np.maximum(F(F(w) + F(band)), F(0))
    return F(F(L) * F(F(1) + F(F(gain) * pen)))


def kwargs_c(**over):
    kw = kwargs_s(objective="clearance", clearance_gain=GAIN_C, clearance_band=BAND_C)
    kw.update(over)
    return kw


@functools.lru_cache(maxsize=None)
def traced_c(gain=GAIN_C, band=BAND_C, seed=SEED_C, submit_all=False):
    """(result, trace, checker) of the referee on case S under the objective"""
    from diffco_amd.rrtstar import host_rrt_star
    ck, trace = SoftDiscs(), []
    res = host_rrt_star(ck, STARTS_S, GOALS_S, sampler=fixed(samples_s(seed)), _trace=trace, _submit_all=submit_all,
                        **kwargs_c(clearance_gain=gain, clearance_band=band))
    return res, trace, ck


def check_state_cost(st, prev, checker, max_step, gain, band):
    """rrtstar_helpers.check_state under the objective: the parent graph is a tree on count nodes rooted at node 0; every tree
    edge is free (its peak w <= 0 under `checker` in the direction parent -> child) and elen[i] holds
    fl(L * fl(1 + fl(gain * pen))) of that edge recomputed here from the checker's worst; cost[i] == fl32(cost[parent[i]] +
    elen[i]); no cost rose since `prev` and no node moved; rows past count are as initialised"""
    nodes, parent, elen, cost, count = (st[k].cpu().numpy() for k in ("nodes", "parent", "elen", "cost", "count"))
    for r in range(len(count)):
        n = int(count[r])
        assert n >= 1 and parent[r, 0] == -1 and bits(cost[r, 0]) == 0 and bits(elen[r, 0]) == 0
        if n > 1:
            w = checker.motion_worst(torch.from_numpy(nodes[r, parent[r, 1:n]]), torch.from_numpy(nodes[r, 1:n]), max_step=max_step,
                                     max_samples=1 << 20)[0].numpy()
            assert (w <= 0).all(), r
        for i in range(1, n):
            p = int(parent[r, i])
            assert 0 <= p < n and p != i, (r, i, p)
            L = length32(nodes[r, p], nodes[r, i])
            assert bits(elen[r, i]) == bits(cost32(L, w[i - 1], gain, band)), (r, i)
            assert elen[r, i] >= L
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
