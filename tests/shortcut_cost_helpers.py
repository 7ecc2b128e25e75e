"""What the tests of the shortcuts under the clearance objective share (include/dcx.h, "Path shortcuts under the clearance
objective"): the events of a round read off host_shortcut_paths' record, the contract's sums restated in numpy float32, and the
provenance of seg - every entry the price of a fresh motion_worst on the segment it stands for."""
import numpy as np
import torch

from rrtstar_cost_helpers import cost32
from rrtstar_helpers import F, bits, length32

EVENTS = ("applied", "blocked", "dearer", "lost", "idle", "two")


class Record:
    """host_shortcut_paths' _record under the objective: the rounds' masks and prices, and the events they show.
    applied; blocked: live but a piece is not free; dearer: free but not gainful; lost: gainful but not applied (it crosses an
    earlier slot of its round, or the path has no room); idle; two: two slots applied to one path in one round."""

    def __init__(self):
        self.rounds, self.seen = [], dict.fromkeys(EVENTS, 0)

    def __call__(self, live, w, free, applied, info):
        g = info["gainful"]
        self.rounds.append(dict(live=live.clone(), w=w.clone(), free=free.clone(), applied=applied.clone(),
                                **{k: v.clone() for k, v in info.items()}))
        self.seen["applied"] += int(applied.sum())
        self.seen["blocked"] += int((live & ~free).sum())
        self.seen["dearer"] += int((free & ~g).sum())
        self.seen["lost"] += int((g & ~applied).sum())
        self.seen["idle"] += int((~live).sum())
        self.seen["two"] += int((applied.sum(dim=1) >= 2).sum())

    def assert_coverage(self, slots):
        for what in EVENTS:
            if slots == 1 and what in ("lost", "two"):   # a round of one slot has no earlier slot to lose to
                continue
            assert self.seen[what] >= 1, (what, self.seen)


def span32(seg, a, b):
    """seg[a] + ... + seg[b] in numpy float32, ascending from seg[a]"""
    old = F(seg[a])
    for k in range(a + 1, b + 1):
        old = F(old + F(seg[k]))
    return old


def path_cost32(seg, n):
    """the serial float32 sum of seg[:n - 1] from +0"""
    c = F(0)
    for k in range(max(n - 1, 0)):
        c = F(c + F(seg[k]))
    return c


def fresh_seg(worst_fn, path, n, gain, band, wrap_len=None):
    """the price of a fresh sweep of the n - 1 consecutive segments of path [n, dof] (numpy): C where free, +inf where not.
    worst_fn(qa, qb) -> worst [n - 1] numpy float32; wrap_len(a, b): the length of a -> b (default: no wrap mask)"""
    if n < 2:
        return np.zeros(0, F)
    w = np.asarray(worst_fn(path[:n - 1], path[1:n]), F)
    ln = wrap_len or length32
    out = np.array([cost32(ln(path[k], path[k + 1]), w[k], gain, band) for k in range(n - 1)], F)
    return np.where(w <= 0, out, F(np.inf)).astype(F)


def assert_provenance(worst_fn, path, count, seg, gain, band, wrap_len=None):
    """seg[r, :count[r] - 1] equals the price of a fresh motion_worst on the current consecutive waypoints, bit for bit"""
    path, count, seg = path.cpu().numpy(), count.cpu().numpy(), seg.cpu().numpy()
    for r, n in enumerate(count.tolist()):
        want = fresh_seg(worst_fn, path[r], n, gain, band, wrap_len)
        assert bits(seg[r, :max(n - 1, 0)]).tolist() == bits(want).tolist(), (r, n, seg[r, :max(n - 1, 0)], want)


def assert_same_state(a, b):
    """two ShortcutResults under the objective agree bit for bit on path[:count], count, accepted and seg[:count - 1]"""
    assert a.count.tolist() == b.count.tolist()
    assert a.accepted.tolist() == b.accepted.tolist()
    for r, n in enumerate(a.count.tolist()):
        assert torch.equal(a.path[r, :n].cpu().view(torch.int32), b.path[r, :n].cpu().view(torch.int32)), r
        m = max(n - 1, 0)
        assert torch.equal(a.seg[r, :m].cpu().view(torch.int32), b.seg[r, :m].cpu().view(torch.int32)), r
    assert torch.equal(a.costs.view(torch.int32), b.costs.view(torch.int32))
