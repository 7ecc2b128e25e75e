"""CPU: the referee of the wrapped motion calls.  motion_wrap_helpers.motion_samples_wrapped restates include/dcx.h's rule
operation by operation in numpy float32; here it is held against utils.anglin (the res rule on the circle), against
helpers.motion_samples (mask 0: the same bits), against the sample counts the rule fixes on the planar arm, and the host routes
of the facades (plain torch, they run without a GPU) are held against it: points, counts and the chain through autograd.

The reference's own utils.anglin does not run under this numpy / torch (np.linspace is handed torch tensors and
torch.from_numpy refuses its result), so no fixture of it is pinned here: utils.anglin is its restatement."""
import numpy as np
import pytest
import torch

from helpers import motion_chain, motion_samples
from motion_wrap_helpers import PI, TWO_PI, motion_samples_wrapped, near_seam, seam_edges, wrap2pi32

F = np.float32


def _angles(seed, E, dof, lo=-np.pi, hi=np.pi):
    g = np.random.default_rng(seed)
    return g.uniform(lo, hi, (E, dof)).astype(F), g.uniform(lo, hi, (E, dof)).astype(F)


def test_wrap2pi32_is_pythons_modulo_in_fp32():
    g = np.random.default_rng(0)
    x = np.concatenate([g.uniform(-20, 20, 4000), [0.0, np.pi, -np.pi, 3 * np.pi, -3 * np.pi, 1e-8, -1e-8]]).astype(F)
    w = wrap2pi32(x)
    assert w.dtype == F
    # [-pi, pi) up to the rounding of the last subtraction, and the same point of the circle
    assert (w >= -PI).all() and (w <= PI).all()
    assert np.abs(np.sin(w.astype(np.float64)) - np.sin(x.astype(np.float64))).max() < 4e-6
    assert np.abs(np.cos(w.astype(np.float64)) - np.cos(x.astype(np.float64))).max() < 4e-6
    # what the rule pins: +pi goes to -pi, a negative full turn is exactly zero, values inside are left within an ulp of pi
    assert wrap2pi32(PI) == -PI and wrap2pi32(-PI) == -PI
    assert wrap2pi32(-TWO_PI) == 0 and wrap2pi32(F(0)) == 0
    inside = g.uniform(-3.0, 3.0, 1000).astype(F)
    assert np.abs(wrap2pi32(inside) - inside).max() <= 2 ** -22
    # torch's fp32 restatement (utils.wrap2pi) agrees on the circle
    from diffco_amd import utils
    t = utils.wrap2pi(torch.from_numpy(x)).numpy().astype(np.float64)
    assert np.abs(np.sin(t) - np.sin(w.astype(np.float64))).max() < 4e-6


def test_res_rule_is_anglin_without_endpoint():
    from diffco_amd import utils
    qa, qb = _angles(1, 200, 3)
    # across the seam both ways, a difference of exactly pi (it goes the negative way), no motion
    qa = np.concatenate([qa, [[3.0, -3.0, 0.0], [0.0, 1.0, -2.0], [0.5, 0.5, 0.5]]]).astype(F)
    qb = np.concatenate([qb, [[-3.0, 3.0, 0.0], [PI, F(F(1.0) + PI), F(F(-2.0) - PI)], [0.5, 0.5, 0.5]]]).astype(F)
    res = 13
    smp = motion_samples_wrapped(qa, qb, 0b111, res=res)
    for (p, t, u, tgt), a, b in zip(smp, qa, qb):
        assert p.shape == (res, 3) and p.dtype == F and u is None and not tgt.any()
        ref = utils.anglin(a, b, res, endpoint=False).numpy()
        assert ref.shape == p.shape
        # fp32 rounding of |x| <= 2 pi before the wrap (k / res, the product, the sum: <= 1.5 ulp of 4.8e-7) and of the two
        # wraps (<= 1 ulp of 2.4e-7 each); anglin interpolates in float64 from the same fp32 delta
        assert np.abs(np.sin(p.astype(np.float64)) - np.sin(ref)).max() < 3e-6
        assert np.abs(np.cos(p.astype(np.float64)) - np.cos(ref)).max() < 3e-6
    # the three seam edges take the short way: 0.28 rad, not 6 rad
    p = smp[200][0].astype(np.float64)
    assert np.abs(np.cos(p[:, 0])).min() > np.cos(0.2) - 1e-6 and np.abs(np.cos(p[:, 1])).min() > np.cos(0.2) - 1e-6
    # exactly pi: the negative way, as anglin's delta wrap2pi(pi) = -pi
    p = smp[201][0].astype(np.float64)
    assert (np.sin(p[1:, 0]) < 0).all() and (np.diff(np.unwrap(p[:, 1])) < 0).all()
    assert (smp[202][0] == F(0.5)).all()


@pytest.mark.parametrize("kw", [dict(res=13), dict(res=1), dict(max_step=0.21), dict(max_step=0.21, open_end=True)])
def test_mask_zero_is_helpers_motion_samples(kw):
    qa, qb = _angles(2, 60, 5, -4, 4)
    qb[:3] = qa[:3]   # zero-length edges
    got = motion_samples_wrapped(qa, qb, 0, **kw)
    ref = motion_samples(qa, qb, **kw)
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert g[0].dtype == r[0].dtype and g[0].shape == r[0].shape and (g[0] == r[0]).all()
        assert (g[1] == r[1]).all() and (g[3] == r[3]).all()
        assert (g[2] is None and r[2] is None) or (g[2] == r[2]).all()


def test_unmasked_coordinates_keep_the_plain_points():
    qa, qb = _angles(3, 40, 4, -4, 4)
    for kw in (dict(res=9), ):
        got = motion_samples_wrapped(qa, qb, 0b0101, **kw)
        ref = motion_samples(qa, qb, **kw)
        for g, r in zip(got, ref):
            assert (g[0][:, [1, 3]] == r[0][:, [1, 3]]).all()


# ---- the counts the rule fixes on the planar 2-DoF arm ----
_A = np.array([[3.0, 0.0]], F)
_B = np.array([[-3.0, 0.0]], F)


def test_counts_on_the_planar_arm():
    L = abs(float(wrap2pi32(F(-6.0))))
    assert abs(L - 0.2831853) < 1e-6
    assert int(np.ceil(L / 0.05)) + 1 == 7
    assert len(motion_samples_wrapped(_A, _B, 0b11, max_step=0.05)[0][0]) == 7
    assert len(motion_samples_wrapped(_A, _B, 0b11, max_step=0.05, open_end=True)[0][0]) == 6
    assert len(motion_samples_wrapped(_A, _B, 0, max_step=0.05)[0][0]) == 121
    assert len(motion_samples(_A, _B, max_step=0.05)[0][0]) == 121
    # the seven samples run 3.0 -> pi -> -3.0 the short way (sample 0 is wrap2pi(qa): an ulp from qa), the target qb as given
    p = motion_samples_wrapped(_A, _B, 0b11, max_step=0.05)[0][0]
    assert (np.abs(p[:, 0]) >= 3.0 - 1e-6).all() and abs(p[0, 0] - F(3.0)) <= 2 ** -22 and p[-1, 0] == F(-3.0) and (p[:, 1] == 0).all()
    assert (p[:3, 0] > 0).all() and (p[3:, 0] < 0).all()


def test_a_full_turn_has_length_zero():
    """L = 0 after wrapping: one sample qb, none with open_end.  In fp32 the turn that wraps to exactly zero is the negative one:
    pi - 2 pi = -pi is exact, so wrap2pi(-2 pi) = 0, while fl(pi + 2 pi) is one ulp below 3 pi (not representable) and
    wrap2pi(+2 pi) = -2.4e-7 - an edge of that length, with the two samples qa and qb (one with open_end)."""
    a = np.array([[3.0, 0.0]], F)
    down = (a - np.array([[TWO_PI, 0.0]], F)).astype(F)
    assert (down - a)[0, 0] == -TWO_PI
    closed = motion_samples_wrapped(a, down, 0b11, max_step=0.05)[0]
    assert len(closed[0]) == 1 and (closed[0][0] == down[0]).all() and closed[3].all()
    assert len(motion_samples_wrapped(a, down, 0b11, max_step=0.05, open_end=True)[0][0]) == 0
    assert len(motion_samples_wrapped(a, down, 0, max_step=0.05)[0][0]) == int(np.ceil(float(TWO_PI) / 0.05)) + 1
    up = (a + np.array([[TWO_PI, 0.0]], F)).astype(F)
    d = wrap2pi32((up - a).astype(F))[0, 0]
    assert d != 0 and abs(float(d)) <= 2 ** -20   # (qb itself is rounded at an ulp of 9.5e-7)
    assert len(motion_samples_wrapped(a, up, 0b11, max_step=0.05)[0][0]) == 2
    assert len(motion_samples_wrapped(a, up, 0b11, max_step=0.05, open_end=True)[0][0]) == 1


def _capture(pts_out):
    def score(p):
        pts_out.append(p.detach().clone())
        return torch.zeros(len(p), 1)
    return score


@pytest.mark.parametrize("kw", [dict(res=13), dict(max_step=0.11)])
def test_host_route_points_and_counts_follow_the_rule(kw):
    from diffco_amd._perceptron import host_motions
    qa, qb, crosses = seam_edges(np.random.default_rng(4).uniform(-np.pi, np.pi, (500, 3)).astype(F), 80, 5, 0b101)
    assert crosses.mean() > 0.25
    seen = []
    first, n = host_motions(_capture(seen), torch.from_numpy(qa), torch.from_numpy(qb), margin=0.0, max_samples=1000, wrap=0b101, **kw)
    smp = motion_samples_wrapped(qa, qb, 0b101, with_pre=True, **kw)
    counts = np.array([len(s[0]) for s in smp])
    # torch's norm may round an edge's length differently from the rule's ordered sum: a count may differ where
    # L / max_step lies within rounding of an integer - not on these seeds
    assert n.tolist() == counts.tolist() and (first == -1).all()
    got = seen[0].numpy().astype(np.float64)
    ref = np.concatenate([s[0] for s in smp]).astype(np.float64)
    assert got.shape == ref.shape
    assert np.abs(np.sin(got) - np.sin(ref))[:, [0, 2]].max() < 3e-6 and np.abs(np.cos(got) - np.cos(ref))[:, [0, 2]].max() < 3e-6
    assert np.abs(got[:, 1] - ref[:, 1]).max() < 3e-6
    # the planar arm's counts through the host route and the default bound
    from diffco_amd._ops import motion_bound
    a, b = torch.from_numpy(_A), torch.from_numpy(_B)
    assert host_motions(_capture([]), a, b, max_step=0.05, wrap=3)[1].tolist() == [7]
    assert host_motions(_capture([]), a, b, max_step=0.05)[1].tolist() == [121]
    assert 7 <= motion_bound(a, b, 0.05, wrap=3) <= 9 and 121 <= motion_bound(a, b, 0.05) <= 123
    assert motion_bound(a, b, 0.05, wrap=[True, False]) == motion_bound(a, b, 0.05, wrap=3)


@pytest.mark.parametrize("rule", ["res", "closed", "open"])
def test_host_route_autograd_is_the_rules_chain(rule):
    """host_motion_cost (differentiable torch ops) against helpers.motion_chain on the referee's samples, u from the wrapped
    delta, for a smooth 2 pi-periodic score whose gradient is known in closed form"""
    from diffco_amd._perceptron import host_motion_cost
    mask, dof = 0b011, 3
    q = np.random.default_rng(6).uniform(-np.pi, np.pi, (400, dof)).astype(F)
    qa, qb, crosses = seam_edges(q, 60, 7, mask)
    assert crosses.mean() > 0.25
    kw = dict(res=11) if rule == "res" else dict(max_step=0.2, open_end=(rule == "open"))
    w = torch.tensor([1.0, -0.7, 0.3], dtype=torch.float64)

    def score(p):   # periodic in the masked coordinates, linear in the plain one
        return (torch.sin(p[:, :2]) * w[:2]).sum(1, keepdim=True) + w[2] * p[:, 2:3]

    a = torch.from_numpy(qa).double().requires_grad_(True)
    b = torch.from_numpy(qb).double().requires_grad_(True)
    cost = host_motion_cost(score, a, b, margin=0.1, weight=0.7, max_samples=1000, wrap=mask, **kw)
    ga, gb = torch.autograd.grad(cost.sum(), (a, b))
    smp = motion_samples_wrapped(qa, qb, mask, **kw)
    assert [len(s[0]) for s in smp] == [len(s[0]) for s in motion_samples_wrapped(qa, qb, mask, **kw)]
    flat = torch.from_numpy(np.concatenate([s[0] for s in smp])).double()
    s = score(flat)[:, 0] - 0.1
    ends = np.cumsum([0] + [len(x[0]) for x in smp])
    corner = (s.abs() < 1e-4).numpy()   # a sample on the hinge's corner: its edge is left out
    keep = np.array([not corner[ends[e]:ends[e + 1]].any() for e in range(len(smp))])
    assert keep.mean() > 0.8
    h = s.clamp(min=0).numpy()
    g = (0.7 * (s > 0).double()[:, None] * torch.cat([torch.cos(flat[:, :2]) * w[:2], w[2].expand(len(flat), 1)], 1)).numpy()
    rc, rga, rgb = motion_chain(smp, h, g, 0.7)
    scale = np.abs(rc).max()
    assert scale > 0 and (rc == 0).any()
    # the host route interpolates in float64 here, the referee's points are fp32: agreement to fp32 rounding of the points
    assert np.abs(cost.detach().numpy() - rc)[keep].max() <= 1e-5 * scale
    gs = max(np.abs(rga).max(), np.abs(rgb).max())
    assert np.abs(ga.numpy() - rga)[keep].max() <= 1e-5 * gs and np.abs(gb.numpy() - rgb)[keep].max() <= 1e-5 * gs


def test_near_seam_flags_a_sample_on_the_seam():
    a = np.array([[3.0, 0.0], [1.0, 0.0]], F)
    b = np.array([[F(PI - F(3.0)) + F(-3.0) + F(0), 0.0], [1.5, 0.0]], F)
    # edge 0: 3.0 -> a target whose third of four samples lands on pi before the wrap; edge 1 stays far from it
    b[0, 0] = wrap2pi32(F(3.0) + F(4.0) * F(PI - F(3.0)) / F(2.0))
    smp = motion_samples_wrapped(a, b, 0b01, res=4, with_pre=True)
    flags = near_seam(smp, 0b01)
    assert flags.tolist() == [True, False]
