"""GPU: motion checks and costs along the shortest arc of circular coordinates (dcx_check_motions_ex, dcx_motion_cost_ex, the
`wrap` argument of ScoreModel and the facades) against the fp64 oracle on the fp32 points of include/dcx.h's rule
(motion_wrap_helpers.motion_samples_wrapped), on edges about half of which cross +-pi: first hits and sample counts under both
rules, the counts the rule fixes on the planar arm, cost and endpoint gradients against the fp64 chain, autograd, mask 0
against the plain entry points bit for bit, the host route and wrap=True through the three facades."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import CASE_ROBOT, case_kernel, load, make_robot, motion_oracle
from motion_wrap_helpers import (COST_CASES, FIRST_HIT_CASES, PI, TWO_PI, WHEEL_ARM_URDF, fixture_model, motion_samples_wrapped,
                                 near_seam, seam_edges, wrap_case)

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def ops():
    from diffco_amd import _lib, _ops
    _lib.require_gpu()
    return _ops


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")


def _model(ops, name):
    d, desc, kern, sup, W = fixture_model(name)
    return ops.ScoreModel(desc, kern[0], kern[1], kern[2], _t(sup), _t(W))


@pytest.mark.parametrize("name,mask,margin,seed", FIRST_HIT_CASES, ids=[c[0] for c in FIRST_HIT_CASES])
@pytest.mark.parametrize("rule", ["res", "closed"])
def test_first_hit_and_counts_match_fp64_oracle(ops, name, mask, margin, seed, rule):
    c = wrap_case(name, mask, margin, seed, rule)
    assert c["crosses"].mean() >= 0.25
    m = _model(ops, name)
    kw = dict(c["kw"])
    kw.pop("open_end", None)
    if rule != "res":
        kw["max_samples"] = 100000
    first, n = m.check_motions(_t(c["qa"]), _t(c["qb"]), margin=c["margin"], wrap=mask, **kw)
    assert n.cpu().numpy().tolist() == c["counts"]
    ref = c["oracle"]["first"]
    keep = ~c["oracle"]["tie"] & ~c["seam"]
    print(name, rule, "kept", int(keep.sum()), "crossing", float(c["crosses"].mean()))
    assert keep.sum() > 200
    got = first.cpu().numpy()
    assert (got[keep] == ref[keep]).all(), np.nonzero(got[keep] != ref[keep])
    assert (got >= -1).all() and (ref[keep] == -1).any() and (ref[keep] >= 0).any()
    # the crossing edges are kept too, and the plain call answers them differently (it samples the long way round)
    assert (keep & c["crosses"]).sum() > 50
    plain, n_plain = m.check_motions(_t(c["qa"]), _t(c["qb"]), margin=c["margin"], **kw)
    if rule != "res":
        more = n_plain.cpu().numpy()[c["crosses"]] - np.array(c["counts"])[c["crosses"]]
        assert (more >= 0).all() and (more > 0).any()
    else:
        assert (plain.cpu().numpy()[keep] != ref[keep]).any()


def _planar(ops):
    return _model(ops, "cfg1_planar2_rq"), fixture_model("cfg1_planar2_rq")


def test_sample_counts_on_the_planar_arm(ops):
    m, (d, desc, kern, sup, W) = _planar(ops)
    two_pi = np.array([TWO_PI, 0.0], F)
    qa = np.array([[3.0, 0.0], [3.0, 0.0], [3.0, 0.0], [0.0, 1.0], [-2.0, 0.5]], F)
    qb = np.stack([np.array([-3.0, 0.0], F),          # 0.28 rad across the seam
                   (qa[1] - two_pi).astype(F),        # a full turn down: the fp32 difference is exactly -2 pi, L = 0
                   (qa[2] + two_pi).astype(F),        # a full turn up: wrap2pi(+2 pi) is not 0 in fp32 (an edge of 7e-7)
                   np.array([PI, F(F(1.0) + PI)], F),  # a difference of exactly pi in joint 0 (it goes the negative way)
                   np.array([F(F(-2.0) - PI), 0.5], F)]).astype(F)
    step = 0.05
    first, n = m.check_motions(_t(qa), _t(qb), max_step=step, wrap=3, max_samples=1000)
    smp = motion_samples_wrapped(qa, qb, 3, max_step=step)
    assert n.cpu().tolist() == [len(s[0]) for s in smp]
    assert n.cpu().tolist()[:3] == [7, 1, 2]
    plain = m.check_motions(_t(qa), _t(qb), max_step=step, max_samples=1000)[1].cpu().tolist()
    assert plain[:3] == [121, 127, 127]   # the plain call walks the long way: ceil(6 / 0.05) + 1, ceil(2 pi / 0.05) + 1
    o = motion_oracle(desc, kern, sup, W, smp, [0.0], grad=False)
    keep = ~o["tie"]
    assert (first.cpu().numpy()[keep] == o["first"][keep]).all()
    # open_end (dcx_motion_cost_ex): the target is no sample - the full turn down has none and costs nothing
    cost, ga, gb, n_open = m.motion_cost_raw(_t(qa), _t(qb), max_step=step, open_end=True, wrap=3, max_samples=1000)
    assert n_open.cpu().tolist() == [len(s[0]) for s in motion_samples_wrapped(qa, qb, 3, max_step=step, open_end=True)]
    assert n_open.cpu().tolist()[:3] == [6, 0, 1]
    assert float(cost[1]) == 0 and not ga[1].any() and not gb[1].any()
    # the default bound follows the longest WRAPPED edge (the plain bound would be 127 + 2)
    assert max(len(s[0]) for s in smp) <= ops.motion_bound(_t(qa), _t(qb), step, wrap=3) <= max(len(s[0]) for s in smp) + 2
    first2, n2 = m.check_motions(_t(qa), _t(qb), max_step=step, wrap=3)
    assert torch.equal(n2, n) and torch.equal(first2, first)
    # a mask bit at or above dof is refused by the library, before any launch
    with pytest.raises(ValueError, match="at or above dof"):
        m.check_motions(_t(qa), _t(qb), max_step=step, wrap=4)
    from diffco_amd import _lib
    opt = _lib.MotionOpts(0, step, 1000, 0)
    work = torch.empty(int(m._lib.dcx_motion_work_bytes(m._h, len(qa))), device="cuda", dtype=torch.uint8)
    rc = m._lib.dcx_check_motions_ex(m._h, _t(qa).data_ptr(), _t(qb).data_ptr(), len(qa), C.byref(opt), None, first.data_ptr(),
                                     None, work.data_ptr(), work.numel(), 4, None)
    assert rc == 1 and b"at or above dof" in m._lib.dcx_last_error()


def test_long_edge_crossing_the_seam_inside_a_tile(ops):
    """70 samples from 2.8 to -2.8 through pi: the seam falls on sample 35, inside the first 64-sample tile; the edges around it
    make the tile's lanes belong to several edges"""
    m, (d, desc, kern, sup, W) = _planar(ops)
    qa = np.array([[2.8, 0.3], [0.1, 0.2], [-3.0, 3.0], [2.8, -1.0]], F)
    qb = np.array([[-2.8, 0.3], [0.15, 0.2], [3.0, -3.0], [-2.8, -1.0]], F)
    step = 0.01
    smp = motion_samples_wrapped(qa, qb, 3, max_step=step, with_pre=True)
    counts = [len(s[0]) for s in smp]
    assert counts[0] > 64 and 20 < int(np.argmax(smp[0][0][:, 0] < 0)) < 50
    first, n = m.check_motions(_t(qa), _t(qb), max_step=step, wrap=3, max_samples=200)
    assert n.cpu().tolist() == counts
    seam = near_seam(smp, 3)
    smp = [s[:4] for s in smp]
    margin = [float(np.percentile(d["score64"], 70))]
    for mg in ([0.0], margin):
        o = motion_oracle(desc, kern, sup, W, smp, mg, weight=1.0)
        first, _ = m.check_motions(_t(qa), _t(qb), max_step=step, wrap=3, margin=mg, max_samples=200)
        keep = ~o["tie"] & ~seam
        assert keep[0] and (first.cpu().numpy()[keep] == o["first"][keep]).all()
        cost = m.motion_cost_raw(_t(qa), _t(qb), max_step=step, wrap=3, margin=mg, max_samples=200)[0].cpu().numpy()
        assert np.abs(cost - o["cost"]).max() <= 1e-5 * max(np.abs(o["cost"]).max(), 1e-30)


def _check(got, ref, tie, what):
    """test_gpu_motion_cost.py's comparison, its tolerances and its cap"""
    cost, ga, gb = (x.cpu().numpy().astype(np.float64) for x in got[:3])
    rc, rga, rgb, = ref
    keep = ~tie
    assert keep.sum() >= 0.5 * len(keep), what
    scale = max(np.abs(rc).max(), 1e-30)
    print(what, "cost err", np.abs(cost - rc).max() / scale, "kept", int(keep.sum()))
    assert np.abs(cost - rc).max() <= 1e-5 * scale, (what, np.abs(cost - rc).max(), scale)
    gs = max(np.abs(rga).max(), np.abs(rgb).max(), 1e-30)
    print(what, "grad err", np.abs(ga[keep] - rga[keep]).max(initial=0) / gs, np.abs(gb[keep] - rgb[keep]).max(initial=0) / gs)
    assert np.abs(ga[keep] - rga[keep]).max(initial=0) <= 1e-4 * gs, (what, np.abs(ga[keep] - rga[keep]).max(), gs)
    assert np.abs(gb[keep] - rgb[keep]).max(initial=0) <= 1e-4 * gs, (what, np.abs(gb[keep] - rgb[keep]).max(), gs)


@pytest.mark.parametrize("name,mask,margin,seed", COST_CASES, ids=[c[0] for c in COST_CASES])
@pytest.mark.parametrize("rule", ["res", "closed", "open"])
def test_cost_and_gradients_match_fp64_chain(ops, name, mask, margin, seed, rule):
    c = wrap_case(name, mask, margin, seed, rule, E=200, grad=True, weight=0.7, divisor=12, res=11)
    assert c["crosses"].mean() >= 0.25
    m = _model(ops, name)
    got = m.motion_cost_raw(_t(c["qa"]), _t(c["qb"]), margin=c["margin"], weight=0.7, wrap=mask,
                            max_samples=5000 if rule != "res" else None, **c["kw"])
    assert got[3].cpu().numpy().tolist() == c["counts"]
    o = c["oracle"]
    tie = o["tie"] | c["seam"]
    assert (o["cost"][~tie] > 0).any() and (o["cost"][~tie] == 0).any()
    _check(got, (o["cost"], o["ga"], o["gb"]), tie, (name, rule))
    # the wrapped direction matters: the plain call's gradients on the crossing edges are another edge's
    plain = m.motion_cost_raw(_t(c["qa"]), _t(c["qb"]), margin=c["margin"], weight=0.7,
                              max_samples=5000 if rule != "res" else None, **c["kw"])
    gs = max(np.abs(o["ga"]).max(), np.abs(o["gb"]).max())
    assert np.abs(plain[2].cpu().numpy() - o["gb"])[c["crosses"]].max() > 1e-2 * gs


def _new_api(name):
    from diffco_amd import kernel
    from diffco_amd.kernel_perceptrons import DiffCo
    d = load(name)
    kind, p0, p1 = case_kernel(d)
    rob = make_robot(CASE_ROBOT[name])
    kf = kernel.Polyharmonic(int(p0), p1) if kind == 1 else kernel.RQKernel(p0, p1)
    dc = DiffCo(kernel_func=kf, transform=rob.fkine)
    dc.support_points = _t(d["sup_q"])
    dc.support_transformed = rob.fkine(dc.support_points)
    dc.gains = _t(d["weights"][:, 0])
    return d, dc, rob


def test_autograd_and_path_cost(ops):
    d, dc, rob = _new_api("cfg1_planar2_rq")
    assert rob.wrap_mask == 3
    qa, qb, crosses = seam_edges(d["q"], 150, 31, 3)
    m = dc._score_fused.model(dc.transform, dc.kernel_func, dc.support_transformed, dc.gains, torch.device("cuda"))
    a, b = _t(qa).requires_grad_(True), _t(qb).requires_grad_(True)
    w = torch.rand(len(qa), device="cuda")
    for wrap in (True, 3, [True, True]):
        cost = dc.motion_cost(a, b, max_step=0.1, margin=-0.5, max_samples=5000, wrap=wrap)
        assert dc.last_route == "fused"
        ga, gb = torch.autograd.grad(cost.mul(w).sum(), (a, b))
        rc, rga, rgb, _ = m.motion_cost_raw(_t(qa), _t(qb), max_step=0.1, margin=-0.5, max_samples=5000, wrap=3)
        assert torch.equal(cost.detach(), rc) and torch.equal(ga, w[:, None] * rga) and torch.equal(gb, w[:, None] * rgb)
    assert float(rga.abs().max()) > 0
    # a path that crosses the seam twice: its cost is the sum over its open-ended edges plus its last waypoint
    paths = np.array([[[2.6, 0.0], [3.1, 0.4], [-2.9, 0.9], [-2.5, 1.2], [3.0, 1.0]],
                      [[-3.0, -2.0], [3.0, -2.5], [2.5, -3.1], [2.0, 3.1], [1.5, 2.8]]], F)
    p = _t(paths).requires_grad_(True)
    got = dc.path_cost(p, max_step=0.05, margin=-0.5, weight=0.5, wrap=True)
    (gp,) = torch.autograd.grad(got.sum(), (p,))
    T, Wp = paths.shape[:2]
    e_a, e_b = _t(paths[:, :-1].reshape(-1, 2)), _t(paths[:, 1:].reshape(-1, 2))
    seg, sga, sgb, n = m.motion_cost_raw(e_a, e_b, max_step=0.05, margin=-0.5, weight=0.5, open_end=True, wrap=3, max_samples=5000)
    last, _, lgb, _ = m.motion_cost_raw(_t(paths[:, -1]), _t(paths[:, -1]), max_step=0.05, margin=-0.5, weight=0.5, wrap=3,
                                        max_samples=5000)
    ref = seg.reshape(T, Wp - 1).sum(1) + last
    assert float(ref.max()) > 0 and float((got.detach() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    # every edge is a short one: waypoints at most 0.85 rad apart along the arc, not 6 rad
    assert int(n.max()) <= int(np.ceil(0.85 / 0.05))
    ref_g = torch.zeros_like(p)
    ref_g[:, :-1] += sga.reshape(T, Wp - 1, 2)
    ref_g[:, 1:] += sgb.reshape(T, Wp - 1, 2)
    ref_g[:, -1] += lgb
    assert float((gp - ref_g).abs().max()) <= 1e-5 * float(ref_g.abs().max())


def test_mask_zero_is_the_plain_call_bit_for_bit(ops):
    from diffco_amd import _lib
    m = _model(ops, "cfg3_baxter_rq_c5")
    d = load("cfg3_baxter_rq_c5")
    qa, qb, _ = seam_edges(d["q"], 300, 3, 0)
    qa_t, qb_t = _t(qa), _t(qb)
    E = len(qa)
    mg = _t(np.percentile(d["score64"], 90, axis=0).astype(F))
    lib, h = m._lib, m._h

    def check(ex, opt):
        first = torch.full((E,), -9, device="cuda", dtype=torch.int32)
        n = torch.full((E,), -9, device="cuda", dtype=torch.int32)
        work = torch.empty(int(lib.dcx_motion_work_bytes(h, E)), device="cuda", dtype=torch.uint8)
        args = (h, qa_t.data_ptr(), qb_t.data_ptr(), E, C.byref(opt), mg.data_ptr(), first.data_ptr(), n.data_ptr(), work.data_ptr(),
                work.numel())
        _lib.check(lib.dcx_check_motions_ex(*args, 0, None) if ex else lib.dcx_check_motions(*args, None))
        torch.cuda.synchronize()
        return first, n

    def cost(ex, opt):
        out = [torch.full((E,), -9.0, device="cuda"), torch.full((E, m.dof), -9.0, device="cuda"),
               torch.full((E, m.dof), -9.0, device="cuda"), torch.full((E,), -9, device="cuda", dtype=torch.int32)]
        nbytes = int(lib.dcx_motion_cost_work_bytes(h, E, opt.max_samples))
        work = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
        args = (h, qa_t.data_ptr(), qb_t.data_ptr(), E, C.byref(opt), mg.data_ptr(), 0.7, out[0].data_ptr(), out[1].data_ptr(),
                out[2].data_ptr(), out[3].data_ptr(), work.data_ptr(), nbytes)
        _lib.check(lib.dcx_motion_cost_ex(*args, 0, None) if ex else lib.dcx_motion_cost(*args, None))
        torch.cuda.synchronize()
        return out

    for opt in (_lib.MotionOpts(13, 0.0, 13, 0), _lib.MotionOpts(0, 0.2, 2000, 0)):
        a, b = check(False, opt), check(True, opt)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool((a[0] >= 0).any()) and bool((a[0] == -1).any())
    for opt in (_lib.MotionCostOpts(11, 0.0, 11, 0), _lib.MotionCostOpts(0, 0.2, 2000, 1)):
        a, b = cost(False, opt), cost(True, opt)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        assert bool((a[0] > 0).any()) and float(a[1].abs().max()) > 0
    # and ScoreModel's wrap=None / 0 / False are that call
    ref = m.check_motions(qa_t, qb_t, res=13, margin=mg)
    for wrap in (0, False, [False] * m.dof):
        got = m.check_motions(qa_t, qb_t, res=13, margin=mg, wrap=wrap)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_host_route_agrees_with_the_fused_one(ops):
    d, dc, rob = _new_api("cfg1_planar2_rq")
    qa, qb, crosses = seam_edges(d["q"], 120, 13, 3)
    assert crosses.mean() >= 0.25
    kw = dict(max_step=0.1, max_samples=2000)
    fused_hit, fused_first = dc.check_motions(_t(qa), _t(qb), return_first=True, wrap=True, **kw)
    assert dc.last_route == "fused"
    fused_cost = dc.motion_cost(_t(qa), _t(qb), margin=-0.5, wrap=True, **kw)
    a2, b2 = _t(qa).requires_grad_(True), _t(qb).requires_grad_(True)
    ga2, gb2 = torch.autograd.grad(dc.motion_cost(a2, b2, margin=-0.5, wrap=3, **kw).sum(), (a2, b2))
    dc.transform = lambda q: rob.fkine(q) * 1.0   # same map, not a diffco_amd robot's fkine: not fusable, and nobody's mask
    with pytest.raises(ValueError, match="wrap=True"):
        dc.check_motions(_t(qa), _t(qb), wrap=True, **kw)
    host_hit, host_first = dc.check_motions(_t(qa), _t(qb), return_first=True, wrap=3, **kw)
    assert dc.last_route == "host"
    # (torch's norm may round an edge's length differently from the kernel's: at most a tie-level disagreement)
    mismatch = (host_first != fused_first).nonzero().reshape(-1).tolist()
    assert len(mismatch) <= 1, mismatch
    assert 0 < int(fused_hit.sum()) < len(qa)
    a, b = _t(qa).requires_grad_(True), _t(qb).requires_grad_(True)
    host = dc.motion_cost(a, b, margin=-0.5, wrap=[True, True], **kw)
    assert dc.last_route == "host"
    assert float((host.detach() - fused_cost).abs().max()) <= 1e-4 * float(fused_cost.abs().max())
    ga, gb = torch.autograd.grad(host.sum(), (a, b))
    gs = float(torch.cat([ga2, gb2]).abs().max())
    assert float((ga - ga2).abs().max()) <= 1e-3 * gs and float((gb - gb2).abs().max()) <= 1e-3 * gs
    # the plain call is another question on these edges
    dc.transform = rob.fkine
    plain = dc.check_motions(_t(qa), _t(qb), return_first=True, **kw)[1]
    assert bool((plain != fused_first).any())


def test_wrap_true_through_the_facades(ops):
    from diffco_amd import kernel
    from diffco_amd.collision_checkers import ForwardKinematicsDiffCo
    from diffco_amd.deprecated import MultiDiffCo
    from diffco_amd.urdf import URDFRobotFK
    # kernel_perceptrons.DiffCo on the planar arm: every joint
    d, dc, rob = _new_api("cfg1_planar2_rq")
    qa, qb, _ = seam_edges(d["q"], 100, 17, 3)
    a, b = dc.check_motions(_t(qa), _t(qb), res=11, return_first=True, wrap=True), \
        dc.check_motions(_t(qa), _t(qb), res=11, return_first=True, wrap=3)
    assert torch.equal(a[1], b[1]) and 0 < int(a[0].sum()) < len(qa)
    assert torch.equal(dc.path_cost(_t(qa[:20].reshape(4, 5, 2)), 0.1, wrap=True), dc.path_cost(_t(qa[:20].reshape(4, 5, 2)), 0.1, wrap=3))
    # a deprecated class on the SE(3) body's keypoints: the Euler angles
    se3 = make_robot("se3")
    g = torch.Generator().manual_seed(0)
    lo, hi = se3.limits[:, 0], se3.limits[:, 1]
    sup = (torch.rand(80, 6, generator=g) * (hi - lo) + lo).cuda()
    mc = MultiDiffCo(None)
    mc.support_points = sup
    mc.fkine = se3.fkine
    mc.support_fkine = se3.fkine(sup)
    mc.rbf_kernel = kernel.RQKernel(0.05)
    mc.rbf_nodes = torch.randn(80, 3, generator=g).cuda()
    q = (torch.rand(400, 6, generator=g) * (hi - lo) + lo).numpy()
    qa, qb, crosses = seam_edges(q, 100, 19, 0b111000)
    assert crosses.mean() >= 0.25
    a = mc.check_motions(_t(qa), _t(qb), max_step=0.5, return_first=True, wrap=True)
    b = mc.check_motions(_t(qa), _t(qb), max_step=0.5, return_first=True, wrap=0b111000)
    assert mc.last_route == "fused" and torch.equal(a[1], b[1]) and bool(a[0].any())
    assert torch.equal(mc.motion_cost(_t(qa), _t(qb), res=9, wrap=True), mc.motion_cost(_t(qa), _t(qb), res=9, wrap=[0, 0, 0, 1, 1, 1]))
    assert not torch.equal(mc.motion_cost(_t(qa), _t(qb), res=9, wrap=True), mc.motion_cost(_t(qa), _t(qb), res=9))
    # collision_checkers on a URDF with two continuous joints: those two
    rob = URDFRobotFK(WHEEL_ARM_URDF)
    assert rob.wrap_mask == 0b1001
    fk = ForwardKinematicsDiffCo(robot=rob, gamma=10)
    p = fk.perceptron
    sup = rob.rand_configs(60).cuda()
    p.support_points = sup
    p.support_transformed = rob.fkine(sup)
    p.rbf_kernel = kernel.Polyharmonic(1, 1.0)
    p.rbf_nodes = torch.randn(60, generator=g).cuda()
    fk.safety_bias = 0
    q = rob.rand_configs(400).numpy()
    qa, qb, crosses = seam_edges(q, 100, 23, 0b1001)
    a = fk.check_motions(_t(qa), _t(qb), max_step=0.2, return_first=True, wrap=True)
    b = fk.check_motions(_t(qa), _t(qb), max_step=0.2, return_first=True, wrap=0b1001)
    assert fk.last_route == "fused" and torch.equal(a[1], b[1])
    assert torch.equal(fk.motion_cost(_t(qa), _t(qb), max_step=0.2, wrap=True), fk.motion_cost(_t(qa), _t(qb), max_step=0.2, wrap=0b1001))
    pts = np.concatenate([s[0] for s in motion_samples_wrapped(qa, qb, 0b1001, max_step=0.2)])
    s = fk.collision_score(_t(pts))[:, 0]
    ends = np.cumsum([0] + [len(x[0]) for x in motion_samples_wrapped(qa, qb, 0b1001, max_step=0.2)])
    agree = 0
    for e in range(len(qa)):
        se = s[ends[e]:ends[e + 1]]
        if (se.abs() <= 1e-4 * s.abs().max()).any():
            continue
        ref = int((se > 0).nonzero()[0]) if (se > 0).any() else -1
        assert int(a[1][e]) == ref, e
        agree += 1
    assert agree > 60
