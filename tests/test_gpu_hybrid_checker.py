"""GPU: HybridForwardKinematicsDiffCo on the URDF Panda arm the suite loads (helpers.urdf_robot).  The perceptron's state comes
from a golden file (the supports and weights of cfg2_panda_rq, the weights centred so that the polyharmonic score takes both
signs): nothing is trained.  gt_check_func is a stub that counts its calls, keeps what it was handed and labels by a fixed rule."""
import pytest
import torch

from helpers import load, urdf_robot

pytestmark = pytest.mark.gpu

TIE = 1e-4    # of max |s|: the project's tie band


class _Stub:
    """the ground truth of the tests: a configuration collides iff its first joint is positive"""

    def __init__(self):
        self.calls = []

    def __call__(self, q):
        q = torch.as_tensor(q)
        self.calls.append(q.detach().clone().reshape(-1, q.shape[-1]))
        return q.reshape(-1, q.shape[-1])[:, 0] > 0


def _checker(cls, lazy=None, n_sup=300):
    from diffco_amd import _lib, kernel
    _lib.require_gpu()
    rob = urdf_robot("urdf_panda_nogripper")
    d = load("cfg2_panda_rq")
    stub = _Stub()
    kw = {} if lazy is None else dict(lazy_line_check=lazy)
    ck = cls(robot=rob, gamma=10, gt_check_func=stub, **kw)
    p = ck.perceptron
    w = torch.as_tensor(d["weights"][:n_sup, 0], dtype=torch.float32)
    p.support_points = torch.as_tensor(d["sup_q"][:n_sup], dtype=torch.float32).cuda()
    p.support_transformed = rob.fkine(p.support_points)
    p.rbf_kernel = kernel.Polyharmonic(1, 1.0)
    p.rbf_nodes = (w - w.mean()).cuda()
    torch.manual_seed(5)
    q = rob.rand_configs(600).cuda()
    ck.safety_bias = float(ck._calculate_safety_bias(q))
    return ck, stub, rob, q


def test_exported_like_the_reference():
    import diffco_amd
    from diffco_amd.collision_checkers import ForwardKinematicsDiffCo, HybridForwardKinematicsDiffCo
    assert diffco_amd.HybridForwardKinematicsDiffCo is HybridForwardKinematicsDiffCo
    assert "HybridForwardKinematicsDiffCo" in diffco_amd.__all__
    assert issubclass(HybridForwardKinematicsDiffCo, ForwardKinematicsDiffCo)
    assert "safe_bias" in HybridForwardKinematicsDiffCo.__doc__


def test_collision_hands_the_band_to_the_ground_truth_once():
    from diffco_amd.collision_checkers import HybridForwardKinematicsDiffCo
    ck, stub, rob, q = _checker(HybridForwardKinematicsDiffCo)
    assert ck.lazy_line_check is False
    band = ck.safety_bias
    s = ck.collision_score(q, bias=0)[:, 0]
    scale = float(s.abs().max())
    clear = ((s - band).abs() > TIE * scale) & ((s + band).abs() > TIE * scale)
    assert int(clear.sum()) >= 590
    labels = ck.collision(q)
    assert ck.last_route == "fused" and labels.shape == (600,) and labels.dtype == torch.bool
    assert len(stub.calls) == 1
    # the reference's lines 538-548 with the band they mean, as a torch composition on the scores this library returns
    unc = ~(s > band) & ~(s <= -band)
    want = s > band
    want[unc] = stub(q[unc])
    assert torch.equal(labels[clear], want[clear])
    assert 150 < int(unc.sum()) < 300 and min(int((s > band).sum()), int((s <= -band).sum())) > 100


def test_collision_band_configurations_in_order():
    from diffco_amd.collision_checkers import HybridForwardKinematicsDiffCo
    ck, stub, rob, q = _checker(HybridForwardKinematicsDiffCo)
    band = ck.safety_bias
    s = ck.collision_score(q, bias=0)[:, 0]
    scale = float(s.abs().max())
    clear = ((s - band).abs() > TIE * scale) & ((s + band).abs() > TIE * scale)
    unc = ~(s > band) & ~(s <= -band)
    labels = ck.collision(q)
    assert len(stub.calls) == 1 and ck.last_gt_checks == len(stub.calls[0])
    handed = stub.calls[0]
    if bool(clear.all()):
        assert torch.equal(handed, q[unc])
    else:   # a configuration at a threshold's tie may fall on either side: the others, in order
        rows = {tuple(r) for r in handed.cpu().tolist()}
        want = q[unc & clear].cpu().tolist()
        assert all(tuple(r) in rows for r in want)
        kept = [r for r in handed.cpu().tolist() if tuple(r) in {tuple(x) for x in want}]
        assert kept == want
    assert bool((handed[1:] != handed[:-1]).any(dim=1).all())
    # leading dimensions are kept; a band= keyword overrides safety_bias; band 0 asks nothing
    stub.calls.clear()
    l3 = ck.collision(q.reshape(6, 100, 7))
    assert l3.shape == (6, 100) and torch.equal(l3.reshape(-1), labels)
    stub.calls.clear()
    l0 = ck.collision(q, band=0.0)
    assert not stub.calls and ck.last_gt_checks == 0
    near0 = s.abs() <= TIE * scale
    assert torch.equal(l0[~near0], (s > 0)[~near0])
    wide = ck.collision(q, band=1e30)
    assert len(stub.calls) == 1 and torch.equal(stub.calls[0], q) and torch.equal(wide, q[:, 0] > 0)


def test_lazy_collision_checks_exactly_one_configuration():
    from diffco_amd.collision_checkers import HybridForwardKinematicsDiffCo
    ck, stub, rob, q = _checker(HybridForwardKinematicsDiffCo, lazy=True)
    s = ck.collision_score(q, bias=0)[:, 0]
    labels = ck.collision(q)
    assert len(stub.calls) == 1 and stub.calls[0].shape == (1, 7) and ck.last_gt_checks == 1
    i = int(s.argmax())
    assert torch.equal(stub.calls[0][0], q[i])
    want = s + ck.safety_bias > 0
    want[i] = bool(q[i, 0] > 0)
    assert torch.equal(labels, want)


@pytest.mark.parametrize("rule", ["res", "max_step"])
def test_check_motions_agrees_with_collision_on_the_materialised_samples(rule):
    """not lazy: an edge collides iff `collision` on its materialised samples reports one; the ground truth sees exactly the
    listed samples in one call; the first collision is the first sure hit or, on an undecided edge, the first confirmed sample"""
    from diffco_amd.collision_checkers import HybridForwardKinematicsDiffCo
    from helpers import motion_points
    ck, stub, rob, q = _checker(HybridForwardKinematicsDiffCo)
    band = ck.safety_bias
    qa, qb = q[:120], q[120:240]
    kw = dict(res=7) if rule == "res" else dict(max_step=0.6)
    hit, first = ck.check_motions(qa, qb, return_first=True, **kw)
    assert ck.last_route == "fused" and hit.dtype == torch.bool and first.dtype == torch.int32
    assert len(stub.calls) == 1
    handed = stub.calls[0]
    m = ck.perceptron._poly_fused.model(ck.perceptron.transform, ck.perceptron.rbf_kernel, ck.perceptron.support_transformed,
                                        ck.perceptron.rbf_nodes, torch.device("cuda"))
    verdict, fh, n_unc, ue, us, uq = m.motion_band(qa, qb, -band, band, **kw)
    assert ck.last_gt_checks == len(ue) == len(handed) and torch.equal(handed, uq)
    assert 0 < int((verdict == 2).sum()) and 0 < int((verdict == 1).sum()) and 0 < int((verdict == 0).sum())
    assert torch.equal(ck.check_motions(qa, qb, **kw), hit)
    # per edge, through collision() on the materialised samples
    pts = motion_points(qa.cpu().numpy(), qb.cpu().numpy(), kw.get("res"), kw.get("max_step"))
    scale = float(ck.collision_score(q, bias=0).abs().max())
    judged = 0
    for e, p in enumerate(pts):
        p = torch.as_tensor(p, device="cuda")
        s = ck.collision_score(p, bias=0)[:, 0]
        if bool((((s - band).abs() <= TIE * scale) | ((s + band).abs() <= TIE * scale)).any()):
            continue
        judged += 1
        lab = ck.collision(p)
        assert bool(lab.any()) == bool(hit[e]), e
        # the first collision: a sure hit decides the edge at its first sample above the band; otherwise the first confirmed one
        sure = (s > band).nonzero().reshape(-1)
        if len(sure):
            assert int(first[e]) == int(sure[0])
        else:
            assert int(first[e]) == (int(lab.nonzero()[0]) if bool(lab.any()) else -1)
    assert judged >= 100
    # band = 0: ForwardKinematicsDiffCo.check_motions(bias=0), and the ground truth is never asked
    stub.calls.clear()
    from diffco_amd.collision_checkers import ForwardKinematicsDiffCo
    h0, f0 = ck.check_motions(qa, qb, band=0.0, return_first=True, **kw)
    b0, g0 = ForwardKinematicsDiffCo.check_motions(ck, qa, qb, bias=0.0, return_first=True, **kw)
    assert not stub.calls and ck.last_gt_checks == 0
    assert torch.equal(h0, b0) and torch.equal(f0, g0)
    with pytest.raises(ValueError, match=r"edges \[.*\] need more than max_samples"):
        ck.check_motions(qa, qb, max_step=0.05, max_samples=4)


def test_lazy_check_motions_checks_the_worst_sample_of_the_undecided_edges():
    from diffco_amd.collision_checkers import HybridForwardKinematicsDiffCo
    from helpers import motion_points
    ck, stub, rob, q = _checker(HybridForwardKinematicsDiffCo, lazy=True)
    band = ck.safety_bias
    qa, qb = q[:120], q[120:240]
    worst, idx, _ = ck.motion_worst(qa, qb, res=7, bias=0.0)
    hit, first = ck.check_motions(qa, qb, res=7, return_first=True)
    unc = ~(worst > band) & ~(worst <= -band)
    assert 10 < int(unc.sum()) < 110
    assert len(stub.calls) == 1 and ck.last_gt_checks == int(unc.sum()) == len(stub.calls[0])
    handed = stub.calls[0]
    pts = motion_points(qa.cpu().numpy(), qb.cpu().numpy(), 7, None)
    want_q = torch.stack([torch.as_tensor(pts[e][int(idx[e])], device="cuda") for e in unc.nonzero().reshape(-1).tolist()])
    assert float((handed - want_q).abs().max()) <= 1e-5
    want = worst > band
    want[unc] = handed[:, 0] > 0
    assert torch.equal(hit, want)
    assert torch.equal(first[hit], idx[hit]) and bool((first[~hit] == -1).all())
