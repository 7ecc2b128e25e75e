"""GPU: optim.Weighted - the routes it takes (fused: the dense-check loop on the device; host: torch on the checker's score), their
agreement, history / mask / normaliser hooks on both, and the fused route against the reference's own record of Weighted.step
(tests/golden/optim_weighted_baxter.npz, tools/make_golden_weighted.py)."""
import numpy as np
import pytest
import torch

from helpers import TorchDHRobot, TorchKernel, load, make_robot, relerr

pytestmark = pytest.mark.gpu


def _setup(transform=None):
    from diffco_amd import kernel
    from diffco_amd.kernel_perceptrons import DiffCo
    d = load("optim_weighted_baxter")
    rob = make_robot("baxter_left")
    dc = DiffCo(transform=rob.fkine if transform is None else transform(rob))
    dc.support_points = torch.from_numpy(d["sup_q"])
    dc.support_transformed = rob.fkine(dc.support_points)
    dc.rbf_kernel, dc.rbf_nodes = kernel.Polyharmonic(1, 1.0), torch.from_numpy(d["weights"])
    return d, rob, dc


def _options(d, optimizer=torch.optim.Adam, params=None, dense_check=True, history=True, maxiter=10):
    return {"n_waypoints": len(d["p0"]), "maxiter": maxiter, "history": history, "max_move_weight": 10, "collision_weight": 10,
            "joint_limit_weight": 10, "safety_bias": float(d["safety_bias"]), "max_speed": float(d["max_speed"]),
            "optimizer": optimizer, "optimizer_params": {"lr": float(d["lr"])} if params is None else params,
            "dense_check": dense_check}


class HostAdam(torch.optim.Adam):
    """torch.optim.Adam under another name: the same arithmetic, not the class the fused route asks for"""


def test_routes():
    from diffco_amd import optim
    d, rob, dc = _setup()
    p0 = torch.from_numpy(d["p0"])
    w = optim.Weighted(rob, dc, _options(d))
    res = w.step(p0, maxiter=2)
    assert w.last_route == "fused" and isinstance(res, optim.OptimizerResult)
    x, misc = res
    assert x is res.x and set(misc) == {"path_history", "time"} and len(misc["path_history"]) == 2
    assert tuple(x.shape) == tuple(p0.shape) and not torch.equal(x, p0) and w.cnt_check == 2 * (int(d["counts32"][0].sum()) + 1)
    for opts in (_options(d, torch.optim.SGD, {"lr": 1e-4}), _options(d, dense_check=False), _options(d, HostAdam),
                 _options(d, params={"lr": 1e-3, "weight_decay": 0.1})):
        w = optim.Weighted(rob, dc, opts)
        res = w.step(p0, maxiter=2)
        assert w.last_route == "host" and len(res.misc["path_history"]) == 2 and not torch.equal(res.x, p0)
    # a foreign transform: the checker's model scores features, the loop cannot be fused
    d, rob, foreign = _setup(transform=lambda rob: (lambda q: rob.fkine(q)))
    w = optim.Weighted(rob, foreign, _options(d))
    res = w.step(p0, maxiter=2)
    assert w.last_route == "host" and not torch.equal(res.x, p0)
    with pytest.raises(ValueError, match="fused route"):
        w.step(p0, maxiter=1, wrap=True)


class _Checker64:
    """the checker's score restated in float64 torch (helpers.TorchKernel on helpers.TorchDHRobot): a foreign callable, host route"""

    def __init__(self, d, rob64):
        self.rob64, self.w = rob64, torch.from_numpy(d["weights"]).double()
        self.sup = rob64.fkine(torch.from_numpy(d["sup_q"]).double()).reshape(len(d["sup_q"]), -1)
        self.kern = TorchKernel("poly1", 1, 1.0)

    def rbf_score(self, p):
        return self.kern(self.rob64.fkine(p).reshape(len(p), -1), self.sup) @ self.w


class _Robot64:
    """the robot as the host route uses it, in float64"""

    def __init__(self, rob):
        from diffco_amd.utils import wrap2pi
        self.fk, self.limits, self.dof, self.wrap = TorchDHRobot(rob), rob.limits.double(), rob.dof, wrap2pi

    def fkine(self, q):
        return self.fk.fkine(q)


def test_fused_and_host_routes_agree():
    """Adam on Baxter, 20 iterations.  Bar: the project's 2e-5 plus the host route's own fp32 distance from a float64 run of the
    same loop (double path, double checker and robot) at iteration 20 - the rule of test_gpu_parity.py."""
    from diffco_amd import optim
    d, rob, dc = _setup()
    p0 = torch.from_numpy(d["p0"])
    fused, host = optim.Weighted(rob, dc, _options(d, maxiter=20)), optim.Weighted(rob, dc, _options(d, HostAdam, maxiter=20))
    a, b = fused.step(p0), host.step(p0)
    assert (fused.last_route, host.last_route) == ("fused", "host")
    rob64 = _Robot64(rob)
    host64 = optim.Weighted(rob64, _Checker64(d, rob64.fk), _options(d, maxiter=20))
    c = host64.step(p0.double())
    assert host64.last_route == "host" and c.x.dtype == torch.float64
    assert len(a.misc["path_history"]) == len(b.misc["path_history"]) == len(c.misc["path_history"]) == 20
    err, own = relerr(a.x.numpy(), b.x.numpy()), relerr(b.x.numpy(), c.x.numpy())
    print(f"fused vs host after 20 iterations: {err:.2e}; host fp32 vs fp64: {own:.2e}; fused vs fp64: {relerr(a.x.numpy(), c.x.numpy()):.2e}")
    assert err < 2e-5 + own
    assert relerr(a.x.numpy(), p0.numpy()) > 1e-3       # the paths did move


@pytest.mark.parametrize("route", ["fused", "host"])
def test_history_mask_and_normaliser_hooks(route):
    from diffco_amd import optim
    d, rob, dc = _setup()
    p0 = torch.from_numpy(d["p0"])
    opt = torch.optim.Adam if route == "fused" else HostAdam
    mask = torch.ones(len(p0), dtype=torch.bool)
    mask[[0, 4, -1]] = False
    plain = optim.Weighted(rob, dc, _options(d, opt))
    ref = plain.step(p0, maxiter=3, mask=mask)
    assert plain.last_route == route and len(ref.misc["path_history"]) == 3
    assert torch.equal(ref.misc["path_history"][-1], ref.x)
    # a masked waypoint gets no gradient, but robot.wrap rounds every coordinate once per step ((pi + q) % 2 pi - pi, an ulp
    # of 2 pi each): "kept" is within 3 steps x 2 ulp(2 pi) = 3e-6; the free ones move by about lr per step
    shift = (ref.x - p0).abs().amax(dim=1)
    assert (shift[~mask] <= 3e-6).all() and (shift[mask] > 1e-3).all(), shift
    # the path comes in through the unnormaliser and every path goes out through the normaliser
    hooked = optim.Weighted(rob, dc, _options(d, opt))
    hooked.set_unnormalizer(lambda x: x * 2.0)
    hooked.set_normalizer(lambda x: x / 2.0)
    got = hooked.step(p0 / 2.0, maxiter=3, mask=mask)
    assert torch.equal(got.x, ref.x / 2.0)
    assert all(torch.equal(g, r / 2.0) for g, r in zip(got.misc["path_history"], ref.misc["path_history"]))
    # history off: no paths kept
    quiet = optim.Weighted(rob, dc, _options(d, opt, history=False))
    res = quiet.step(p0, maxiter=3, mask=mask)
    assert res.misc["path_history"] == [] and torch.equal(res.x, ref.x)
    # set_checker / set_robot replace what step() uses
    quiet.set_checker(dc)
    quiet.set_robot(rob)
    assert quiet.checker is dc and quiet.robot is rob


def test_fused_route_reproduces_the_reference_record():
    """the reference's own Weighted.step (dense_check=True, Adam; the path after k iterations from step(maxiter=k)) on a reference
    checker: iteration 1 to 2e-5,
    iteration 10 to 2e-5 plus the reference's own fp32 distance from its fp64 rerun at that iteration (the rule of
    test_gpu_parity.py).  Condition, checked when the record was generated and asserted from it: the reference's fp32 and fp64
    runs sample every segment with the same count at all 10 iterations."""
    from diffco_amd import optim
    d, rob, dc = _setup()
    assert d["counts32"].shape == (10, len(d["p0"]) - 1) and np.array_equal(d["counts32"], d["counts64"])
    w = optim.Weighted(rob, dc, _options(d))
    res = w.step(torch.from_numpy(d["p0"]))
    assert w.last_route == "fused" and len(res.misc["path_history"]) == 10
    hist = np.stack([h.numpy() for h in res.misc["path_history"]])
    own = relerr(d["history32"][9], d["history64"][9])
    e1, e10 = relerr(hist[0], d["history32"][0]), relerr(hist[9], d["history32"][9])
    print(f"iteration 1: {e1:.2e}  iteration 10: {e10:.2e}  (reference fp32 vs fp64 at 10: {own:.2e})")
    assert e1 < 2e-5
    assert e10 < 2e-5 + own
    assert w.cnt_check == int(d["counts32"].sum()) + 10
