#!/usr/bin/env python3
"""Generate tests/golden/optim_weighted_baxter.npz from the REFERENCE: optim.Weighted.step (optim.py:662-761) with
dense_check=True and torch.optim.Adam on a Baxter left arm, the path after each of 10 iterations - the fused dense-check loop's
parity record (tests/test_gpu_weighted.py).

Runs ONLY in the build container (needs /root/reference, imported unedited through tools/make_golden.py), on the CPU.  The
record holds the inputs, every iteration's path of the reference's own fp32 run, and an fp64 rerun of the same class on the
same inputs (double path, double checker): the test's bar at iteration 10 is 2e-5 plus the reference's own fp32 distance from
that rerun.  Condition, checked here and stored: both runs sample every segment with the same count at all 10 iterations -
the start path's segment lengths are (k + 1/2) max_speed and lr is small enough that ten Adam steps cannot carry one across
a multiple of max_speed.

usage: python tools/make_golden_weighted.py [--out tests/golden]
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (imports the reference)

R = mg.R
MAX_SPEED, LR, N_WP, ITERS, S = 0.3, 0.002, 12, 10, 80


def seg_counts(p, max_step):
    d = (p[1:] - p[:-1]).norm(dim=-1)
    return torch.ceil(d / max_step).long()


def run(rob, checker, p0, options):
    """the path after each of ITERS iterations: step(maxiter=k) for k = 1 .. ITERS, each from p0 (the loop is deterministic).  The
    class's own path_history cannot serve: on the CPU its entries are one tensor, the final path, ITERS times."""
    hist = []
    for k in range(1, ITERS + 1):
        res = R.optim.Weighted(rob, checker, dict(options)).step(p0.clone(), maxiter=k)
        assert len(res.misc["path_history"]) == k, "the loop stopped early: the record needs all iterations"
        hist.append(res.x.detach().clone())
    hist = torch.stack(hist)
    before = [p0] + list(hist[:-1])
    return hist, torch.stack([seg_counts(b.to(hist.dtype), MAX_SPEED) for b in before])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
    out = ap.parse_args().out
    gen = torch.Generator().manual_seed(4100)
    rob = mg.make_robots()["baxter_left"]
    dof = 7
    # the start path: a random walk with segment lengths (k + 1/2) max_speed
    dirn = torch.randn((N_WP - 1, dof), generator=gen).double()
    dirn /= dirn.norm(dim=1, keepdim=True)
    length = (torch.randint(1, 4, (N_WP - 1, 1), generator=gen).double() + 0.5) * MAX_SPEED
    start = (torch.rand((1, dof), generator=gen).double() - 0.5) * 1.5
    p0 = torch.cat([start, dirn * length]).cumsum(dim=0).float()
    # supports on and around the path, so that the dense samples meet them
    pick = p0[torch.randint(0, N_WP, (S,), generator=gen)]
    sup_q = pick + 0.3 * torch.randn((S, dof), generator=gen)
    w = 0.05 * torch.randn(S, generator=gen)
    dc = mg.new_diffco(rob, "poly", (1, 1.0), sup_q, w, "poly")
    chk32 = types.SimpleNamespace(rbf_score=dc.poly_score, device="cpu")
    sup64 = mg.fk64(rob, sup_q).reshape(S, -1)
    fk = mg.fk64_fn(rob)
    chk64 = types.SimpleNamespace(
        rbf_score=lambda p: mg.k64("poly", (1, 1.0), fk(p).reshape(len(p), -1), sup64) @ w.double(), device="cpu")
    # the bias puts the hinge through the middle of the start path's scores: about half its samples in collision
    bias = -round(float((dc.poly_score(R.utils.dense_path(p0, MAX_SPEED))).median()), 3)
    options = {"n_waypoints": N_WP, "maxiter": ITERS, "history": True, "max_move_weight": 10, "collision_weight": 10,
               "joint_limit_weight": 10, "safety_bias": bias, "max_speed": MAX_SPEED, "optimizer": torch.optim.Adam,
               "optimizer_params": {"lr": LR}, "dense_check": True}
    h32, n32 = run(rob, chk32, p0, options)
    h64, n64 = run(rob, chk64, p0.double(), options)
    assert h32.dtype == torch.float32 and h64.dtype == torch.float64
    assert torch.equal(n32, n64), "fp32 and fp64 runs sample a segment differently: pick another start"
    s0 = dc.poly_score(R.utils.dense_path(p0, MAX_SPEED)) + bias
    assert 0.2 < float((s0 > 0).float().mean()) < 0.8, "the start path should be partly in collision"
    mg.save(out, "optim_weighted_baxter", sup_q=sup_q, weights=w, p0=p0, history32=h32, history64=h64, counts32=n32, counts64=n64,
            max_speed=np.float64(MAX_SPEED), lr=np.float64(LR), safety_bias=np.float64(bias),
            weights_loss=np.array([1.0, 10.0, 10.0, 10.0]), limits=rob.limits)
    d = (h32.double() - h64).abs().amax(dim=(1, 2)) / h64.abs().amax(dim=(1, 2))
    print(f"  weighted record: {ITERS} iterations, samples per iteration {n32.sum(dim=1).tolist()}, "
          f"fp32 vs fp64 rel. distance it 1 / it 10 = {float(d[0]):.2e} / {float(d[-1]):.2e}")


if __name__ == "__main__":
    main()
