"""GPU: the dense-check Adam trajectory loop (dcx_traj_dense_run / dcx_traj_dense_step, traj.DenseAdamRun): the step against a
float64 restatement built on the fp64 oracle, the run against the same launches enqueued by hand (bit for bit, eagerly and
replayed from a HIP graph), the collision term against ScoreModel.path_cost and its autograd gradient (linear and shortest-arc
sampling), and the rules: move mask, wrap after the update, the stop on the constraint value, a segment over max_samples,
history rows, no-op calls."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import relerr
from traj_dense_common import (F, MAX_STEP, Fixture, dense_io, dense_run, dense_state, dense_step, off_multiples)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from diffco_amd import _lib, _ops
    _lib.require_gpu()
    return _ops


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype, device="cuda")


def _opts(lr=0.05, weights=(1, 10, 10, 10), margin=0.0, max_speed=0.3, valid_tol=1e-2, grad_tol=1e-4):
    from diffco_amd import _lib
    return _lib.TrajOpts(lr, 0.9, 0.999, 1e-8, *weights, margin, max_speed, valid_tol, grad_tol)


def _dopts(max_step, max_samples=16, wrap=0, rewrap=0, normalize=0, stop_tol=0.0):
    from diffco_amd import _lib
    return _lib.TrajDenseOpts(max_step, max_samples, wrap, rewrap, normalize, stop_tol)


# ---- 1. the step against the float64 restatement -----------------------------------------------------------------------------
# (robot, kernel, C, W, fixture seed: the smallest one whose float64 run meets the test's conditions - they are checked on the CPU)
STEP_CASES = [("baxter", "poly", 1, 2, 0), ("baxter", "poly", 1, 5, 0), ("baxter", "poly", 5, 65, 4), ("baxter", "rq", 3, 5, 0),
              ("planar3", "rq", 3, 5, 0), ("planar3", "poly", 1, 65, 0), ("tree", "poly", 5, 5, 0), ("tree", "rq", 1, 65, 0)]


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("name,kern,Cn,W,seed", STEP_CASES, ids=[f"{c[0]}-{c[1]}-C{c[2]}-W{c[3]}" for c in STEP_CASES])
def test_step_matches_float64_restatement(ops, name, kern, Cn, W, seed, normalize):
    """three iterations, one dcx_traj_dense_run call each, against traj_dense_common.dense_step; the project's bars of
    test_single_adam_step_matches_float64_restatement: relerr(stats[:7]) < 5e-5, relerr(path) < 2e-5, and the gradient itself
    (adam_m / (1 - beta1) behind step 1) < 2e-5.  Conditions, asserted here on the CPU: the restatement's per-edge sample counts
    are the device's at every iteration (no segment length within 1e-3 relative of a multiple of max_step: the fixture's
    lengths are (k + 1/2) max_step and lr = 0.002 moves one by at most 2 sqrt(dof) lr per step), and no sample's score lies
    within 1e-5 max|score| of its margin (ten times the fp32 sweep's rounding: both precisions switch the same hinges on)."""
    from diffco_amd import _lib
    lib = _lib.require_gpu()
    fx = Fixture(name, kern, Cn, 3, W, seed=seed)
    model = fx.model(ops)
    lr, ms, step = 0.002, 0.3, MAX_STEP
    st, b = dense_state(model, fx.limits, fx.paths)
    opt, dopt, io = _opts(lr, max_speed=ms), _dopts(step, 16, normalize=normalize), dense_io(b)
    mg = _t(fx.margin)
    R, dof = 3, fx.dof
    ref_p = [torch.from_numpy(fx.paths[r]).double() for r in range(R)]
    ref_m = [torch.zeros(W, dof, dtype=torch.float64) for _ in range(R)]
    ref_v = [torch.zeros(W, dof, dtype=torch.float64) for _ in range(R)]
    total = np.zeros(R, np.int64)
    for t in (1, 2, 3):
        dense_run(lib, model, st, opt, dopt, io, mg, t, 1)
        torch.cuda.synchronize()
        n_dev = b["n_samples"].cpu().numpy().reshape(R, W)
        first = n_dev if t == 1 else first
        for r in range(R):
            assert off_multiples(ref_p[r].numpy(), step), (t, r)
            ref_p[r], ref_m[r], ref_v[r], terms, g, counts, gap = dense_step(fx, ref_p[r], ref_m[r], ref_v[r], t, lr, step, ms,
                                                                             fx.margin, normalize)
            assert n_dev[r].tolist() == counts.tolist(), (t, r)
            assert gap > 1e-5 and float(terms[4]) > 0, (t, r, gap)     # samples above their margin, none on it
            total[r] += counts.sum()
            got = b["stats"][r, :7].cpu().double().numpy()
            print(f"t={t} r={r} stats {relerr(got, terms.numpy()):.2e} path {relerr(b['path'][r].cpu().numpy(), ref_p[r].numpy()):.2e}")
            assert relerr(got, terms.numpy()) < 5e-5, (t, r, got, terms)
            assert relerr(b["path"][r].cpu().numpy(), ref_p[r].numpy()) < 2e-5, (t, r)
            if t == 1 and W > 2:
                assert relerr(b["adam_m"][r].cpu().numpy() / 0.1, g.numpy()) < 2e-5, r
            assert torch.equal(b["path"][r, 0].cpu(), torch.from_numpy(fx.paths[r, 0]))
            assert torch.equal(b["path"][r, -1].cpu(), torch.from_numpy(fx.paths[r, -1]))
    if W >= 5:
        assert first[1, 1] == 0 and float(b["stats"][2, 6]) > 0   # the repeated waypoint (before the steps part it), the joint limits
    assert b["steps"].tolist() == [3, 3, 3] and b["n_checks"].cpu().numpy().tolist() == total.tolist()
    assert b["stats"][:, 7].tolist() == [0, 0, 0]


# ---- 2. the run = the same launches enqueued by hand, bit for bit ------------------------------------------------------------
def _hand_loop(lib, model, st, b, opt, dopt, mg, n_iters, history):
    from diffco_amd import _lib
    R, W = st.n_paths, st.n_waypoints
    dof = b["path"].shape[2]
    dev, f32 = model.dev, dict(device=model.dev, dtype=torch.float32)
    need = int(lib.dcx_motion_cost_work_bytes(model._h, R * W, dopt.max_samples))
    work = torch.empty(need, device=dev, dtype=torch.uint8)
    cc, cga, cgb = torch.empty(R, **f32), torch.empty((R, dof), **f32), torch.empty((R, dof), **f32)
    cn = torch.empty(R, device=dev, dtype=torch.int32)
    p = lambda t: C.c_void_p(t.data_ptr())
    mo = _lib.MotionCostOpts(0, dopt.max_step, dopt.max_samples, 1)
    mc = _lib.MotionCostOpts(0, dopt.max_step, dopt.max_samples, 0)
    fk = model.desc
    for it in range(n_iters):
        path = b["path"]
        qb = torch.cat([path[:, 1:], path[:, -1:]], dim=1).contiguous()
        ql = path[:, -1].contiguous()
        _lib.check(lib.dcx_motion_cost_ex(model._h, p(path), p(qb), R * W, C.byref(mo), p(mg), 1.0, p(b["edge_cost"]), p(b["grad_a"]),
                                          p(b["grad_b"]), p(b["n_samples"]), p(work), need, dopt.wrap_mask, model._st()))
        _lib.check(lib.dcx_motion_cost_ex(model._h, p(ql), p(ql), R, C.byref(mc), p(mg), 1.0, p(cc), p(cga), p(cgb), p(cn), p(work),
                                          need, dopt.wrap_mask, model._st()))
        b["edge_cost"].view(R, W)[:, W - 1] = cc
        b["grad_a"].view(R, W, dof)[:, W - 1] = cga
        b["grad_b"].view(R, W, dof)[:, W - 1] = cgb
        b["n_samples"].view(R, W)[:, W - 1] = cn
        io = dense_io(b, history=None if history is None else history[it])
        _lib.check(lib.dcx_traj_dense_step(model.dev.index or 0, C.byref(fk), C.byref(st), C.byref(opt), C.byref(dopt), C.byref(io),
                                           model.C, it + 1, model._st()))


KEYS = ("path", "adam_m", "adam_v", "stats", "lowest_loss", "lowest_obj", "lowest_path", "best_valid_obj", "best_valid_path", "done",
        "steps", "n_checks", "edge_cost", "grad_a", "grad_b", "n_samples")


@pytest.mark.parametrize("R,W,Cn", [(1, 5, 1), (4, 5, 5), (4, 65, 1), (1, 65, 5)])
def test_run_is_the_hand_enqueued_loop_bit_for_bit(ops, R, W, Cn):
    from diffco_amd import _lib
    lib = _lib.require_gpu()
    fx = Fixture("baxter", "poly", Cn, R, W, seed=5 + R + W)
    model = fx.model(ops)
    opt, dopt, mg = _opts(0.002), _dopts(0.11, 16, normalize=1), _t(fx.margin)   # (a small lr: still in collision after 3 steps)
    n = 3
    st_a, a = dense_state(model, fx.limits, fx.paths)
    hist_a = torch.zeros((n, R, W, fx.dof), device=model.dev)
    _hand_loop(lib, model, st_a, a, opt, dopt, mg, n, hist_a)
    st_b, b = dense_state(model, fx.limits, fx.paths)
    hist_b = torch.zeros_like(hist_a)
    dense_run(lib, model, st_b, opt, dopt, dense_io(b, history=hist_b), mg, 1, n)
    torch.cuda.synchronize()
    assert float(a["stats"][:, 4].min()) > 0 and a["steps"].tolist() == [n] * R
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(hist_a, hist_b) and torch.equal(hist_a[-1], a["path"])
    # the per-edge arrays left NULL: carved from the workspace, the same bits
    st_c, c = dense_state(model, fx.limits, fx.paths)
    dense_run(lib, model, st_c, opt, dopt, dense_io(c, edges=False), mg, 1, n)
    torch.cuda.synchronize()
    for k in KEYS[:12]:
        assert torch.equal(a[k], c[k]), k
    # margin NULL = opt->safety_margin for every class (written into the workspace by the edge-list launch): the bits of a
    # constant margin tensor
    c0 = float(fx.margin.min())
    opt_c = _opts(0.002, margin=c0)
    st_e, e = dense_state(model, fx.limits, fx.paths)
    dense_run(lib, model, st_e, opt_c, dopt, dense_io(e), _t(np.full(Cn, c0, F)), 1, n)
    st_f, f = dense_state(model, fx.limits, fx.paths)
    dense_run(lib, model, st_f, opt_c, dopt, dense_io(f), None, 1, n)
    torch.cuda.synchronize()
    assert float(e["stats"][:, 4].min()) > 0
    for k in KEYS:
        assert torch.equal(e[k], f[k]), k
    # ... and captured in a HIP graph, replayed once, after one eager call on the stream
    st_d, d = dense_state(model, fx.limits, fx.paths)
    init = {k: v.clone() for k, v in d.items()}
    hist_d = torch.zeros_like(hist_a)
    io_d = dense_io(d, history=hist_d)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        work = dense_run(lib, model, st_d, opt, dopt, io_d, mg, 1, n)
        for k, v in init.items():
            d[k].copy_(v)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        dense_run(lib, model, st_d, opt, dopt, io_d, mg, 1, n, work=work)
    hist_d.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(a[k], d[k]), k
    assert torch.equal(hist_a, hist_d)


# ---- 3. the collision term = ScoreModel.path_cost and its autograd gradient --------------------------------------------------
@pytest.mark.parametrize("wrap", [0, 0b111])
def test_collision_term_is_path_cost(ops, wrap):
    """lr = 0, the other weights 0: stats[:, 4] is path_cost and adam_m / (1 - beta1) its gradient (w_collision = 1), for
    linear and shortest-arc sampling of paths whose consecutive waypoints straddle +-pi"""
    from diffco_amd import _lib
    lib = _lib.require_gpu()
    R, W = 3, 6
    fx = Fixture("planar3", "rq", 3, R, W, seed=3, quirks=False)
    g = np.random.default_rng(8)
    paths = fx.paths.copy()
    paths[:, :, 0] = np.where(np.arange(W)[None] % 2 == 0, 3.0, -3.0) + 0.1 * g.normal(size=(R, W))   # across +-pi and back
    paths = paths.astype(F)
    fx.sup_q[:20, 0] = np.pi - 0.05 * g.random(20)                                                      # supports on the short arc
    from oracle import oracle
    fx.sup = oracle.fkine(fx.desc, fx.sup_q, F)
    model = fx.model(ops)
    step, cap = 0.2, 64
    margin = fx.margin.tolist()
    pt = _t(paths).requires_grad_(True)
    cost = model.path_cost(pt, step, margin=margin, max_samples=cap, wrap=wrap)
    (gr,) = torch.autograd.grad(cost.sum(), pt)
    assert float(cost.detach().min()) > 0
    st, b = dense_state(model, fx.limits, paths)
    opt, dopt = _opts(0.0, weights=(0, 1, 0, 0)), _dopts(step, cap, wrap=wrap)
    move = torch.ones(W, dtype=torch.uint8, device="cuda")
    dense_run(lib, model, st, opt, dopt, dense_io(b, move=move), _t(margin), 1, 1)
    torch.cuda.synchronize()
    print("cost", relerr(b["stats"][:, 4].cpu().numpy(), cost.detach().cpu().numpy()), "grad",
          relerr(b["adam_m"].cpu().numpy() / 0.1, gr.cpu().numpy()))
    assert relerr(b["stats"][:, 4].cpu().numpy(), cost.detach().cpu().numpy()) < 1e-6
    assert relerr((b["adam_m"].double() / 0.1).cpu().numpy(), gr.cpu().numpy()) < 1e-6
    assert torch.equal(b["path"].cpu(), torch.from_numpy(paths))          # lr = 0
    # the two samplings really differ on these paths: the linear one walks the long way round
    counts = b["n_samples"].cpu().numpy().reshape(R, W)
    if wrap:
        assert counts[:, :-1].max() <= 10     # the short way across +-pi
    else:
        assert counts[:, :-1].min() >= 25     # about 6 rad in joint 0 at 0.2 per sample


# ---- 4. the rules ------------------------------------------------------------------------------------------------------------
def test_move_mask_and_endpoints(ops):
    from diffco_amd import _lib
    lib = _lib.require_gpu()
    R, W = 2, 7
    fx = Fixture("baxter", "poly", 1, R, W, seed=21)
    model = fx.model(ops)
    opt, dopt, mg = _opts(0.05), _dopts(0.11, 16), _t(fx.margin)
    move = torch.tensor([1, 0, 1, 1, 0, 1, 1], dtype=torch.uint8, device="cuda")
    st, b = dense_state(model, fx.limits, fx.paths)
    dense_run(lib, model, st, opt, dopt, dense_io(b, move=move), mg, 1, 2)
    p0, p1 = torch.from_numpy(fx.paths), b["path"].cpu()
    for w in range(W):
        same = torch.equal(p0[:, w], p1[:, w])
        assert same == (int(move[w]) == 0), w                    # exactly its rows, the endpoints free
    assert float(b["adam_m"][:, [1, 4]].abs().max()) == 0
    st, b = dense_state(model, fx.limits, fx.paths)
    dense_run(lib, model, st, opt, dopt, dense_io(b), mg, 1, 2)   # NULL: the endpoints are pinned bit for bit
    p1 = b["path"].cpu()
    assert torch.equal(p0[:, 0], p1[:, 0]) and torch.equal(p0[:, -1], p1[:, -1])
    assert not any(torch.equal(p0[:, w], p1[:, w]) for w in range(1, W - 1))


def _np_wrap2pi(x):
    pi, two_pi = F(3.14159265358979323846), F(6.28318530717958647692)
    r = np.fmod((pi + x).astype(F), two_pi).astype(F)
    r = np.where(r < 0, (r + two_pi).astype(F), r)
    return (r - pi).astype(F)


def test_rewrap_after_the_update(ops):
    from diffco_amd import _lib
    lib = _lib.require_gpu()
    R, W = 2, 6
    fx = Fixture("planar3", "rq", 1, R, W, seed=4, quirks=False)
    paths = fx.paths.copy()
    paths[:, :, 1] = 3.1 + 0.02 * np.arange(W)[None]     # joint 1 close to +pi: lr-sized steps cross it
    paths[:, :, 2] = -3.13
    model = fx.model(ops)
    mg = _t(fx.margin)
    move = torch.ones(W, dtype=torch.uint8, device="cuda")
    opt = _opts(0.05)
    st, a = dense_state(model, fx.limits, paths)
    dense_run(lib, model, st, opt, _dopts(0.11, 64), dense_io(a, move=move), mg, 1, 1)
    st, b = dense_state(model, fx.limits, paths)
    dense_run(lib, model, st, opt, _dopts(0.11, 64, rewrap=0b110), dense_io(b, move=move), mg, 1, 1)
    raw, got = a["path"].cpu().numpy(), b["path"].cpu().numpy()
    assert (np.abs(raw[:, :, 1:]) > np.pi).any()                                # the unwrapped update does leave the interval
    assert (got[:, :, 1:] >= -np.pi).all() and (got[:, :, 1:] < np.pi).all()
    assert np.array_equal(got[:, :, 1:], _np_wrap2pi(raw[:, :, 1:]))            # the same bits as numpy's wrap2pi of it
    assert np.array_equal(got[:, :, 0], raw[:, :, 0])                           # bit 0 is not set
    assert torch.equal(a["adam_m"], b["adam_m"])


def test_stop_tol_freezes_after_the_step(ops):
    from diffco_amd import _lib
    lib = _lib.require_gpu()
    R, W = 3, 6
    fx = Fixture("baxter", "poly", 1, R, W, seed=9, quirks=False)
    hi = fx.limits[:, 1].numpy()
    paths = fx.paths.copy()
    paths[1, 2, 0] = hi[0] + 1.0      # paths 1 and 2 stay far above stop_tol through their joint-limit term (10 * ~1);
    paths[2, 3, 0] = hi[0] + 1.0      # path 0's constraint is its small collision term alone
    model = fx.model(ops)
    opt, dopt, mg = _opts(0.05, weights=(1, 1e-4, 10, 10), max_speed=10.0), _dopts(0.11, 64, stop_tol=0.5), _t(fx.margin)
    st, b = dense_state(model, fx.limits, paths)
    hist = torch.zeros((3, R, W, fx.dof), device="cuda")
    con = []
    for t in (1, 2, 3):   # one call per iteration: the constraint value each path saw
        dense_run(lib, model, st, opt, dopt, dense_io(b, history=hist[t - 1]), mg, t, 1)
        con.append(b["stats"][:, 2].cpu().tolist())
    # path 0 took the step whose constraint was <= stop_tol - steps counts it - and froze; its history rows repeat from there
    k = next(t for t in range(3) if con[t][0] <= 0.5)
    assert k < 2 and all(con[t][0] > 0.5 for t in range(k)) and con[k][0] > 0, con
    assert min(con[2][1:]) > 0.5, con
    assert b["done"].tolist() == [1, 0, 0] and b["steps"].tolist() == [k + 1, 3, 3]
    before = torch.from_numpy(paths[0]).cuda() if k == 0 else hist[k - 1, 0]
    assert not torch.equal(hist[k, 0], before)
    assert all(torch.equal(hist[t, 0], hist[k, 0]) for t in range(k + 1, 3))
    assert not torch.equal(hist[2, 1], hist[1, 1]) and torch.equal(hist[2], b["path"])


def test_segment_over_max_samples_freezes_the_path_alone(ops):
    from diffco_amd import _lib
    lib = _lib.require_gpu()
    R, W = 3, 5
    fx = Fixture("baxter", "poly", 1, R, W, seed=13, quirks=False)
    paths = fx.paths.copy()
    paths[1, 2] += 3.0                                   # two long segments in path 1: ~30 samples each at 0.11
    model = fx.model(ops)
    opt, dopt, mg = _opts(0.05), _dopts(0.11, 12), _t(fx.margin)
    st, b = dense_state(model, fx.limits, paths)
    hist = torch.zeros((2, R, W, fx.dof), device="cuda")
    m0 = torch.randn_like(b["adam_m"])      # moments as if from earlier steps: a frozen path's must come back untouched
    b["adam_m"].copy_(m0)
    b["adam_v"].copy_(m0 * m0)
    dense_run(lib, model, st, opt, dopt, dense_io(b, history=hist), mg, 1, 2)
    torch.cuda.synchronize()
    assert b["done"].tolist() == [0, 1, 0] and b["steps"].tolist() == [2, 0, 2]
    assert b["stats"][:, 7].tolist() == [0, -2, 0] and int(b["n_checks"][1]) == 0
    assert torch.equal(b["path"][1].cpu(), torch.from_numpy(paths[1])) and torch.equal(b["adam_m"][1], m0[1])
    assert torch.equal(b["adam_v"][1], (m0 * m0)[1]) and float(b["lowest_loss"][1]) == float("inf")
    assert torch.equal(hist[0, 1], b["path"][1]) and torch.equal(hist[1, 1], b["path"][1])
    assert not torch.equal(b["path"][0].cpu(), torch.from_numpy(paths[0])) and int(b["n_checks"][0]) > 0


def test_no_op_calls(ops):
    from diffco_amd import _lib
    lib = _lib.require_gpu()
    fx = Fixture("baxter", "poly", 1, 2, 5, seed=2)
    model = fx.model(ops)
    opt, dopt, mg = _opts(0.05), _dopts(0.11, 16), _t(fx.margin)
    st, b = dense_state(model, fx.limits, fx.paths)
    keep = {k: v.clone() for k, v in b.items()}
    dense_run(lib, model, st, opt, dopt, dense_io(b), mg, 1, 0)
    torch.cuda.synchronize()
    for k in b:
        assert torch.equal(b[k], keep[k]), k
    st0, b0 = dense_state(model, fx.limits, fx.paths[:0])
    dense_run(lib, model, st0, opt, dopt, dense_io(b0), mg, 1, 4)
    torch.cuda.synchronize()


def test_dense_adam_run(ops):
    """traj.DenseAdamRun is the C loop behind buffers"""
    from diffco_amd import _lib, traj
    lib = _lib.require_gpu()
    R, W = 3, 6
    fx = Fixture("baxter", "poly", 1, R, W, seed=17, quirks=False)
    model = fx.model(ops)
    run = traj.DenseAdamRun(model, fx.limits, torch.from_numpy(fx.paths), 0.05, fx.margin.tolist(), 0.11, max_speed=0.3,
                            max_samples=16, history=True)
    run.run(2)
    run.run(1)
    st, b = dense_state(model, fx.limits, fx.paths)
    dense_run(lib, model, st, _opts(0.05), _dopts(0.11, 16), dense_io(b), _t(fx.margin), 1, 3)
    torch.cuda.synchronize()
    assert torch.equal(run.t["path"], b["path"]) and torch.equal(run.n_checks, b["n_checks"])
    assert [tuple(h.shape) for h in run.history] == [(2, R, W, fx.dof), (1, R, W, fx.dof)]
    assert torch.equal(run.history[1][0], b["path"]) and not run.all_done() and not bool(run.over_bound().any())
    summ, bvp, lop = run.finish()
    run.close()
    assert summ.shape == (R, 5) and summ[:, 3].tolist() == [3, 3, 3] and summ[:, 4].tolist() == b["n_checks"].tolist()


def _baxter_problem():
    from diffco_amd import kernel
    from diffco_amd.kernel_perceptrons import DiffCo
    from helpers import load, make_robot
    d = load("optim_adam_baxter")
    rob = make_robot("baxter_left")
    dc = DiffCo(transform=rob.fkine)
    dc.support_points = torch.from_numpy(d["sup_q"])
    dc.support_transformed = rob.fkine(dc.support_points)
    dc.rbf_kernel, dc.rbf_nodes = kernel.Polyharmonic(1, 1.0), torch.from_numpy(d["weights"])
    return rob, dc, torch.from_numpy(d["start"]), torch.from_numpy(d["target"])


def _restarts(rob, start, target, options):
    from diffco_amd.optim import _PathProblem
    torch.manual_seed(options["seed"])
    prob = _PathProblem(rob, start, target, options)
    return torch.stack([prob.make_init(t).clone() for t in range(options["NUM_RE_TRIALS"])])


@pytest.mark.parametrize("margin", [-1e3, 0.0], ids=["never-valid", "feasible"])
def test_fused_optimizer_honours_dense_check(ops, margin):
    """fused_adam_traj_optimize with options['dense_check']: the record, its default sample bound, cnt_check from n_checks and
    the selection policy, against a DenseAdamRun on the same restarts"""
    from diffco_amd import fused_adam_traj_optimize, traj
    rob, dc, start, target = _baxter_problem()
    opts = {"N_WAYPOINTS": 20, "NUM_RE_TRIALS": 4, "MAXITER": 30, "max_speed": 0.3, "seed": 77, "history": False,
            "extra_optimizer_options": {"lr": 0.05}, "safety_margin": margin, "dense_check": True}
    rec = fused_adam_traj_optimize(rob, dc.poly_score, start, target, dict(opts))
    assert {"start_cfg", "target_cfg", "cnt_check", "cost", "time", "success", "seed", "solution", "trial", "cnt_check_batched",
            "iterations_enqueued", "dense_check", "dense_max_samples", "dense_frozen_on_bound"} <= set(rec)
    inits = _restarts(rob, start, target, opts)
    bound = ops.motion_bound(inits[:, :-1].reshape(-1, 7).float().cuda(), inits[:, 1:].reshape(-1, 7).float().cuda(), 0.3)
    assert rec["dense_max_samples"] == 2 * bound + 8 and rec["dense_frozen_on_bound"] == [] and rec["dense_check"] is True
    run = traj.DenseAdamRun(traj._resolve_model(dc.poly_score), rob.limits, inits, 0.05, margin, 0.3,
                            max_samples=rec["dense_max_samples"])
    run.run(30)
    summ, bvp, lop = run.finish()
    run.close()
    t, found = rec["trial"], rec["success"]
    assert found == bool(torch.isfinite(summ[:, 0]).any())
    if margin < 0:
        assert not found and t == int(torch.argmin(summ[:, 1]))
    want = (bvp if found else lop)[t].double().cpu().numpy()
    assert np.array_equal(np.array(rec["solution"]), want)
    assert rec["cnt_check_batched"] == int(summ[:, 4].sum()) and rec["cnt_check_batched"] >= int(summ[:, 3].sum()) * 20
    assert rec["cnt_check"] == int(summ[:t + 1, 4].sum() if found else summ[:, 4].sum())


def test_fused_optimizer_dense_bound_and_wrap(ops):
    from diffco_amd import fused_adam_traj_optimize
    rob, dc, start, target = _baxter_problem()
    opts = {"N_WAYPOINTS": 20, "NUM_RE_TRIALS": 4, "MAXITER": 10, "max_speed": 0.3, "seed": 77, "history": False,
            "extra_optimizer_options": {"lr": 0.05}, "safety_margin": -1e3, "dense_check": True}
    # a tight bound: the random restarts' long segments need more samples - they freeze where they stand and are named
    inits = _restarts(rob, start, target, opts)
    need = torch.ceil((inits[:, 1:] - inits[:, :-1]).norm(dim=2).max(dim=1).values / 0.3)
    tight = int(need[0]) + 4     # (three steps of lr = 0.05 lengthen a segment by at most 3 * 2 sqrt(7) * 0.05 = 0.8: three samples)
    assert int(need[1:].min()) > tight
    rec = fused_adam_traj_optimize(rob, dc.poly_score, start, target, dict(opts, dense_max_samples=tight, MAXITER=3))
    assert rec["dense_max_samples"] == tight and rec["dense_frozen_on_bound"] == [1, 2, 3]
    assert rec["trial"] == 0 and not rec["success"] and rec["cnt_check"] == rec["cnt_check_batched"] > 0
    # wrap=: every joint on the circle - the random restarts' segments longer than pi in a joint go the short way: fewer samples
    plain = fused_adam_traj_optimize(rob, dc.poly_score, start, target, dict(opts, dense_max_samples=200))
    short = fused_adam_traj_optimize(rob, dc.poly_score, start, target, dict(opts, dense_max_samples=200), wrap=[True] * 7)
    assert plain["dense_frozen_on_bound"] == short["dense_frozen_on_bound"] == []
    assert short["cnt_check_batched"] < plain["cnt_check_batched"]
    same = fused_adam_traj_optimize(rob, dc.poly_score, start, target, dict(opts, dense_max_samples=200), wrap=0)
    assert same["solution"] == plain["solution"] and same["cnt_check"] == plain["cnt_check"]
    with pytest.raises(ValueError, match="dense_check"):
        fused_adam_traj_optimize(rob, dc.poly_score, start, target, dict(opts, dense_check=False), wrap=[True] * 7)
