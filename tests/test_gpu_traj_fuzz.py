"""Shape fuzz of the Adam trajectory kernels against a float64 referee: dcx_traj_adam_run (C = 1) and dcx_traj_adam_run_mc
(C > 1, per-class margins) at every compiled feature width, class counts 1 .. 8, every kernel family and FK kind, path lengths
on both sides of the one-wave boundary.  The case table, the inputs (tie-free hinges by construction) and the referee are
tests/traj_fuzz_helpers.py; tests/test_traj_referee.py checks the referee against central differences and what the table covers.

Every launch form of a case is judged against the SAME referee: the rule's own choice, the launch loop (traj_fused = 0), the
cluster form (traj_ys = 2), the direct sweep (xf = 0) where the expanded one exists, one forced wave count.  Per form:
 (a) one step from zero moments: loss terms, the gradient through adam_m, adam_v, the lr * sign(g) move;
 (b) one step from caller-supplied warm moments at first_step = 5: m, v and the new path, where the update is smooth in g;
 (c) invariants: endpoints, the best-so-far records, a path handed in as done, sentinel rows behind every [R, W, dof] array;
 (d) three iterations in one call = three calls of one iteration, bit for bit.
Then (e): the persistent kernel against the launch loop under pinned slices, bit for bit, on the rows that have both."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import kernel_family, relerr, template_d_for
from traj_fuzz_helpers import OPT_FIELDS, TRAJ_CASES, adam_update, case_id, has_persistent_form, traj_reference, traj_setup

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = 123.25
ARRAYS = ("path", "adam_m", "adam_v", "lowest_path", "best_valid_path")          # [R, W, dof], one sentinel row behind each
COMPARED = ARRAYS + ("stats", "lowest_loss", "lowest_obj", "best_valid_obj", "done", "steps")


def _xf_applies(Dt, C_, kf):
    """score_kernel.h xf_applies at the model's compiled class count"""
    Cc = C_ if C_ <= 1 else 4 if C_ <= 4 else 5 if C_ == 5 else 8
    used = Dt + Cc + (1 if Cc > 1 else 0)
    parts = 0 if 4 * used <= 56 else (used + 37) // 38
    return kf in (0, 1) and used + 1 <= 38 and parts <= 1


def _model(x):
    from diffco_amd import _ops
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")  # noqa: E731
    return _ops.ScoreModel(x["desc"], *x["kern"], t(x["sup"]), t(x["weights"]))


def _state(model, x, m0=None, v0=None, done=None, lowest_loss=None):
    """device buffers + ctypes state of a case's R paths; every [R, W, dof] array (and col_grad) carries one more path's worth of
    sentinel rows behind it"""
    from diffco_amd import _lib
    paths = x["paths"]
    R, W, dof = paths.shape
    Cn = model.C
    dev = model.dev
    f32 = dict(device=dev, dtype=torch.float32)

    def padded(a):
        full = torch.full((R + 1, W, dof), SENTINEL, **f32)
        full[:R] = torch.as_tensor(np.asarray(a, F), **f32)
        return full
    zero = np.zeros_like(paths)
    b = dict(path=padded(paths), adam_m=padded(zero if m0 is None else m0), adam_v=padded(zero if v0 is None else v0),
             limits=torch.as_tensor(x["limits32"], **f32).contiguous(),
             col_score=torch.full(((R + 1) * W * Cn,), SENTINEL, **f32), col_grad=torch.full(((R + 1) * W, dof), SENTINEL, **f32),
             stats=torch.full((R, 8), -7.0, **f32),
             lowest_loss=torch.as_tensor(np.full(R, np.inf, F) if lowest_loss is None else np.asarray(lowest_loss, F), **f32),
             lowest_obj=torch.full((R,), float("inf"), **f32), lowest_path=padded(paths),
             best_valid_obj=torch.full((R,), float("inf"), **f32), best_valid_path=padded(paths),
             done=torch.as_tensor(np.zeros(R, np.int32) if done is None else np.asarray(done, np.int32), device=dev),
             steps=torch.zeros(R, device=dev, dtype=torch.int32))
    st = _lib.TrajState(R, W, *(C.c_void_p(t.data_ptr()) for t in b.values()))
    return st, b


def _run(lib, model, x, st, first_step, n_iters, **over):
    from diffco_amd import _lib
    o = dict(x["opts"], **over)
    opt = _lib.TrajOpts(*[o[k] for k in OPT_FIELDS])
    stream = C.c_void_p(torch.cuda.current_stream(model.dev).cuda_stream)
    if model.C == 1:
        _lib.check(lib.dcx_traj_adam_run(model._h, C.byref(st), C.byref(opt), first_step, n_iters, stream))
    else:
        _lib.check(lib.dcx_traj_adam_run_mc(model._h, C.byref(st), C.byref(opt), model.margins(x["margin"].tolist()), first_step,
                                            n_iters, stream))
    torch.cuda.synchronize()


def _host(b):
    return {k: v.detach().cpu().numpy().copy() for k, v in b.items()}


def _ulp(a):
    return np.spacing(np.abs(np.asarray(a, F))).astype(np.float64)


def _check_sentinels(h, R, what):
    for k in ARRAYS:
        assert (h[k][R] == SENTINEL).all(), (what, k, "the lanes past W, or a block past R, wrote")
    assert (h["col_grad"].reshape(R + 1, -1)[R] == SENTINEL).all(), (what, "col_grad")
    assert (h["col_score"].reshape(R + 1, -1)[R] == SENTINEL).all(), (what, "col_score")


def _check_records(h0, h, r, valid_tol, grad_tol, what):
    """the lowest-loss / best-valid / stop records of path r follow traj_kernels.hip's rule, given the kernel's own stats"""
    loss, obj, con, gn = (h["stats"][r, i] for i in range(4))
    if loss < h0["lowest_loss"][r]:
        assert h["lowest_loss"][r] == loss and h["lowest_obj"][r] == obj, what
        assert np.array_equal(h["lowest_path"][r], h["path"][r]), what
    else:
        assert h["lowest_loss"][r] == h0["lowest_loss"][r] and h["lowest_obj"][r] == h0["lowest_obj"][r], what
        assert np.array_equal(h["lowest_path"][r], h0["lowest_path"][r]), what
    valid = con <= F(valid_tol)
    if valid and obj < h0["best_valid_obj"][r]:
        assert h["best_valid_obj"][r] == obj and np.array_equal(h["best_valid_path"][r], h["path"][r]), what
    else:
        assert h["best_valid_obj"][r] == h0["best_valid_obj"][r], what
        assert np.array_equal(h["best_valid_path"][r], h0["best_valid_path"][r]), what
    assert h["done"][r] == (1 if (valid and gn < F(grad_tol)) else 0), what


def _legs(case, x):
    Dt, fam = template_d_for(case.D), kernel_family(*x["kern"])
    legs = [("rule", {}), ("loop", {"traj_fused": 0}), ("cluster", {"traj_ys": 2, "min_rows": 1})]
    # the direct sweep where the rule's route would expand: Polyharmonic(1) everywhere; RQKernel(p = 2) only where the route is the
    # launch loop (the persistent kernel keeps RQ models in the direct form, the sweep kernel's rule may expand them)
    if _xf_applies(Dt, case.C, fam) and (fam == 1 or not has_persistent_form(case)):
        legs.append(("xf0", {"xf": 0}))
    # one forced wave count: 2; 4 for two-chain DH arms - the block size whose waves hold phase R1 of the several-wave J^T for
    # one chain only (regression: traj_run once took that route there and left the second chain's gradient wrong)
    two_chains = int(x["desc"].kind) == 2 and int(x["desc"].n_chains) == 2
    legs.append(("nw", {"nw": 4 if two_chains else 2}))
    return legs


def _cold_step(lib, model, case, x, what):
    """(a) and the invariants of (c) on one step from zero moments"""
    ref, _, _, _ = traj_reference(case, False)
    R, W, dof = x["paths"].shape
    o = x["opts"]
    st, b = _state(model, x)
    h0 = _host(b)
    _run(lib, model, x, st, 1, 1)
    h = _host(b)
    worst = dict(stats=0.0, g=0.0, v=0.0, move=0.0)
    for r in range(R):
        rr = ref[r]
        e = relerr(h["stats"][r, :7], rr["stats"])
        worst["stats"] = max(worst["stats"], e / 5e-5)
        assert e < 5e-5, (what, r, h["stats"][r, :7], rr["stats"])
        assert h["stats"][r, 7] == 0 and h["steps"][r] == 1, (what, r)
        gmax = np.abs(rr["g"]).max()
        g_bar = 2e-5 * gmax
        err = np.abs(h["adam_m"][r].astype(np.float64) / (1.0 - o["beta1"]) - rr["g"]).max()
        worst["g"] = max(worst["g"], err / g_bar if g_bar > 0 else float(err > 0))
        assert err <= g_bar, (what, r, err, g_bar)
        v_bar = (1.0 - o["beta2"]) * (2.0 * np.abs(rr["g"]) * g_bar + g_bar * g_bar)
        err = np.abs(h["adam_v"][r].astype(np.float64) - (1.0 - o["beta2"]) * rr["g"] ** 2)
        worst["v"] = max(worst["v"], float((err / np.maximum(v_bar, 1e-300)).max()) if gmax > 0 else float(err.max() > 0))
        assert (err <= v_bar).all(), (what, r, float(err.max()))
        big = np.abs(rr["g"]) > 1e-4 * gmax
        move = h["path"][r].astype(np.float64) - x["paths"][r].astype(np.float64)
        if big.any():
            err = np.abs(move + o["lr"] * np.sign(rr["g"]))[big].max()
            worst["move"] = max(worst["move"], err / 1e-5)
            assert err < 1e-5, (what, r, err)
        assert np.array_equal(h["path"][r, 0], x["paths"][r, 0]) and np.array_equal(h["path"][r, -1], x["paths"][r, -1]), (what, r)
        _check_records(h0, h, r, o["valid_tol"], o["grad_tol"], (what, r))
    _check_sentinels(h, R, what)
    return worst


def _warm_step(lib, model, case, x, what):
    """(b) and the invariants of (c) on one step from warm moments at first_step = 5: every live path becomes valid and stops
    (valid_tol, grad_tol large), path 1 starts from a lowest loss it cannot beat, the last path is handed in as done"""
    ref, m0, v0, t = traj_reference(case, True)
    R, W, dof = x["paths"].shape
    o = x["opts"]
    done, lowest = np.zeros(R, np.int32), np.full(R, np.inf, F)
    if R >= 3:
        done[R - 1] = 1
        lowest[1] = 0.0
    st, b = _state(model, x, m0, v0, done, lowest)
    h0 = _host(b)
    _run(lib, model, x, st, t, 1, valid_tol=1e9, grad_tol=1e9)
    h = _host(b)
    worst = dict(m=0.0, v=0.0, q=0.0)
    for r in range(R):
        if done[r]:   # untouched in every buffer
            for k in COMPARED:
                assert np.array_equal(h[k][r], h0[k][r]), (what, r, k)
            continue
        rr = ref[r]
        q0 = x["paths"][r].astype(np.float64)
        g_bar = 2e-5 * np.abs(rr["g"]).max()
        # first-order propagation of g_bar through the scalar update, the derivative numerically from the referee's formula
        hh = max(1e-3 * g_bar, 1e-12)
        up = adam_update(q0, rr["g"] + hh, m0[r].astype(np.float64), v0[r].astype(np.float64), t, o)
        dn = adam_update(q0, rr["g"] - hh, m0[r].astype(np.float64), v0[r].astype(np.float64), t, o)
        for name, got, want, a, c, scale in (("m", h["adam_m"][r], rr["m"], up[0], dn[0], rr["m"]),
                                             ("v", h["adam_v"][r], rr["v"], up[1], dn[1], rr["v"]),
                                             ("q", h["path"][r], rr["q_new"], up[2], dn[2], q0)):
            tol = np.abs(a - c) / (2 * hh) * g_bar + 4.0 * _ulp(scale)
            err = np.abs(got.astype(np.float64) - want)
            worst[name] = max(worst[name], float((err / tol).max()))
            assert (err <= tol).all(), (what, r, name, float((err / tol).max()), float(err.max()))
        assert h["steps"][r] == 1 and h["stats"][r, 7] == 0, (what, r)
        assert relerr(h["stats"][r, :7], rr["stats"]) < 5e-5, (what, r)
        assert np.array_equal(h["path"][r, 0], x["paths"][r, 0]) and np.array_equal(h["path"][r, -1], x["paths"][r, -1]), (what, r)
        _check_records(h0, h, r, 1e9, 1e9, (what, r))
        assert h["done"][r] == 1 and h["best_valid_obj"][r] == h["stats"][r, 1], (what, r)
    if R >= 3:
        assert h["lowest_loss"][1] == 0.0 and np.array_equal(h["lowest_path"][1], h0["lowest_path"][1]), what
    _check_sentinels(h, R, what)
    return worst


def _iterate(lib, model, x, calls, **over):
    """the compared buffers after `calls` = [(first_step, n_iters), ...] from zero moments"""
    st, b = _state(model, x)
    for first, n in calls:
        _run(lib, model, x, st, first, n, **over)
    h = _host(b)
    _check_sentinels(h, len(x["paths"]), calls)
    R = len(x["paths"])
    return dict({k: h[k] for k in COMPARED}, col_score=h["col_score"].reshape(R + 1, -1)[:R])


@pytest.mark.parametrize("case", TRAJ_CASES, ids=case_id)
def test_traj_adam_shapes(case, knob):
    from diffco_amd import _lib
    lib = _lib.require_gpu()
    x = traj_setup(case)
    model = _model(x)
    for name, knobs in _legs(case, x):
        for k, v in knobs.items():
            knob(k, v)
        what = (case_id(case), name)
        wa = _cold_step(lib, model, case, x, what)
        wb = _warm_step(lib, model, case, x, what)
        # (d) state crosses a launch boundary through HBM alone: three iterations in one call = three calls of one
        one = _iterate(lib, model, x, [(1, 3)], grad_tol=0.0)
        three = _iterate(lib, model, x, [(1, 1), (2, 1), (3, 1)], grad_tol=0.0)
        for k in COMPARED:
            assert np.array_equal(one[k], three[k]), (what, "3 x 1 against 1 x 3", k)
        assert (one["steps"] == 3).all(), what
        for k in knobs:
            knob(k, -1)
        print("TRAJFUZZ", case_id(case), name, " ".join(f"{k}={v:.3g}" for k, v in {**wa, **{'w' + k: v for k, v in wb.items()}}.items()))
    # the route traj_run took is read off col_score: the launch loop writes it, the persistent kernel never touches it
    if not case.bitwise:
        assert not (_iterate(lib, model, x, [(1, 1)])["col_score"] == SENTINEL).any(), (case_id(case), "a persistent launch ran", case.reason)
        return
    # (e) the persistent kernel against the launch loop on the same slices: one workgroup per path, nw waves in both (2 where
    # the narrow widths' partial rows fit the sweep's 64 KB block whatever the transform, else 1), RQ kernels in the direct form
    knob("nw", 2 if template_d_for(case.D) <= 24 else 1)
    knob("ys", 1)
    knob("traj_ys", 1)
    if x["kern"][0] == 0:
        knob("xf", 0)
    outs = []
    for fused in (0, 1):
        knob("traj_fused", fused)
        outs.append(_iterate(lib, model, x, [(1, 2), (3, 1)], grad_tol=0.0))
    assert not (outs[0]["col_score"] == SENTINEL).any() and (outs[1]["col_score"] == SENTINEL).all(), (case_id(case), "routes")
    for k in COMPARED:
        assert np.array_equal(outs[0][k], outs[1][k]), (case_id(case), "persistent against loop", k,
                                                        float(np.abs(outs[0][k].astype(np.float64) - outs[1][k]).max()))


def test_a_path_too_long_for_the_transform_is_refused_before_any_launch():
    """the step kernel's carve of a 96-wide keypoint body at W = 1024 (16 slabs of 64 waypoints: ~ 840 KB) exceeds a CU's LDS:
    DCX_ERR_UNSUPPORTED from host arithmetic alone, path and moments untouched, from the loop entry and the step entry alike"""
    from diffco_amd import _lib
    from traj_fuzz_helpers import TrajCase
    lib = _lib.require_gpu()
    x = dict(traj_setup(TrajCase("se3", 96, 1, 1, 8, 1)))
    rng = np.random.default_rng(7)
    x["paths"] = rng.uniform(-1.0, 1.0, (1, 1024, x["dof"])).astype(F)
    model = _model(x)
    m0 = rng.standard_normal(x["paths"].shape).astype(F)
    st, b = _state(model, x, m0, np.abs(m0))
    h0 = _host(b)
    with pytest.raises(_lib.DcxUnsupported, match="n_waypoints is too large"):
        _run(lib, model, x, st, 1, 3)
    opt = _lib.TrajOpts(*[x["opts"][k] for k in OPT_FIELDS])
    with pytest.raises(_lib.DcxUnsupported, match="n_waypoints is too large"):
        _lib.check(lib.dcx_traj_adam_step(model.dev.index, C.byref(x["desc"]), C.byref(st), C.byref(opt), 1, None))
    torch.cuda.synchronize()
    h = _host(b)
    for k in h:
        assert np.array_equal(h[k], h0[k]), k
    # a length the carve still holds goes through (W = 65: two slabs)
    x["paths"] = x["paths"][:, :65].copy()
    st, b = _state(model, x)
    _run(lib, model, x, st, 1, 1)
    assert _host(b)["steps"].tolist() == [1]
