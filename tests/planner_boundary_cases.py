"""Shared by tools/record_planner_host_parent.py and the two tests that hold the library to its recordings
(test_planner_boundary_recorded.py on the CPU, test_gpu_work_bytes_recorded.py on the GPU): the cases, and how one is run.

CPU part - the order of the argument checks of the three lockstep planners (dcx_rrt_connect_run, dcx_path_shortcut_run,
dcx_path_shortcut_partial_run).  A fault is one wrong value in one argument, taken from the lists of test_rrt_abi.py,
test_shortcut_abi.py and test_shortcut_partial_abi.py plus R = 2^31 (unsupported); a case is one fault, or two faults in
DIFFERENT arguments (a field of the options counts as an argument of its own; the options pointer itself goes with none of its
fields).  With two faults the first failing check names the error, so (rc, message) over all pairs pins the order of the checks.
Every case holds a fault, so every call is refused before any device work: the stand-in model and the made-up addresses are
never read.  The fault-free call would reach a launch, and boundary_cases() refuses to emit it.

GPU part - every dcx_*_work_bytes over a grid, on three real models (the stand-in model reads dof = C = Dt = 0, where most terms
of most layouts vanish)."""
import itertools
import math

import test_rrt_abi as rrt_abi
import test_shortcut_abi as shortcut_abi
import test_shortcut_partial_abi as partial_abi

GOLDEN_BOUNDARY = "planner_boundary_parent.json"
GOLDEN_WORK_BYTES = "planner_work_bytes_parent.json"

# (argument, the _run keyword it sets, value): ("opt.x", "opt", {...}) sets fields of _opts(); "need - 1" is resolved by run_case
_COMMON = [("model", "model", None), ("opt", "opt", False), ("state", "state", False), ("work", "work", 0), ("R", "R", -1),
           ("R", "R", 1 << 31), ("T", "T", -1), ("work_bytes", "work_bytes", "need - 1"),
           ("opt.max_step", "opt", dict(max_step=0.0)), ("opt.max_step", "opt", dict(max_step=-1.0)),
           ("opt.max_step", "opt", dict(max_step=math.nan)), ("opt.max_samples", "opt", dict(max_samples=0)),
           ("opt.slots", "opt", dict(slots=0)), ("opt.slots", "opt", dict(slots=17)),
           ("opt.mask", "opt", dict(mask=1)), ("opt.mask", "opt", dict(mask=1 << 63)),
           ("opt.reserved", "opt", dict(reserved=(1, 0))), ("opt.reserved", "opt", dict(reserved=(0, 1)))]
_RRT = [("samples", "samples", 0), ("round0", "round0", -1), ("round0", "round0", (1 << 31) - 2),
        ("opt.rng", "opt", dict(rng=0.0)), ("opt.rng", "opt", dict(rng=-1.0)), ("opt.rng", "opt", dict(rng=math.nan)),
        ("opt.cap", "opt", dict(cap=0)), ("opt.cap", "opt", dict(cap=(1 << 20) + 1)), ("opt.r0", "opt", dict(r0=1))]
_SHORTCUT = [("draws", "draws", 0), ("opt.W", "opt", dict(W=0)), ("opt.W", "opt", dict(W=65537))]

# call -> (its ABI test module: _run, _opts, _state; the size query and the arguments `need` is asked for; the faults)
CALLS = {
    "dcx_rrt_connect_run": (rrt_abi, rrt_abi, "dcx_rrt_work_bytes", (8, 4),
                            _COMMON + _RRT + [("state", "state", {f: True}) for f in rrt_abi._STATE]),
    "dcx_path_shortcut_run": (shortcut_abi, shortcut_abi, "dcx_path_shortcut_work_bytes", (8, 4),
                              _COMMON + _SHORTCUT + [("state", "state", {f: True}) for f in shortcut_abi._STATE]),
    "dcx_path_shortcut_partial_run": (partial_abi, shortcut_abi, "dcx_path_shortcut_partial_work_bytes", (8, 4, 32),
                                      _COMMON + _SHORTCUT + [("state", "state", {f: True}) for f in shortcut_abi._STATE]),
}


def _same_argument(a, b):
    return a == b or (a == "opt" and b.startswith("opt.")) or (b == "opt" and a.startswith("opt."))


def boundary_cases(call):
    """[(case id, faults)]: every single fault and every unordered pair of faults in different arguments - never no fault"""
    faults = CALLS[call][4]
    cases = [(f,) for f in faults] + [p for p in itertools.combinations(faults, 2) if not _same_argument(p[0][0], p[1][0])]
    assert all(len(c) >= 1 for c in cases), "a case without a fault would reach a launch"
    out = [(" & ".join(f"{arg}={value!r}" for arg, _, value in c), c) for c in cases]
    assert len({i for i, _ in out}) == len(out)
    return out


def run_case(lib, call, model, faults):
    """(rc, message) of `call` with the faults applied to the ABI test's own defaults"""
    run_mod, opt_mod, size_fn, size_args, _ = CALLS[call]
    assert len(faults) >= 1, "a case without a fault would reach a launch"
    kw, opt = {}, {}
    for _, key, value in faults:
        if key == "opt" and value is not False:
            opt.update(value)
        elif key == "state" and value is not False:
            kw["state"] = opt_mod._state(**value)
        elif value == "need - 1":
            kw[key] = getattr(lib, size_fn)(model, *size_args) - 1
        else:
            kw[key] = value
    if opt:
        kw["opt"] = opt_mod._opts(**opt)
    rc = run_mod._run(lib, kw.pop("model", model), **kw)
    return [int(rc), lib.dcx_last_error().decode()]


def run_boundary(lib):
    """{call: {case id: [rc, message]}} and {size query: {arguments: bytes}} on the stand-in model"""
    keep, m = rrt_abi._fake_model()
    out = {call: {cid: run_case(lib, call, m, faults) for cid, faults in boundary_cases(call)} for call in CALLS}
    sizes = {}
    for fn, grid in STAND_IN_GRIDS.items():
        sizes[fn] = {repr(a): int(getattr(lib, fn)(*(m if x == "m" else x for x in a))) for a in grid}
    return out, sizes


# the grids of the ABI tests' size queries ("m": the stand-in model)
_RS = [("m", R, 4) for R in (0, 1, 7, 8, 64, 100, 1000, 1 << 20)] + [("m", 100, P) for P in (1, 2, 5, 16)]
_BAD = [(None, 8, 4), ("m", -1, 4), ("m", 8, 0), ("m", 8, 17), ("m", 1 << 31, 4)]
STAND_IN_GRIDS = {
    "dcx_rrt_work_bytes": _BAD + _RS,
    "dcx_path_shortcut_work_bytes": _BAD + _RS,
    "dcx_path_shortcut_partial_work_bytes":
        [a + (32,) for a in _BAD] + [("m", 8, 4, 0), ("m", 8, 4, -1), ("m", 8, 4, 65537), ("m", 8, 4, 32)] +
        [a + (4096,) for a in _RS] + [("m", 100, 4, W) for W in (1, 3, 32, 2048, 2049, 65536)],
}

# ---- GPU part ------------------------------------------------------------------------------------------------------------
MODELS = ("cfg1_planar2_rq", "cfg2_baxter_rq", "cfg3_baxter_rq_c5")   # dof 2, one class; dof 7, one class; five classes
_N = (0, 1, 63, 64, 65, 1000)          # E, B and R
_SAMPLES = (1, 7, 64)
_SLOTS = (1, 4, 16)
_W = (1, 32, 2048, 2049)               # either side of kResampleLdsWaypoints
# size query -> its arguments behind the model (dcx_path_resample_work_bytes takes no model)
WORK_BYTES_GRIDS = {
    "dcx_escape_work_bytes": [(n,) for n in _N],
    "dcx_motion_work_bytes": [(n,) for n in _N],
    "dcx_motion_worst_work_bytes": [(n,) for n in _N],
    "dcx_motion_band_work_bytes": list(itertools.product(_N, _SAMPLES)),
    "dcx_motion_cost_work_bytes": list(itertools.product(_N, _SAMPLES)),
    "dcx_traj_dense_work_bytes": list(itertools.product(_N, _W, _SAMPLES)),
    "dcx_rrt_work_bytes": list(itertools.product(_N, _SLOTS)),
    "dcx_path_shortcut_work_bytes": list(itertools.product(_N, _SLOTS)),
    "dcx_path_shortcut_partial_work_bytes": list(itertools.product(_N, _SLOTS, _W)),
    "dcx_path_resample_work_bytes": list(itertools.product(_N, _W)),
}


def build_models(ops):
    """{name: ScoreModel} of MODELS, built as the motion tests build theirs (motion_wrap_helpers.fixture_model)"""
    import torch
    from motion_wrap_helpers import fixture_model
    models = {}
    for name in MODELS:
        d, desc, (kind, p0, p1), sup, W = fixture_model(name)
        t = lambda a: torch.as_tensor(a, dtype=torch.float32, device="cuda")
        models[name] = ops.ScoreModel(desc, kind, p0, p1, t(sup), t(W))
        assert (d["q"].shape[1], W.shape[1]) == {MODELS[0]: (2, 1), MODELS[1]: (7, 1), MODELS[2]: (7, 5)}[name]
    return models


def run_work_bytes(lib, models):
    """{model: {size query: {arguments: bytes}}}; nothing is launched"""
    out = {}
    for name, m in models.items():
        out[name] = {}
        for fn, grid in WORK_BYTES_GRIDS.items():
            head = () if fn == "dcx_path_resample_work_bytes" else (m._h,)
            out[name][fn] = {repr(a): int(getattr(lib, fn)(*head, *a)) for a in grid}
    return out
