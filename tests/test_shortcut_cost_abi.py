"""CPU-side checks of the boundary of the shortcuts under the clearance objective (dcx_path_shortcut_run_cost,
dcx_path_shortcut_partial_run_cost and their size queries): the symbols exist and the version stays 109, the header and the
ctypes table declare the same arguments, every new argument error - and every error of the calls they extend - is reported before
anything touches a device, the workspace sizes are 0 for refused arguments and non-decreasing, and the header states the
contract - on a machine without a GPU.  (The length modes' own sizes are pinned by tests/golden/planner_work_bytes_parent.json
on real models: test_gpu_work_bytes_recorded.py.)"""
import ctypes
import math

import pytest

from test_rrt_abi import HEADER, _declared, _fake_model
from test_rrtstar_cost_abi import _cost
from test_shortcut_abi import _STATE, _opts, _state

_NAMES = ["dcx_path_shortcut_cost_work_bytes", "dcx_path_shortcut_run_cost", "dcx_path_shortcut_partial_cost_work_bytes",
          "dcx_path_shortcut_partial_run_cost"]
_RUNS = ["dcx_path_shortcut_run_cost", "dcx_path_shortcut_partial_run_cost"]


@pytest.mark.parametrize("name", _NAMES)
def test_symbols_exist_and_version_stays(name):
    from diffco_amd import _lib
    res, args = _declared(name)
    assert _lib.SYMBOLS[name][0] is res
    assert list(_lib.SYMBOLS[name][1]) == args
    lib = _lib.load()
    assert hasattr(lib, name)
    assert lib.dcx_version() == 109


def test_the_calls_take_the_length_modes_arguments_with_seg_and_the_cost_options():
    base = _declared("dcx_path_shortcut_run")
    for name in _RUNS:
        res, args = _declared(name)
        # seg after the state, the cost options after the options
        assert res is base[0] and args == base[1][:2] + [ctypes.c_void_p] + base[1][2:6] + [ctypes.c_void_p] + base[1][6:]
    assert _declared("dcx_path_shortcut_cost_work_bytes") == _declared("dcx_path_shortcut_work_bytes")
    assert _declared("dcx_path_shortcut_partial_cost_work_bytes") == _declared("dcx_path_shortcut_partial_work_bytes")


def test_header_states_the_contract_under_109():
    src = open(HEADER).read()
    at = src.index("Path shortcuts under the clearance objective:")
    end = src.index("/* ---- roadmap queries")
    assert src.index("dcx_path_shortcut_partial_run(const") < at < src.index("dcx_path_shortcut_run_cost(const") < end
    body = src[at:end]
    for word in ("dcx_rrtstar_cost_opts", "C = L * (1 + gain * fmaxf(w + band, +0))", "rounded alone, never contracted", "seg [R, W] float",
                 "+inf where it is not", "1. pick", "2. sweep", "3. price", "4. apply", "5. compact", "5. apply and rewrite",
                 "ascending order starting from seg[i]", "new = (C0 + C1) + C2", "j_p <= i_q || j_q <= i_p", "A zero-length piece",
                 "gain == 0 gives C == L bit for bit", "never-lengthening", "dcx_motion_worst_work_bytes", "non-decreasing",
                 "NULL seg with R > 0", "2^24 - 1", "can be\n *   captured"):
        assert word in body, word
    assert "#define DCX_VERSION 109" in src
    # the length modes' structs are as they were: the objective travels beside them
    assert "    int64_t  reserved[2];  /* 0 " in src[src.index("typedef struct dcx_shortcut_opts"):][:900]


def _run(name):
    def run(lib, model, R=8, T=2, opt=None, cost=None, state=None, seg=1, draws=1, work=1, work_bytes=1 << 40):
        # (the addresses are never read: every case below is refused, or has nothing to do, before any device work)
        p = ctypes.c_void_p
        opt = _opts() if opt is None else opt
        cost = _cost() if cost is None else cost
        state = _state() if state is None else state
        return getattr(lib, name)(model, ctypes.byref(state) if state is not False else None, p(seg), R, p(draws), T,
                                  ctypes.byref(opt) if opt is not False else None, ctypes.byref(cost) if cost is not False else None,
                                  None, p(work), work_bytes, None)
    return run


_ERRORS = [
    # the objective's
    (dict(seg=0), "seg is NULL"),
    (dict(cost=False), "cost options are NULL"),
    (dict(cost=_cost(mode=0)), "cost mode must be DCX_RRTSTAR_COST_PEAK"),
    (dict(cost=_cost(mode=2)), "cost mode must be DCX_RRTSTAR_COST_PEAK"),
    (dict(cost=_cost(gain=-1.0)), "cost gain must be >= 0"),
    (dict(cost=_cost(gain=math.nan)), "cost gain must be >= 0"),
    (dict(cost=_cost(band=-0.5)), "cost band must be >= 0"),
    (dict(cost=_cost(band=math.nan)), "cost band must be >= 0"),
    (dict(cost=_cost(r0=1)), "reserved fields of the cost options must be 0"),
    (dict(cost=_cost(reserved=(1, 0))), "reserved fields of the cost options must be 0"),
    (dict(cost=_cost(reserved=(0, 1))), "reserved fields of the cost options must be 0"),
    # the length modes'
    (dict(model=None), "model is NULL"),
    (dict(opt=False), "options are NULL"),
    (dict(state=False), "state or one of its pointers is NULL"),
    (dict(draws=0), "draws is NULL"),
    (dict(work=0), "work is NULL"),
    (dict(R=-1), "R < 0"),
    (dict(T=-1), "T < 0"),
    (dict(opt=_opts(max_step=0.0)), "max_step must be > 0"),
    (dict(opt=_opts(max_step=-1.0)), "max_step must be > 0"),
    (dict(opt=_opts(max_step=math.nan)), "max_step must be > 0"),
    (dict(opt=_opts(max_samples=0)), "max_samples must be >= 1"),
    (dict(opt=_opts(slots=0)), "slots must be in [1, DCX_SHORTCUT_MAX_SLOTS]"),
    (dict(opt=_opts(slots=17)), "slots must be in [1, DCX_SHORTCUT_MAX_SLOTS]"),
    (dict(opt=_opts(W=0)), "W must be in [1, DCX_SHORTCUT_MAX_WAYPOINTS]"),
    (dict(opt=_opts(W=65537)), "W must be in [1, DCX_SHORTCUT_MAX_WAYPOINTS]"),
    (dict(opt=_opts(mask=1)), "wrap_mask has a bit at or above dof"),
    (dict(opt=_opts(mask=1 << 63)), "wrap_mask has a bit at or above dof"),
    (dict(opt=_opts(reserved=(1, 0))), "reserved fields must be 0"),
    (dict(opt=_opts(reserved=(0, 1))), "reserved fields must be 0"),
] + [(dict(state=_state(**{f: True})), "state or one of its pointers is NULL") for f in _STATE]


@pytest.mark.parametrize("name", _RUNS)
def test_argument_errors_before_any_device_use(name):
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    run, partial = _run(name), "partial" in name
    if partial:
        need = lib.dcx_path_shortcut_partial_cost_work_bytes(m, 8, 4, 32)
        assert need >= lib.dcx_motion_worst_work_bytes(m, 8 * 4 * 3) > 0
        size_fn = "dcx_path_shortcut_partial_cost_work_bytes"
    else:
        need = lib.dcx_path_shortcut_cost_work_bytes(m, 8, 4)
        assert need >= lib.dcx_motion_worst_work_bytes(m, 8 * 4) > 0
        size_fn = "dcx_path_shortcut_cost_work_bytes"
    for kw, text in _ERRORS + [(dict(work_bytes=need - 1), "smaller than " + size_fn)]:
        kw = dict(kw)
        rc = run(lib, kw.pop("model", m), **kw)
        msg = lib.dcx_last_error().decode()
        assert rc == 1, (kw, rc, msg)
        assert text in msg and msg.startswith("shortcut"), (kw, msg)
    if partial:   # the workspace is the one of the options' own W
        assert lib.dcx_path_shortcut_partial_cost_work_bytes(m, 8, 4, 4096) > need
        assert run(lib, m, opt=_opts(W=4096), work_bytes=need) == 1
        assert "smaller than " + size_fn in lib.dcx_last_error().decode()
    # the cost options are read even where there is nothing to do, and a good set is then no error; gain and band may be 0
    assert run(lib, m, R=0, cost=False, state=False, seg=0, draws=0, work=0, work_bytes=0) == 1
    assert run(lib, m, R=0, state=False, seg=0, draws=0, work=0, work_bytes=0) == 0
    assert run(lib, m, T=0, draws=0, work_bytes=need) == 0
    assert run(lib, m, T=0, cost=_cost(gain=0.0, band=0.0), work_bytes=need) == 0
    # unsupported, not invalid, and still before any device work (the stand-in model names device 0 and is never used): more
    # samples than a packed key holds, a feature width without a worst-sample kernel (the stand-in's reads 0), too many edges
    assert run(lib, m, opt=_opts(max_samples=1 << 24), work_bytes=1 << 62) == 2
    assert "max_samples above 2^24 - 1" in lib.dcx_last_error().decode()
    assert run(lib, m, opt=_opts(max_samples=(1 << 24) - 1), work_bytes=1 << 62) == 2
    assert "no worst-sample kernel" in lib.dcx_last_error().decode()
    assert run(lib, m, R=1 << 31, work_bytes=1 << 62) == 2
    if partial:   # R * slots fits, R * slots * 3 does not
        assert run(lib, m, R=1 << 28, work_bytes=1 << 62) == 2
        assert "more than 2^31 - 1 edges per round" in lib.dcx_last_error().decode()


def test_work_bytes_are_zero_for_refused_arguments_and_monotone():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    wb = lib.dcx_path_shortcut_cost_work_bytes
    for bad in [(None, 8, 4), (m, -1, 4), (m, 8, 0), (m, 8, 17), (m, 1 << 31, 4), (m, 1 << 29, 4)]:
        assert wb(*bad) == 0, bad
    sizes = [wb(m, R, 4) for R in (0, 1, 7, 64, 1000, 1 << 20)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    sizes = [wb(m, 100, P) for P in (1, 2, 5, 16)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    # dcx_motion_worst's workspace of the batch at the head, then the scratch
    assert wb(m, 100, 4) > lib.dcx_motion_worst_work_bytes(m, 400)
    wp = lib.dcx_path_shortcut_partial_cost_work_bytes
    for bad in [(None, 8, 4, 32), (m, -1, 4, 32), (m, 8, 0, 32), (m, 8, 17, 32), (m, 1 << 31, 4, 32), (m, 1 << 28, 4, 32), (m, 8, 4, 0),
                (m, 8, 4, -1), (m, 8, 4, 65537)]:
        assert wp(*bad) == 0, bad
    sizes = [wp(m, R, 4, 4096) for R in (0, 1, 7, 64, 1000, 1 << 20)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    sizes = [wp(m, 100, P, 4096) for P in (1, 2, 5, 16)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    sizes = [wp(m, 100, 4, W) for W in (1, 3, 32, 2048, 2049, 4096, 65536)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    # three edges per slot, the stage of seg [R, W], and c and len [R, W] where a path can outgrow a block's LDS
    assert wp(m, 100, 4, 32) > lib.dcx_motion_worst_work_bytes(m, 1200) + 100 * 32 * 4
    assert wp(m, 100, 4, 4096) >= wp(m, 100, 4, 32) + 3 * 100 * (4096 - 32) * 4
