"""CPU-side checks of the partial shortcut boundary (dcx_path_shortcut_partial_run, dcx_path_shortcut_partial_work_bytes): the
symbols exist and the version stays 109, the header and the ctypes table declare the same arguments, every argument error is
reported before anything touches a device, the workspace size is 0 for refused arguments and non-decreasing in R, slots and W,
and the header states the contract under the 109 section - on a machine without a GPU."""
import ctypes
import math

import pytest

from test_rrt_abi import HEADER, _declared, _fake_model
from test_shortcut_abi import _STATE, _opts, _state


@pytest.mark.parametrize("name", ["dcx_path_shortcut_partial_run", "dcx_path_shortcut_partial_work_bytes"])
def test_symbols_exist_and_version_stays(name):
    from diffco_amd import _lib
    res, args = _declared(name)
    assert _lib.SYMBOLS[name][0] is res
    assert list(_lib.SYMBOLS[name][1]) == args
    lib = _lib.load()
    assert hasattr(lib, name)
    assert lib.dcx_version() == 109


def test_the_two_modes_take_the_same_arguments():
    assert _declared("dcx_path_shortcut_partial_run") == _declared("dcx_path_shortcut_run")
    assert _declared("dcx_path_shortcut_partial_work_bytes")[1] == _declared("dcx_path_shortcut_work_bytes")[1] + [ctypes.c_int32]


def test_header_states_the_contract_under_109():
    src = open(HEADER).read()
    at = src.index("batched path shortcutting and RRT path extraction (added under DCX_VERSION 109)")
    end = src.index("/* ---- roadmap queries")
    assert at < src.index("Partial shortcuts:") < src.index("dcx_path_shortcut_partial_run(const") < end
    body = src[src.index("Partial shortcuts:"):end]
    for word in ("1. arc length", "2. pick", "3. check", "4. apply", "5. rewrite", "DCX_RESAMPLE_CHUNK", "ea == eb idles the slot",
                 "eb_p < ea_q || eb_q < ea_p", "cnt + 2 - (eb_p - ea_p) <= W", "Only the new middle edge is checked", "Fixed batch",
                 "non-decreasing in R, slots and W"):
        assert word in body, word
    assert "#define DCX_VERSION 109" in src


def _run(lib, model, R=8, T=2, opt=None, state=None, draws=1, work=1, work_bytes=1 << 40):
    # (the addresses are never read: every case below is refused, or has nothing to do, before any device work)
    p = ctypes.c_void_p
    opt = _opts() if opt is None else opt
    state = _state() if state is None else state
    return lib.dcx_path_shortcut_partial_run(model, ctypes.byref(state) if state is not False else None, R, p(draws), T,
                                             ctypes.byref(opt) if opt is not False else None, None, p(work), work_bytes, None)


def test_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    need = lib.dcx_path_shortcut_partial_work_bytes(m, 8, 4, 32)
    assert need >= lib.dcx_path_shortcut_work_bytes(m, 8, 4) >= lib.dcx_motion_work_bytes(m, 32) > 0
    cases = [
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
        (dict(work_bytes=need - 1), "smaller than dcx_path_shortcut_partial_work_bytes"),
    ] + [(dict(state=_state(**{f: True})), "state or one of its pointers is NULL") for f in _STATE]
    for kw, text in cases:
        kw = dict(kw)
        rc = _run(lib, kw.pop("model", m), **kw)
        msg = lib.dcx_last_error().decode()
        assert rc == 1, (kw, rc, msg)
        assert text in msg, (kw, msg)
    # the workspace is the one of the options' own W: what suffices for W = 32 does not for a W that keeps c and len there
    big = lib.dcx_path_shortcut_partial_work_bytes(m, 8, 4, 4096)
    assert big > need
    assert _run(lib, m, opt=_opts(W=4096), work_bytes=need) == 1
    assert "smaller than dcx_path_shortcut_partial_work_bytes" in lib.dcx_last_error().decode()
    # nothing to do is not an error, with or without buffers
    assert _run(lib, m, R=0, state=False, draws=0, work=0, work_bytes=0) == 0
    assert _run(lib, m, T=0, draws=0, work_bytes=need) == 0
    assert _run(lib, m, opt=_opts(W=65536), T=0, work_bytes=lib.dcx_path_shortcut_partial_work_bytes(m, 8, 4, 65536)) == 0
    # beyond one launch: unsupported, not invalid
    assert _run(lib, m, R=1 << 31, work_bytes=1 << 62) == 2


def test_work_bytes_is_zero_for_refused_arguments_and_monotone():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    wb = lib.dcx_path_shortcut_partial_work_bytes
    for bad in [(None, 8, 4, 32), (m, -1, 4, 32), (m, 8, 0, 32), (m, 8, 17, 32), (m, 1 << 31, 4, 32), (m, 8, 4, 0), (m, 8, 4, -1),
                (m, 8, 4, 65537)]:
        assert wb(*bad) == 0, bad
    sizes = [wb(m, R, 4, 4096) for R in (0, 1, 7, 64, 1000, 1 << 20)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0] > 0
    sizes = [wb(m, 100, P, 4096) for P in (1, 2, 5, 16)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    sizes = [wb(m, 100, 4, W) for W in (1, 3, 32, 2048, 2049, 4096, 65536)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    # never less than the vertex mode's, and c and len [R, W] on top of it where a path can outgrow a block's LDS (the stand-in
    # model's dof reads 0, so the [R, W, dof] stage is empty here)
    assert wb(m, 100, 4, 32) >= lib.dcx_path_shortcut_work_bytes(m, 100, 4)
    assert wb(m, 100, 4, 4096) >= lib.dcx_path_shortcut_work_bytes(m, 100, 4) + 2 * 100 * 4096 * 4
