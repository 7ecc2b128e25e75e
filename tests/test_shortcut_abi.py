"""CPU-side checks of the path shortcutting boundary (dcx_path_shortcut_run, dcx_path_shortcut_work_bytes,
dcx_rrt_extract_paths): the symbols exist and the version stays 109, the header and the ctypes table declare the same arguments,
dcx_shortcut_state / dcx_shortcut_opts have the C layout, every argument error is reported before anything touches a device,
the workspace size is 0 for refused arguments, and the header section is marked as added under version 109 - on a machine
without a GPU."""
import ctypes
import math
import os
import subprocess

import pytest

from test_rrt_abi import HEADER, ROOT, _declared, _fake_model

_OPTS = ("max_step", "max_samples", "slots", "W", "wrap_mask", "reserved")
_STATE = ("path", "count", "accepted")
_RRT_STATE = ("nodes", "parent", "count", "status", "link", "solved_round")


@pytest.mark.parametrize("name", ["dcx_path_shortcut_run", "dcx_path_shortcut_work_bytes", "dcx_rrt_extract_paths"])
def test_symbols_exist_and_version_stays(name):
    from diffco_amd import _lib
    res, args = _declared(name)
    assert _lib.SYMBOLS[name][0] is res
    assert list(_lib.SYMBOLS[name][1]) == args
    lib = _lib.load()
    assert hasattr(lib, name)
    assert lib.dcx_version() == 109


def test_struct_layouts_match_c(tmp_path):
    from diffco_amd._lib import SHORTCUT_MAX_SLOTS, SHORTCUT_MAX_WAYPOINTS, ShortcutOpts, ShortcutState
    prog = tmp_path / "szs.c"
    offs = ", ".join([f"offsetof(dcx_shortcut_opts, {f})" for f in _OPTS] + [f"offsetof(dcx_shortcut_state, {f})" for f in _STATE])
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dcx.h"\n'
                    'int main(){size_t v[] = {sizeof(dcx_shortcut_opts), sizeof(dcx_shortcut_state), DCX_SHORTCUT_MAX_SLOTS, '
                    'DCX_SHORTCUT_MAX_WAYPOINTS, ' + offs + '};\nfor (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%zu ", v[i]);}')
    exe = tmp_path / "szs"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [ctypes.sizeof(ShortcutOpts), ctypes.sizeof(ShortcutState), SHORTCUT_MAX_SLOTS, SHORTCUT_MAX_WAYPOINTS] + \
        [getattr(ShortcutOpts, f).offset for f in _OPTS] + [getattr(ShortcutState, f).offset for f in _STATE]
    assert [f for f, _ in ShortcutOpts._fields_] == list(_OPTS) and [f for f, _ in ShortcutState._fields_] == list(_STATE)
    assert ctypes.sizeof(ShortcutOpts) == 40 and ctypes.sizeof(ShortcutState) == 24
    assert SHORTCUT_MAX_SLOTS == 16 and SHORTCUT_MAX_WAYPOINTS == 65536


def test_header_section_is_marked_109():
    src = open(HEADER).read()
    at = src.index("batched path shortcutting")
    assert "added under DCX_VERSION 109" in src[at - 40:][:200]
    body = src[at:][:9000]
    for word in ("1. pick", "2. check", "3. apply", "4. compact", "Fixed batch", "an exact duplicate", "j_p <= i_q || j_q <= i_p",
                 "count[r] = -n", "bounded by cap hops"):
        assert word in body, word
    assert "#define DCX_VERSION 109" in src


def _opts(max_step=0.1, max_samples=16, slots=4, W=32, mask=0, reserved=(0, 0)):
    from diffco_amd._lib import ShortcutOpts
    return ShortcutOpts(max_step, max_samples, slots, W, mask, (ctypes.c_int64 * 2)(*reserved))


def _state(**null):
    from diffco_amd._lib import ShortcutState
    return ShortcutState(*(0 if null.get(f) else 1 for f in _STATE))


def _run(lib, model, R=8, T=2, opt=None, state=None, draws=1, work=1, work_bytes=1 << 40):
    # (the addresses are never read: every case below is refused, or has nothing to do, before any device work)
    p = ctypes.c_void_p
    opt = _opts() if opt is None else opt
    state = _state() if state is None else state
    return lib.dcx_path_shortcut_run(model, ctypes.byref(state) if state is not False else None, R, p(draws), T,
                                     ctypes.byref(opt) if opt is not False else None, None, p(work), work_bytes, None)


def test_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    need = lib.dcx_path_shortcut_work_bytes(m, 8, 4)
    assert need >= lib.dcx_motion_work_bytes(m, 32) > 0
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
        (dict(work_bytes=need - 1), "smaller than dcx_path_shortcut_work_bytes"),
    ] + [(dict(state=_state(**{f: True})), "state or one of its pointers is NULL") for f in _STATE]
    for kw, text in cases:
        kw = dict(kw)
        rc = _run(lib, kw.pop("model", m), **kw)
        msg = lib.dcx_last_error().decode()
        assert rc == 1, (kw, rc, msg)
        assert text in msg, (kw, msg)
    # nothing to do is not an error, with or without buffers
    assert _run(lib, m, R=0, state=False, draws=0, work=0, work_bytes=0) == 0
    assert _run(lib, m, T=0, draws=0, work_bytes=need) == 0
    assert _run(lib, m, opt=_opts(W=65536), T=0, work_bytes=need) == 0
    # beyond one launch: unsupported, not invalid
    assert _run(lib, m, R=1 << 31, work_bytes=1 << 62) == 2


def test_work_bytes_is_zero_for_refused_arguments_and_grows():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    wb = lib.dcx_path_shortcut_work_bytes
    for bad in [(None, 8, 4), (m, -1, 4), (m, 8, 0), (m, 8, 17), (m, 1 << 31, 4)]:
        assert wb(*bad) == 0, bad
    sizes = [wb(m, R, 4) for R in (0, 1, 7, 64, 1000, 1 << 20)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0] > 0
    sizes = [wb(m, 100, P) for P in (1, 2, 5, 16)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    # the motion workspace for R * P edges, then the per-slot scratch: first_hit and the picks at the least
    assert wb(m, 100, 4) >= lib.dcx_motion_work_bytes(m, 400) + 400 * 4 + 400 * 8


def test_extract_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    lib = _lib.load()

    def run(R=4, cap=64, dof=3, W=8, path=1, count=1, state=None, **null):
        st = _lib.RrtState(*(0 if null.get(f) else 1 for f in _RRT_STATE))
        p = ctypes.c_void_p
        return lib.dcx_rrt_extract_paths(0, None if state is False else ctypes.byref(st), R, cap, dof, p(path), p(count), W, None)

    cases = [
        (dict(R=-1), "R < 0"),
        (dict(cap=0), "cap must be in [1, DCX_RRT_MAX_CAP]"),
        (dict(cap=(1 << 20) + 1), "cap must be in [1, DCX_RRT_MAX_CAP]"),
        (dict(dof=0), "dof < 1"),
        (dict(W=-1), "W < 0"),
        (dict(state=False), "pointers is NULL"),
        (dict(count=0), "count is NULL"),
        (dict(path=0), "path is NULL with W > 0"),
    ] + [(dict(**{f: True}), "pointers is NULL") for f in ("nodes", "parent", "status", "link")]
    for kw, text in cases:
        rc = run(**kw)
        msg = lib.dcx_last_error().decode()
        assert rc == 1, (kw, rc, msg)
        assert text in msg, (kw, msg)
    assert run(R=1 << 31) == 2
    # nothing to do is not an error; the trees' sizes and solved_round are not needed
    assert run(R=0, state=False, path=0, count=0) == 0


def test_python_layer_rejects_bad_arguments_without_a_device():
    import torch
    from diffco_amd import shortcut

    class NoFused:
        def check_motions(self, *a, **k):
            raise AssertionError("not reached")

    p = [torch.zeros(4, 3)]
    with pytest.raises(ValueError, match="slots"):
        shortcut.shortcut_paths(NoFused(), p, max_step=0.1, slots=0)
    with pytest.raises(ValueError, match="bit at or above dof"):
        shortcut.shortcut_paths(NoFused(), p, max_step=0.1, wrap=0b1000)
    with pytest.raises(ValueError, match="max_step"):
        shortcut.shortcut_paths(NoFused(), p, max_step=0.0)
