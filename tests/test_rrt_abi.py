"""CPU-side checks of the batched RRT-Connect boundary (dcx_rrt_connect_run, dcx_rrt_work_bytes): the symbols exist and the
version stays 109, the header and the ctypes table declare the same arguments, dcx_rrt_state / dcx_rrt_opts have the C layout,
every argument error is reported before anything touches a device, the workspace size is 0 for refused arguments, and the
header section is marked as added under version 109 - on a machine without a GPU."""
import ctypes
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dcx.h")

_CTYPE = {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
          "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t}
_OPTS = ("range", "max_step", "max_samples", "slots", "cap", "reserved0", "wrap_mask", "reserved")
_STATE = ("nodes", "parent", "count", "status", "link", "solved_round")


def _declared(name):
    """(restype, argtypes) of a function as include/dcx.h declares it: every pointer travels as an address"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    args = []
    for a in m.group(2).split(","):
        a = a.strip()
        args.append(ctypes.c_void_p if "*" in a else _CTYPE[a.replace("const ", "").split()[0]])
    return _CTYPE[m.group(1)], args


@pytest.mark.parametrize("name", ["dcx_rrt_connect_run", "dcx_rrt_work_bytes"])
def test_symbols_exist_and_version_stays(name):
    from diffco_amd import _lib
    res, args = _declared(name)
    assert _lib.SYMBOLS[name][0] is res
    assert list(_lib.SYMBOLS[name][1]) == args
    lib = _lib.load()
    assert hasattr(lib, name)
    assert lib.dcx_version() == 109


def test_struct_layouts_match_c(tmp_path):
    from diffco_amd._lib import RRT_MAX_CAP, RRT_MAX_SLOTS, RrtOpts, RrtState
    prog = tmp_path / "szr.c"
    offs = ", ".join([f"offsetof(dcx_rrt_opts, {f})" for f in _OPTS] + [f"offsetof(dcx_rrt_state, {f})" for f in _STATE])
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dcx.h"\n'
                    'int main(){size_t v[] = {sizeof(dcx_rrt_opts), sizeof(dcx_rrt_state), DCX_RRT_MAX_SLOTS, DCX_RRT_MAX_CAP, '
                    + offs + '};\nfor (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%zu ", v[i]);}')
    exe = tmp_path / "szr"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [ctypes.sizeof(RrtOpts), ctypes.sizeof(RrtState), RRT_MAX_SLOTS, RRT_MAX_CAP] + \
        [getattr(RrtOpts, f).offset for f in _OPTS] + [getattr(RrtState, f).offset for f in _STATE]
    assert [f for f, _ in RrtOpts._fields_] == list(_OPTS) and [f for f, _ in RrtState._fields_] == list(_STATE)
    assert ctypes.sizeof(RrtOpts) == 48 and ctypes.sizeof(RrtState) == 48 and RRT_MAX_SLOTS == 16


def test_header_section_is_marked_109():
    src = open(HEADER).read()
    at = src.index("batched RRT-Connect")
    assert "added under DCX_VERSION 109" in src[at - 40:][:200]
    body = src[at:][:9000]
    for word in ("Phase 1, extend", "Phase 2, connect", "Fixed batch", "Solved wins over full", "bits(dist2) << 32 | index"):
        assert word in body, word


def _fake_model():
    # a zeroed stand-in handle as large as any model struct (dof reads 0: every mask bit lies at or above it)
    buf = ctypes.create_string_buffer(1 << 20)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _opts(rng=0.5, max_step=0.1, max_samples=16, slots=4, cap=64, r0=0, mask=0, reserved=(0, 0)):
    from diffco_amd._lib import RrtOpts
    return RrtOpts(rng, max_step, max_samples, slots, cap, r0, mask, (ctypes.c_int64 * 2)(*reserved))


def _state(**null):
    from diffco_amd._lib import RrtState
    return RrtState(*(0 if null.get(f) else 1 for f in _STATE))


def _run(lib, model, R=8, T=2, round0=0, opt=None, state=None, samples=1, work=1, work_bytes=1 << 40):
    # (the addresses are never read: every case below is refused, or has nothing to do, before any device work)
    p = ctypes.c_void_p
    opt = _opts() if opt is None else opt
    state = _state() if state is None else state
    return lib.dcx_rrt_connect_run(model, ctypes.byref(state) if state is not False else None, R, p(samples), T, round0,
                                   ctypes.byref(opt) if opt is not False else None, None, p(work), work_bytes, None)


def test_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    need = lib.dcx_rrt_work_bytes(m, 8, 4)
    assert need >= lib.dcx_motion_work_bytes(m, 32) > 0
    cases = [
        (dict(model=None), "model is NULL"),
        (dict(opt=False), "options are NULL"),
        (dict(state=False), "state or one of its pointers is NULL"),
        (dict(samples=0), "samples is NULL"),
        (dict(work=0), "work is NULL"),
        (dict(R=-1), "R < 0"),
        (dict(T=-1), "T < 0"),
        (dict(round0=-1), "round0 < 0"),
        (dict(round0=(1 << 31) - 2), "round0 + T above 2^31 - 1"),
        (dict(opt=_opts(rng=0.0)), "range must be > 0"),
        (dict(opt=_opts(rng=-1.0)), "range must be > 0"),
        (dict(opt=_opts(rng=math.nan)), "range must be > 0"),
        (dict(opt=_opts(max_step=0.0)), "max_step must be > 0"),
        (dict(opt=_opts(max_step=math.nan)), "max_step must be > 0"),
        (dict(opt=_opts(max_samples=0)), "max_samples must be >= 1"),
        (dict(opt=_opts(slots=0)), "slots must be in [1, DCX_RRT_MAX_SLOTS]"),
        (dict(opt=_opts(slots=17)), "slots must be in [1, DCX_RRT_MAX_SLOTS]"),
        (dict(opt=_opts(cap=0)), "cap must be in [1, DCX_RRT_MAX_CAP]"),
        (dict(opt=_opts(cap=(1 << 20) + 1)), "cap must be in [1, DCX_RRT_MAX_CAP]"),
        (dict(opt=_opts(mask=1)), "wrap_mask has a bit at or above dof"),
        (dict(opt=_opts(mask=1 << 63)), "wrap_mask has a bit at or above dof"),
        (dict(opt=_opts(r0=1)), "reserved fields must be 0"),
        (dict(opt=_opts(reserved=(1, 0))), "reserved fields must be 0"),
        (dict(opt=_opts(reserved=(0, 1))), "reserved fields must be 0"),
        (dict(work_bytes=need - 1), "smaller than dcx_rrt_work_bytes"),
    ] + [(dict(state=_state(**{f: True})), "state or one of its pointers is NULL") for f in _STATE]
    for kw, text in cases:
        kw = dict(kw)
        rc = _run(lib, kw.pop("model", m), **kw)
        msg = lib.dcx_last_error().decode()
        assert rc == 1, (kw, rc, msg)
        assert text in msg, (kw, msg)
    # nothing to do is not an error, with or without buffers
    assert _run(lib, m, R=0, state=False, samples=0, work=0, work_bytes=0) == 0
    assert _run(lib, m, T=0, samples=0, work_bytes=need) == 0
    # beyond one launch: unsupported, not invalid
    assert _run(lib, m, R=1 << 31, work_bytes=1 << 62) == 2


def test_work_bytes_is_zero_for_refused_arguments_and_grows():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    wb = lib.dcx_rrt_work_bytes
    for bad in [(None, 8, 4), (m, -1, 4), (m, 8, 0), (m, 8, 17), (m, 1 << 31, 4)]:
        assert wb(*bad) == 0, bad
    sizes = [wb(m, R, 4) for R in (0, 1, 7, 64, 1000, 1 << 20)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0] > 0
    sizes = [wb(m, 100, P) for P in (1, 2, 5, 16)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    # the motion workspace for R * P edges, then the per-slot scratch
    assert wb(m, 100, 4) > lib.dcx_motion_work_bytes(m, 400)


def test_python_layer_rejects_bad_arguments_without_a_device():
    import torch
    from diffco_amd import rrt

    class NoFused:
        def check_motions(self, *a, **k):
            raise AssertionError("not reached")

    s = torch.zeros(2, 3)
    with pytest.raises(ValueError, match="slots"):
        rrt.rrt_connect(NoFused(), s, s, range=0.5, max_step=0.1, slots=0, limits=[[0, 1]] * 3)
    with pytest.raises(ValueError, match="bit at or above dof"):
        rrt.rrt_connect(NoFused(), s, s, range=0.5, max_step=0.1, wrap=0b1000, limits=[[0, 1]] * 3)
    with pytest.raises(ValueError, match="limits"):
        rrt.rrt_connect(NoFused(), s, s, range=0.5, max_step=0.1)
