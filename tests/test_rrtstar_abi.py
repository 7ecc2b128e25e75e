"""CPU-side checks of the batched RRT* boundary (dcx_rrtstar_run, dcx_rrtstar_work_bytes, dcx_rrtstar_extract_paths): the
symbols exist and the version stays 109, the header and the ctypes table declare the same arguments, dcx_rrtstar_state /
dcx_rrtstar_opts have the C layout, every argument error is reported before anything touches a device, the workspace size is 0
for refused arguments, and the header section states the contract - on a machine without a GPU."""
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
_OPTS = ("range", "max_step", "radius", "max_samples", "slots", "near", "cap", "reserved0", "wrap_mask", "reserved")
_STATE = ("nodes", "parent", "elen", "cost", "count", "status", "goal_node", "first_round")


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


@pytest.mark.parametrize("name", ["dcx_rrtstar_run", "dcx_rrtstar_work_bytes", "dcx_rrtstar_extract_paths"])
def test_symbols_exist_and_version_stays(name):
    from diffco_amd import _lib
    res, args = _declared(name)
    assert _lib.SYMBOLS[name][0] is res
    assert list(_lib.SYMBOLS[name][1]) == args
    lib = _lib.load()
    assert hasattr(lib, name)
    assert lib.dcx_version() == 109


def test_struct_layouts_match_c(tmp_path):
    from diffco_amd._lib import RRTSTAR_MAX_CAP, RRTSTAR_MAX_NEAR, RrtStarOpts, RrtStarState
    prog = tmp_path / "szs.c"
    offs = ", ".join([f"offsetof(dcx_rrtstar_opts, {f})" for f in _OPTS] + [f"offsetof(dcx_rrtstar_state, {f})" for f in _STATE])
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dcx.h"\n'
                    'int main(){size_t v[] = {sizeof(dcx_rrtstar_opts), sizeof(dcx_rrtstar_state), DCX_RRTSTAR_MAX_NEAR, '
                    'DCX_RRTSTAR_MAX_CAP, ' + offs + '};\nfor (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%zu ", v[i]);}')
    exe = tmp_path / "szs"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [ctypes.sizeof(RrtStarOpts), ctypes.sizeof(RrtStarState), RRTSTAR_MAX_NEAR, RRTSTAR_MAX_CAP] + \
        [getattr(RrtStarOpts, f).offset for f in _OPTS] + [getattr(RrtStarState, f).offset for f in _STATE]
    assert [f for f, _ in RrtStarOpts._fields_] == list(_OPTS) and [f for f, _ in RrtStarState._fields_] == list(_STATE)
    assert ctypes.sizeof(RrtStarOpts) == 56 and ctypes.sizeof(RrtStarState) == 64
    assert RRTSTAR_MAX_NEAR == 16 and RRTSTAR_MAX_CAP == 65536


def test_header_section_states_the_contract():
    src = open(HEADER).read()
    at = src.index("batched RRT* (added")
    assert "added under DCX_VERSION 109" in src[at:][:60]
    assert at > src.index("batched RRT-Connect (added") and at < src.index("batched path shortcutting and RRT path extraction (added")
    body = src[at:][:12000]
    for word in ("1. extend", "2. near set", "3. choose parent", "4. append", "5. rewire", "6. refresh", "Fixed batch", "the snapshot",
                 "(bits(cj), u_j) < (bits(c0), near)", "(bits(c'), p)", "L' = sqrtf(dist2_j)", "compare-all in LDS",
                 "DCX_RRTSTAR_MAX_CAP: the refresh", "T rounds in one call equal T calls of one round each",
                 "R * P * K edges each in (r, p, j) order", "dcx_rrtstar_work_bytes is 0 for arguments the call refuses"):
        assert word in body, word


def _fake_model():
    # a zeroed stand-in handle as large as any model struct (dof reads 0: every mask bit lies at or above it)
    buf = ctypes.create_string_buffer(1 << 20)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _opts(rng=0.5, max_step=0.1, radius=1.0, max_samples=16, slots=4, near=8, cap=64, r0=0, mask=0, reserved=(0, 0)):
    from diffco_amd._lib import RrtStarOpts
    return RrtStarOpts(rng, max_step, radius, max_samples, slots, near, cap, r0, mask, (ctypes.c_int64 * 2)(*reserved))


def _state(**null):
    from diffco_amd._lib import RrtStarState
    return RrtStarState(*(0 if null.get(f) else 1 for f in _STATE))


def _run(lib, model, R=8, T=2, round0=0, opt=None, state=None, goals=1, samples=1, work=1, work_bytes=1 << 40):
    # (the addresses are never read: every case below is refused, or has nothing to do, before any device work)
    p = ctypes.c_void_p
    opt = _opts() if opt is None else opt
    state = _state() if state is None else state
    return lib.dcx_rrtstar_run(model, ctypes.byref(state) if state is not False else None, R, p(goals), p(samples), T, round0,
                               ctypes.byref(opt) if opt is not False else None, None, p(work), work_bytes, None)


def test_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    need = lib.dcx_rrtstar_work_bytes(m, 8, 4, 8)
    assert need >= lib.dcx_motion_work_bytes(m, 8 * 4 * 8) > 0
    cases = [
        (dict(model=None), "model is NULL"),
        (dict(opt=False), "options are NULL"),
        (dict(state=False), "state or one of its pointers is NULL"),
        (dict(goals=0), "state or one of its pointers is NULL"),
        (dict(samples=0), "samples is NULL"),
        (dict(work=0), "work is NULL"),
        (dict(R=-1), "R < 0"),
        (dict(T=-1), "T < 0"),
        (dict(round0=-1), "round0 < 0"),
        (dict(round0=(1 << 31) - 2), "round0 + T above 2^31 - 1"),
        (dict(opt=_opts(rng=0.0)), "range must be > 0"),
        (dict(opt=_opts(rng=-1.0)), "range must be > 0"),
        (dict(opt=_opts(rng=math.nan)), "range must be > 0"),
        (dict(opt=_opts(radius=-1.0)), "radius must be >= 0"),
        (dict(opt=_opts(radius=math.nan)), "radius must be >= 0"),
        (dict(opt=_opts(max_step=0.0)), "max_step must be > 0"),
        (dict(opt=_opts(max_step=math.nan)), "max_step must be > 0"),
        (dict(opt=_opts(max_samples=0)), "max_samples must be >= 1"),
        (dict(opt=_opts(slots=0)), "slots must be in [1, DCX_RRT_MAX_SLOTS]"),
        (dict(opt=_opts(slots=17)), "slots must be in [1, DCX_RRT_MAX_SLOTS]"),
        (dict(opt=_opts(near=-1)), "near must be in [0, DCX_RRTSTAR_MAX_NEAR]"),
        (dict(opt=_opts(near=17)), "near must be in [0, DCX_RRTSTAR_MAX_NEAR]"),
        (dict(opt=_opts(cap=0)), "cap must be in [1, DCX_RRTSTAR_MAX_CAP]"),
        (dict(opt=_opts(cap=(1 << 16) + 1)), "cap must be in [1, DCX_RRTSTAR_MAX_CAP]"),
        (dict(opt=_opts(mask=1)), "wrap_mask has a bit at or above dof"),
        (dict(opt=_opts(mask=1 << 63)), "wrap_mask has a bit at or above dof"),
        (dict(opt=_opts(r0=1)), "reserved fields must be 0"),
        (dict(opt=_opts(reserved=(1, 0))), "reserved fields must be 0"),
        (dict(opt=_opts(reserved=(0, 1))), "reserved fields must be 0"),
        (dict(work_bytes=need - 1), "smaller than dcx_rrtstar_work_bytes"),
    ] + [(dict(state=_state(**{f: True})), "state or one of its pointers is NULL") for f in _STATE]
    for kw, text in cases:
        kw = dict(kw)
        rc = _run(lib, kw.pop("model", m), **kw)
        msg = lib.dcx_last_error().decode()
        assert rc == 1, (kw, rc, msg)
        assert text in msg and msg.startswith("rrtstar"), (kw, msg)
    # nothing to do is not an error, with or without buffers; the radius may be 0 and near may be 0
    assert _run(lib, m, R=0, state=False, goals=0, samples=0, work=0, work_bytes=0) == 0
    assert _run(lib, m, T=0, samples=0, work_bytes=need) == 0
    assert _run(lib, m, T=0, opt=_opts(radius=0.0, near=0), work_bytes=need) == 0
    # beyond one launch: unsupported, not invalid - in the slots, and in the places alone
    assert _run(lib, m, R=1 << 31, work_bytes=1 << 62) == 2
    assert _run(lib, m, R=1 << 27, opt=_opts(slots=4, near=8), work_bytes=1 << 62) == 2
    assert "2^31 - 1 edges per phase" in lib.dcx_last_error().decode()


def test_extract_argument_errors():
    from diffco_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p

    def run(R=4, cap=64, dof=7, W=8, state=None, path=1, count=1):
        state = _state() if state is None else state
        return lib.dcx_rrtstar_extract_paths(0, ctypes.byref(state) if state is not False else None, R, cap, dof, p(path), W,
                                             p(count), None)

    cases = [(dict(R=-1), "R < 0"), (dict(cap=0), "cap must be in [1, DCX_RRTSTAR_MAX_CAP]"),
             (dict(cap=(1 << 16) + 1), "cap must be in [1, DCX_RRTSTAR_MAX_CAP]"), (dict(dof=0), "dof < 1"), (dict(W=-1), "W < 0"),
             (dict(state=False), "pointers is NULL"), (dict(count=0), "count_out is NULL"), (dict(path=0), "path is NULL with W > 0")]
    cases += [(dict(state=_state(**{f: True})), "pointers is NULL") for f in ("nodes", "parent", "count", "goal_node")]
    for kw, text in cases:
        rc = run(**kw)
        msg = lib.dcx_last_error().decode()
        assert rc == 1 and text in msg and msg.startswith("rrtstar extract"), (kw, rc, msg)
    assert run(R=1 << 31) == 2
    assert run(R=0, state=False, path=0, count=0) == 0


def test_work_bytes_is_zero_for_refused_arguments_and_grows():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    wb = lib.dcx_rrtstar_work_bytes
    for bad in [(None, 8, 4, 8), (m, -1, 4, 8), (m, 8, 0, 8), (m, 8, 17, 8), (m, 8, 4, -1), (m, 8, 4, 17), (m, 1 << 31, 4, 8),
                (m, 1 << 27, 4, 8)]:
        assert wb(*bad) == 0, bad
    sizes = [wb(m, R, 4, 8) for R in (0, 1, 7, 64, 1000, 1 << 20)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0] > 0
    sizes = [wb(m, 100, P, 8) for P in (1, 2, 5, 16)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    sizes = [wb(m, 100, 4, K) for K in (0, 1, 8, 16)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0] > 0
    # the motion workspace of the larger batch, then the scratch
    assert wb(m, 100, 4, 8) > lib.dcx_motion_work_bytes(m, 3200)
    assert wb(m, 100, 4, 0) > lib.dcx_motion_work_bytes(m, 400)


def test_python_layer_rejects_bad_arguments_without_a_device():
    import torch
    from diffco_amd import rrtstar

    class NoFused:
        def check_motions(self, *a, **k):
            raise AssertionError("not reached")

    s = torch.zeros(2, 3)
    kw = dict(range=0.5, max_step=0.1, limits=[[0, 1]] * 3)
    with pytest.raises(ValueError, match="slots"):
        rrtstar.rrt_star(NoFused(), s, s, slots=0, **kw)
    with pytest.raises(ValueError, match="near"):
        rrtstar.rrt_star(NoFused(), s, s, near=17, **kw)
    with pytest.raises(ValueError, match="cap"):
        rrtstar.rrt_star(NoFused(), s, s, cap=1, **kw)
    with pytest.raises(ValueError, match="radius"):
        rrtstar.rrt_star(NoFused(), s, s, radius=-1.0, **kw)
    with pytest.raises(ValueError, match="bit at or above dof"):
        rrtstar.rrt_star(NoFused(), s, s, wrap=0b1000, **kw)
    with pytest.raises(ValueError, match="limits"):
        rrtstar.rrt_star(NoFused(), s, s, range=0.5, max_step=0.1)
