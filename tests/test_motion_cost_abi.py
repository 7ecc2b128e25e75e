"""CPU-side checks of the differentiable motion costs' boundary (dcx_motion_cost): the dcx_motion_cost_opts mirror has the C
layout, the header, the ctypes table and the library agree, and every argument error is reported with its code and text before
anything touches a device - on a machine without a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dcx.h")
NAMES = ("dcx_motion_cost_work_bytes", "dcx_motion_cost")


def test_motion_cost_opts_layout_matches_c(tmp_path):
    from diffco_amd._lib import MotionCostOpts
    prog = tmp_path / "szc.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dcx.h"\n'
                    'int main(){printf("%zu %zu %zu %zu %zu %zu", sizeof(dcx_motion_cost_opts), offsetof(dcx_motion_cost_opts, res),'
                    ' offsetof(dcx_motion_cost_opts, max_step), offsetof(dcx_motion_cost_opts, max_samples),'
                    ' offsetof(dcx_motion_cost_opts, open_end), offsetof(dcx_motion_cost_opts, reserved));}')
    exe = tmp_path / "szc"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [ctypes.sizeof(MotionCostOpts), MotionCostOpts.res.offset, MotionCostOpts.max_step.offset,
                   MotionCostOpts.max_samples.offset, MotionCostOpts.open_end.offset, MotionCostOpts.reserved.offset]
    assert ctypes.sizeof(MotionCostOpts) == 32


def test_motion_cost_symbols_in_header_table_and_library():
    from diffco_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name)
    assert lib.dcx_version() == 109


def _fake_model():
    # a zeroed stand-in handle as large as any model struct: the argument checks and the work-size query read host fields of
    # the model at most; nothing selects a device (the call would answer DCX_ERR_NO_DEVICE or crash otherwise)
    buf = ctypes.create_string_buffer(1 << 20)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _call(lib, model, E=4, opt=None, qa=1, qb=1, cost=1, ga=1, gb=1, work=1, work_bytes=1 << 30):
    from diffco_amd._lib import MotionCostOpts
    opt = MotionCostOpts(8, 0.0, 8, 0) if opt is None else opt
    # the pointers are never dereferenced: every case below fails its argument check first
    return lib.dcx_motion_cost(model, ctypes.c_void_p(qa), ctypes.c_void_p(qb), E, ctypes.byref(opt) if opt is not False else None,
                               None, 1.0, ctypes.c_void_p(cost), ctypes.c_void_p(ga), ctypes.c_void_p(gb), None,
                               ctypes.c_void_p(work), work_bytes, None)


def test_motion_cost_work_bytes():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    need = lib.dcx_motion_cost_work_bytes(m, 4, 8)
    assert need > 0
    assert lib.dcx_motion_cost_work_bytes(None, 4, 8) == 0
    assert lib.dcx_motion_cost_work_bytes(m, -1, 8) == 0
    assert lib.dcx_motion_cost_work_bytes(m, 4, 0) == 0
    assert lib.dcx_motion_cost_work_bytes(m, 1000, 8) > lib.dcx_motion_cost_work_bytes(m, 10, 8)
    assert lib.dcx_motion_cost_work_bytes(m, 1000, 64) > lib.dcx_motion_cost_work_bytes(m, 1000, 8)


def test_motion_cost_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    from diffco_amd._lib import MotionCostOpts
    lib = _lib.load()
    keep, m = _fake_model()
    need = lib.dcx_motion_cost_work_bytes(m, 4, 8)

    def opts(res, step, ms, open_end=0, reserved=(0, 0, 0, 0)):
        o = MotionCostOpts(res, step, ms, open_end)
        for i, v in enumerate(reserved):
            o.reserved[i] = v
        return o

    cases = [
        (dict(model=None), "model is NULL"),
        (dict(opt=False), "options are NULL"),
        (dict(E=-1), "E < 0"),
        (dict(qa=0), "NULL"),
        (dict(qb=0), "NULL"),
        (dict(cost=0), "NULL"),
        (dict(ga=0), "NULL"),
        (dict(gb=0), "NULL"),
        (dict(work=0), "NULL"),
        (dict(opt=opts(8, 0.5, 8)), "exactly one sampling rule"),     # both rules
        (dict(opt=opts(0, 0.0, 8)), "exactly one sampling rule"),     # neither
        (dict(opt=opts(-3, 0.5, 8)), "exactly one sampling rule"),
        (dict(opt=opts(0, float("nan"), 8)), "exactly one sampling rule"),
        (dict(opt=opts(8, 0.0, 0)), "max_samples >= 1"),
        (dict(opt=opts(0, 0.1, -1)), "max_samples >= 1"),
        (dict(opt=opts(0, 0.1, 8, open_end=2)), "open_end must be 0 or 1"),
        (dict(opt=opts(0, 0.1, 8, reserved=(0, 0, 1, 0))), "reserved"),
        (dict(work_bytes=need - 1), "smaller than dcx_motion_cost_work_bytes"),
    ]
    for kw, text in cases:
        rc = _call(lib, kw.pop("model", m), **kw)
        msg = lib.dcx_last_error().decode()
        assert rc == 1, (kw, rc, msg)
        assert text in msg, (kw, msg)
    # nothing to cost is not an error, and needs no buffers
    assert _call(lib, m, E=0, qa=0, qb=0, cost=0, ga=0, gb=0, work=0, work_bytes=0) == 0


def test_facade_rejects_two_rules_without_gpu():
    from diffco_amd._perceptron import MotionSource, motion_cost

    class Owner:
        pass
    with pytest.raises(ValueError, match="exactly one"):
        motion_cost(MotionSource(Owner(), None, None, None, None, None), [[0.0]], [[1.0]], res=4, max_step=0.1)
    with pytest.raises(ValueError, match="exactly one"):
        motion_cost(MotionSource(Owner(), None, None, None, None, None), [[0.0]], [[1.0]])
