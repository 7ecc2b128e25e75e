"""CPU-side checks of the batched motion checks' boundary (dcx_check_motions): the dcx_motion_opts mirror has the C layout,
the header and the ctypes table agree, and every argument error is reported with its code and text before anything touches
the model or a device - on a machine without a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dcx.h")


def test_motion_opts_layout_matches_c(tmp_path):
    from diffco_amd._lib import MotionOpts
    prog = tmp_path / "szm.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dcx.h"\n'
                    'int main(){printf("%zu %zu %zu %zu %zu", sizeof(dcx_motion_opts), offsetof(dcx_motion_opts, res),'
                    ' offsetof(dcx_motion_opts, max_step), offsetof(dcx_motion_opts, max_samples),'
                    ' offsetof(dcx_motion_opts, reserved));}')
    exe = tmp_path / "szm"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [ctypes.sizeof(MotionOpts), MotionOpts.res.offset, MotionOpts.max_step.offset, MotionOpts.max_samples.offset,
                   MotionOpts.reserved.offset]


def test_motion_symbols_in_header_and_table():
    from diffco_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("dcx_motion_work_bytes", "dcx_check_motions"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "dcx_check_motions") and hasattr(lib, "dcx_motion_work_bytes")
    assert lib.dcx_version() == 109


def _call(lib, model, E=4, opt=None, qa=1, qb=1, first=1, work=1, work_bytes=None, fake_model=None):
    from diffco_amd._lib import MotionOpts
    opt = MotionOpts(8, 0.0, 8, 0) if opt is None else opt
    if work_bytes is None:
        work_bytes = lib.dcx_motion_work_bytes(fake_model, max(E, 0)) if fake_model else 1 << 30
    # the pointers are never dereferenced: every case below fails its argument check first
    return lib.dcx_check_motions(model, ctypes.c_void_p(qa), ctypes.c_void_p(qb), E, ctypes.byref(opt) if opt is not False else None,
                                 None, ctypes.c_void_p(first), None, ctypes.c_void_p(work), work_bytes, None)


def test_motion_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    from diffco_amd._lib import MotionOpts
    lib = _lib.load()
    # a stand-in handle: the argument checks run before the call reads the model or selects a device (it would crash or
    # answer DCX_ERR_NO_DEVICE otherwise)
    fake = ctypes.create_string_buffer(4096)
    m = ctypes.cast(fake, ctypes.c_void_p)
    need = lib.dcx_motion_work_bytes(m, 4)
    assert need > 0 and lib.dcx_motion_work_bytes(None, 4) == 0 and lib.dcx_motion_work_bytes(m, -1) == 0
    assert lib.dcx_motion_work_bytes(m, 1000) > lib.dcx_motion_work_bytes(m, 10)

    def rc_msg(**kw):
        rc = _call(lib, kw.pop("model", m), **kw)
        return rc, lib.dcx_last_error().decode()

    cases = [
        (dict(model=None), "model is NULL"),
        (dict(opt=False), "options are NULL"),
        (dict(E=-1), "E < 0"),
        (dict(qa=0), "NULL"),
        (dict(qb=0), "NULL"),
        (dict(first=0), "NULL"),
        (dict(work=0), "NULL"),
        (dict(opt=MotionOpts(8, 0.5, 8, 0)), "exactly one sampling rule"),     # both rules
        (dict(opt=MotionOpts(0, 0.0, 8, 0)), "exactly one sampling rule"),     # neither
        (dict(opt=MotionOpts(-3, 0.5, 8, 0)), "exactly one sampling rule"),
        (dict(opt=MotionOpts(0, float("nan"), 8, 0)), "exactly one sampling rule"),
        (dict(opt=MotionOpts(8, 0.0, 0, 0)), "max_samples >= 1"),
        (dict(opt=MotionOpts(0, 0.1, -1, 0)), "max_samples >= 1"),
        (dict(work_bytes=need - 1), "smaller than dcx_motion_work_bytes"),
    ]
    for kw, text in cases:
        rc, msg = rc_msg(**kw)
        assert rc == 1, (kw, rc, msg)
        assert text in msg, (kw, msg)
    # nothing to check is not an error, and needs no buffers
    assert _call(lib, m, E=0, qa=0, qb=0, first=0, work=0, work_bytes=0) == 0


def test_facade_rejects_two_rules_without_gpu():
    from diffco_amd._perceptron import MotionSource, check_motions

    class Owner:
        pass
    with pytest.raises(ValueError, match="exactly one"):
        check_motions(MotionSource(Owner(), None, None, None, None, None), [[0.0]], [[1.0]], res=4, max_step=0.1)
    with pytest.raises(ValueError, match="exactly one"):
        check_motions(MotionSource(Owner(), None, None, None, None, None), [[0.0]], [[1.0]])
