"""CPU-side checks of the worst-sample motion call's boundary (dcx_motion_worst): the symbols exist and the version stays 109,
the header and the ctypes table declare the same arguments, every argument error is reported before anything touches a device,
the workspace size is monotone in E, and the header section is marked as added under version 109 - on a machine without a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dcx.h")

_CTYPE = {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
          "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t}


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


@pytest.mark.parametrize("name", ["dcx_motion_worst", "dcx_motion_worst_work_bytes"])
def test_symbols_exist_and_version_stays(name):
    from diffco_amd import _lib
    res, args = _declared(name)
    assert _lib.SYMBOLS[name][0] is res
    assert list(_lib.SYMBOLS[name][1]) == args
    lib = _lib.load()
    assert hasattr(lib, name)
    assert lib.dcx_version() == 109


def test_header_section_is_marked_109():
    src = open(HEADER).read()
    at = src.index("worst-sample motion queries")
    assert "added under DCX_VERSION 109" in src[at - 40:][:200]
    # the call takes dcx_motion_opts as it is: no new options struct, no new field
    from diffco_amd import _lib
    assert ctypes.sizeof(_lib.MotionOpts) == 16
    assert "dcx_motion_worst_opts" not in src


def _fake_model():
    # a zeroed stand-in handle as large as any model struct (dof reads 0: every mask bit lies at or above it)
    buf = ctypes.create_string_buffer(1 << 20)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _worst(lib, model, mask=0, E=4, opt=None, qa=1, qb=1, worst=1, idx=1, cls=0, n=0, ga=0, gb=0, work=1, work_bytes=1 << 30):
    from diffco_amd._lib import MotionOpts
    opt = MotionOpts(8, 0.0, 8, 0) if opt is None else opt
    p = ctypes.c_void_p
    return lib.dcx_motion_worst(model, p(qa), p(qb), E, ctypes.byref(opt) if opt is not False else None, None, p(worst), p(idx),
                                p(cls), p(n), p(ga), p(gb), p(work), work_bytes, mask, None)


def test_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    from diffco_amd._lib import MotionOpts
    lib = _lib.load()
    keep, m = _fake_model()
    need = lib.dcx_motion_worst_work_bytes(m, 4)
    assert need >= lib.dcx_motion_work_bytes(m, 4) > 0
    cases = [
        # those of dcx_check_motions_ex
        (dict(model=None), "model is NULL"),
        (dict(model=None, mask=1), "model is NULL"),
        (dict(opt=False), "options are NULL"),
        (dict(E=-1), "E < 0"),
        (dict(qa=0), "NULL"),
        (dict(qb=0), "NULL"),
        (dict(work=0), "NULL"),
        (dict(opt=MotionOpts(8, 0.5, 8, 0)), "exactly one sampling rule"),
        (dict(opt=MotionOpts(0, 0.0, 8, 0)), "exactly one sampling rule"),
        (dict(opt=MotionOpts(-1, 0.5, 8, 0)), "exactly one sampling rule"),
        (dict(opt=MotionOpts(8, 0.0, 0, 0)), "max_samples >= 1"),
        (dict(mask=1), "wrap_mask has a bit at or above dof"),
        (dict(mask=1 << 63), "wrap_mask has a bit at or above dof"),
        # its own
        (dict(worst=0), "NULL"),
        (dict(idx=0), "NULL"),
        (dict(ga=1), "both grad_a and grad_b or neither"),
        (dict(gb=1), "both grad_a and grad_b or neither"),
        (dict(opt=MotionOpts(8, 0.0, 8, 1)), "reserved must be 0"),
        (dict(work_bytes=need - 1), "smaller than dcx_motion_worst_work_bytes"),
    ]
    for kw, text in cases:
        kw = dict(kw)
        rc = _worst(lib, kw.pop("model", m), **kw)
        msg = lib.dcx_last_error().decode()
        assert rc == 1, (kw, rc, msg)
        assert text in msg, (kw, msg)
    # nothing to do is not an error, with or without buffers
    assert _worst(lib, m, E=0, qa=0, qb=0, worst=0, idx=0, work=0, work_bytes=0) == 0
    assert _worst(lib, m, E=0) == 0


def test_work_bytes_monotone_and_zero_for_null():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    assert lib.dcx_motion_worst_work_bytes(None, 100) == 0
    assert lib.dcx_motion_worst_work_bytes(m, -1) == 0
    sizes = [lib.dcx_motion_worst_work_bytes(m, E) for E in (0, 1, 2, 63, 64, 65, 1000, 4096, 65536, 1 << 20)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0] > 0
    # it holds dcx_check_motions' workspace and, per edge, at least the status word and the 64-bit key
    for E in (1, 1000, 65536):
        assert lib.dcx_motion_worst_work_bytes(m, E) >= lib.dcx_motion_work_bytes(m, E) + 12 * E


def test_python_layers_reject_bad_rules_without_a_device():
    from diffco_amd._perceptron import MotionSource, motion_worst, path_worst
    import torch

    class _Owner:
        pass
    with pytest.raises(ValueError, match="exactly one of res and max_step"):
        motion_worst(MotionSource(_Owner(), None, None, None, None, None), [[0.0, 0.0]], [[1.0, 1.0]])
    with pytest.raises(ValueError, match="exactly one of res and max_step"):
        motion_worst(MotionSource(_Owner(), None, None, None, None, None), [[0.0, 0.0]], [[1.0, 1.0]], res=4, max_step=0.1)
    with pytest.raises(ValueError, match="wrap=True"):
        motion_worst(MotionSource(_Owner(), None, None, None, None, None), [[0.0, 0.0]], [[1.0, 1.0]], res=4, wrap=True)
    with pytest.raises(ValueError, match="wrap=True"):
        path_worst(MotionSource(_Owner(), None, lambda q: q, None, None, None), torch.zeros(1, 3, 2), 0.1, wrap=True)
