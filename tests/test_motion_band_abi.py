"""CPU-side checks of the hybrid motion check's boundary (dcx_motion_band): the symbols exist and the version stays 109, the
header and the ctypes table declare the same arguments, dcx_motion_band_out has the C layout, every argument error is reported
before anything touches a device, the workspace size grows with E * max_samples, and the header section is marked as added under
version 109 - on a machine without a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dcx.h")

_CTYPE = {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
          "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t}
_FIELDS = ("verdict", "first_hit", "n_samples", "n_uncertain", "unc_total", "unc_edge", "unc_sample", "unc_q", "unc_cap", "reserved")


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


@pytest.mark.parametrize("name", ["dcx_motion_band", "dcx_motion_band_work_bytes"])
def test_symbols_exist_and_version_stays(name):
    from diffco_amd import _lib
    res, args = _declared(name)
    assert _lib.SYMBOLS[name][0] is res
    assert list(_lib.SYMBOLS[name][1]) == args
    lib = _lib.load()
    assert hasattr(lib, name)
    assert lib.dcx_version() == 109


def test_band_out_layout_matches_c(tmp_path):
    from diffco_amd._lib import MotionBandOut
    prog = tmp_path / "szb.c"
    offs = ", ".join(f"offsetof(dcx_motion_band_out, {f})" for f in _FIELDS)
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dcx.h"\n'
                    'int main(){size_t v[] = {sizeof(dcx_motion_band_out), ' + offs + '};\n'
                    'for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%zu ", v[i]);}')
    exe = tmp_path / "szb"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [ctypes.sizeof(MotionBandOut)] + [getattr(MotionBandOut, f).offset for f in _FIELDS]
    assert [f for f, _ in MotionBandOut._fields_] == list(_FIELDS)
    assert ctypes.sizeof(MotionBandOut) == 8 * 8 + 8 + 16


def test_header_section_is_marked_109():
    src = open(HEADER).read()
    at = src.index("hybrid motion checks")
    assert "added under DCX_VERSION 109" in src[at - 40:][:200]
    # the call takes dcx_motion_opts as it is
    from diffco_amd import _lib
    assert ctypes.sizeof(_lib.MotionOpts) == 16
    assert "dcx_motion_band_opts" not in src


def _fake_model():
    # a zeroed stand-in handle as large as any model struct (dof reads 0: every mask bit lies at or above it)
    buf = ctypes.create_string_buffer(1 << 20)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _band(lib, model, mask=0, E=4, opt=None, qa=1, qb=1, out=None, work=1, work_bytes=1 << 30, **fields):
    from diffco_amd._lib import MotionBandOut, MotionOpts
    opt = MotionOpts(8, 0.0, 8, 0) if opt is None else opt
    p = ctypes.c_void_p
    f = dict(verdict=1, first_hit=0, n_samples=0, n_uncertain=0, unc_total=1, unc_edge=1, unc_sample=1, unc_q=0, unc_cap=16)
    reserved = fields.pop("reserved", (0, 0))
    f.update(fields)
    o = MotionBandOut(*(p(f[k]) for k in _FIELDS[:8]), f["unc_cap"], (ctypes.c_int64 * 2)(*reserved))
    return lib.dcx_motion_band(model, p(qa), p(qb), E, ctypes.byref(opt) if opt is not False else None, None, None,
                               ctypes.byref(o) if out is not False else None, p(work), work_bytes, mask, None)


def test_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    from diffco_amd._lib import MotionOpts
    lib = _lib.load()
    keep, m = _fake_model()
    need = lib.dcx_motion_band_work_bytes(m, 4, 8)
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
        (dict(out=False), "out is NULL"),
        (dict(verdict=0), "verdict / unc_total is NULL"),
        (dict(unc_total=0), "verdict / unc_total is NULL"),
        (dict(unc_cap=-1), "unc_cap < 0"),
        (dict(unc_edge=0), "unc_edge / unc_sample is NULL"),
        (dict(unc_sample=0), "unc_edge / unc_sample is NULL"),
        (dict(reserved=(1, 0)), "reserved fields must be 0"),
        (dict(reserved=(0, 1)), "reserved fields must be 0"),
        (dict(opt=MotionOpts(8, 0.0, 8, 1)), "reserved must be 0"),
        (dict(work_bytes=need - 1), "smaller than dcx_motion_band_work_bytes"),
    ]
    for kw, text in cases:
        kw = dict(kw)
        rc = _band(lib, kw.pop("model", m), **kw)
        msg = lib.dcx_last_error().decode()
        assert rc == 1, (kw, rc, msg)
        assert text in msg, (kw, msg)
    # a list of capacity 0 needs no list arrays; the optional outputs may all be NULL
    # (nothing to do is not an error, with or without buffers)
    assert _band(lib, m, E=0, qa=0, qb=0, verdict=0, unc_total=0, unc_edge=0, unc_sample=0, unc_cap=0, work=0, work_bytes=0) == 0
    assert _band(lib, m, E=0) == 0
    # over the limits of one launch: unsupported, not invalid
    assert _band(lib, m, E=1 << 31, opt=MotionOpts(1, 0.0, 1, 0), work_bytes=1 << 62) == 2
    assert _band(lib, m, E=1 << 30, opt=MotionOpts(1 << 20, 0.0, 1 << 20, 0), work_bytes=1 << 62) == 2


def test_work_bytes_grows_with_the_samples():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    assert lib.dcx_motion_band_work_bytes(None, 100, 8) == 0
    assert lib.dcx_motion_band_work_bytes(m, -1, 8) == 0
    assert lib.dcx_motion_band_work_bytes(m, 100, 0) == 0
    for ms in (1, 8, 64, 1000):
        sizes = [lib.dcx_motion_band_work_bytes(m, E, ms) for E in (0, 1, 2, 63, 64, 65, 1000, 4096, 65536, 1 << 20)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0] > 0
    for E in (1, 1000, 65536):
        by_ms = [lib.dcx_motion_band_work_bytes(m, E, ms) for ms in (1, 2, 63, 64, 65, 1000, 10000)]
        assert all(b >= a for a, b in zip(by_ms, by_ms[1:])) and by_ms[-1] > by_ms[0]
        for ms, got in zip((1, 2, 63, 64, 65, 1000, 10000), by_ms):
            # never below the check's workspace; it holds a code byte per possible sample, the status word and the offsets
            assert got >= lib.dcx_motion_work_bytes(m, E) + E * ms + 4 * E + 8 * (E + 1)


def test_python_layers_reject_bad_rules_without_a_device():
    from diffco_amd._perceptron import MotionSource, motion_band

    class _Owner:
        pass
    with pytest.raises(ValueError, match="exactly one of res and max_step"):
        motion_band(MotionSource(_Owner(), None, None, None, None, None), [[0.0, 0.0]], [[1.0, 1.0]], -1.0, 1.0)
    with pytest.raises(ValueError, match="exactly one of res and max_step"):
        motion_band(MotionSource(_Owner(), None, None, None, None, None), [[0.0, 0.0]], [[1.0, 1.0]], -1.0, 1.0, res=4, max_step=0.1)
    with pytest.raises(ValueError, match="wrap=True"):
        motion_band(MotionSource(_Owner(), None, None, None, None, None), [[0.0, 0.0]], [[1.0, 1.0]], -1.0, 1.0, res=4, wrap=True)
