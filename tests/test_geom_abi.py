"""CPU-side checks of dcx_geom_clearance's boundary: the symbol exists and the version stays 109, the header and the ctypes table
declare the same arguments, the two structs have the C layout (an obstacle row is 64 bytes), every argument error is
DCX_ERR_INVALID before anything touches a device, and without a GPU a valid call fails loudly - on a machine without a GPU."""
import ctypes
import os
import re
import subprocess

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


def test_symbol_exists_and_version_stays():
    from diffco_amd import _lib
    from diffco_amd._fkdesc import FkDesc
    res, args = _declared("dcx_geom_clearance")
    assert _lib.SYMBOLS["dcx_geom_clearance"][0] is res
    # (the table spells the description's pointer as POINTER(FkDesc); every other pointer as an address)
    table = [ctypes.c_void_p if a is ctypes.POINTER(FkDesc) else a for a in _lib.SYMBOLS["dcx_geom_clearance"][1]]
    assert table == args
    lib = _lib.load()
    assert hasattr(lib, "dcx_geom_clearance")
    assert lib.dcx_version() == 109


def test_struct_layouts_match_c(tmp_path):
    from diffco_amd import _lib
    of, pf = ("type_group", "rt", "c", "p"), ("n_groups", "sphere_base", "accumulate", "reserved")
    offs = ", ".join([f"offsetof(dcx_geom_obstacle, {f})" for f in of] + [f"offsetof(dcx_geom_opts, {f})" for f in pf])
    prog = tmp_path / "szg.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dcx.h"\n'
                    'int main(){size_t v[] = {sizeof(dcx_geom_obstacle), sizeof(dcx_geom_opts), DCX_GEOM_SPHERE, DCX_GEOM_BOX, '
                    'DCX_GEOM_CAPSULE, DCX_GEOM_CYLINDER, DCX_GEOM_TYPE_GROUP(3, 5), DCX_MAX_C, DCX_MAX_POINTS, ' + offs + '};\n'
                    'for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%zu ", v[i]);}')
    exe = tmp_path / "szg"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    from diffco_amd import _fkdesc
    assert out == [ctypes.sizeof(_lib.GeomObstacle), ctypes.sizeof(_lib.GeomOpts), _lib.GEOM_SPHERE, _lib.GEOM_BOX,
                   _lib.GEOM_CAPSULE, _lib.GEOM_CYLINDER, 3 | (5 << 8), _fkdesc.MAX_C, _fkdesc.MAX_POINTS] + \
        [getattr(_lib.GeomObstacle, f).offset for f in of] + [getattr(_lib.GeomOpts, f).offset for f in pf]
    assert ctypes.sizeof(_lib.GeomObstacle) == 64 and ctypes.sizeof(_lib.GeomOpts) == 16


def test_world_rows_are_the_c_struct():
    """World.rows() is an array of dcx_geom_obstacle"""
    import numpy as np
    from diffco_amd import _lib, geometry
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = [1, 2, 3]
    w = geometry.World().add_box("b", [2, 4, 6], T, group=5)
    row = _lib.GeomObstacle.from_buffer_copy(w.rows().tobytes())
    assert row.type_group == _lib.GEOM_BOX | (5 << 8)
    assert list(row.rt) == [0, 1, 0, -1, 0, 0, 0, 0, 1] and list(row.c) == [1, 2, 3] and list(row.p) == [1, 2, 3]


def test_header_section_is_marked_109_and_cites_the_reference():
    src = open(HEADER).read()
    at = src.index("geometric ground truth")
    assert "added under DCX_VERSION 109" in src[at:][:80]
    assert "env_interface.py:35-122" in src[at:][:6000] and "collision_checkers.py:28-125" in src[at:][:6000]


def _opts(n_groups=2, sphere_base=0, accumulate=0, reserved=0):
    from diffco_amd._lib import GeomOpts
    return GeomOpts(n_groups, sphere_base, accumulate, reserved)


def _desc(**kw):
    from helpers import make_robot
    from diffco_amd._fkdesc import FkDesc
    d = FkDesc.from_buffer_copy(bytes(make_robot("baxter_left").fk_desc()))
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(lib, desc=None, opt=None, O=3, B=8, radii=1, obstacles=1, q=1, clearance=1, witness=1, grad=1):
    # (the addresses are never read: every case below is refused, or has nothing to do, before any device work)
    p = ctypes.c_void_p
    desc = _desc() if desc is None else desc
    opt = _opts() if opt is None else opt
    return lib.dcx_geom_clearance(0, ctypes.byref(desc) if desc is not False else None, p(radii), p(obstacles), O, p(q), B,
                                  ctypes.byref(opt) if opt is not False else None, p(clearance), p(witness), p(grad), None)


def test_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    from diffco_amd._fkdesc import none_desc
    lib = _lib.load()
    cases = [
        (dict(desc=False), "spheres_fk is NULL"),
        (dict(opt=False), "options are NULL"),
        (dict(B=-1), "B < 0 or O < 0"),
        (dict(O=-1), "B < 0 or O < 0"),
        (dict(opt=_opts(reserved=1)), "reserved fields must be 0"),
        (dict(opt=_opts(n_groups=0)), "n_groups must be in [1, DCX_MAX_C]"),
        (dict(opt=_opts(n_groups=9)), "n_groups must be in [1, DCX_MAX_C]"),
        (dict(opt=_opts(sphere_base=-1)), "sphere_base < 0"),
        (dict(opt=_opts(accumulate=2)), "accumulate must be 0 or 1"),
        (dict(opt=_opts(accumulate=-1)), "accumulate must be 0 or 1"),
        (dict(desc=none_desc(3)), "points of dimension 2 or 3"),
        (dict(desc=_desc(n_points=0)), "points of dimension 2 or 3"),
        (dict(desc=_desc(n_points=33)), "points of dimension 2 or 3"),
        (dict(desc=_desc(dof=0)), "fk.dof out of range"),
        (dict(desc=_desc(kind=77)), "unknown fk.kind"),
        (dict(radii=0), "is NULL"),
        (dict(q=0), "is NULL"),
        (dict(clearance=0), "is NULL"),
        (dict(obstacles=0), "obstacles is NULL"),
    ]
    for kw, text in cases:
        rc = _call(lib, **kw)
        msg = lib.dcx_last_error().decode()
        assert rc == 1, (kw, rc, msg)
        assert text in msg, (kw, msg)
    # nothing to do is not an error, with or without buffers
    assert _call(lib, B=0) == 0
    assert _call(lib, B=0, radii=0, obstacles=0, q=0, clearance=0, witness=0, grad=0) == 0
    # more obstacles than a witness index holds: unsupported, not invalid
    assert _call(lib, O=1 << 31) == 2


def _gpu_visible():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_gpu_visible(), reason="checks the no-GPU behaviour")
def test_without_a_gpu_the_call_fails_loudly():
    import torch
    from diffco_amd import _lib, geometry
    from helpers import make_robot
    lib = _lib.load()
    # valid arguments, no obstacle (nothing would be read): refused for the missing device, not answered
    rc = _call(lib, O=0, obstacles=0, witness=0, grad=0)
    assert rc == 4 and "no HIP device" in lib.dcx_last_error().decode()
    checker = geometry.SphereWorldChecker(geometry.spheres_on_control_points(make_robot("baxter_left"), 0.05),
                                          geometry.World().add_sphere("s", 0.2))
    with pytest.raises(_lib.DcxError, match="no MI355X/HIP device"):
        checker(torch.zeros(4, 7))
