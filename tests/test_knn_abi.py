"""CPU-side checks of dcx_knn's boundary: the symbols exist and the version stays 109, the header and the ctypes table declare the
same arguments, dcx_knn_opts has the C layout, every argument error is reported before anything touches a device, the workspace
size never shrinks as Q, N or k grow, and the header section is marked as added under version 109 - on a machine without a GPU."""
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
_FIELDS = ("k", "reserved0", "wrap_mask", "max_dist2", "reserved1", "self_offset", "reserved")


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


@pytest.mark.parametrize("name", ["dcx_knn", "dcx_knn_work_bytes"])
def test_symbols_exist_and_version_stays(name):
    from diffco_amd import _lib
    res, args = _declared(name)
    assert _lib.SYMBOLS[name][0] is res
    assert list(_lib.SYMBOLS[name][1]) == args
    lib = _lib.load()
    assert hasattr(lib, name)
    assert lib.dcx_version() == 109


def test_opts_layout_matches_c(tmp_path):
    from diffco_amd._lib import KNN_MAX_K, KnnOpts
    prog = tmp_path / "szk.c"
    offs = ", ".join(f"offsetof(dcx_knn_opts, {f})" for f in _FIELDS)
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dcx.h"\n'
                    'int main(){size_t v[] = {sizeof(dcx_knn_opts), DCX_KNN_MAX_K, ' + offs + '};\n'
                    'for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%zu ", v[i]);}')
    exe = tmp_path / "szk"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [ctypes.sizeof(KnnOpts), KNN_MAX_K] + [getattr(KnnOpts, f).offset for f in _FIELDS]
    assert [f for f, _ in KnnOpts._fields_] == list(_FIELDS)
    assert ctypes.sizeof(KnnOpts) == 48 and KNN_MAX_K == 64


def test_header_section_is_marked_109():
    src = open(HEADER).read()
    at = src.index("k-nearest neighbours")
    assert "added under DCX_VERSION 109" in src[at - 40:][:200]
    # the header says that a wrapped distance depends on the direction
    assert "depends on the" in src[at:][:3000] and "direction" in src[at:][:3000]


def _opts(k=4, mask=0, max_dist2=math.inf, self_offset=-1, r0=0, r1=0, reserved=(0, 0)):
    from diffco_amd._lib import KnnOpts
    return KnnOpts(k, r0, mask, max_dist2, r1, self_offset, (ctypes.c_int64 * 2)(*reserved))


def _knn(lib, Q=8, N=100, dof=3, opt=None, queries=1, points=1, idx=1, dist2=1, work=1, work_bytes=1 << 40):
    # (the addresses are never read: every case below is refused, or has nothing to do, before any device work)
    p = ctypes.c_void_p
    opt = _opts() if opt is None else opt
    return lib.dcx_knn(0, p(queries), Q, p(points), N, dof, ctypes.byref(opt) if opt is not False else None, p(idx), p(dist2),
                       p(work), work_bytes, None)


def test_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    lib = _lib.load()
    need = lib.dcx_knn_work_bytes(8, 100, 3, 4)
    assert need > 0
    cases = [
        (dict(opt=False), "options are NULL"),
        (dict(queries=0), "is NULL"),
        (dict(points=0), "points is NULL"),
        (dict(idx=0), "is NULL"),
        (dict(dist2=0), "is NULL"),
        (dict(work=0), "is NULL"),
        (dict(Q=-1), "Q < 0 or N < 0"),
        (dict(N=-1), "Q < 0 or N < 0"),
        (dict(dof=0), "dof must be in [1, 64]"),
        (dict(dof=65), "dof must be in [1, 64]"),
        (dict(opt=_opts(k=0)), "k must be in [1, DCX_KNN_MAX_K]"),
        (dict(opt=_opts(k=65)), "k must be in [1, DCX_KNN_MAX_K]"),
        (dict(opt=_opts(mask=0b1000)), "wrap_mask has a bit at or above dof"),
        (dict(opt=_opts(mask=1 << 63)), "wrap_mask has a bit at or above dof"),
        (dict(opt=_opts(max_dist2=math.nan)), "max_dist2 is NaN or negative"),
        (dict(opt=_opts(max_dist2=-1.0)), "max_dist2 is NaN or negative"),
        (dict(opt=_opts(self_offset=-2)), "self_offset < -1"),
        (dict(opt=_opts(r0=1)), "reserved fields must be 0"),
        (dict(opt=_opts(r1=1)), "reserved fields must be 0"),
        (dict(opt=_opts(reserved=(1, 0))), "reserved fields must be 0"),
        (dict(opt=_opts(reserved=(0, 1))), "reserved fields must be 0"),
        (dict(work_bytes=need - 1), "smaller than dcx_knn_work_bytes"),
    ]
    for kw, text in cases:
        rc = _knn(lib, **kw)
        msg = lib.dcx_last_error().decode()
        assert rc == 1, (kw, rc, msg)
        assert text in msg, (kw, msg)
    # a full mask at dof = 64 is a valid one (refused here only for its workspace, the check after the mask's)
    assert _knn(lib, dof=64, opt=_opts(mask=(1 << 64) - 1), work_bytes=0) == 1
    assert "smaller than dcx_knn_work_bytes" in lib.dcx_last_error().decode()
    # nothing to do is not an error, with or without buffers
    assert _knn(lib, Q=0) == 0
    assert _knn(lib, Q=0, queries=0, points=0, idx=0, dist2=0, work=0, work_bytes=0) == 0
    # beyond one launch: unsupported, not invalid
    assert _knn(lib, N=1 << 31, work_bytes=1 << 62) == 2
    assert _knn(lib, Q=1 << 40, N=1 << 20, work_bytes=1 << 62) == 2
    assert _knn(lib, N=(1 << 31) - 1, work_bytes=0) == 1   # (the largest N is a size the call takes)


def test_work_bytes_is_monotone_and_zero_for_invalid_arguments():
    from diffco_amd import _lib
    lib = _lib.load()
    wb = lib.dcx_knn_work_bytes
    for bad in [(-1, 10, 3, 4), (10, -1, 3, 4), (10, 10, 0, 4), (10, 10, 65, 4), (10, 10, 3, 0), (10, 10, 3, 65), (10, 1 << 31, 3, 4),
                (1 << 40, 1 << 20, 3, 4)]:
        assert wb(*bad) == 0, bad
    Qs = (0, 1, 2, 63, 64, 65, 300, 4096, 16320, 16384, 32704, 32768, 65536, 1 << 20)
    Ns = (0, 1, 4, 63, 64, 65, 1000, 1024, 1025, 4097, 100000, 1000000, 1 << 24, (1 << 31) - 1)
    ks = (1, 2, 5, 16, 63, 64)
    for k in ks:
        for N in Ns:
            sizes = [wb(Q, N, 7, k) for Q in Qs]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0] > 0, (k, N, sizes)
        for Q in Qs:
            sizes = [wb(Q, N, 7, k) for N in Ns]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, (k, Q, sizes)
    for Q in Qs:
        for N in Ns:
            sizes = [wb(Q, N, 7, k) for k in ks]
            assert all(b > a for a, b in zip(sizes, sizes[1:])), (Q, N, sizes)
    # a forced split is what the size follows (the GPU tests hold the results to be the same under it)
    try:
        assert lib.dcx_debug_set(b"knn_split", 7) == 0
        assert wb(300, 1000, 7, 16) >= 300 * 7 * 16 * 8
        assert lib.dcx_debug_set(b"knn_split", 1) == 0
        assert 0 < wb(300, 1000, 7, 16) < 300 * 7 * 16 * 8
    finally:
        assert lib.dcx_debug_set(b"knn_split", 0) == 0


def test_python_layer_rejects_bad_arguments_without_a_device():
    import torch
    from diffco_amd import roadmap
    x = torch.zeros(5, 3)
    with pytest.raises(ValueError, match="must be"):
        roadmap.host_knn(torch.zeros(5, 2), x, 2)
    with pytest.raises(ValueError, match="k must be"):
        roadmap.host_knn(x, x, 65)
    with pytest.raises(ValueError, match="exclude_self"):
        roadmap.host_knn(torch.zeros(4, 3), x, 2, exclude_self=True)
    with pytest.raises(ValueError, match="bit at or above dof"):
        roadmap.host_knn(x, x, 2, wrap=0b1000)
