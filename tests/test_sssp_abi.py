"""CPU-side checks of the roadmap queries' boundary (dcx_sssp_run, dcx_sssp_extract_paths): the symbols exist and the version
stays 109, the header and the ctypes table declare the same arguments, the three structs have the C layout, every argument
error is reported with its message before anything touches a device, and the header section is marked as added under version
109 - on a machine without a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dcx.h")

_CTYPE = {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
          "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t}
_STRUCTS = {"dcx_graph": ("Graph", ("rowptr", "col", "weight", "N", "nnz", "reserved"), 56),
            "dcx_sssp_state": ("SsspState", ("dist", "pred", "reserved"), 32),
            "dcx_sssp_links": ("SsspLinks", ("idx", "len", "reserved"), 32)}


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


@pytest.mark.parametrize("name", ["dcx_sssp_run", "dcx_sssp_extract_paths"])
def test_symbols_exist_and_version_stays(name):
    from diffco_amd import _lib
    res, args = _declared(name)
    assert _lib.SYMBOLS[name][0] is res
    assert list(_lib.SYMBOLS[name][1]) == args
    lib = _lib.load()
    assert hasattr(lib, name)
    assert lib.dcx_version() == 109


def test_struct_layouts_match_c(tmp_path):
    from diffco_amd import _lib
    prog = tmp_path / "szs.c"
    vals = []
    for cname, (_, fields, _) in _STRUCTS.items():
        vals += [f"sizeof({cname})"] + [f"offsetof({cname}, {f})" for f in fields]
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dcx.h"\n'
                    'int main(){size_t v[] = {' + ", ".join(vals) + '};\n'
                    'for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%zu ", v[i]);}')
    exe = tmp_path / "szs"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for pyname, fields, size in _STRUCTS.values():
        cls = getattr(_lib, pyname)
        assert [f for f, _ in cls._fields_] == list(fields) and ctypes.sizeof(cls) == size
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    assert out == want


def test_header_section_is_marked_109():
    src = open(HEADER).read()
    at = src.index("roadmap queries")
    assert "added under DCX_VERSION 109" in src[at - 40:][:200]
    body = src[at:][:8000]
    # the header says that the graph is the caller's word, and what the rounds promise
    assert "do NOT check" in body and "strict decrease" in body and "does not depend on how the rounds are split" in body


def _struct(cls, *ptrs, sizes=(), reserved=(0, 0)):
    return cls(*ptrs, *sizes, (ctypes.c_int64 * 2)(*reserved))


def _run(lib, *, graph=1, links=1, state=1, Q=8, k=4, N=100, nnz=600, round0=0, n_rounds=3, changed=1, rowptr=1, col=1, weight=1,
         dist=1, pred=1, idx=1, length=1, g_res=(0, 0), s_res=(0, 0), l_res=(0, 0)):
    # (the addresses are never read: every case below is refused, or has nothing to do, before any device work)
    from diffco_amd import _lib
    p = ctypes.c_void_p
    g = _struct(_lib.Graph, rowptr, col, weight, sizes=(N, nnz), reserved=g_res)
    s = _struct(_lib.SsspState, dist, pred, reserved=s_res)
    ln = _struct(_lib.SsspLinks, idx, length, reserved=l_res)
    return lib.dcx_sssp_run(0, ctypes.byref(g) if graph else None, Q, ctypes.byref(ln) if links else None, k,
                            ctypes.byref(s) if state else None, round0, n_rounds, p(changed), None)


def _extract(lib, *, graph=1, links=1, state=1, Q=8, k=4, N=100, nnz=600, dof=3, rounds_done=5, W=16, nodes=1, mode=1, starts=1,
             goals=1, direct_len=1, path=1, count=1, out_len=1, rowptr=1, col=1, weight=1, dist=1, pred=1, idx=1, length=1,
             g_res=(0, 0), s_res=(0, 0), l_res=(0, 0)):
    from diffco_amd import _lib
    p = ctypes.c_void_p
    g = _struct(_lib.Graph, rowptr, col, weight, sizes=(N, nnz), reserved=g_res)
    s = _struct(_lib.SsspState, dist, pred, reserved=s_res)
    ln = _struct(_lib.SsspLinks, idx, length, reserved=l_res)
    return lib.dcx_sssp_extract_paths(0, ctypes.byref(g) if graph else None, p(nodes), dof, ctypes.byref(s) if state else None,
                                      rounds_done, Q, k, p(mode), p(starts), p(goals), ctypes.byref(ln) if links else None,
                                      p(direct_len), p(path), p(count), p(out_len), W, None)


_SHARED = [
    (dict(graph=0), "graph, state or links is NULL"),
    (dict(state=0), "graph, state or links is NULL"),
    (dict(links=0), "graph, state or links is NULL"),
    (dict(Q=-1), "Q < 0, N < 0 or nnz < 0"),
    (dict(N=-1), "Q < 0, N < 0 or nnz < 0"),
    (dict(nnz=-1), "Q < 0, N < 0 or nnz < 0"),
    (dict(k=0), "k must be in [1, DCX_KNN_MAX_K]"),
    (dict(k=65), "k must be in [1, DCX_KNN_MAX_K]"),
    (dict(g_res=(1, 0)), "reserved fields must be 0"),
    (dict(g_res=(0, 1)), "reserved fields must be 0"),
    (dict(s_res=(1, 0)), "reserved fields must be 0"),
    (dict(s_res=(0, 1)), "reserved fields must be 0"),
    (dict(l_res=(1, 0)), "reserved fields must be 0"),
    (dict(l_res=(0, 1)), "reserved fields must be 0"),
    (dict(rowptr=0), "rowptr, col or weight is NULL"),
    (dict(col=0), "rowptr, col or weight is NULL"),
    (dict(weight=0), "rowptr, col or weight is NULL"),
    (dict(dist=0), "dist or pred is NULL"),
    (dict(pred=0), "dist or pred is NULL"),
    (dict(idx=0), "a link array is NULL"),
    (dict(length=0), "a link array is NULL"),
]


def _refused(call, lib, cases, code=1):
    for kw, text in cases:
        rc = call(lib, **kw)
        msg = lib.dcx_last_error().decode()
        assert rc == code, (kw, rc, msg)
        assert text in msg, (kw, msg)


def test_run_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    lib = _lib.load()
    _refused(_run, lib, _SHARED + [
        (dict(round0=-1), "round0 < 0"),
        (dict(n_rounds=-1), "n_rounds < 0"),
        (dict(changed=0), "changed is NULL"),
    ])
    # nothing to do is not an error, with or without buffers; later rounds do not read the links
    assert _run(lib, Q=0) == 0
    assert _run(lib, Q=0, rowptr=0, col=0, weight=0, dist=0, pred=0, idx=0, length=0, changed=0) == 0
    assert _run(lib, n_rounds=0, changed=0) == 0
    assert _run(lib, round0=1, n_rounds=0, idx=0, length=0) == 0
    # beyond int32 indexing or one launch: unsupported, not invalid
    _refused(_run, lib, [
        (dict(N=(1 << 31) - 1), "beyond int32 indexing"),
        (dict(nnz=1 << 31), "beyond int32 indexing"),
        (dict(N=1 << 20, Q=1 << 11), "beyond int32 indexing"),
        (dict(N=1, Q=1 << 31), "beyond int32 indexing"),
        (dict(N=16, Q=65536 * 64), "more query blocks than one launch takes"),
        (dict(round0=(1 << 31) - 2, n_rounds=2), "round0 + n_rounds beyond int32"),
    ], code=2)
    assert _run(lib, N=1 << 20, Q=(1 << 11) - 1, changed=0) == 1     # (the largest N * Q is a size the call takes)
    assert "changed is NULL" in lib.dcx_last_error().decode()


def test_extract_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    lib = _lib.load()
    _refused(_extract, lib, _SHARED + [
        (dict(dof=0), "dof must be in [1, 64]"),
        (dict(dof=65), "dof must be in [1, 64]"),
        (dict(rounds_done=0), "rounds_done < 1"),
        (dict(W=-1), "W < 0"),
        (dict(nodes=0), "nodes is NULL"),
        (dict(mode=0), "count or length is NULL"),
        (dict(starts=0), "count or length is NULL"),
        (dict(goals=0), "count or length is NULL"),
        (dict(direct_len=0), "count or length is NULL"),
        (dict(count=0), "count or length is NULL"),
        (dict(out_len=0), "count or length is NULL"),
        (dict(path=0), "path is NULL with W > 0"),
    ])
    assert _extract(lib, Q=0) == 0
    assert _extract(lib, Q=0, rowptr=0, col=0, weight=0, dist=0, pred=0, idx=0, length=0, nodes=0, mode=0, starts=0, goals=0,
                    direct_len=0, path=0, count=0, out_len=0) == 0
    _refused(_extract, lib, [
        (dict(N=1 << 20, Q=1 << 11), "beyond int32 indexing"),
        (dict(N=16, Q=65536 * 64), "more query blocks than one launch takes"),
    ], code=2)
