"""CPU-side checks of the lazy roadmap queries' boundary (dcx_sssp_mark_routes_work_bytes, dcx_sssp_mark_routes,
dcx_graph_apply_checks): the symbols exist and the version stays 109, the header and the ctypes table declare the same
arguments, dcx_lazy_graph has the C layout, the workspace size follows the plan, every argument error is reported with its
message before anything touches a device, and the header section is marked as added under version 109 - on a machine without a
GPU."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dcx.h")

_CTYPE = {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
          "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t}
_FIELDS = ("eid", "ent", "ends", "state", "M", "reserved")


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


@pytest.mark.parametrize("name", ["dcx_sssp_mark_routes_work_bytes", "dcx_sssp_mark_routes", "dcx_graph_apply_checks"])
def test_symbols_exist_and_version_stays(name):
    from diffco_amd import _lib
    res, args = _declared(name)
    assert _lib.SYMBOLS[name][0] is res
    assert list(_lib.SYMBOLS[name][1]) == args
    lib = _lib.load()
    assert hasattr(lib, name)
    assert lib.dcx_version() == 109


def test_struct_layout_matches_c(tmp_path):
    from diffco_amd import _lib
    vals = ["sizeof(dcx_lazy_graph)"] + [f"offsetof(dcx_lazy_graph, {f})" for f in _FIELDS]
    prog = tmp_path / "szs.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dcx.h"\n'
                    'int main(){size_t v[] = {' + ", ".join(vals) + '};\n'
                    'for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%zu ", v[i]);}')
    exe = tmp_path / "szs"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    cls = _lib.LazyGraph
    assert [f for f, _ in cls._fields_] == list(_FIELDS) and ctypes.sizeof(cls) == 56
    assert out == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in _FIELDS]


def test_header_section_is_marked_109():
    src = open(HEADER).read()
    at = src.index("lazy roadmap queries")
    assert "added under DCX_VERSION 109" in src[at - 40:][:200]
    body = src[at:][:9000]
    # the header says that the index arrays are the caller's word, that the graph is written, and why the loop starts over
    assert "do NOT check" in body and "weight IS WRITTEN" in body and "distances only grow when edges go" in body
    assert "ascending order" in body and "plain store" in body


def test_work_bytes_follow_the_plan():
    from diffco_amd import _lib
    fn = _lib.load().dcx_sssp_mark_routes_work_bytes
    assert fn(0) == 0 and fn(-1) == 0 and fn(1 << 31) == 0
    last = 0
    for M in (1, 15, 16, 17, 4095, 4096, 4097, 1 << 20, (1 << 31) - 1):
        groups = (M + 15) // 16
        need = 16 * groups + 4 * (groups + 1)                       # a mark byte per edge in whole groups, an offset per group
        got = fn(M)
        assert need <= got <= need + 512 and got % 256 == 0 and got >= last, M
        last = got


def _struct(cls, *ptrs, sizes=(), reserved=(0, 0)):
    return cls(*ptrs, *sizes, (ctypes.c_int64 * 2)(*reserved))


def _graph_args(kw):
    from diffco_amd import _lib
    g = _struct(_lib.Graph, kw["rowptr"], kw["col"], kw["weight"], sizes=(kw["N"], kw["nnz"]), reserved=kw["g_res"])
    lz = _struct(_lib.LazyGraph, kw["eid"], kw["ent"], kw["ends"], kw["edge_state"], sizes=(kw["M"],), reserved=kw["z_res"])
    return (ctypes.byref(g) if kw["graph"] else None), (ctypes.byref(lz) if kw["lazy"] else None)


_DEFAULTS = dict(graph=1, lazy=1, state=1, links=1, Q=8, k=4, N=100, nnz=600, M=300, dof=3, rounds_done=5, capacity=300, rowptr=1,
                 col=1, weight=1, eid=1, ent=1, ends=1, edge_state=1, dist=1, pred=1, idx=1, length=1, nodes=1, mode=1, pending=1,
                 lst=1, qa=1, qb=1, n_out=1, work=256, work_bytes=1 << 20, hit=1, any_blocked=1, g_res=(0, 0), z_res=(0, 0),
                 s_res=(0, 0), l_res=(0, 0))


def _mark(lib, **over):
    # (the addresses are never read: every case below is refused, or has nothing to do, before any device work)
    from diffco_amd import _lib
    kw = dict(_DEFAULTS, **over)
    p = ctypes.c_void_p
    g, lz = _graph_args(kw)
    s = _struct(_lib.SsspState, kw["dist"], kw["pred"], reserved=kw["s_res"])
    ln = _struct(_lib.SsspLinks, kw["idx"], kw["length"], reserved=kw["l_res"])
    return lib.dcx_sssp_mark_routes(0, g, lz, p(kw["nodes"]), kw["dof"], ctypes.byref(s) if kw["state"] else None, kw["rounds_done"],
                                    kw["Q"], kw["k"], p(kw["mode"]), ctypes.byref(ln) if kw["links"] else None, p(kw["pending"]),
                                    p(kw["lst"]), p(kw["qa"]), p(kw["qb"]), kw["capacity"], p(kw["n_out"]), p(kw["work"]),
                                    kw["work_bytes"], None)


def _apply(lib, **over):
    kw = dict(_DEFAULTS, **over)
    p = ctypes.c_void_p
    g, lz = _graph_args(kw)
    return lib.dcx_graph_apply_checks(0, g, lz, p(kw["lst"]), p(kw["n_out"]), p(kw["hit"]), p(kw["any_blocked"]), None)


def _refused(call, lib, cases, code=1):
    for kw, text in cases:
        rc = call(lib, **kw)
        msg = lib.dcx_last_error().decode()
        assert rc == code, (kw, rc, msg)
        assert text in msg, (kw, msg)


_SHARED = [
    (dict(graph=0), "graph or lazy is NULL"),
    (dict(lazy=0), "graph or lazy is NULL"),
    (dict(N=-1), "N < 0, nnz < 0 or M < 0"),
    (dict(nnz=-1), "N < 0, nnz < 0 or M < 0"),
    (dict(M=-1), "N < 0, nnz < 0 or M < 0"),
    (dict(g_res=(1, 0)), "reserved fields must be 0"),
    (dict(g_res=(0, 1)), "reserved fields must be 0"),
    (dict(z_res=(1, 0)), "reserved fields must be 0"),
    (dict(z_res=(0, 1)), "reserved fields must be 0"),
    (dict(ent=0), "the edges' state is NULL"),
    (dict(edge_state=0), "the edges' state is NULL"),
]


def test_mark_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    lib = _lib.load()
    _refused(_mark, lib, _SHARED + [
        (dict(state=0), "graph, state or links is NULL"),
        (dict(links=0), "graph, state or links is NULL"),
        (dict(Q=-1), "Q < 0, N < 0 or nnz < 0"),
        (dict(k=0), "k must be in [1, DCX_KNN_MAX_K]"),
        (dict(k=65), "k must be in [1, DCX_KNN_MAX_K]"),
        (dict(s_res=(1, 0)), "reserved fields must be 0"),
        (dict(l_res=(0, 1)), "reserved fields must be 0"),
        (dict(dof=0), "dof must be in [1, 64]"),
        (dict(dof=65), "dof must be in [1, 64]"),
        (dict(rounds_done=0), "rounds_done < 1"),
        (dict(capacity=-1), "capacity < 0"),
        (dict(rowptr=0), "rowptr or col is NULL"),
        (dict(col=0), "rowptr or col is NULL"),
        (dict(dist=0), "dist or pred is NULL"),
        (dict(pred=0), "dist or pred is NULL"),
        (dict(eid=0), "the edges' state is NULL"),
        (dict(ends=0), "the edges' state is NULL"),
        (dict(idx=0), "a link array is NULL"),
        (dict(length=0), "a link array is NULL"),
        (dict(nodes=0), "nodes is NULL"),
        (dict(mode=0), "mode, pending or n_out is NULL"),
        (dict(pending=0), "mode, pending or n_out is NULL"),
        (dict(n_out=0), "mode, pending or n_out is NULL"),
        (dict(lst=0), "list, qa or qb is NULL with capacity > 0"),
        (dict(qa=0), "list, qa or qb is NULL with capacity > 0"),
        (dict(qb=0), "list, qa or qb is NULL with capacity > 0"),
        (dict(work=0), "the workspace is NULL, misaligned or smaller"),
        (dict(work=264), "the workspace is NULL, misaligned or smaller"),
        (dict(work_bytes=lib.dcx_sssp_mark_routes_work_bytes(300) - 1), "the workspace is NULL, misaligned or smaller"),
    ])
    # nothing to do is not an error, with or without buffers
    nothing = dict(rowptr=0, col=0, weight=0, eid=0, ent=0, ends=0, edge_state=0, dist=0, pred=0, idx=0, length=0, nodes=0, mode=0,
                   pending=0, lst=0, qa=0, qb=0, n_out=0, work=0, work_bytes=0)
    assert _mark(lib, Q=0) == 0 and _mark(lib, M=0) == 0
    assert _mark(lib, Q=0, **nothing) == 0 and _mark(lib, M=0, **nothing) == 0
    # beyond int32 indexing: unsupported, not invalid
    _refused(_mark, lib, [
        (dict(N=(1 << 31) - 1), "beyond int32 indexing"),
        (dict(nnz=1 << 31), "beyond int32 indexing"),
        (dict(M=1 << 31), "beyond int32 indexing"),
        (dict(N=1 << 20, Q=1 << 11), "beyond int32 indexing"),
    ], code=2)
    # the weight is not read, and capacity 0 needs no list
    assert _mark(lib, weight=0, mode=0) == 1 and "mode, pending or n_out" in lib.dcx_last_error().decode()
    assert _mark(lib, capacity=0, lst=0, qa=0, qb=0, work=0) == 1 and "the workspace is NULL" in lib.dcx_last_error().decode()


def test_apply_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    lib = _lib.load()
    _refused(_apply, lib, _SHARED + [
        (dict(weight=0), "weight, ent or the edges' state is NULL"),
        (dict(lst=0), "list, n_out, hit or any_blocked is NULL"),
        (dict(n_out=0), "list, n_out, hit or any_blocked is NULL"),
        (dict(hit=0), "list, n_out, hit or any_blocked is NULL"),
        (dict(any_blocked=0), "list, n_out, hit or any_blocked is NULL"),
    ])
    assert _apply(lib, M=0) == 0
    assert _apply(lib, M=0, weight=0, ent=0, edge_state=0, lst=0, n_out=0, hit=0, any_blocked=0) == 0
    _refused(_apply, lib, [
        (dict(nnz=1 << 31), "beyond int32 indexing"),
        (dict(M=1 << 31), "beyond int32 indexing"),
    ], code=2)
