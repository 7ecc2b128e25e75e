"""CPU-side checks of the dense-check trajectory loop's boundary (dcx_traj_dense_step / _work_bytes / _run): the ctypes mirrors
of dcx_traj_dense_opts and dcx_traj_dense_io have the C layout, the header, the ctypes table and the library agree, and every
argument error is reported with its code and text before anything touches a device - on a machine without a GPU."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dcx.h")
NAMES = ("dcx_traj_dense_step", "dcx_traj_dense_work_bytes", "dcx_traj_dense_run")
OPT_FIELDS = ("max_step", "max_samples", "wrap_mask", "rewrap_mask", "normalize", "stop_tol", "reserved")
IO_FIELDS = ("move", "history", "n_checks", "edge_cost", "grad_a", "grad_b", "n_samples")


def test_dense_structs_layout_matches_c(tmp_path):
    from diffco_amd._lib import TrajDenseIO, TrajDenseOpts
    offs = ", ".join([f"offsetof(dcx_traj_dense_opts, {f})" for f in OPT_FIELDS] + [f"offsetof(dcx_traj_dense_io, {f})" for f in IO_FIELDS])
    prog = tmp_path / "szd.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dcx.h"\n'
                    'int main(){size_t v[] = {sizeof(dcx_traj_dense_opts), sizeof(dcx_traj_dense_io), ' + offs + '};\n'
                    'for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%zu ", v[i]);}')
    exe = tmp_path / "szd"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [ctypes.sizeof(TrajDenseOpts), ctypes.sizeof(TrajDenseIO)] + \
        [getattr(TrajDenseOpts, f).offset for f in OPT_FIELDS] + [getattr(TrajDenseIO, f).offset for f in IO_FIELDS]
    assert ctypes.sizeof(TrajDenseOpts) == 48 and ctypes.sizeof(TrajDenseIO) == 56


def test_dense_symbols_in_header_table_and_library():
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
    # the model at most (its dof reads 0); nothing selects a device
    buf = ctypes.create_string_buffer(1 << 20)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _state(R=2, W=5, null=None):
    from diffco_amd._lib import TrajState
    names = ("path", "adam_m", "adam_v", "limits", "col_score", "col_grad", "stats", "lowest_loss", "lowest_obj", "lowest_path",
             "best_valid_obj", "best_valid_path", "done", "steps")
    # (col_score / col_grad are not read by the dense calls: NULL throughout)
    return TrajState(R, W, *(None if n in ("col_score", "col_grad", null) else ctypes.c_void_p(1) for n in names))


def _opt(lr=0.1, beta1=0.9, beta2=0.999):
    from diffco_amd._lib import TrajOpts
    return TrajOpts(lr, beta1, beta2, 1e-8, 1, 10, 10, 10, 0.0, 0.3, 1e-2, 1e-4)


def _dopt(max_step=0.1, max_samples=8, wrap=0, rewrap=0, normalize=0, stop_tol=0.0, reserved=(0, 0, 0, 0)):
    from diffco_amd._lib import TrajDenseOpts
    o = TrajDenseOpts(max_step, max_samples, wrap, rewrap, normalize, stop_tol)
    for i, v in enumerate(reserved):
        o.reserved[i] = v
    return o


def _io(n_checks=1, edges=(1, 1, 1, 1)):
    from diffco_amd._lib import TrajDenseIO
    p = lambda v: ctypes.c_void_p(v) if v else None
    return TrajDenseIO(None, None, p(n_checks), *(p(e) for e in edges))


def _run(lib, model, st=None, opt=None, dopt=None, io=None, first_step=1, n_iters=1, work=1, work_bytes=1 << 40):
    ref = lambda o, default: None if o is False else ctypes.byref(default if o is None else o)
    keep = (_state(), _opt(), _dopt(), _io())
    # the pointers are never dereferenced: every case below fails its argument check first
    return lib.dcx_traj_dense_run(model, ref(st, keep[0]), ref(opt, keep[1]), ref(dopt, keep[2]), ref(io, keep[3]), None, first_step,
                                  n_iters, ctypes.c_void_p(work) if work else None, work_bytes, None)


def test_dense_work_bytes():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    assert lib.dcx_traj_dense_work_bytes(m, 2, 5, 8) > 0
    assert lib.dcx_traj_dense_work_bytes(None, 2, 5, 8) == 0
    assert lib.dcx_traj_dense_work_bytes(m, -1, 5, 8) == 0
    assert lib.dcx_traj_dense_work_bytes(m, 2, 1, 8) == 0
    assert lib.dcx_traj_dense_work_bytes(m, 2, 5, 0) == 0
    assert lib.dcx_traj_dense_work_bytes(m, 200, 5, 8) > lib.dcx_traj_dense_work_bytes(m, 2, 5, 8)
    assert lib.dcx_traj_dense_work_bytes(m, 2, 50, 8) > lib.dcx_traj_dense_work_bytes(m, 2, 5, 8)
    assert lib.dcx_traj_dense_work_bytes(m, 2, 5, 64) > lib.dcx_traj_dense_work_bytes(m, 2, 5, 8)


def test_dense_run_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    need = lib.dcx_traj_dense_work_bytes(m, 2, 5, 8)
    cases = [
        (dict(model=None), "model is NULL"),
        (dict(st=False), "is NULL"),
        (dict(opt=False), "is NULL"),
        (dict(dopt=False), "is NULL"),
        (dict(io=False), "is NULL"),
        (dict(n_iters=-1), "n_iters >= 0"),
        (dict(first_step=0), "first_step is 1-based"),
        (dict(st=_state(null="path")), "state pointer is NULL"),
        (dict(st=_state(null="steps")), "state pointer is NULL"),
        (dict(opt=_opt(beta1=1.0)), "Adam options"),
        (dict(dopt=_dopt(max_step=0.0)), "max_step must be > 0"),
        (dict(dopt=_dopt(max_step=-1.0)), "max_step must be > 0"),
        (dict(dopt=_dopt(max_step=float("nan"))), "max_step must be > 0"),
        (dict(dopt=_dopt(max_samples=0)), "max_samples must be >= 1"),
        (dict(dopt=_dopt(normalize=2)), "normalize must be 0 or 1"),
        (dict(dopt=_dopt(stop_tol=-0.5)), "stop_tol must be >= 0"),
        (dict(dopt=_dopt(wrap=1)), "bit at or above dof"),      # (the stand-in model's dof reads 0)
        (dict(dopt=_dopt(rewrap=1 << 40)), "bit at or above dof"),
        (dict(dopt=_dopt(reserved=(0, 1, 0, 0))), "reserved"),
        (dict(dopt=_dopt(reserved=(0, 0, 0, 7))), "reserved"),
        (dict(io=_io(edges=(1, 1, 0, 1))), "all four per-edge arrays or none"),
        (dict(io=_io(n_checks=0)), "n_checks is NULL"),
        (dict(work=0), "work is NULL"),
        (dict(work_bytes=need - 1), "smaller than dcx_traj_dense_work_bytes"),
    ]
    for kw, text in cases:
        rc = _run(lib, kw.pop("model", m), **kw)
        msg = lib.dcx_last_error().decode()
        assert rc == 1, (kw, rc, msg)
        assert text in msg, (kw, msg)
    # a path of one waypoint, or of more than a block's lanes: outside the compiled set
    for W in (1, 1025):
        assert _run(lib, m, st=_state(W=W)) == 2
    # what the motion-cost calls inside could refuse is refused up front as well (the stand-in model's feature width reads 0)
    assert _run(lib, m) == 2 and "no motion-cost kernel" in lib.dcx_last_error().decode()
    assert _run(lib, m, st=_state(R=1 << 20, W=1024), dopt=_dopt(max_samples=1 << 30), work_bytes=1 << 63) == 2
    assert "too large for one launch" in lib.dcx_last_error().decode()
    # nothing to do is not an error, and needs no buffers: no iterations, no paths (the per-edge arrays may all be NULL)
    assert _run(lib, m, n_iters=0, work=0, work_bytes=0, io=_io(edges=(0, 0, 0, 0))) == 0
    from diffco_amd._lib import TrajState
    assert _run(lib, m, st=TrajState(0, 5), io=_io(n_checks=0, edges=(0, 0, 0, 0)), work=0, work_bytes=0) == 0


def test_dense_step_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    from diffco_amd._fkdesc import none_desc
    lib = _lib.load()
    fk = none_desc(3)

    def step(fk_=fk, st=None, dopt=None, io=None, C_=1, step_=1):
        st, opt, dopt, io = st or _state(), _opt(), dopt or _dopt(), io or _io()
        return lib.dcx_traj_dense_step(0, ctypes.byref(fk_) if fk_ is not None else None, ctypes.byref(st), ctypes.byref(opt),
                                       ctypes.byref(dopt), ctypes.byref(io), C_, step_, None)

    cases = [
        (dict(fk_=None), 1, "fk is NULL"),
        (dict(step_=0), 1, "step is 1-based"),
        (dict(C_=0), 2, "DCX_MAX_C"),
        (dict(io=_io(edges=(0, 0, 0, 0))), 1, "per-edge array is NULL"),
        (dict(io=_io(edges=(1, 0, 1, 1))), 1, "all four per-edge arrays or none"),
        (dict(dopt=_dopt(rewrap=0b1000)), 1, "bit at or above dof"),
        (dict(dopt=_dopt(max_samples=-2)), 1, "max_samples must be >= 1"),
        (dict(st=_state(null="done")), 1, "state pointer is NULL"),
    ]
    for kw, code, text in cases:
        rc = step(**kw)
        msg = lib.dcx_last_error().decode()
        assert rc == code, (kw, rc, msg)
        assert text in msg, (kw, msg)
