"""CPU-side checks of the boundary of RRT* under clearance-weighted edge costs (dcx_rrtstar_run_cost,
dcx_rrtstar_run_sampled_cost and their size queries): the symbols exist and the version stays 109, the header and the ctypes
table declare the same arguments, dcx_rrtstar_cost_opts has the C layout, every new argument error - and every error of the calls
they extend - is reported before anything touches a device, the workspace sizes are 0 for refused arguments and not below the
length planner's, and the header section states the contract - on a machine without a GPU."""
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
_COST = ("mode", "gain", "band", "reserved0", "reserved")
_STATE = ("nodes", "parent", "elen", "cost", "count", "status", "goal_node", "first_round")
_NAMES = ["dcx_rrtstar_cost_work_bytes", "dcx_rrtstar_run_cost", "dcx_rrtstar_sampled_cost_work_bytes", "dcx_rrtstar_run_sampled_cost"]


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


@pytest.mark.parametrize("name", _NAMES)
def test_symbols_exist_and_version_stays(name):
    from diffco_amd import _lib
    res, args = _declared(name)
    assert _lib.SYMBOLS[name][0] is res
    assert list(_lib.SYMBOLS[name][1]) == args
    lib = _lib.load()
    assert hasattr(lib, name)
    assert lib.dcx_version() == 109


def test_struct_layout_matches_c(tmp_path):
    from diffco_amd._lib import RRTSTAR_COST_PEAK, RrtStarCostOpts
    prog = tmp_path / "szs.c"
    offs = ", ".join(f"offsetof(dcx_rrtstar_cost_opts, {f})" for f in _COST)
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dcx.h"\n'
                    'int main(){size_t v[] = {sizeof(dcx_rrtstar_cost_opts), DCX_RRTSTAR_COST_PEAK, ' + offs + '};\n'
                    'for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%zu ", v[i]);}')
    exe = tmp_path / "szs"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [ctypes.sizeof(RrtStarCostOpts), RRTSTAR_COST_PEAK] + [getattr(RrtStarCostOpts, f).offset for f in _COST]
    assert [f for f, _ in RrtStarCostOpts._fields_] == list(_COST)
    assert ctypes.sizeof(RrtStarCostOpts) == 32 and RRTSTAR_COST_PEAK == 1


def test_header_section_states_the_contract():
    src = open(HEADER).read()
    at = src.index("batched RRT*: clearance-weighted edge costs (added")
    assert "added under DCX_VERSION 109" in src[at:][:80]
    assert src.index("batched RRT*: samples drawn on the device (added") < at < src.index("batched path shortcutting and RRT path extraction (added")
    body = src[at:][:9000]
    for word in ("free  <=>  w <= 0", "pen = fmaxf(w + band, +0)", "f   = 1 + gain * pen", "C   = L * f", "rounded alone, never contracted",
                 "a hinge where the reference has exp", "bit for bit", "expf", "score_dist", "motionCost",
                 "(bits(cost[u_j] + Lj), u_j) < (bits(c0), near)", "cost[x] + L' < cost[v]", "The pruning by the lower bounds is exact",
                 "gain == 0 gives f == 1 and C == L bit for bit", "stays admissible because C >= L", "DESIGN.md 3.4q",
                 "The size queries are 0 for arguments the calls refuse"):
        assert word in body, word
    # the length planner's own section and structs are as they were: the objective travels beside them
    assert "    int64_t  reserved[2];  /* 0 " in src[src.index("typedef struct dcx_rrtstar_opts"):][:1200]


def _fake_model():
    # a zeroed stand-in handle as large as any model struct (dof reads 0: every mask bit lies at or above it)
    buf = ctypes.create_string_buffer(1 << 20)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _opts(rng=0.5, max_step=0.1, radius=1.0, max_samples=16, slots=4, near=8, cap=64, r0=0, mask=0, reserved=(0, 0)):
    from diffco_amd._lib import RrtStarOpts
    return RrtStarOpts(rng, max_step, radius, max_samples, slots, near, cap, r0, mask, (ctypes.c_int64 * 2)(*reserved))


def _cost(mode=1, gain=1.0, band=0.1, r0=0, reserved=(0, 0)):
    from diffco_amd._lib import RrtStarCostOpts
    return RrtStarCostOpts(mode, gain, band, r0, (ctypes.c_int64 * 2)(*reserved))


def _sample(limits=1, tries=8, goal_bias=0.1, uniform_mix=0.0, mode=1, slots=4, cap=64, dof=0, r0=0, mask=0):
    from diffco_amd._lib import RrtStarSampleOpts
    return RrtStarSampleOpts(limits, 0, goal_bias, uniform_mix, mode, tries, slots, cap, dof, r0, mask, (ctypes.c_int64 * 2)(0, 0))


def _state(**null):
    from diffco_amd._lib import RrtStarState
    return RrtStarState(*(0 if null.get(f) else 1 for f in _STATE))


def _run(lib, model, R=8, T=2, round0=0, opt=None, cost=None, state=None, goals=1, samples=1, work=1, work_bytes=1 << 40):
    # (the addresses are never read: every case below is refused, or has nothing to do, before any device work)
    p = ctypes.c_void_p
    opt = _opts() if opt is None else opt
    cost = _cost() if cost is None else cost
    state = _state() if state is None else state
    return lib.dcx_rrtstar_run_cost(model, ctypes.byref(state) if state is not False else None, R, p(goals), p(samples), T, round0,
                                    ctypes.byref(opt) if opt is not False else None, ctypes.byref(cost) if cost is not False else None,
                                    None, p(work), work_bytes, None)


def _run_sampled(lib, model, R=8, T=2, round0=0, opt=None, cost=None, sample=None, state=None, goals=1, work=1, work_bytes=1 << 40):
    p = ctypes.c_void_p
    opt = _opts() if opt is None else opt
    cost = _cost() if cost is None else cost
    sample = _sample() if sample is None else sample
    state = _state() if state is None else state
    return lib.dcx_rrtstar_run_sampled_cost(model, ctypes.byref(state) if state is not False else None, R, p(goals),
                                            ctypes.byref(sample) if sample is not False else None, T, round0,
                                            ctypes.byref(opt) if opt is not False else None,
                                            ctypes.byref(cost) if cost is not False else None, None, p(work), work_bytes, None, None, None)


_COST_ERRORS = [
    (dict(cost=False), "cost options are NULL"),
    (dict(cost=_cost(mode=0)), "cost mode must be DCX_RRTSTAR_COST_PEAK"),
    (dict(cost=_cost(mode=2)), "cost mode must be DCX_RRTSTAR_COST_PEAK"),
    (dict(cost=_cost(gain=-1.0)), "cost gain must be >= 0"),
    (dict(cost=_cost(gain=math.nan)), "cost gain must be >= 0"),
    (dict(cost=_cost(band=-0.5)), "cost band must be >= 0"),
    (dict(cost=_cost(band=math.nan)), "cost band must be >= 0"),
    (dict(cost=_cost(r0=1)), "reserved fields of the cost options must be 0"),
    (dict(cost=_cost(reserved=(1, 0))), "reserved fields of the cost options must be 0"),
    (dict(cost=_cost(reserved=(0, 1))), "reserved fields of the cost options must be 0"),
]
# those of dcx_rrtstar_run, which both calls extend
_RUN_ERRORS = [
    (dict(model=None), "model is NULL"),
    (dict(opt=False), "options are NULL"),
    (dict(state=False), "state or one of its pointers is NULL"),
    (dict(goals=0), "state or one of its pointers is NULL"),
    (dict(work=0), "work is NULL"),
    (dict(R=-1), "R < 0"),
    (dict(T=-1), "T < 0"),
    (dict(round0=-1), "round0 < 0"),
    (dict(round0=(1 << 31) - 2), "round0 + T above 2^31 - 1"),
    (dict(opt=_opts(rng=0.0)), "range must be > 0"),
    (dict(opt=_opts(rng=math.nan)), "range must be > 0"),
    (dict(opt=_opts(radius=-1.0)), "radius must be >= 0"),
    (dict(opt=_opts(max_step=0.0)), "max_step must be > 0"),
    (dict(opt=_opts(max_samples=0)), "max_samples must be >= 1"),
    (dict(opt=_opts(slots=17)), "slots must be in [1, DCX_RRT_MAX_SLOTS]"),
    (dict(opt=_opts(near=17)), "near must be in [0, DCX_RRTSTAR_MAX_NEAR]"),
    (dict(opt=_opts(cap=0)), "cap must be in [1, DCX_RRTSTAR_MAX_CAP]"),
    (dict(opt=_opts(mask=1)), "wrap_mask has a bit at or above dof"),
    (dict(opt=_opts(r0=1)), "reserved fields must be 0"),
    (dict(opt=_opts(reserved=(0, 1))), "reserved fields must be 0"),
] + [(dict(state=_state(**{f: True})), "state or one of its pointers is NULL") for f in _STATE]


def _refused(lib, run, m, cases):
    for kw, text in cases:
        kw = dict(kw)
        rc = run(lib, kw.pop("model", m), **kw)
        msg = lib.dcx_last_error().decode()
        assert rc == 1, (kw, rc, msg)
        assert text in msg and msg.startswith("rrtstar"), (kw, msg)


def test_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    need = lib.dcx_rrtstar_cost_work_bytes(m, 8, 4, 8)
    assert need >= lib.dcx_motion_worst_work_bytes(m, 8 * 4 * 8) > 0
    _refused(lib, _run, m, _COST_ERRORS + _RUN_ERRORS + [(dict(samples=0), "samples is NULL"),
                                                        (dict(work_bytes=need - 1), "smaller than dcx_rrtstar_cost_work_bytes")])
    # the cost options are read even where there is nothing to do, and a good set is then no error; gain and band may be 0
    assert _run(lib, m, R=0, cost=False, state=False, goals=0, samples=0, work=0, work_bytes=0) == 1
    assert _run(lib, m, R=0, state=False, goals=0, samples=0, work=0, work_bytes=0) == 0
    assert _run(lib, m, T=0, samples=0, work_bytes=need) == 0
    assert _run(lib, m, T=0, cost=_cost(gain=0.0, band=0.0), opt=_opts(radius=0.0, near=0), work_bytes=need) == 0
    # beyond one launch: unsupported, not invalid
    assert _run(lib, m, R=1 << 31, work_bytes=1 << 62) == 2
    assert _run(lib, m, R=1 << 27, opt=_opts(slots=4, near=8), work_bytes=1 << 62) == 2


def test_sampled_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    need = lib.dcx_rrtstar_sampled_cost_work_bytes(m, 8, 4, 8)
    assert need >= lib.dcx_rrtstar_cost_work_bytes(m, 8, 4, 8) > 0
    _refused(lib, _run_sampled, m, _COST_ERRORS + _RUN_ERRORS + [
        (dict(sample=False), "sample options are NULL"),
        (dict(sample=_sample(tries=0)), "tries must be in [1, DCX_RRTSTAR_MAX_TRIES]"),
        (dict(sample=_sample(goal_bias=1.5)), "goal_bias must be in [0, 1]"),
        (dict(sample=_sample(mode=7)), "mode must be DCX_RRTSTAR_SAMPLE_UNIFORM or DCX_RRTSTAR_SAMPLE_INFORMED"),
        (dict(sample=_sample(r0=1)), "reserved fields of the sample options must be 0"),
        (dict(sample=_sample(slots=5)), "differ from the options' or the model's"),
        (dict(sample=_sample(cap=65)), "differ from the options' or the model's"),
        (dict(sample=_sample(dof=3)), "differ from the options' or the model's"),
        (dict(sample=_sample(limits=0)), "limits is NULL"),
        (dict(work_bytes=need - 1), "smaller than dcx_rrtstar_sampled_cost_work_bytes")])
    assert _run_sampled(lib, m, R=0, state=False, goals=0, work=0, work_bytes=0) == 0
    assert _run_sampled(lib, m, T=0, work_bytes=need) == 0


def test_work_bytes_are_zero_for_refused_arguments_and_not_below_the_length_planner_s():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    for wb, base in ((lib.dcx_rrtstar_cost_work_bytes, lib.dcx_rrtstar_work_bytes),
                     (lib.dcx_rrtstar_sampled_cost_work_bytes, lib.dcx_rrtstar_sampled_work_bytes)):
        for bad in [(None, 8, 4, 8), (m, -1, 4, 8), (m, 8, 0, 8), (m, 8, 17, 8), (m, 8, 4, -1), (m, 8, 4, 17), (m, 1 << 31, 4, 8),
                    (m, 1 << 27, 4, 8)]:
            assert wb(*bad) == 0, bad
        for R, P, K in [(0, 4, 8), (1, 1, 0), (7, 4, 8), (64, 16, 16), (1000, 4, 1), (1 << 20, 4, 8)]:
            assert wb(m, R, P, K) >= base(m, R, P, K) > 0, (R, P, K)
        sizes = [wb(m, R, 4, 8) for R in (0, 1, 7, 64, 1000, 1 << 20)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0] > 0
        sizes = [wb(m, 100, 4, K) for K in (0, 1, 8, 16)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0] > 0
    # dcx_motion_worst's workspace of the larger batch at the head, then the scratch
    assert lib.dcx_rrtstar_cost_work_bytes(m, 100, 4, 8) > lib.dcx_motion_worst_work_bytes(m, 3200)
    assert lib.dcx_rrtstar_cost_work_bytes(m, 100, 4, 0) > lib.dcx_motion_worst_work_bytes(m, 400)


def test_python_layer_rejects_bad_arguments_without_a_device():
    import torch
    from diffco_amd import rrtstar

    class NoFused:
        def check_motions(self, *a, **k):
            raise AssertionError("not reached")

        def motion_worst(self, *a, **k):
            raise AssertionError("not reached")

    s = torch.zeros(2, 3)
    kw = dict(range=0.5, max_step=0.1, limits=[[0, 1]] * 3)
    with pytest.raises(ValueError, match="clearance_band"):
        rrtstar.rrt_star(NoFused(), s, s, objective="clearance", **kw)
    with pytest.raises(ValueError, match="clearance_band"):
        rrtstar.rrt_star(NoFused(), s, s, objective="clearance", clearance_band=-0.1, **kw)
    with pytest.raises(ValueError, match="clearance_gain"):
        rrtstar.rrt_star(NoFused(), s, s, objective="clearance", clearance_band=0.1, clearance_gain=float("nan"), **kw)
    with pytest.raises(ValueError, match="objective"):
        rrtstar.rrt_star(NoFused(), s, s, objective="peak", **kw)
    with pytest.raises(ValueError, match="near"):
        rrtstar.rrt_star(NoFused(), s, s, near=17, objective="clearance", clearance_band=0.1, **kw)
