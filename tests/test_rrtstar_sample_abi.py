"""CPU-side checks of the boundary of RRT*'s device-side sampling (dcx_rrtstar_sample, dcx_rrtstar_sampled_work_bytes,
dcx_rrtstar_run_sampled): the symbols exist and the version stays 109, the header and the ctypes table declare the same
arguments, dcx_rrtstar_sample_opts has the C layout, every argument error is reported before anything touches a device, the
workspace is dcx_rrtstar_work_bytes' plus one round's sample rows, and the header section states the contract - on a machine
without a GPU."""
import ctypes
import math
import os
import subprocess

import pytest

from test_rrtstar_abi import _declared, _fake_model, _opts, _state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dcx.h")
_SOPTS = ("limits", "seed", "goal_bias", "uniform_mix", "mode", "tries", "slots", "cap", "dof", "reserved0", "wrap_mask", "reserved")


@pytest.mark.parametrize("name", ["dcx_rrtstar_sample", "dcx_rrtstar_sampled_work_bytes", "dcx_rrtstar_run_sampled"])
def test_symbols_exist_and_version_stays(name):
    from diffco_amd import _lib
    res, args = _declared(name)
    assert _lib.SYMBOLS[name][0] is res
    assert list(_lib.SYMBOLS[name][1]) == args
    lib = _lib.load()
    assert hasattr(lib, name)
    assert lib.dcx_version() == 109


def test_struct_layout_matches_c(tmp_path):
    from diffco_amd._lib import RRTSTAR_MAX_TRIES, RRTSTAR_SAMPLE_MAX_PROBLEMS, RRTSTAR_SAMPLE_MODES, RrtStarSampleOpts
    prog = tmp_path / "szs.c"
    offs = ", ".join(f"offsetof(dcx_rrtstar_sample_opts, {f})" for f in _SOPTS)
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dcx.h"\n'
                    'int main(){size_t v[] = {sizeof(dcx_rrtstar_sample_opts), DCX_RRTSTAR_MAX_TRIES, DCX_RRTSTAR_SAMPLE_UNIFORM, '
                    'DCX_RRTSTAR_SAMPLE_INFORMED, DCX_RRTSTAR_SAMPLE_MAX_PROBLEMS, ' + offs + '};\n'
                    'for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf("%zu ", v[i]);}')
    exe = tmp_path / "szs"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [ctypes.sizeof(RrtStarSampleOpts), RRTSTAR_MAX_TRIES, RRTSTAR_SAMPLE_MODES["uniform"], RRTSTAR_SAMPLE_MODES["informed"],
                   RRTSTAR_SAMPLE_MAX_PROBLEMS] + [getattr(RrtStarSampleOpts, f).offset for f in _SOPTS]
    assert [f for f, _ in RrtStarSampleOpts._fields_] == list(_SOPTS)
    assert ctypes.sizeof(RrtStarSampleOpts) == 72 and RRTSTAR_MAX_TRIES == 16


def test_header_section_states_the_contract():
    src = open(HEADER).read()
    at = src.index("batched RRT*: samples drawn on the device (added")
    assert "added under DCX_VERSION 109" in src[at:][:80]
    assert src.index("batched RRT* (added") < at < src.index("batched path shortcutting and RRT path extraction (added")
    body = src[at:][:12000]
    for word in ("Philox4x32-10", "(g, r * 16 + p, t, b)", "(word >> 8) * 2^-24", "((word >> 8) + 1) * 2^-24", "block 0, try 0",
                 "blocks 1 .. 8, try 0", "blocks 9 .. 17, try t", "Box-Muller", "1. goal", "2. uniform", "3. informed",
                 "one rounded fp32 product and one rounded fp32 sum", "Householder", "v = a^ + sign(a^_0) e_0",
                 "H y = y - 2 v (v.y) / (v.v)", "2 + tries informed", "shortest-arc image of the goal", "uniform_mix",
                 "not on T, on the chunking", "Capturable", "dcx_rrtstar_work_bytes itself is unchanged",
                 "dcx_rrtstar_sampled_work_bytes is 0 for arguments the call refuses"):
        assert word in body, word


def _sopts(limits=1, seed=5, goal_bias=0.1, uniform_mix=0.0, mode=1, tries=8, slots=4, cap=64, dof=0, r0=0, mask=0, reserved=(0, 0)):
    from diffco_amd._lib import RrtStarSampleOpts
    return RrtStarSampleOpts(limits, seed, goal_bias, uniform_mix, mode, tries, slots, cap, dof, r0, mask, (ctypes.c_int64 * 2)(*reserved))


_VALUE_CASES = [
    (dict(tries=0), "tries must be in [1, DCX_RRTSTAR_MAX_TRIES]"),
    (dict(tries=17), "tries must be in [1, DCX_RRTSTAR_MAX_TRIES]"),
    (dict(goal_bias=-0.1), "goal_bias must be in [0, 1]"),
    (dict(goal_bias=1.5), "goal_bias must be in [0, 1]"),
    (dict(goal_bias=math.nan), "goal_bias must be in [0, 1]"),
    (dict(uniform_mix=-0.1), "uniform_mix must be in [0, 1]"),
    (dict(uniform_mix=1.5), "uniform_mix must be in [0, 1]"),
    (dict(uniform_mix=math.nan), "uniform_mix must be in [0, 1]"),
    (dict(mode=2), "mode must be"),
    (dict(mode=-1), "mode must be"),
    (dict(r0=1), "reserved fields of the sample options must be 0"),
    (dict(reserved=(1, 0)), "reserved fields of the sample options must be 0"),
    (dict(reserved=(0, 1)), "reserved fields of the sample options must be 0"),
]


def test_sample_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p

    def run(R=8, state=None, goals=1, so=None, rnd=3, samples=1, info=1):
        state = _state() if state is None else state
        so = _sopts(dof=7) if so is None else so
        return lib.dcx_rrtstar_sample(0, ctypes.byref(state) if state is not False else None, R, p(goals),
                                      ctypes.byref(so) if so is not False else None, rnd, p(samples), p(info), None)

    cases = [(dict(so=False), "options are NULL"), (dict(R=-1), "R < 0"), (dict(rnd=-1), "round < 0"), (dict(rnd=1 << 31), "above 2^31 - 1"),
             (dict(so=_sopts(dof=7, slots=0)), "slots must be in [1, DCX_RRT_MAX_SLOTS]"),
             (dict(so=_sopts(dof=7, slots=17)), "slots must be in [1, DCX_RRT_MAX_SLOTS]"),
             (dict(so=_sopts(dof=7, cap=0)), "cap must be in [1, DCX_RRTSTAR_MAX_CAP]"),
             (dict(so=_sopts(dof=7, cap=(1 << 16) + 1)), "cap must be in [1, DCX_RRTSTAR_MAX_CAP]"),
             (dict(so=_sopts(dof=0)), "dof must be in [1, DCX_MAX_DOF]"), (dict(so=_sopts(dof=33)), "dof must be in [1, DCX_MAX_DOF]"),
             (dict(so=_sopts(dof=7, mask=1 << 7)), "wrap_mask has a bit at or above dof"),
             (dict(state=False), "is NULL"), (dict(goals=0), "is NULL"), (dict(samples=0), "samples is NULL"),
             (dict(so=_sopts(dof=7, limits=0)), "limits is NULL")]
    cases += [(dict(state=_state(**{f: True})), "is NULL") for f in ("nodes", "cost", "status", "goal_node")]
    cases += [(dict(so=_sopts(dof=7, **kw)), text) for kw, text in _VALUE_CASES]
    for kw, text in cases:
        rc = run(**kw)
        msg = lib.dcx_last_error().decode()
        assert rc == 1 and text in msg and msg.startswith("rrtstar sample"), (kw, rc, msg)
    # the pointers the draw does not read may be NULL; info may be NULL; nothing to do is not an error
    assert run(R=0, state=False, goals=0, samples=0, info=0, so=_sopts(dof=7, limits=0)) == 0
    assert run(R=(1 << 28) + 1, so=_sopts(dof=7, slots=1)) == 2
    assert run(R=1 << 31) == 2


def _run(lib, model, R=8, T=2, round0=0, opt=None, so=None, state=None, goals=1, work=1, work_bytes=1 << 40, samples_out=0, info_out=0):
    p = ctypes.c_void_p
    opt = _opts() if opt is None else opt
    so = _sopts() if so is None else so
    state = _state() if state is None else state
    return lib.dcx_rrtstar_run_sampled(model, ctypes.byref(state) if state is not False else None, R, p(goals),
                                       ctypes.byref(so) if so is not False else None, T, round0,
                                       ctypes.byref(opt) if opt is not False else None, None, p(work), work_bytes, p(samples_out),
                                       p(info_out), None)


def test_run_sampled_argument_errors_before_any_device_use():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()   # (its dof reads 0)
    need = lib.dcx_rrtstar_sampled_work_bytes(m, 8, 4, 8)
    cases = [
        # dcx_rrtstar_run's own
        (dict(model=None), "model is NULL"), (dict(opt=False), "options are NULL"), (dict(state=False), "state or one of its pointers is NULL"),
        (dict(goals=0), "state or one of its pointers is NULL"), (dict(work=0), "work is NULL"), (dict(R=-1), "R < 0"), (dict(T=-1), "T < 0"),
        (dict(round0=-1), "round0 < 0"), (dict(round0=(1 << 31) - 2), "round0 + T above 2^31 - 1"),
        (dict(opt=_opts(rng=0.0)), "range must be > 0"), (dict(opt=_opts(radius=math.nan)), "radius must be >= 0"),
        (dict(opt=_opts(max_step=0.0)), "max_step must be > 0"), (dict(opt=_opts(max_samples=0)), "max_samples must be >= 1"),
        (dict(opt=_opts(slots=17)), "slots must be in [1, DCX_RRT_MAX_SLOTS]"), (dict(opt=_opts(near=17)), "near must be in"),
        (dict(opt=_opts(cap=0)), "cap must be in [1, DCX_RRTSTAR_MAX_CAP]"), (dict(opt=_opts(mask=1)), "wrap_mask has a bit at or above dof"),
        (dict(opt=_opts(r0=1)), "reserved fields must be 0"),
        # the sample options'
        (dict(so=False), "sample options are NULL"),
        (dict(so=_sopts(limits=0)), "limits is NULL"),
        (dict(so=_sopts(slots=5)), "differ from the options' or the model's"),
        (dict(so=_sopts(cap=65)), "differ from the options' or the model's"),
        (dict(so=_sopts(dof=7)), "differ from the options' or the model's"),
        (dict(so=_sopts(mask=1)), "differ from the options' or the model's"),
        (dict(work_bytes=need - 1), "smaller than dcx_rrtstar_sampled_work_bytes"),
    ] + [(dict(so=_sopts(**kw)), text) for kw, text in _VALUE_CASES] \
      + [(dict(state=_state(**{f: True})), "state or one of its pointers is NULL") for f in _STATE_FIELDS]
    for kw, text in cases:
        kw = dict(kw)
        rc = _run(lib, kw.pop("model", m), **kw)
        msg = lib.dcx_last_error().decode()
        assert rc == 1, (kw, rc, msg)
        assert text in msg and msg.startswith("rrtstar"), (kw, msg)
    # nothing to do is not an error; the outputs are optional
    assert _run(lib, m, R=0, state=False, goals=0, work=0, work_bytes=0, so=_sopts(limits=0)) == 0
    assert _run(lib, m, T=0, work_bytes=need) == 0
    assert _run(lib, m, T=0, work_bytes=need, samples_out=1, info_out=1) == 0
    assert _run(lib, m, R=1 << 31, work_bytes=1 << 62) == 2


_STATE_FIELDS = ("nodes", "parent", "elen", "cost", "count", "status", "goal_node", "first_round")


def test_work_bytes_is_the_run_calls_plus_one_round_of_rows():
    from diffco_amd import _lib
    lib = _lib.load()
    keep, m = _fake_model()
    wb, base = lib.dcx_rrtstar_sampled_work_bytes, lib.dcx_rrtstar_work_bytes
    for bad in [(None, 8, 4, 8), (m, -1, 4, 8), (m, 8, 0, 8), (m, 8, 17, 8), (m, 8, 4, -1), (m, 8, 4, 17), (m, 1 << 31, 4, 8), (m, 1 << 27, 4, 8)]:
        assert wb(*bad) == 0, bad
    for R, P, K in [(0, 4, 8), (1, 1, 0), (7, 4, 8), (256, 16, 16), (1000, 5, 1)]:
        assert wb(m, R, P, K) >= base(m, R, P, K) > 0
        assert (wb(m, R, P, K) - base(m, R, P, K)) % 256 == 0   # the carver's alignment (the stand-in model's dof reads 0: no rows)


def test_python_layer_rejects_bad_arguments_without_a_device():
    import torch
    from diffco_amd import rrtstar

    class NoFused:
        def check_motions(self, *a, **k):
            raise AssertionError("not reached")

    s = torch.zeros(2, 3)
    kw = dict(range=0.5, max_step=0.1, limits=[[0, 1]] * 3)
    with pytest.raises(ValueError, match="sampler"):
        rrtstar.rrt_star(NoFused(), s, s, sampling="informed", sampler=lambda T, R, P: None, **kw)
    with pytest.raises(ValueError, match="sampler"):
        rrtstar.rrt_star(NoFused(), s, s, sampling="device", sampler=lambda T, R, P: None, **kw)
    with pytest.raises(ValueError, match="sampling"):
        rrtstar.rrt_star(NoFused(), s, s, sampling="philox", **kw)
    with pytest.raises(ValueError, match="informed_tries"):
        rrtstar.rrt_star(NoFused(), s, s, sampling="informed", informed_tries=0, **kw)
    with pytest.raises(ValueError, match="uniform_mix"):
        rrtstar.rrt_star(NoFused(), s, s, sampling="informed", uniform_mix=-0.5, **kw)
    with pytest.raises(ValueError, match="limits"):
        rrtstar.rrt_star(NoFused(), s, s, sampling="informed", range=0.5, max_step=0.1)
