"""GPU tests of the four-row pipeline's addressing (score_kernel.h sweep_rows, PARTS == 0): a wave carries ONE pointer to the row it
stands on, advanced once per iteration, every row of the iteration is loaded at a compile-time offset from it, and the look-ahead
is not clamped to the slice - its loads reach up to kSweepLookahead rows past the slice's end: the next wave's rows inside the
model, the zero tail of the storage (dcx_api.hip rows_tail_floats) behind its last row.  None of that may move a bit: every launch
of sweep_lookahead_cases.py (the table is in that file: every remainder of the four-row loop, slices around a flush, the skewed
slices of 16- and 8-wave blocks, a model at exactly its capacity by both packing routes and the same model refilled in place) equals
what the commit before gave for the same inputs, recorded with that commit's library (tests/golden/sweep_lookahead_parent_bits.npz,
tools/record_sweep_lookahead_parent_bits.py).  Beside that, every launch against the fp64 oracle at test_gpu_spare_lean.py's TOL."""
import numpy as np
import pytest

import sweep_lookahead_cases as cases
from helpers import load, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-5                      # test_gpu_spare_lean.py: max|a - ref| / max|ref| against the fp64 referee


@pytest.fixture(scope="module")
def runs():
    from diffco_amd import _lib
    lib = _lib.require_gpu()
    set_knob = lambda name, v: _lib.check(lib.dcx_debug_set(name.encode(), int(v)))  # noqa: E731
    try:
        yield cases.run_all(set_knob)
    finally:
        cases.reset_knobs(lib)


def test_the_shapes_the_cases_promise():
    names = {name for name, *_ in cases.PLAIN_LAUNCHES}
    assert {f"S{S}_nw1" for S in (15, 16, 17, 18, 63, 64, 65, 67, 68)} <= names and {"S2000_nw16", "S2000_nw8"} <= names
    assert {name for name, _ in cases.STORAGE_LAUNCHES} == {f"cap_{r}" for r in ("dev", "host")} | {
        f"upd_{r}_{step}" for r in ("dev", "host") for step in ("small", "back")}
    assert cases.B == 70 and sorted(cases.KERNELS) == ["poly1", "rq2"]


@pytest.mark.parametrize("key", cases.keys())
def test_bits_of_the_commit_before(runs, key):
    """score and gradient, bit for bit; and knob spare = 0 moves them, so the spare form is what ran"""
    out, plain, _ = runs
    gold = load("sweep_lookahead_parent_bits")
    s, g = out[key]
    assert np.isfinite(s).all() and np.isfinite(g).all()
    assert np.array_equal(s, gold[key + "_s"]) and np.array_equal(g, gold[key + "_g"]), key
    ps, pg = plain[key]
    assert not (np.array_equal(s, ps) and np.array_equal(g, pg)), "the spare form did not run"


def test_every_recorded_launch_is_checked(runs):
    out, _, _ = runs
    gold = load("sweep_lookahead_parent_bits")
    assert sorted(gold.files) == sorted(f"{k}_{part}" for k in out for part in "sg")
    assert sorted(out) == sorted(cases.keys())


@pytest.fixture(scope="module")
def referee(runs):
    """the fp64 oracle's score and gradient, per kernel function and model size: each computed once.  It walks the arm in float64
    and gets ITS OWN features of the support configurations (test_gpu_spare_lean.py)"""
    from oracle import oracle
    c = runs[2]
    sup64 = oracle.fkine(c["desc"], c["sup_q"].numpy().astype(np.float64), dtype=np.float64).reshape(cases.S_MAX, -1)
    w64, q64 = c["w"].numpy().astype(np.float64), c["q"].numpy().astype(np.float64)
    ref = {}
    for key in cases.keys():
        kname, S = key.split("_")[0], cases.size_of(key)
        if (kname, S) not in ref:
            so, go, _ = oracle.score_grad(c["desc"], *cases.KERNELS[kname], sup64[:S], w64[:S], q64, dtype=np.float64)
            ref[(kname, S)] = (so, go)
    return ref


@pytest.mark.parametrize("key", cases.keys())
def test_against_float64(runs, referee, key):
    out, _, _ = runs
    s, g = out[key]
    so, go = referee[(key.split("_")[0], cases.size_of(key))]
    es, eg = relerr(s, so.reshape(s.shape)), relerr(g, go)
    print(f"{key}: score {es:.2e} grad {eg:.2e}")
    assert es < TOL and eg < TOL, (key, es, eg)
