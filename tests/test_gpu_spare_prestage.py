"""GPU tests of the pre-staged spare-slot sweep (score_kernel.h score_body SP, sweep_rows PRE, fold_mine_sp): a block centres its
features and exchanges the agreed column with the last one ONCE, in LDS, every wave sweeps them as they are and leaves its gradient
in that order, and the exchange is undone by index where the partial rows meet.  None of that may move a bit: every launch of
spare_prestage_cases.py - Baxter's left arm at every block size, unsplit and split, through every hand-over the host's rules reach
at this size (the table is in that file); a padded planar arm whose agreed column is the last one (the identity exchange, d_fk != D);
a model with no agreed column (the plain kernel) - equals what the commit before gave for the same inputs, recorded with that
commit's library (tests/golden/spare_prestage_parent_bits.npz, tools/record_spare_prestage_parent_bits.py).  Beside that, the Baxter
launches against the fp64 oracle at test_gpu_parity.py's TOL."""
import numpy as np
import pytest

import spare_prestage_cases as cases
from helpers import load, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-5                      # test_gpu_parity.py: max|a - ref| / max|ref| against the fp64 referee


@pytest.fixture(scope="module")
def runs():
    from diffco_amd import _lib
    lib = _lib.require_gpu()
    set_knob = lambda name, v: _lib.check(lib.dcx_debug_set(name.encode(), int(v)))  # noqa: E731
    try:
        yield cases.run_all(set_knob)
    finally:
        cases.reset_knobs(lib)


def _keys(tag):
    launches = cases.BAXTER_LAUNCHES if tag == "baxter" else cases.PLANAR_LAUNCHES
    kernels = sorted(cases.KERNELS) if tag == "baxter" else ["poly1"]
    return [f"{tag}_{k}_{name}" for k in kernels for name, *_ in launches]


def test_the_grid_the_cases_promise():
    names = {name for name, *_ in cases.BAXTER_LAUNCHES}
    assert {f"nw{nw}_ys{ys}" for nw in (1, 2, 4, 8, 16) for ys in (1, 2)} <= names
    assert cases.B == 70 and cases.S == 203


@pytest.mark.parametrize("key", _keys("baxter") + _keys("planar5"))
def test_bits_of_the_commit_before(runs, key):
    """score and gradient, bit for bit; and knob spare = 0 moves them, so the spare form is what ran"""
    out, plain, _ = runs
    gold = load("spare_prestage_parent_bits")
    s, g = out[key]
    assert np.isfinite(s).all() and np.isfinite(g).all()
    assert np.array_equal(s, gold[key + "_s"]) and np.array_equal(g, gold[key + "_g"]), key
    ps, pg = plain[key]
    assert not (np.array_equal(s, ps) and np.array_equal(g, pg)), "the spare form did not run"


@pytest.mark.parametrize("key", _keys("planar6"))
def test_a_model_without_an_agreed_column_keeps_the_plain_kernel(runs, key):
    out, plain, _ = runs
    gold = load("spare_prestage_parent_bits")
    s, g = out[key]
    assert np.array_equal(s, gold[key + "_s"]) and np.array_equal(g, gold[key + "_g"]), key
    assert np.array_equal(s, plain[key][0]) and np.array_equal(g, plain[key][1]), key   # the rule and spare = 0: the same kernel


def test_every_recorded_launch_is_checked(runs):
    out, _, _ = runs
    gold = load("spare_prestage_parent_bits")
    assert sorted(gold.files) == sorted(f"{k}_{part}" for k in out for part in "sg")
    assert sorted(out) == sorted(_keys("baxter") + _keys("planar5") + _keys("planar6"))


@pytest.fixture(scope="module")
def referee(runs):
    """the fp64 oracle's score and gradient of the Baxter batch, per kernel function: computed once.  It walks the arm in float64
    and gets ITS OWN features of the support configurations (test_gpu_spare_lean.py)"""
    from oracle import oracle
    c = runs[2]["baxter"]
    sup64 = oracle.fkine(c["desc"], c["sup_q"].numpy().astype(np.float64), dtype=np.float64).reshape(cases.S, -1)
    ref = {}
    for kname, kern in cases.KERNELS.items():
        so, go, _ = oracle.score_grad(c["desc"], *kern, sup64, c["w"].numpy().astype(np.float64), c["q"].numpy().astype(np.float64),
                                      dtype=np.float64)
        ref[kname] = (so, go)
    return ref


@pytest.mark.parametrize("key", _keys("baxter"))
def test_baxter_against_float64(runs, referee, key):
    out, _, _ = runs
    s, g = out[key]
    so, go = referee[key.split("_")[1]]
    es, eg = relerr(s, so.reshape(s.shape)), relerr(g, go)
    print(f"{key}: score {es:.2e} grad {eg:.2e}")
    assert es < TOL and eg < TOL, (key, es, eg)
