"""GPU: the four motion calls keep the bits they had before their kernels were moved onto one shared tile prologue, block fold
and split hand-over (motion_tile.h).  tests/golden/motion_parent_bits.npz holds every output of motion_parent_bits_cases.run_all()
from the library of commit 705e9b0 ("Spare-slot sweep: near gate before the clamp, one packed coef multiply"), the last one with
four separate kernels, recorded with tools/record_motion_parent_bits.py and DCX_LIB on that commit's build - never with the code
under test.  The cases: D = 12 with one and five classes, D = 4 under a wrap mask, D = 24; 130 edges of 1 - 70 samples (tiles of
many short edges, an edge over three tiles, a partial last tile, empty edges, one over max_samples); res = 9 and max_step, the
cost's open end; test_batch_sizes_and_launch_forms' five launch forms (both block folds, the split hand-over).  first_hit under
the early exit, the packed keys and the codes do not depend on the order of arrival and the cost path has no floating atomics:
every array is compared exactly ([n, dof] float arrays as a hash per row, motion_parent_bits_cases.fold; the gradients of
the one- and the five-class model under max_step also whole, at the rule's launch form and at a split one)."""
import numpy as np
import pytest

import motion_parent_bits_cases as cases
from helpers import load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs():
    from diffco_amd import _lib, _ops
    lib = _lib.require_gpu()
    knob = lambda name, v: _lib.check(lib.dcx_debug_set(name.encode(), int(v)))
    try:
        yield cases.run_all(_ops, knob, lambda v: knob("motion_early_exit", v))
    finally:
        for k in ("ys", "nw", "motion_early_exit"):
            lib.dcx_debug_set(k.encode(), -1)


def test_the_work_list_has_the_layout_the_cases_exist_for(runs):
    n = runs["cfg2_baxter_poly1|step|check_n_samples_ee1"][0]
    assert n[cases.ZERO_EDGE] == 1
    assert np.delete(n, cases.LONG_EDGE).tolist() == np.delete(cases.sample_counts(), cases.LONG_EDGE).tolist()
    assert cases.layout_ok(n)
    first = runs["cfg2_baxter_poly1|step|check_first_hit_ee1"][0]
    assert first[cases.LONG_EDGE] == -2 and (first >= 0).any() and (first == -1).any()


@pytest.mark.parametrize("name", [m for m, _ in cases.MODELS])
def test_every_output_has_the_parent_commits_bits(runs, name):
    gold = load("motion_parent_bits")
    assert sorted(gold.files) == sorted(runs)
    keys = [k for k in runs if k.startswith(name + "|")]
    assert len(keys) > 40 and all(len(runs[k]) in (len(cases.FORMS), len(cases.FULL_FORMS)) for k in keys)
    if name in cases.GRAD_MODELS:
        assert all(runs[f"{name}|step|{k}"].shape[0] == len(cases.FULL_FORMS) for k in ("worst_grad_a", "worst_grad_b", "cost_grad_a", "cost_grad_b"))
    bad = [k for k in keys if runs[k].dtype != gold[k].dtype or not np.array_equal(runs[k], gold[k], equal_nan=runs[k].dtype.kind == "f")]
    assert not bad, bad
