"""GPU: every workspace size query answers, on three real models (a planar arm, dof 2; Baxter, dof 7; five classes, where
dcx_motion_cost's layout takes its C > 1 fields), the bytes the library answered before every layout was moved onto one carver
(work_layout.h).  The recording (tests/golden/planner_work_bytes_parent.json, tools/record_planner_host_parent.py gpu) is of
that earlier library, never of the one under test.  Nothing is launched beyond creating the models."""
import json
import os

import pytest

import planner_boundary_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", cases.GOLDEN_WORK_BYTES)


@pytest.fixture(scope="module")
def got():
    from diffco_amd import _lib, _ops
    lib = _lib.require_gpu()
    return cases.run_work_bytes(lib, cases.build_models(_ops))


@pytest.mark.parametrize("name", cases.MODELS)
def test_work_bytes_are_the_recorded_ones(name, got):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    assert sorted(want) == sorted(cases.WORK_BYTES_GRIDS)
    for fn, grid in cases.WORK_BYTES_GRIDS.items():
        assert sorted(want[fn]) == sorted(repr(a) for a in grid), fn
        assert got[name][fn] == want[fn], (fn, {a: (got[name][fn][a], v) for a, v in want[fn].items() if got[name][fn][a] != v})
        assert max(want[fn].values()) > 0, fn
