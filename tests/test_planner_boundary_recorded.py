"""CPU: the three lockstep planners (dcx_rrt_connect_run, dcx_path_shortcut_run, dcx_path_shortcut_partial_run) refuse every
single argument fault and every pair of faults in different arguments with the return code AND the message the library gave
before their checks were moved onto one prelude - which pins the ORDER of the checks, as the first failing one names the
error - and their size queries answer the recorded bytes on the stand-in model.  The recording
(tests/golden/planner_boundary_parent.json, tools/record_planner_host_parent.py cpu) is of that earlier library, never of the one
under test.  Every case holds a fault, so nothing here reaches a device."""
import json
import os

import pytest

import planner_boundary_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", cases.GOLDEN_BOUNDARY)


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got():
    from diffco_amd import _lib
    return cases.run_boundary(_lib.load())


@pytest.mark.parametrize("call", sorted(cases.CALLS))
def test_every_fault_and_pair_is_refused_as_recorded(call, recorded, got):
    want, have = recorded["boundary"][call], got[0][call]
    assert sorted(want) == sorted(cid for cid, _ in cases.boundary_cases(call)) == sorted(have)
    assert sum(" & " in cid for cid in want) > 200 > sum(" & " not in cid for cid in want) > 20   # the pairs and the singles
    for cid in want:
        assert have[cid][0] != 0, cid
        assert have[cid] == want[cid], (cid, have[cid], want[cid])
    assert {rc for rc, _ in want.values()} == {1, 2}   # invalid, and R = 2^31: unsupported


@pytest.mark.parametrize("fn", sorted(cases.STAND_IN_GRIDS))
def test_size_queries_answer_the_recorded_bytes(fn, recorded, got):
    want, have = recorded["work_bytes"][fn], got[1][fn]
    assert sorted(want) == sorted(repr(a) for a in cases.STAND_IN_GRIDS[fn])
    assert have == want
    assert min(want.values()) == 0 < max(want.values())
