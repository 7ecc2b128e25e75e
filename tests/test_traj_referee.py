"""CPU: the referee of the trajectory fuzz (tests/test_gpu_traj_fuzz.py) and what its case table covers.  The referee's gradient
(traj_fuzz_helpers.traj_terms: the chain through the oracle's Jacobian and FK vjp, the hinges, the endpoint mask) is checked
against float64 central differences of its own loss, so the fuzz compares the kernels with an independent reference; the band
condition that makes every hinge tie-free is asserted for every row; the coverage guard fails when a compiled width, class
count, kernel family, FK kind or path length the host routes differently has no case."""
import numpy as np
import pytest

from helpers import KERNELS, kernel_family, template_d_for, template_widths
from traj_fuzz_helpers import (BAND_FACTOR, LDS_BYTES, TRAJ_CASES, TrajCase, case_id, has_persistent_form, step_carve_bytes,
                               traj_reference, traj_setup, traj_terms)

# one case of every FK kind: none, planar, SE(2), SE(3), one-chain DH, two-chain DH, a URDF tree, the 84-wide tree
FD_CASES = [TrajCase("none", 5, 1, 0, 6, 1), TrajCase("planar", 8, 2, 5, 6, 1), TrajCase("se2", 6, 3, 1, 6, 1),
            TrajCase("se3", 24, 1, 2, 6, 1), TrajCase("baxter", 12, 1, 0, 6, 1), TrajCase("baxter_dual", 24, 2, 3, 6, 1),
            TrajCase("urdf_panda", 27, 1, 1, 6, 1), TrajCase("urdf_iiwa7_allegro", 84, 5, 0, 5, 1)]


@pytest.mark.parametrize("case", FD_CASES, ids=case_id)
def test_referee_gradient_matches_central_differences(case):
    """h = 1e-6 on the referee's loss; the case's construction keeps every hinge (scores, segment lengths) far from its kink and
    the limit hinges sit 0.1 / 0.2 outside; bound: 1e-6 x the largest difference quotient"""
    x = traj_setup(case)
    args = (x["desc"], x["kern"], x["sup"], x["weights"], x["limits32"])
    p = x["paths"][0].astype(np.float64)
    ref = traj_terms(*args, p, x["margin"], x["opts"])
    W, dof = p.shape
    h = 1e-6
    fd = np.zeros_like(p)
    for w in range(1, W - 1):
        for j in range(dof):
            v = []
            for sgn in (1.0, -1.0):
                pp = p.copy()
                pp[w, j] += sgn * h
                v.append(traj_terms(*args, pp, x["margin"], x["opts"], want_grad=False)["stats"][0])
            fd[w, j] = (v[0] - v[1]) / (2 * h)
    scale = np.abs(fd).max()
    assert scale > 0
    err = np.abs(ref["g"] - fd).max()
    assert err <= 1e-6 * scale, (case, err, scale)
    assert (ref["g"][[0, -1]] == 0).all()
    assert ref["stats"][4] > 0 and ref["stats"][5] > 0 and ref["stats"][6] > 0, ref["stats"]   # every term's gradient took part


@pytest.mark.parametrize("case", TRAJ_CASES, ids=case_id)
def test_every_hinge_of_a_case_is_tie_free_and_every_term_is_live(case):
    x = traj_setup(case)
    assert (x["gap_s"] >= BAND_FACTOR * x["err_s"]).all(), (case, x["gap_s"], x["err_s"])
    assert x["gap_seg"] >= BAND_FACTOR * x["err_seg"], (case, x["gap_seg"], x["err_seg"])
    # the margins and max_speed^2 are inside their gaps: no score / segment within the half-gap of them
    assert (np.abs(x["s64"] - x["margin"].astype(np.float64)).min(axis=(0, 1)) >= x["gap_s"] * (1 - 1e-9)).all()
    seg = x["seg64"][x["seg64"] > 0]
    assert np.abs(seg - x["opts"]["max_speed"] ** 2).min() >= x["gap_seg"] * (1 - 1e-9)
    ref, _, _, _ = traj_reference(case, False)
    st = np.array([r["stats"] for r in ref])
    assert (st[:, 4:7] > 0).all(axis=1).any(), (case, st[:, 4:7])      # collision, max-move and joint-limit positive on one path
    assert any((~r["active"]).any() for r in ref), case                 # and a waypoint whose hinge is inactive
    if case.W >= 5:
        assert (x["seg64"][0, 0] == 0).all()                            # the zero-length segment


def test_traj_fuzz_covers_every_compiled_shape_and_route():
    from diffco_amd import _fkdesc as fd
    widths = template_widths()
    seen_w, seen_c, fams, kinds, padded = set(), set(), {"narrow": set(), "wide": set()}, set(), set()
    lengths, narrow_long, wide_long, paths, two_chain_8_waves = set(), set(), False, set(), False
    assert len({tuple(c[:6]) for c in TRAJ_CASES}) == len(TRAJ_CASES)
    for case in TRAJ_CASES:
        x = traj_setup(case)
        desc = x["desc"]
        assert desc.n_points * desc.point_dim == case.D and 1 <= case.C <= 8 and case.W >= 2 and case.R >= 1, case
        Dt = template_d_for(case.D, widths)
        seen_w.add(Dt)
        seen_c.add(case.C)
        kinds.add(int(desc.kind))
        lengths.add(case.W)
        paths.add(case.R)
        if Dt > case.D:
            padded.add(case.D)
        fam = kernel_family(*KERNELS[case.ki])
        if Dt <= 24:
            fams["narrow"].add(fam)
            if case.W > 64:
                narrow_long.add(case.W)
        if Dt > 48:
            fams["wide"].add(fam)
        if Dt >= 72 and case.W == 65 and int(desc.kind) in (fd.DCX_FK_NONE, fd.DCX_FK_SE2, fd.DCX_FK_SE3):
            # (these transforms keep no frames; the staged program is bounded by step_carve_bytes' default)
            wide_long = wide_long or step_carve_bytes(x["dof"], case.D, 0, case.W) <= LDS_BYTES
        # a row is exempt from the bit-identity leg when the persistent kernel is not instantiated for it, or - the one wide
        # tree - when its carve does not fit (test_gpu_traj_fuzz.py checks the route taken on the device), and says why
        assert not (case.bitwise and not has_persistent_form(case)), case
        assert case.bitwise == (not case.reason), case
        if has_persistent_form(case) and not case.bitwise:
            assert "carve" in case.reason and int(desc.kind) == fd.DCX_FK_TREE and Dt >= 84, case
        if int(desc.kind) == fd.DCX_FK_DH and desc.n_chains == 2 and case.C == 1 and int((x["weights"] != 0).any(axis=1).sum()) >= 120:
            two_chain_8_waves = True
    assert not set(widths) - seen_w, f"no case at compiled width(s) {sorted(set(widths) - seen_w)}"
    assert not set(range(1, 9)) - seen_c, f"no case with class count(s) {sorted(set(range(1, 9)) - seen_c)}"
    for k, v in fams.items():
        assert v == {0, 1, 2}, f"kernel families {sorted({0, 1, 2} - v)} missing at {k} widths"
    all_kinds = {fd.DCX_FK_NONE, fd.DCX_FK_PLANAR, fd.DCX_FK_DH, fd.DCX_FK_SE2, fd.DCX_FK_SE3, fd.DCX_FK_TREE}
    assert not all_kinds - kinds, f"no case of FK kind(s) {sorted(all_kinds - kinds)}"
    assert len(padded) >= 3, f"padded widths {sorted(padded)}"
    assert {2, 3, 63, 64} <= lengths, sorted(lengths)
    assert {65, 130} <= narrow_long, f"path lengths over one wave at widths <= 24: {sorted(narrow_long)}"
    assert wide_long, "no W = 65 case at a width >= 72 whose step-kernel carve fits the LDS"
    assert 1 in paths and max(paths) >= 3, sorted(paths)
    assert two_chain_8_waves, "no two-chain arm with >= 120 active supports (8 waves by traj_run's rule: J^T on several waves)"
    assert any(has_persistent_form(c) and not c.bitwise for c in TRAJ_CASES), "no row whose persistent carve does not fit"
    # the C == 1 instantiations of the persistent kernel no other test runs: RQ2 and GEN
    assert {kernel_family(*KERNELS[c.ki]) for c in TRAJ_CASES if c.C == 1 and c.W <= 64} == {0, 1, 2}


def test_step_entry_refuses_a_carve_over_the_lds_from_host_arithmetic():
    """dcx_traj_adam_step on the D = 96 keypoint body at W = 1024 (16 slabs of 64 waypoints, ~ 840 KB): DCX_ERR_UNSUPPORTED where no
    device exists at all, so the refusal precedes every HIP call.  n_paths = 0 with NULL arrays: whatever the entry point
    answers, nothing can be launched."""
    import ctypes as C
    from diffco_amd import _fkdesc as fd, _lib
    lib = _lib.load()
    desc = fd.keypoint_desc(np.random.default_rng(0).uniform(-0.5, 0.5, (32, 3)), 3)
    assert step_carve_bytes(6, 96, 0, 1024, prog_floats=0) > LDS_BYTES
    st = _lib.TrajState(0, 1024, *([None] * 14))
    opt = _lib.TrajOpts(0.02, 0.9, 0.999, 1e-8, 1, 10, 10, 10, 0.0, 0.3, 1e-2, 1e-4)
    assert lib.dcx_traj_adam_step(0, C.byref(desc), C.byref(st), C.byref(opt), 1, None) == 2
    assert b"n_waypoints is too large" in lib.dcx_last_error()
