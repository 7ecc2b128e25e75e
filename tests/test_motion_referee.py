"""CPU: the referee of the motion calls' shape fuzz (tests/test_gpu_fuzz.py) and what its case table covers.  The chain rule
that judges dcx_motion_cost's endpoint gradients (helpers.motion_chain) is checked against float64 central differences of the
float64 oracle cost, so the fuzz compares the kernels with an independent reference, not with a restatement of themselves;
the coverage guard fails when a compiled width, class count, kernel family or FK kind has no case."""
import zlib

import numpy as np
import pytest

from helpers import (KERNELS, fuzz_desc, kernel_family, motion_cases, motion_oracle, motion_samples, motion_scores,
                     template_d_for, template_widths)

# one robot of each kind: none, planar, SE(3) keypoints, single-chain DH, two-chain DH, a URDF tree
CHAIN_CASES = [("none", 5, 1, 0), ("planar", 8, 2, 5), ("se3", 24, 1, 2), ("baxter", 12, 1, 0), ("baxter_dual", 24, 2, 3),
               ("urdf_panda", 27, 1, 0)]


@pytest.mark.parametrize("rule", ["res", "closed", "open"])
@pytest.mark.parametrize("kind,D,C,ki", CHAIN_CASES)
def test_chain_rule_matches_central_differences(kind, D, C, ki, rule):
    from oracle import oracle
    rng = np.random.default_rng(zlib.crc32(repr(("chain", kind, D, C, ki, rule)).encode()))
    desc, dof, lim = fuzz_desc(kind, D, rng)
    kern = KERNELS[ki]
    cfg = lambda n: rng.uniform(lim[:, 0], lim[:, 1], (n, dof))  # noqa: E731
    sup = oracle.fkine(desc, cfg(40), dtype=np.float64).reshape(40, -1)
    W = rng.standard_normal((40, C))
    weight = 0.7
    qa = cfg(200)
    qb = qa + 0.5 * (cfg(200) - qa)
    L = np.linalg.norm(qb - qa, axis=1)
    step = float(np.median(L)) / 4
    kw = dict(res=5) if rule == "res" else dict(max_step=step, open_end=rule == "open")
    smp = motion_samples(qa, qb, dtype=np.float64, **kw)
    s = motion_scores(desc, kern, sup, W, smp)
    margin = np.median(s, axis=0)
    band = 1e-3 * np.abs(s).max()
    # edges away from the hinge kink (every sample off every margin by the band) and from a change in the sample count
    ends = np.cumsum([0] + [len(p) for p, *_ in smp])
    hit, free = [], []
    for e in range(len(smp)):
        se = s[ends[e]:ends[e + 1]] - margin
        if len(se) == 0 or (np.abs(se) <= band).any():
            continue
        if rule != "res" and abs(L[e] / step - np.round(L[e] / step)) < 1e-3:
            continue
        (hit if (se > 0).any() else free).append(e)
    keep = hit[:4] + free[:1]
    counts = [len(smp[e][0]) for e in keep]
    ref = motion_oracle(desc, kern, sup, W, [smp[e] for e in keep], margin, weight)
    assert (ref["cost"] > 0).sum() >= 2, (kind, rule)
    # every +-h perturbation of every coordinate of qa and qb, at the edge's sample count, in one oracle call
    h = 1e-6
    pert = []
    for i, e in enumerate(keep):
        for side in (0, 1):
            for j in range(dof):
                for sgn in (1, -1):
                    a, b = qa[e].copy(), qb[e].copy()
                    (a if side == 0 else b)[j] += sgn * h
                    sm = motion_samples(a[None], b[None], dtype=np.float64, counts=[counts[i]], **kw)
                    assert len(sm[0][0]) == counts[i]
                    pert += sm
    sp = np.clip(motion_scores(desc, kern, sup, W, pert) - margin[None], 0, None).sum(1)
    c = weight * np.add.reduceat(sp, np.cumsum([0] + [len(p) for p, *_ in pert[:-1]]))
    fd = ((c[0::2] - c[1::2]) / (2 * h)).reshape(len(keep), 2, dof)
    for i, e in enumerate(keep):
        got = np.stack([ref["ga"][i], ref["gb"][i]])
        scale = np.abs(fd[i]).max()
        assert scale > 0 or ref["cost"][i] == 0
        assert np.abs(got - fd[i]).max() <= 1e-6 * max(scale, 1e-300), (kind, rule, e, np.abs(got - fd[i]).max(), scale)


@pytest.mark.parametrize("entry", ["check", "cost"])
def test_motion_fuzz_covers_every_compiled_shape(entry):
    """the motion fuzz's case table reaches every compiled width, every class count 1 .. 8, every kernel family at narrow
    (<= 24) and wide (> 48) widths, every FK kind and padded widths, for each entry point"""
    widths = template_widths()
    seen_w, seen_c, fams, kinds, padded = set(), set(), {"narrow": set(), "wide": set()}, set(), set()
    for kind, D, C, ki, rule, empty in motion_cases(entry):
        desc, dof, lim = fuzz_desc(kind, D, np.random.default_rng(0))
        assert desc.n_points * desc.point_dim == D, (kind, D)
        assert rule in ("res", "closed", "open") and 1 <= C <= 8
        Dt = template_d_for(D, widths)
        seen_w.add(Dt)
        seen_c.add(C)
        kinds.add(int(desc.kind))
        if Dt > D:
            padded.add(D)
        fam = kernel_family(*KERNELS[ki])
        if Dt <= 24:
            fams["narrow"].add(fam)
        if Dt > 48:
            fams["wide"].add(fam)
    assert not set(widths) - seen_w, f"{entry}: no case at compiled width(s) {sorted(set(widths) - seen_w)}"
    assert not set(range(1, 9)) - seen_c, f"{entry}: no case with class count(s) {sorted(set(range(1, 9)) - seen_c)}"
    for k, v in fams.items():
        assert v == {0, 1, 2}, f"{entry}: kernel families {sorted({0, 1, 2} - v)} missing at {k} widths"
    from diffco_amd import _fkdesc as fd
    all_kinds = {fd.DCX_FK_NONE, fd.DCX_FK_PLANAR, fd.DCX_FK_DH, fd.DCX_FK_SE2, fd.DCX_FK_SE3, fd.DCX_FK_TREE}
    assert not all_kinds - kinds, f"{entry}: no case of FK kind(s) {sorted(all_kinds - kinds)}"
    assert len(padded) >= 3, f"{entry}: padded widths {sorted(padded)}"
