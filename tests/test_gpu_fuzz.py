"""Shape fuzz of the fused sweep against the fp64 oracle: every compiled feature width (through keypoint bodies,
planar arms and the identity transform), class counts 1..8, all kernel families, supports that do and do not divide
among the waves, batches with ragged tiles.  Exercises the width-dependent scalar pipelines (whole rows / two rows /
half rows, weights straddling the halves) and both cross-wave fold modes."""
import zlib

import numpy as np
import pytest
import torch

from helpers import (KERNELS, fuzz_desc, kernel_family, motion_cases, motion_oracle, motion_samples, motion_scores, relerr,
                     template_d_for)

pytestmark = pytest.mark.gpu


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")


def _n(t):
    return t.detach().cpu().numpy()


def _desc(kind, D, rng):
    """(FK description, dof) of a case: identity, planar arm, SE(2) / SE(3) keypoints, DH robots, URDF trees (helpers.fuzz_desc)"""
    return fuzz_desc(kind, D, rng)[:2]


CASES = []
_rng = np.random.default_rng(2024)
for D in (2, 3, 5, 7, 9, 12, 13, 14, 16, 17, 18, 19, 21, 23, 24, 25, 27, 30, 31, 32):
    CASES.append(("none", D, int(_rng.integers(1, 9)), int(_rng.integers(len(KERNELS)))))
for D in (4, 8, 18, 22, 26, 36, 38, 42, 44, 48, 54, 60, 62, 64):
    CASES.append(("planar", D, int(_rng.integers(1, 9)), int(_rng.integers(len(KERNELS)))))
for D in (27, 33, 39, 45, 51, 57, 63, 66, 69, 72, 75, 78, 84, 87, 90, 96):
    CASES.append(("se3", D, int(_rng.integers(1, 9)), int(_rng.integers(len(KERNELS)))))
for C in range(1, 9):  # every class count at a half-row width and at a two-row width
    CASES.append(("planar", 40, C, C % len(KERNELS)))
    CASES.append(("none", 20, C, (C + 1) % len(KERNELS)))


@pytest.mark.parametrize("kind,D,C,ki", CASES)
def test_fused_sweep_shapes(kind, D, C, ki):
    from diffco_amd import _ops
    from oracle import oracle
    seed = zlib.crc32(repr((kind, D, C, ki)).encode())  # deterministic across processes
    rng = np.random.default_rng(seed)
    desc, dof = _desc(kind, D, rng)
    kern = KERNELS[ki]
    S = int(rng.choice([37, 150, 333, 1000]))
    B = int(rng.choice([1, 63, 130, 700, 3000]))
    lo, hi = (-1.5, 1.5)
    sq = rng.uniform(lo, hi, (S, dof)).astype(np.float32)
    q = rng.uniform(lo, hi, (B, dof)).astype(np.float32)
    W = rng.standard_normal((S, C)).astype(np.float32)
    W[rng.random((S, C)) < 0.2] = 0.0
    up = rng.standard_normal((B, C)).astype(np.float32)
    sup = _n(_ops.fkine(desc, _t(sq))).reshape(S, -1)
    assert sup.shape[1] == D
    m = _ops.ScoreModel(desc, *kern, _t(sup), _t(W))
    rs, rg, rj = oracle.score_grad(desc, *kern, sup, W, q, up if C > 1 else None, want_jac=True, dtype=np.float64)
    s, g = m.score_grad_raw(_t(q), _t(up) if C > 1 else None)
    assert relerr(_n(s), rs) < 1e-5, (kind, D, C, kern, S, B)
    assert relerr(_n(g), rg) < 2e-5, (kind, D, C, kern, S, B)
    assert relerr(_n(m.score_raw(_t(q))), rs) < 1e-5
    if C > 1:  # row-sum (all-ones upstream) path and the Jacobian
        s1, g1 = m.score_grad_raw(_t(q), None)
        _, rg1, _ = oracle.score_grad(desc, *kern, sup, W, q, None, dtype=np.float64)
        assert relerr(_n(g1), rg1) < 2e-5
    if B <= 700:
        _, jac = m.score_jac_raw(_t(q))
        assert relerr(_n(jac), rj) < 2e-5


HESS_CASES = []
for D in (2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 14, 15, 16):          # widths that land on the compiled 2 .. 16 (odd ones are padded)
    HESS_CASES.append(("none", D, int(_rng.integers(1, 9)), int(_rng.integers(len(KERNELS)))))
for D in (4, 8, 12, 16):
    HESS_CASES.append(("planar", D, int(_rng.integers(1, 9)), int(_rng.integers(len(KERNELS)))))
for D in (6, 9, 12, 15):
    HESS_CASES.append(("se3", D, int(_rng.integers(1, 6)), int(_rng.integers(len(KERNELS)))))


@pytest.mark.parametrize("kind,D,C,ki", HESS_CASES)
def test_hessian_moments_form_shapes(kind, D, C, ki):
    """shape fuzz of dcx_score_hess's moments form (hess_kernel.hip hess_moments_kernel) against the lanes form - which the reference's
    double backward and the float64 oracle pin (tests/test_gpu_hess.py): every width the form is compiled for, class counts 1 .. 8
    with and without an upstream, all kernel families (the generic ones through KF_GEN), supports that do not fill the block's
    waves, ragged batches, forced splits of the supports"""
    from diffco_amd import _lib, _ops
    lib = _lib.load()
    seed = zlib.crc32(repr(("hess", kind, D, C, ki)).encode())
    rng = np.random.default_rng(seed)
    desc, dof = _desc(kind, D, rng)
    kern = KERNELS[ki]
    S = int(rng.choice([5, 37, 150, 333, 1000]))
    B = int(rng.choice([1, 63, 130, 700, 3000]))
    sq = rng.uniform(-1.5, 1.5, (S, dof)).astype(np.float32)
    q = _t(rng.uniform(-1.5, 1.5, (B, dof)).astype(np.float32))
    W = rng.standard_normal((S, C)).astype(np.float32)
    W[rng.random((S, C)) < 0.2] = 0.0
    W[0, :] = 1.0   # (at least one active support)
    sup = _ops.fkine(desc, _t(sq)).reshape(S, -1)
    m = _ops.ScoreModel(desc, *kern, sup, _t(W))
    ups = [None] + ([_t(rng.standard_normal((B, C)).astype(np.float32))] if C > 1 or rng.random() < 0.5 else [])
    try:
        for up in ups:
            _lib.check(lib.dcx_debug_set(b"hess_form", 0))
            g0, H0 = m.score_hess_raw(q, up)
            for ys in (-1, 3):
                _lib.check(lib.dcx_debug_set(b"hess_form", 1))
                _lib.check(lib.dcx_debug_set(b"hess_ys", ys))
                g1, H1 = m.score_hess_raw(q, up)
                lib.dcx_debug_set(b"hess_ys", -1)
                scale = max(float(H0.abs().max()), 1e-30)
                assert float((H1 - H0).abs().max()) / scale < 1e-5, (kind, D, C, kern, S, B, ys, up is None)
                assert relerr(_n(g1), _n(g0)) < 5e-6, (kind, D, C, kern, S, B, ys, up is None)
    finally:
        lib.dcx_debug_set(b"hess_form", -1)
        lib.dcx_debug_set(b"hess_ys", -1)


# ---- batched motion checks (dcx_check_motions) and motion costs (dcx_motion_cost) against the fp64 oracle -------------------
# The case table is helpers.MOTION_CASES (tests/test_motion_referee.py checks what it covers).  Per case: random supports
# through the GPU FK, random weights (about 20 % zero), 150 - 300 edges between random configurations, short and long (1 up to
# a few hundred samples under max_step), margins at per-class percentiles of the oracle's scores.  Each launch form runs on the
# same inputs and is judged against the oracle: the default, the direct form (xf = 0) where the expanded one exists, one
# forced wave count, a forced split of the supports (sized so that dcx_api.hip's split bounds hold).
F = np.float32
MOTION_RUN = 70   # edges in a run of empty ones: more than the 64 samples of one tile end there


def _xf_applies(Dt, C, kf):
    """score_kernel.h xf_applies at the model's compiled class count"""
    Cc = C if C <= 1 else 4 if C <= 4 else 5 if C == 5 else 8
    used = Dt + Cc + (1 if Cc > 1 else 0)
    parts = 0 if 4 * used <= 56 else (used + 37) // 38
    return kf in (0, 1) and used + 1 <= 38 and parts <= 1


def _motion_setup(case, entry):
    """model inputs, edges, host samples and the fp64 referee of one case for one entry point (both entry points of a case
    draw the same supports, weights and edges; the checks take the closed rule where the costs take open_end)"""
    from diffco_amd import _ops
    kind, D, C, ki, rule, empty = case
    rng = np.random.default_rng(zlib.crc32(repr(("motion", case)).encode()))   # deterministic across processes
    desc, dof, lim = fuzz_desc(kind, D, rng)
    kern = KERNELS[ki]
    S = int(rng.choice([37, 150, 333, 1000]))
    cfg = lambda n: rng.uniform(lim[:, 0], lim[:, 1], (n, dof)).astype(F)  # noqa: E731
    sup = _n(_ops.fkine(desc, _t(cfg(S)))).reshape(S, -1)
    assert sup.shape[1] == D
    W = rng.standard_normal((S, C)).astype(F)
    W[rng.random((S, C)) < 0.2] = 0.0
    E = int(rng.integers(150, 301))
    qa, far = cfg(E), cfg(E)
    if rule == "res":
        kw = dict(res=int(rng.integers(7, 14)))
        qb = far
    else:
        step = float(np.median(np.linalg.norm(far - qa, axis=1))) / 30
        scale = np.exp(rng.uniform(np.log(1e-3), np.log(1.5 if empty else 4.0), E))
        scale[rng.random(E) < 0.03] = 0.0   # zero length: one sample (qb), none under open_end
        qb = (qa + scale[:, None] * (far - qa)).astype(F)
        kw = dict(max_step=step, open_end=(rule == "open" and entry == "cost"))
    smp = motion_samples(qa, qb, kw.get("res"), kw.get("max_step"), kw.get("open_end", False))
    ms = max(len(p) for p, *_ in smp)
    over = np.zeros(E, bool)
    if empty:   # after 20 edges: a run of zero-length edges, then a run of edges over max_samples, then the rest.  The long
        # edges' L / max_step lands within an ulp of an integer: their counts still match exactly (regression: the prep
        # kernel once took the 1-ulp native square root for L and answered one sample more on some of them)
        dirn = rng.standard_normal((MOTION_RUN, dof))
        dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
        a0 = cfg(2 * MOTION_RUN)
        b0 = np.concatenate([a0[:MOTION_RUN], a0[MOTION_RUN:] + dirn * kw["max_step"] * (ms + 20)]).astype(F)
        qa, qb = np.concatenate([qa[:20], a0, qa[20:]]), np.concatenate([qb[:20], b0, qb[20:]])
        smp = motion_samples(qa, qb, kw.get("res"), kw.get("max_step"), kw.get("open_end", False))
        over = np.array([len(p) > ms for p, *_ in smp])
        assert over.sum() == MOTION_RUN
    counts = np.array([len(p) for p, *_ in smp])
    judged = [(p[:0], t[:0], u, g[:0]) if o else (p, t, u, g) for (p, t, u, g), o in zip(smp, over)]
    s = motion_scores(desc, kern, sup, W, judged)
    # per-class margins: a quantile of the edges' largest scores, so that about half of the edges hit some class
    ends = np.cumsum([0] + [len(p) for p, *_ in judged])
    emax = np.stack([s[ends[e]:ends[e + 1]].max(0) for e in range(len(judged)) if ends[e + 1] > ends[e]])
    margin = np.quantile(emax, 1 - 0.5 / C, axis=0).astype(F)
    weight = float(rng.choice([0.5, 1.0, 1.7]))
    ref = motion_oracle(desc, kern, sup, W, judged, margin.astype(np.float64), weight, scores=s, grad=(entry == "cost"))
    return dict(desc=desc, kern=kern, sup=sup, W=W, qa=qa, qb=qb, kw=kw, ms=ms, over=over, counts=counts, margin=margin,
               weight=weight, ref=ref, device_margin=bool(rng.random() < 0.5), nw=int(rng.choice([1, 2, 4, 8])),
               ys=int(rng.choice([2, 4])), derived_bound=bool(rng.random() < 0.5) and not empty, S=S, dof=dof)


def _motion_legs(case, x):
    """[(name, knobs, edge slice)] of the launch forms a case runs"""
    kind, D, C, ki, rule, empty = case
    legs = [("default", {}, slice(None))]
    if _xf_applies(template_d_for(D), C, kernel_family(*x["kern"])):
        legs.append(("xf0", {"xf": 0}, slice(None)))
    legs.append(("nw", {"nw": x["nw"], "ys": 1}, slice(None)))
    # a split: at most 256 tiles of 64 samples and 512 (tile, slice) rows in the bound (dcx_api.hip kMotionSplitTiles / Rows);
    # waves per slice so that every wave keeps >= 15 supports (pick_geometry's min_rows rule)
    s_act = int((x["W"] != 0).any(axis=1).sum())
    ys = x["ys"] if s_act >= 15 * x["ys"] else 2
    nw = 1
    while nw < 16 and s_act // (ys * nw * 2) >= 15:
        nw *= 2
    E_s = min(len(x["qa"]), (min(256, 512 // ys) * 64) // x["ms"])
    knobs = {"ys": ys, "nw": nw}
    if s_act // ys < 15:
        knobs["min_rows"] = max(1, s_act // ys)
    legs.append(("split", knobs, slice(0, E_s)))
    return legs


def _margin_arg(x):
    return _t(x["margin"]) if x["device_margin"] else x["margin"].tolist()


@pytest.fixture
def motion_early_exit():
    from diffco_amd import _lib
    lib = _lib.load()
    yield lambda v: _lib.check(lib.dcx_debug_set(b"motion_early_exit", int(v)))
    lib.dcx_debug_set(b"motion_early_exit", -1)


def _motion_id(c):
    return f"{c[0]}-D{c[1]}-C{c[2]}-k{c[3]}-{c[4]}" + ("-empty" if c[5] else "")


@pytest.mark.parametrize("case", motion_cases("check"), ids=_motion_id)
def test_motion_checks_shapes(case, knob, motion_early_exit):
    from diffco_amd import _ops
    x = _motion_setup(case, "check")
    m = _ops.ScoreModel(x["desc"], *x["kern"], _t(x["sup"]), _t(x["W"]))
    ref, over, counts = x["ref"], x["over"], x["counts"]
    norm = ~over
    keep = norm & ~ref["tie"]
    assert keep.sum() >= 0.7 * norm.sum(), (case, keep.sum(), norm.sum())
    assert (ref["first"][keep] >= 0).any() and (ref["first"][keep] == -1).any(), case
    kw = x["kw"]
    for name, knobs, sl in _motion_legs(case, x):
        for k, v in knobs.items():
            knob(k, v)
        ms = None if (x["derived_bound"] and name == "default") else x["ms"]
        eex = (1, 0) if name == "split" else (-1,)
        for ee in eex:
            motion_early_exit(ee)
            first, n = m.check_motions(_t(x["qa"][sl]), _t(x["qb"][sl]), res=kw.get("res"), max_step=kw.get("max_step"),
                                       margin=_margin_arg(x), max_samples=ms if kw.get("res") is None else None)
            first, n = _n(first), _n(n)
            what = (case, name, ee, len(first))
            assert n.tolist() == counts[sl].tolist(), what
            k = keep[sl]
            bad = np.nonzero(first[k] != ref["first"][sl][k])[0]
            assert len(bad) == 0, (what, np.nonzero(k)[0][bad][:8], first[k][bad][:8], ref["first"][sl][k][bad][:8])
            assert (first[over[sl]] == -2).all() and (first[norm[sl]] >= -1).all(), what
        motion_early_exit(-1)
        for k in knobs:
            knob(k, -1)


@pytest.mark.parametrize("case", motion_cases("cost"), ids=_motion_id)
def test_motion_cost_shapes(case, knob):
    from diffco_amd import _ops
    x = _motion_setup(case, "cost")
    m = _ops.ScoreModel(x["desc"], *x["kern"], _t(x["sup"]), _t(x["W"]))
    ref, over, counts = x["ref"], x["over"], x["counts"]
    norm = ~over
    keep = norm & ~ref["tie"]
    empty = norm & (counts == 0)
    assert keep.sum() >= 0.7 * norm.sum(), (case, keep.sum(), norm.sum())
    assert (ref["cost"][keep] > 0).any() and (ref["cost"][keep] == 0).any(), case
    c_bar = 1e-5 * x["weight"] * ref["abs_s"][norm].max()
    g_bar = 2e-5 * max(ref["g_inf"][norm].max(), 1e-30)
    kw = x["kw"]
    ms = x["ms"] if kw.get("res") is None else None
    for name, knobs, sl in _motion_legs(case, x):
        for k, v in knobs.items():
            knob(k, v)
        runs = []
        for _ in range(2 if name == "split" else 1):
            got = m.motion_cost_raw(_t(x["qa"][sl]), _t(x["qb"][sl]), margin=_margin_arg(x), weight=x["weight"],
                                    max_samples=None if (x["derived_bound"] and name == "default") else ms, **kw)
            runs.append([_n(v) for v in got])
        for k in knobs:
            knob(k, -1)
        cost, ga, gb, n = runs[0]
        what = (case, name, len(cost))
        if name == "split":   # the same bits on a second call
            for a, b in zip(runs[0], runs[1]):
                assert np.array_equal(a, b, equal_nan=True), what
        assert n.tolist() == counts[sl].tolist(), what
        nm, kp, o = norm[sl], keep[sl], over[sl]
        err = np.abs(cost[nm] - ref["cost"][sl][nm]).max(initial=0)
        assert err <= c_bar, (what, err, c_bar)
        for g, rg in ((ga, ref["ga"]), (gb, ref["gb"])):
            err = np.abs(g[kp] - rg[sl][kp]).max(initial=0)
            assert err <= g_bar, (what, err, g_bar)
        assert np.isnan(cost[o]).all() and np.isnan(ga[o]).all() and np.isnan(gb[o]).all(), what
        e0 = empty[sl]
        assert (cost[e0] == 0).all() and (ga[e0] == 0).all() and (gb[e0] == 0).all(), what
        if name == "default":
            assert (cost[kp] > 0).any() and (cost[kp] == 0).any(), what
            # away from ties, a positive cost exactly where check_motions finds a hit (under open_end: before the target)
            open_end = kw.get("open_end", False)
            first, _ = m.check_motions(_t(x["qa"]), _t(x["qb"]), res=kw.get("res"), max_step=kw.get("max_step"),
                                       margin=_margin_arg(x), max_samples=None if ms is None else ms + 1)
            first = _n(first)
            hit = (first >= 0) & ((first < counts) if open_end else True)
            assert ((cost[kp] > 0) == hit[kp]).all(), (what, np.nonzero((cost[kp] > 0) != hit[kp])[0][:8])
