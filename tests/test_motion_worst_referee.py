"""CPU: the referee of the worst-sample motion queries (motion_worst_helpers.worst_oracle).  Its endpoint gradients - the score
gradient at the worst sample chained through the interpolation - are checked against float64 central differences of the float64
peak at a held sample count, so the GPU tests compare the kernels with an independent reference, not with a restatement of
themselves; the host composition (host_motion_worst) with a float64 torch score function agrees with the referee; the tie flags
leave enough edges for the GPU oracle test's condition; and the fuzz's case table reaches every compiled width."""
import zlib

import numpy as np
import pytest

from helpers import (KERNELS, MOTION_CASES, TorchKernel, fuzz_desc, motion_samples, motion_scores, template_d_for,
                     template_widths)
from motion_worst_helpers import worst_oracle
from test_motion_referee import CHAIN_CASES


def _peak(desc, kern, sup, W, smp, margin):
    s = motion_scores(desc, kern, sup, W, smp) - margin[None]
    ends = np.cumsum([0] + [len(p) for p, *_ in smp])
    return np.array([s[ends[e]:ends[e + 1]].max() for e in range(len(smp))])


@pytest.mark.parametrize("rule", ["res", "closed"])
@pytest.mark.parametrize("kind,D,C,ki", CHAIN_CASES)
def test_worst_gradient_matches_central_differences(kind, D, C, ki, rule):
    from oracle import oracle
    rng = np.random.default_rng(zlib.crc32(repr(("worst", kind, D, C, ki, rule)).encode()))
    desc, dof, lim = fuzz_desc(kind, D, rng)
    kern = KERNELS[ki]
    cfg = lambda n: rng.uniform(lim[:, 0], lim[:, 1], (n, dof))  # noqa: E731
    sup = oracle.fkine(desc, cfg(40), dtype=np.float64).reshape(40, -1)
    W = rng.standard_normal((40, C))
    qa = cfg(200)
    qb = qa + 0.5 * (cfg(200) - qa)
    L = np.linalg.norm(qb - qa, axis=1)
    step = float(np.median(L)) / 4
    kw = dict(res=5) if rule == "res" else dict(max_step=step)
    smp = motion_samples(qa, qb, dtype=np.float64, **kw)
    s = motion_scores(desc, kern, sup, W, smp)
    margin = np.median(s, axis=0)
    full = worst_oracle(desc, kern, sup, W, smp, margin, scores=s, grad=False)
    band = 1e-3 * np.abs(s).max()
    ends = np.cumsum([0] + [len(p) for p, *_ in smp])
    # edges whose runner-up (another sample or class) is clear of the peak and whose length is away from a count change;
    # peaks at the start, inside and (closed rule) at the target all take part where the batch has them
    by_place = {"first": [], "inner": [], "last": []}
    for e in range(len(smp)):
        v = (s[ends[e]:ends[e + 1]] - margin).reshape(-1)
        if len(v) > 1 and full["worst"][e] - np.sort(v)[-2] <= band:
            continue
        if rule != "res" and abs(L[e] / step - np.round(L[e] / step)) < 1e-3:
            continue
        n = ends[e + 1] - ends[e]
        k = full["idx"][e]
        by_place["first" if k == 0 else "last" if k == n - 1 else "inner"].append(e)
    keep = by_place["first"][:2] + by_place["inner"][:3] + by_place["last"][:2]
    assert len(by_place["inner"]) >= 1 and len(keep) >= 4, (kind, rule, {k: len(v) for k, v in by_place.items()})
    if rule == "closed":
        assert len(by_place["last"]) >= 1, (kind, "no edge peaks at its target")
    counts = [len(smp[e][0]) for e in keep]
    ref = worst_oracle(desc, kern, sup, W, [smp[e] for e in keep], margin)
    assert (ref["idx"] == full["idx"][keep]).all() and not ref["tie"].any()
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
    c = _peak(desc, kern, sup, W, pert, margin)
    fd = ((c[0::2] - c[1::2]) / (2 * h)).reshape(len(keep), 2, dof)
    for i, e in enumerate(keep):
        got = np.stack([ref["ga"][i], ref["gb"][i]])
        scale = np.abs(fd[i]).max()
        assert scale > 0
        assert np.abs(got - fd[i]).max() <= 1e-6 * scale, (kind, rule, e, np.abs(got - fd[i]).max(), scale)
        if rule == "closed" and ref["idx"][i] == counts[i] - 1:
            assert (ref["ga"][i] == 0).all()          # a peak at the target does not move with qa


def test_referee_ties_and_empty_edges():
    from diffco_amd import _fkdesc as fd
    desc = fd.none_desc(2)
    sup = np.array([[0.0, 0.0], [1.0, 0.0]])
    W = np.array([[1.0, 1.0], [0.0, 0.0]])     # two identical classes: every sample ties across classes
    qa, qb = np.array([[-1.0, 0.0], [0.3, 0.0]]), np.array([[1.0, 0.0], [0.3, 0.0]])
    smp = motion_samples(qa, qb, max_step=0.5, dtype=np.float64)
    r = worst_oracle(desc, KERNELS[0], sup, W, smp + [(np.zeros((0, 2)), np.zeros(0), np.zeros(2), np.zeros(0, bool))], [0.0, 0.0])
    assert r["idx"].tolist() == [2, 0, -2] and r["cls"].tolist() == [0, 0, -1]      # the first class of a tie, the support itself
    assert r["tie"].all() and np.isnan(r["worst"][2]) and np.isnan(r["ga"][2]).all()
    assert r["n"].tolist() == [5, 1, 0]
    r1 = worst_oracle(desc, KERNELS[0], sup, W[:, :1], smp, [0.0])
    assert r1["tie"].tolist() == [False, False] and r1["worst"][0] == pytest.approx(1.0)
    # zero length: one sample, the target - its gradient goes to qb alone
    assert (r1["ga"][1] == 0).all() and np.abs(r1["gb"][1]).max() > 0


@pytest.mark.parametrize("kname,ki,C", [("rq", 0, 3), ("poly1", 1, 1)])
@pytest.mark.parametrize("rule", ["res", "closed"])
def test_host_composition_agrees_with_referee(kname, ki, C, rule):
    import torch
    from diffco_amd import _fkdesc as fd
    from diffco_amd._perceptron import host_motion_worst
    rng = np.random.default_rng(zlib.crc32(repr(("host", kname, C, rule)).encode()))
    dof = 5
    desc = fd.none_desc(dof)
    kern = KERNELS[ki]
    sup = rng.uniform(-1.5, 1.5, (40, dof))
    W = rng.standard_normal((40, C))
    qa = rng.uniform(-1.5, 1.5, (60, dof))
    qb = qa + 0.5 * (rng.uniform(-1.5, 1.5, (60, dof)) - qa)
    qb[7] = qa[7]                                              # a zero-length edge
    step = float(np.median(np.linalg.norm(qb - qa, axis=1))) / 4
    kw = dict(res=5) if rule == "res" else dict(max_step=step)
    smp = motion_samples(qa, qb, dtype=np.float64, **kw)
    s = motion_scores(desc, kern, sup, W, smp)
    margin = np.median(s, axis=0)
    ref = worst_oracle(desc, kern, sup, W, smp, margin, scores=s)
    k = TorchKernel(kname, kern[1], kern[2])
    sup_t, W_t = torch.tensor(sup), torch.tensor(W)
    score_fn = lambda p: k(p, sup_t).reshape(len(p), -1) @ W_t  # noqa: E731
    a, b = torch.tensor(qa, requires_grad=True), torch.tensor(qb, requires_grad=True)
    worst, idx, cls, n = host_motion_worst(score_fn, a, b, margin=torch.tensor(margin), max_samples=1000, **kw)
    assert n.tolist() == ref["n"].tolist()
    keep = ~ref["tie"]
    assert keep.sum() >= 40
    assert np.abs(worst.detach().numpy() - ref["worst"]).max() <= 1e-12 * ref["s_max"]
    assert (idx.numpy()[keep] == ref["idx"][keep]).all() and (cls.numpy()[keep] == ref["cls"][keep]).all()
    worst.sum().backward()
    gs = max(np.abs(ref["ga"]).max(), np.abs(ref["gb"]).max())
    assert np.abs(a.grad.numpy()[keep] - ref["ga"][keep]).max() <= 1e-9 * gs
    assert np.abs(b.grad.numpy()[keep] - ref["gb"][keep]).max() <= 1e-9 * gs
    # an edge over max_samples: NaN / -2 / -1 and the count it needs; the others unchanged
    if rule == "closed":
        lens = ref["n"]
        cap = int(np.median(lens))
        w2, i2, c2, n2 = host_motion_worst(score_fn, a.detach(), b.detach(), margin=torch.tensor(margin), max_samples=cap, **kw)
        over = lens > cap
        assert over.any() and (~over).any()
        assert torch.isnan(w2[over]).all() and (i2[over] == -2).all() and (c2[over] == -1).all()
        assert torch.equal(w2[~over], worst.detach()[~over]) and torch.equal(i2[~over], idx[~over])
        assert n2.tolist() == lens.tolist()


def test_fuzz_table_reaches_every_compiled_width():
    """the worst-sample fuzz runs every entry of helpers.MOTION_CASES: every compiled width must have one"""
    widths = template_widths()
    seen = {template_d_for(D, widths) for _, D, *_ in MOTION_CASES}
    assert not set(widths) - seen, f"no case at compiled width(s) {sorted(set(widths) - seen)}"
    assert {C for _, _, C, *_ in MOTION_CASES} >= set(range(1, 9))


@pytest.mark.parametrize("margin_kind", ["zero", "pct"])
@pytest.mark.parametrize("rule", ["res", "max_step"])
@pytest.mark.parametrize("name", __import__("motion_worst_helpers").ORACLE_FIXTURES)
def test_gpu_oracle_cases_keep_enough_edges(name, rule, margin_kind):
    """the condition of tests/test_gpu_motion_worst.py's oracle test, checked without a GPU: at least 200 of its 300 edges lie
    outside the referee's tie band for every fixture, rule and margin set"""
    from motion_worst_helpers import ORACLE_MIN_KEEP, oracle_case
    c = oracle_case(name, rule, margin_kind)
    keep = ~c["ref"]["tie"]
    assert keep.sum() >= ORACLE_MIN_KEEP, (name, rule, margin_kind, int(keep.sum()))
    assert np.isfinite(c["ref"]["worst"]).all() and (c["ref"]["n"] >= 1).all()


@pytest.mark.parametrize("case", MOTION_CASES, ids=lambda c: f"{c[0]}-D{c[1]}-C{c[2]}-k{c[3]}-{c[4]}" + ("-empty" if c[5] else ""))
def test_fuzz_cases_keep_enough_edges(case):
    """the condition of tests/test_gpu_motion_worst_fuzz.py, checked without a GPU for every case: at least 70 % of the judged
    edges lie outside the referee's tie band, some of them peak above their margin and some below, and the edges still make
    tiles span edges and edges span tiles"""
    from motion_worst_helpers import FUZZ_MIN_KEEP, FUZZ_RUN, fuzz_case
    x = fuzz_case(case)
    norm = ~x["over"]
    keep = norm & ~x["ref"]["tie"]
    assert keep.sum() >= FUZZ_MIN_KEEP * norm.sum(), (case, int(keep.sum()), int(norm.sum()))
    w = x["ref"]["worst"][keep]
    assert (w > 0).any() and (w < 0).any(), case
    assert x["over"].sum() == (FUZZ_RUN if case[5] else 0)
    assert x["counts"][norm].sum() > 64 and x["counts"].max() >= 7
    if case[4] != "res":
        assert (x["counts"] == 1).any() and len(set(x["counts"][norm].tolist())) > 5, case
