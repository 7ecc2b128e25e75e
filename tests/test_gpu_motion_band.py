"""GPU: hybrid motion checks (dcx_motion_band, ScoreModel.motion_band_raw / motion_band / score_band and the perceptron's
routing) against the fp64 referee (motion_band_helpers.band_oracle) on the judged edges, against dcx_check_motions and
dcx_motion_worst with no tolerance (the three calls score a sample to the same bits), the list's order, content, capacity and
configurations, the limits of the band, edges over max_samples, tile shapes, per-class thresholds, determinism and graph
capture, score_band and the host route."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import CASE_ROBOT, case_kernel, load, make_robot, motion_scores
from motion_band_helpers import (BAND_MIN_EACH, BAND_MIN_JUDGED, BAND_RULES, ORACLE_FIXTURES, band_case, band_oracle, judged_list,
                                 listed_points32)
from motion_worst_helpers import TIE_BAND, class_margins, fixture_edges, fixture_model, samples32

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def ops():
    from diffco_amd import _lib, _ops
    _lib.require_gpu()
    return _ops


@pytest.fixture
def early_exit():
    from diffco_amd import _lib
    lib = _lib.load()
    yield lambda v: _lib.check(lib.dcx_debug_set(b"motion_early_exit", int(v)))
    lib.dcx_debug_set(b"motion_early_exit", -1)


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")


_models = {}


def _model(ops, name):
    if name not in _models:
        d, desc, kern, sup, W = fixture_model(name)
        _models[name] = (d, ops.ScoreModel(desc, kern[0], kern[1], kern[2], _t(sup), _t(W)), desc, kern, sup, W)
    return _models[name]


def _band(d):
    return class_margins(d["score64"], 90), class_margins(d["score64"], 97)


def _pairs(r, total=None):
    total = int(r["unc_total"]) if total is None else total
    return list(zip(r["unc_edge"][:total].cpu().tolist(), r["unc_sample"][:total].cpu().tolist()))


def _step(qa, qb, div=20):
    return max(float(np.median(np.linalg.norm(qb - qa, axis=1))) / div, 1e-3)


# ---- against the fp64 oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", BAND_RULES)
@pytest.mark.parametrize("name", ORACLE_FIXTURES)
def test_band_matches_fp64_oracle(ops, name, rule):
    c = band_case(name, rule)
    ref = c["ref"]
    j = ref["judged"]
    m = _model(ops, name)[1]
    r = m.motion_band_raw(_t(c["qa"]), _t(c["qb"]), c["lo"], c["hi"], unc_cap=2 * ref["total"] + 64, **c["kw"])
    verdict, first, n_unc, n = (r[k].cpu().numpy() for k in ("verdict", "first_hit", "n_uncertain", "n_samples"))
    each = [int((ref["verdict"][j] == v).sum()) for v in (0, 1, 2)]
    print(f"{name} {rule}: judged {int(j.sum())}, free / colliding / uncertain {each}; verdicts off on "
          f"{int((verdict[j] != ref['verdict'][j]).sum())} judged and {int((verdict[~j] != ref['verdict'][~j]).sum())} other edges")
    assert j.sum() >= BAND_MIN_JUDGED and min(each) >= BAND_MIN_EACH
    assert n.tolist() == ref["n"].tolist()
    assert (verdict[j] == ref["verdict"][j]).all()
    assert (first[j] == ref["first"][j]).all()
    assert (n_unc[j] == ref["n_unc"][j]).all()
    assert [p for p in _pairs(r) if j[p[0]]] == judged_list(ref)
    assert int(r["unc_total"]) == int(n_unc.sum())


# ---- the siblings, no tolerance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [0, 0x7f])
@pytest.mark.parametrize("rule", BAND_RULES)
@pytest.mark.parametrize("E", [300, 5000])
@pytest.mark.parametrize("name", ["cfg2_baxter_poly1", "cfg3_baxter_rq_c5"])
def test_exact_ties_to_the_siblings(ops, early_exit, name, E, rule, mask):
    """same options and mask: first_hit and n_samples are dcx_check_motions(margin = hi)'s with the check's early exit on and
    off; verdict == 0 exactly where dcx_motion_worst(margin = lo) answers worst <= 0 and verdict == 1 exactly where
    dcx_motion_worst(margin = hi) answers worst > 0 - on every edge, at a batch that splits its launch and one that does not"""
    d, m, *_ = _model(ops, name)
    lo, hi = _band(d)
    qa, qb = fixture_edges(d["q"], E, 3 + E)
    kw = dict(res=13) if rule == "res" else dict(max_step=_step(qa, qb), max_samples=4000)
    a, b = _t(qa), _t(qb)
    r = m.motion_band_raw(a, b, lo, hi, wrap=mask, unc_cap=16, **kw)
    for ee in (0, 1):
        early_exit(ee)
        first, n = m.check_motions(a, b, margin=hi, wrap=mask, **kw)
        assert torch.equal(r["first_hit"], first), ee
        assert torch.equal(r["n_samples"], n), ee
    w_lo = m.motion_worst_raw(a, b, margin=lo, wrap=mask, **kw)[0]
    w_hi = m.motion_worst_raw(a, b, margin=hi, wrap=mask, **kw)[0]
    assert not bool(torch.isnan(w_lo).any())
    assert torch.equal(r["verdict"] == 0, w_lo <= 0)
    assert torch.equal(r["verdict"] == 1, w_hi > 0)
    assert torch.equal(r["verdict"] == 1, r["first_hit"] >= 0)
    counts = [int((r["verdict"] == v).sum()) for v in (0, 1, 2)]
    assert min(counts) > 0 and sum(counts) == E, counts
    assert int(r["unc_total"]) == int(r["n_uncertain"].sum()) > 16          # (the list itself was cut at 16 entries)
    assert bool((r["n_uncertain"][r["verdict"] != 2] == 0).all()) and bool((r["n_uncertain"][r["verdict"] == 2] > 0).all())


# ---- the list ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [0, 0b0100101, 0x7f])
@pytest.mark.parametrize("rule", BAND_RULES)
def test_the_list(ops, rule, mask):
    """strictly ascending in (edge, sample); n_uncertain counts its entries per edge and sums to unc_total; it holds exactly the
    code-2 samples of the verdict-2 edges (against dcx_score on the restated points, away from the thresholds' tie band); unc_q
    is the float32 restatement of the listed samples, bit for bit - with no, a partial and a full wrap mask"""
    d, m, *_ = _model(ops, "cfg2_baxter_poly1")
    lo, hi = _band(d)
    qa, qb = fixture_edges(d["q"], 400, 21)
    kw = dict(res=13) if rule == "res" else dict(max_step=_step(qa, qb), max_samples=4000)
    verdict, first, n_unc, ue, us, uq = m.motion_band(_t(qa), _t(qb), lo, hi, wrap=mask, **kw)
    r = m.motion_band_raw(_t(qa), _t(qb), lo, hi, wrap=mask, unc_cap=len(ue), **kw)
    assert int(r["unc_total"]) == len(ue) == len(us) == len(uq) == int(n_unc.sum()) > 100
    assert torch.equal(r["unc_edge"], ue) and torch.equal(r["unc_sample"], us) and torch.equal(r["unc_q"], uq)
    e, k, n = ue.cpu().numpy().astype(np.int64), us.cpu().numpy().astype(np.int64), r["n_samples"].cpu().numpy()
    key = e * (int(n.max()) + 1) + k
    assert (np.diff(key) > 0).all()
    assert (k >= 0).all() and (k < n[e]).all()
    v = verdict.cpu().numpy()
    assert (v[e] == 2).all()
    assert (np.bincount(e, minlength=len(qa)) == n_unc.cpu().numpy()).all()
    # the configurations, bit for bit
    ref_q = listed_points32(qa, qb, mask, e, k, kw.get("res"), kw.get("max_step"))
    got_q = uq.cpu().numpy()
    assert (got_q.view(np.uint32) == ref_q.view(np.uint32)).all(), int((got_q.view(np.uint32) != ref_q.view(np.uint32)).sum())
    # exactly the band samples of the undecided edges: every sample of those edges, scored by dcx_score on its restated point
    und = np.nonzero(v != 1)[0]
    ends = np.concatenate([[0], np.cumsum(n[und])])
    all_e = np.repeat(und, n[und])
    all_k = np.arange(ends[-1]) - np.repeat(ends[:-1], n[und])
    s = m.score_raw(_t(listed_points32(qa, qb, mask, all_e, all_k, kw.get("res"), kw.get("max_step")))).cpu().numpy()
    band = TIE_BAND * np.abs(s).max()
    clear_of = (np.abs(s - np.asarray(lo, F)[None]) > band).all(axis=1) & (np.abs(s - np.asarray(hi, F)[None]) > band).all(axis=1)
    assert clear_of.mean() > 0.9
    assert not (s[clear_of] - np.asarray(hi, F)[None] > 0).any()              # no sure hit on an undecided edge
    in_band = (s - np.asarray(lo, F)[None] > 0).any(axis=1)
    listed = np.zeros(len(all_e), bool)
    pos = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(all_e, all_k))}
    listed[[pos[p] for p in zip(e.tolist(), k.tolist())]] = True
    assert (listed[clear_of] == in_band[clear_of]).all()


def test_capacity_and_canaries(ops):
    """unc_cap = 0 and unc_cap = total // 2 return the prefix of the full list and the same unc_total; nothing is written at or
    beyond unc_cap in any of the three list arrays"""
    from diffco_amd import _lib
    from diffco_amd._lib import MotionBandOut, MotionOpts
    d, m, *_ = _model(ops, "cfg3_baxter_rq_c5")
    lo, hi = _band(d)
    qa, qb = fixture_edges(d["q"], 300, 9)
    a, b = _t(qa), _t(qb)
    full = m.motion_band_raw(a, b, lo, hi, res=13, unc_cap=100000)
    total = int(full["unc_total"])
    assert 64 < total < 100000
    lo_t, hi_t = _t(lo), _t(hi)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for cap in (0, total // 2):
        room = total + 32
        verdict = torch.empty(len(qa), dtype=torch.int32, device="cuda")
        n_unc = torch.empty(len(qa), dtype=torch.int32, device="cuda")
        tot = torch.zeros(1, dtype=torch.int64, device="cuda")
        ue = torch.full((room,), -7, dtype=torch.int32, device="cuda")
        us = torch.full((room,), -7, dtype=torch.int32, device="cuda")
        uq = torch.full((room, m.dof), -7.0, dtype=torch.float32, device="cuda")
        out = MotionBandOut(p(verdict), None, None, p(n_unc), p(tot), p(ue), p(us), p(uq), cap)
        opt = MotionOpts(13, 0.0, 13, 0)
        nbytes = m._lib.dcx_motion_band_work_bytes(m._h, len(qa), 13)
        work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        _lib.check(m._lib.dcx_motion_band(m._h, p(a), p(b), len(qa), ctypes.byref(opt), p(lo_t), p(hi_t), ctypes.byref(out),
                                          p(work), nbytes, 0, m._st()))
        torch.cuda.synchronize()
        assert int(tot) == total and torch.equal(verdict, full["verdict"]) and torch.equal(n_unc, full["n_uncertain"])
        assert torch.equal(ue[:cap], full["unc_edge"][:cap]) and torch.equal(us[:cap], full["unc_sample"][:cap])
        assert torch.equal(uq[:cap], full["unc_q"][:cap])
        assert bool((ue[cap:] == -7).all()) and bool((us[cap:] == -7).all()) and bool((uq[cap:] == -7).all())
        # the Python layer's fixed capacity: the same prefix, unc_total as a tensor, nothing read back
        got = m.motion_band(a, b, lo, hi, res=13, max_uncertain=cap)
        assert len(got) == 7 and int(got[6]) == total and len(got[3]) == cap
        assert torch.equal(got[3], full["unc_edge"][:cap]) and torch.equal(got[5], full["unc_q"][:cap])
    # without a capacity the Python layer sizes the list itself, also when its first guess is too small
    big_a, big_b = a.repeat(30, 1), b.repeat(30, 1)
    v, f, nu, e2, k2, q2 = m.motion_band(big_a, big_b, -1e30, 1e30, res=13)
    assert len(e2) == 13 * len(big_a) > max(4096, 2 * len(big_a)) and int(nu.sum()) == len(e2)
    v0, f0, nu0, e0, k0, q0 = m.motion_band(a, b, lo, hi, res=13, want_q=False)
    assert q0 is None and torch.equal(e0, full["unc_edge"][:total]) and torch.equal(k0, full["unc_sample"][:total])


# ---- the limits of the band ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg2_baxter_poly1", "cfg3_baxter_rq_c5"])
def test_limits_of_the_band(ops, name):
    d, m, *_ = _model(ops, name)
    lo, hi = _band(d)
    qa, qb = fixture_edges(d["q"], 300, 5)
    a, b = _t(qa), _t(qb)
    for kw in (dict(res=13), dict(max_step=_step(qa, qb), max_samples=4000)):
        # lo == hi: no uncertain edge, the verdicts are the check's
        r = m.motion_band_raw(a, b, hi, hi, unc_cap=8, **kw)
        first, n = m.check_motions(a, b, margin=hi, **kw)
        assert int(r["unc_total"]) == 0 and not bool((r["verdict"] == 2).any()) and not bool(r["n_uncertain"].any())
        assert torch.equal(r["verdict"] == 1, first >= 0) and torch.equal(r["first_hit"], first)
        assert 0 < int((first >= 0).sum()) < len(qa)
        # lo = -inf, hi = +inf: every sample of every edge is listed
        total = int(n.sum())
        r = m.motion_band_raw(a, b, -float("inf"), float("inf"), unc_cap=total + 8, **kw)
        assert int(r["unc_total"]) == total and bool((r["verdict"] == 2).all()) and torch.equal(r["n_uncertain"], n)
        nn = n.cpu().numpy()
        assert r["unc_edge"][:total].cpu().tolist() == np.repeat(np.arange(len(qa)), nn).tolist()
        assert r["unc_sample"][:total].cpu().tolist() == np.concatenate([np.arange(c) for c in nn]).tolist()


def test_edges_over_max_samples(ops):
    d, m, *_ = _model(ops, "cfg2_baxter_poly1")
    lo, hi = _band(d)
    qa, qb = fixture_edges(d["q"], 300, 15)
    a, b = _t(qa), _t(qb)
    step = _step(qa, qb)
    full = m.motion_band_raw(a, b, lo, hi, max_step=step, max_samples=4000, unc_cap=20000)
    n = full["n_samples"]
    cap = int(n.float().median())
    over = n > cap
    assert 50 < int(over.sum()) < 250
    r = m.motion_band_raw(a, b, lo, hi, max_step=step, max_samples=cap, unc_cap=20000)
    assert torch.equal(r["n_samples"], n)
    assert bool((r["verdict"][over] == -2).all()) and bool((r["first_hit"][over] == -2).all()) and not bool(r["n_uncertain"][over].any())
    for k in ("verdict", "first_hit", "n_uncertain"):
        assert torch.equal(r[k][~over], full[k][~over]), k
    keep = ~over[full["unc_edge"][:int(full["unc_total"])].long()]
    tot = int(r["unc_total"])
    assert tot == int(keep.sum()) > 0
    assert torch.equal(r["unc_edge"][:tot], full["unc_edge"][:int(full["unc_total"])][keep])
    assert torch.equal(r["unc_sample"][:tot], full["unc_sample"][:int(full["unc_total"])][keep])
    assert torch.equal(r["unc_q"][:tot], full["unc_q"][:int(full["unc_total"])][keep])


# ---- tile shapes ---------------------------------------------------------------------------------------------------------------
def _against_referee(m, model, qa, qb, lo, hi, what, **kw):
    desc, kern, sup, W = model
    smp = samples32(qa, qb, kw.get("res"), kw.get("max_step"))
    ref = band_oracle(smp, motion_scores(desc, kern, sup, W, smp), lo, hi)
    r = m.motion_band_raw(_t(qa), _t(qb), lo, hi, unc_cap=int(ref["n"].sum()) + 8, **dict(kw, max_samples=int(ref["n"].max())))
    j = ref["judged"]
    assert r["n_samples"].cpu().tolist() == ref["n"].tolist(), what
    for k, rk in (("verdict", "verdict"), ("first_hit", "first"), ("n_uncertain", "n_unc")):
        assert (r[k].cpu().numpy()[j] == ref[rk][j]).all(), (what, k)
    assert [p for p in _pairs(r) if j[p[0]]] == judged_list(ref), what
    assert int(r["unc_total"]) == int(r["n_uncertain"].sum()), what
    return ref, r


def test_tile_shapes(ops):
    """the smallest shapes at which the tiles can go wrong, on the D = 12 Baxter fixture with its own supports"""
    d, m, desc, kern, sup, W = _model(ops, "cfg2_baxter_poly1")
    assert m.D == 12
    model = (desc, kern, sup, W)
    lo, hi = _band(d)
    q = d["q"].astype(F)
    # E = 1, short and long: a single tile with idle lanes, and one edge spanning three tiles
    qa, qb = fixture_edges(q, 1, 2)
    _against_referee(m, model, qa, qb, lo, hi, "E = 1", res=5)
    ref, _ = _against_referee(m, model, qa, qb, lo, hi, "one edge, three tiles", res=131)
    assert ref["n"].tolist() == [131]
    ref, _ = _against_referee(m, model, qa, qb, lo, hi, "one edge, three tiles, closed", max_step=float(np.linalg.norm(qb - qa)) / 140.5)
    assert 130 <= ref["n"][0] <= 192
    # a total that is no multiple of 64, edges shorter and longer than a tile
    qa, qb = fixture_edges(q, 37, 4)
    ref, _ = _against_referee(m, model, qa, qb, lo, hi, "ragged total", max_step=_step(qa, qb, 45))
    assert ref["n"].sum() % 64 != 0 and ref["n"].max() > 64 > ref["n"].min() and ref["judged"].sum() >= 25
    assert set(ref["verdict"][ref["judged"]].tolist()) == {0, 1, 2}
    # 200 one-sample edges: more than 64 edges end in one tile
    qa, _ = fixture_edges(q, 200, 6)
    ref, r = _against_referee(m, model, qa, qa, lo, hi, "one-sample edges", res=1)
    assert set(ref["verdict"][ref["judged"]].tolist()) == {0, 1, 2} and not bool(r["unc_sample"][:int(r["unc_total"])].any())
    # E = 0
    z = torch.zeros((0, 7), device="cuda")
    r = m.motion_band_raw(z, z, lo, hi, res=4, unc_cap=4)
    assert len(r["verdict"]) == 0 and int(r["unc_total"]) == 0
    got = m.motion_band(z, z, lo, hi, max_step=0.1)
    assert [len(x) for x in got] == [0] * 6 and got[5].shape == (0, 7)


def test_per_class_thresholds_and_their_order(ops):
    d, m, *_ = _model(ops, "cfg3_baxter_rq_c5")
    assert m.C == 5
    lo, hi = _band(d)
    qa, qb = fixture_edges(d["q"], 100, 8)
    a, b = _t(qa), _t(qb)
    base = m.motion_band_raw(a, b, lo, hi, res=9, unc_cap=2000)
    # one class alone decides: with every other class out of reach the verdicts are that class's
    for c in (0, 3):
        lo_c = [lo[i] if i == c else 1e30 for i in range(5)]
        hi_c = [hi[i] if i == c else 1e30 for i in range(5)]
        r = m.motion_band_raw(a, b, lo_c, hi_c, res=9, unc_cap=2000)
        w = m.motion_worst_raw(a, b, res=9, margin=hi_c)[0]
        assert torch.equal(r["verdict"] == 1, w > 0)
        assert bool(((r["verdict"] == 1) <= (base["verdict"] == 1)).all())
    bad = list(hi)
    bad[2] = lo[2] - 1.0
    with pytest.raises(ValueError, match="lo > hi for class 2"):
        m.motion_band(a, b, lo, bad, res=9)
    with pytest.raises(ValueError, match="lo > hi"):
        m.motion_band(a, b, 1.0, 0.0, res=9)
    with pytest.raises(ValueError, match="exactly one of res and max_step"):
        m.motion_band(a, b, lo, hi)


# ---- determinism and graph capture -------------------------------------------------------------------------------------------
def test_deterministic_and_capturable(ops):
    d, m, *_ = _model(ops, "cfg3_baxter_rq_c5")
    qa, qb = fixture_edges(d["q"], 500, 11)
    a, b = _t(qa), _t(qb)
    lo, hi = (_t(x) for x in _band(d))             # on the device: nothing crosses from the host in a capture
    for kw in (dict(max_step=0.1, max_samples=4096, unc_cap=30000), dict(res=9, unc_cap=30000)):
        keys = ("verdict", "first_hit", "n_samples", "n_uncertain", "unc_total", "unc_edge", "unc_sample", "unc_q")
        ref = m.motion_band_raw(a, b, lo, hi, **kw)
        total = int(ref["unc_total"])
        assert 100 < total < 30000
        cut = lambda r: [r[k][:total] if k.startswith("unc_") and k != "unc_total" else r[k] for k in keys]  # noqa: E731
        want = [x.clone() for x in cut(ref)]
        for x, y in zip(want, cut(m.motion_band_raw(a, b, lo, hi, **kw))):
            assert torch.equal(x, y)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            warm = m.motion_band_raw(a, b, lo, hi, **kw)
        torch.cuda.current_stream().wait_stream(s)
        for x, y in zip(want, cut(warm)):
            assert torch.equal(x, y)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = m.motion_band_raw(a, b, lo, hi, **kw)
        for _ in range(2):
            for k in keys:
                out[k].fill_(-7)
            g.replay()
            torch.cuda.synchronize()
            for x, y in zip(want, cut(out)):
                assert torch.equal(x, y)
            assert bool((out["unc_edge"][total:] == -7).all())
        assert len(set(ref["verdict"].cpu().tolist())) == 3


# ---- the Python surface ----------------------------------------------------------------------------------------------------
def _new_api(name):
    from diffco_amd import kernel
    from diffco_amd.kernel_perceptrons import DiffCo
    d = load(name)
    kind, p0, p1 = case_kernel(d)
    rob = make_robot(CASE_ROBOT[name])
    kf = kernel.Polyharmonic(int(p0), p1) if kind == 1 else kernel.RQKernel(p0, p1)
    dc = DiffCo(kernel_func=kf, transform=rob.fkine)
    dc.support_points = _t(d["sup_q"])
    dc.support_transformed = rob.fkine(dc.support_points)
    dc.gains = _t(d["weights"][:, 0])
    return d, dc, rob


def test_score_band(ops):
    """score_band(q, lo, hi) is the thresholding of the one-sample sweep: label 1 where check_motions(q, q, res=1, margin=hi)
    hits, 0 where the worst (only) sample lies at or below lo; unc_idx lists the label-2 configurations in ascending order"""
    d, m, *_ = _model(ops, "cfg2_baxter_poly1")
    lo, hi = _band(d)
    q = _t(d["q"][:700])
    label, idx = m.score_band(q, lo, hi)
    first, _ = m.check_motions(q, q, res=1, margin=hi)
    w = m.motion_worst_raw(q, q, res=1, margin=lo)[0]
    assert label.dtype == torch.int32 and idx.dtype == torch.int64
    assert torch.equal(label == 1, first >= 0) and torch.equal(label == 0, w <= 0)
    assert torch.equal(idx, (label == 2).nonzero().reshape(-1))
    assert min(int((label == v).sum()) for v in (0, 1, 2)) > 0
    # the perceptron's method: the same call on its own model
    d2, dc, rob = _new_api("cfg2_baxter_rq")
    s = dc.score(q).reshape(-1)
    lo2, hi2 = float(s.quantile(0.6)), float(s.quantile(0.85))
    lab, ix = dc.score_band(q, lo2, hi2)
    assert dc.last_route == "fused"
    clear = ((s - lo2).abs() > TIE_BAND * float(s.abs().max())) & ((s - hi2).abs() > TIE_BAND * float(s.abs().max()))
    want = torch.where(s > hi2, 1, torch.where(s <= lo2, 0, 2)).to(torch.int32)
    assert int(clear.sum()) > 650 and torch.equal(lab[clear], want[clear])
    assert torch.equal(ix, (lab == 2).nonzero().reshape(-1))


def test_a_foreign_transform_takes_the_host_route(ops):
    d, dc, rob = _new_api("cfg2_baxter_rq")
    qa, qb = fixture_edges(d["q"], 120, 13)
    a, b = _t(qa), _t(qb)
    s0 = dc.score(_t(d["q"][:500])).reshape(-1)
    lo, hi = float(s0.quantile(0.8)), float(s0.quantile(0.95))
    fused = dc.motion_band(a, b, lo, hi, max_step=0.2)
    assert dc.last_route == "fused"
    dc.transform = lambda q: rob.fkine(q) * 1.0   # same map, not a diffco_amd robot's fkine: not fusable
    host = dc.motion_band(a, b, lo, hi, max_step=0.2)
    assert dc.last_route == "host"
    # judged edges: no sample of the host's own scores within the tie band of a threshold
    from helpers import motion_points
    pts = motion_points(qa, qb, max_step=0.2)
    s = dc.score(_t(np.concatenate(pts))).reshape(-1).cpu().numpy()
    near = (np.abs(s - lo) <= TIE_BAND * np.abs(s).max()) | (np.abs(s - hi) <= TIE_BAND * np.abs(s).max())
    ends = np.cumsum([0] + [len(p) for p in pts])
    j = np.array([not near[ends[e]:ends[e + 1]].any() for e in range(len(pts))])
    assert j.sum() >= 100
    jt = torch.as_tensor(j, device="cuda")
    for x, y in zip(fused[:3], host[:3]):
        assert x.dtype == y.dtype == torch.int32 and torch.equal(x[jt], y[jt])
    assert len(set(fused[0][jt].cpu().tolist())) == 3
    fp = [(e, k) for e, k in zip(fused[3].cpu().tolist(), fused[4].cpu().tolist()) if j[e]]
    hp = [(e, k) for e, k in zip(host[3].cpu().tolist(), host[4].cpu().tolist()) if j[e]]
    assert fp == hp and len(fp) > 20
    fq = {(e, k): x for e, k, x in zip(fused[3].cpu().tolist(), fused[4].cpu().tolist(), fused[5].cpu().numpy())}
    hq = {(e, k): x for e, k, x in zip(host[3].cpu().tolist(), host[4].cpu().tolist(), host[5].cpu().numpy())}
    assert max(np.abs(fq[p] - hq[p]).max() for p in fp) <= 1e-5
    with pytest.raises(ValueError, match="lo > hi"):
        dc.motion_band(a, b, 1.0, 0.0, max_step=0.2)
