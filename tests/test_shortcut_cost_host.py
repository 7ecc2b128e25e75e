"""host_shortcut_paths(objective="clearance") (diffco_amd/shortcut.py) on CPU tensors, the referee of the fused rounds, over
rrtstar_cost_helpers.SoftDiscs - discs with a signed-distance score: every applied slot restated in numpy float32 (each piece
free, C or new < old in the contract's own sums), the provenance of seg after every round (bit for bit the price of a fresh
motion_worst on the current waypoints), all-free paths stay all-free and cost what clearance_cost_paths says, a colliding segment
is repaired, a hand-built corner keeps its distance where the length mode skims the disc, gain 0, and the coverage of the draws
asserted on the referee's own record.  No GPU."""
import numpy as np
import pytest
import torch

from rrtstar_cost_helpers import SoftDiscs, cost32
from rrtstar_helpers import F, bits, fixed, length32
from shortcut_cost_helpers import Record, assert_provenance, assert_same_state, path_cost32, span32

from diffco_amd.rrtstar import clearance_cost_paths
from diffco_amd.shortcut import host_shortcut_paths, shortcut_paths

MAX_STEP, MAX_SAMPLES, T, R, CAP = 0.05, 400, 24, 3, 20
GAIN, BAND = 4.0, 0.15   # rrtstar_cost_helpers' GAIN_C and BAND_C: a motion within 0.15 of a disc is charged
# the seed of the paths and the draws was chosen here on the CPU against the referee's own record (Record.seen) so that every
# case below - both modes, slots 1 and 4 - shows every event it can: applied, blocked, dearer, lost, idle and two applied in one
# round (a round of one slot has no earlier slot to lose to and applies at most one: Record.assert_coverage leaves those two out
# there).  The coverage is a condition of the tests, asserted on the record
SEED = 3
CASES = [(False, 1), (False, 4), (True, 1), (True, 4)]


def _paths(seed=SEED):
    """three zig-zags of 8, 12 and 16 waypoints around SoftDiscs' discs, every segment free: two under the large disc (the
    small one at (0, -0.55) stays inside the arc), one over it and over the small disc at (0, 0.8)"""
    rng = np.random.default_rng(seed)
    out = []
    for n, (a0, a1) in zip((8, 12, 16), ((np.pi, 2 * np.pi), (1.1 * np.pi, 1.9 * np.pi), (np.pi, 0.0))):
        ang = np.linspace(a0, a1, n)
        rad = 0.82 + 0.13 * (-1.0) ** np.arange(n) + 0.04 * (rng.random(n) - 0.5)
        if a1 == 0.0:
            rad = rad + 0.35
        out.append(torch.tensor(np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1).astype(F)))
    return out


def _draws(P, seed=SEED):
    u = np.random.default_rng(100 + seed).random((T, R, P, 2), dtype=F)
    u[1, 0, 0, 0] = np.nan   # a spoilt draw idles its slot
    return torch.from_numpy(u)


def _kw(partial, P, **over):
    kw = dict(max_step=MAX_STEP, max_samples=MAX_SAMPLES, slots=P, rounds=T, partial=partial, objective="clearance",
              clearance_gain=GAIN, clearance_band=BAND)
    if partial:
        kw["capacity"] = CAP
    kw.update(over)
    return kw


def _worst(qa, qb):
    return SoftDiscs().motion_worst(torch.from_numpy(np.ascontiguousarray(qa)), torch.from_numpy(np.ascontiguousarray(qb)),
                                    max_step=MAX_STEP, max_samples=1 << 20)[0].numpy()


def _check_applied(rec, path, seg, partial, gain):
    """every applied slot of the one round in `rec`, restated from the state before it"""
    rd = rec.rounds[-1]
    for r, p in zip(*np.nonzero(rd["applied"].numpy())):
        w = rd["w"][r, p].numpy().reshape(-1)
        assert (w <= 0).all(), (r, p, w)
        if partial:
            ea, eb = int(rd["ea"][r, p]), int(rd["eb"][r, p])
            xa, xb = rd["xa"][r, p].numpy(), rd["xb"][r, p].numpy()
            ends = [(path[r, ea], xa), (xa, xb), (xb, path[r, eb + 1])]
            C = [cost32(length32(a, b), w[k], gain, BAND) for k, (a, b) in enumerate(ends)]
            new, old = F(F(C[0] + C[1]) + C[2]), span32(seg[r], ea, eb)
            assert bits(rd["pieces"][r, p].numpy()).tolist() == bits(np.array(C, F)).tolist()
        else:
            i, j = int(rd["i"][r, p]), int(rd["j"][r, p])
            new, old = cost32(length32(path[r, i], path[r, j]), w[0], gain, BAND), span32(seg[r], i, j - 1)
        assert new < old, (r, p, new, old)
        assert bits(rd["cost"][r, p].numpy()) == bits(new) and bits(rd["old"][r, p].numpy()) == bits(old), (r, p)


def _chained(partial, P, gain=GAIN, paths=None):
    """24 calls of one round each, every call on the state the last one left (its seg formed afresh): after every round the
    applied slots, the provenance of seg and the endpoints; (the last result, the record)"""
    draws, rec = _draws(P), Record()
    first = _paths() if paths is None else paths
    res = host_shortcut_paths(SoftDiscs(), first, **_kw(partial, P, rounds=0, clearance_gain=gain))
    accepted = torch.zeros(R, dtype=torch.int32)
    for t in range(T):
        before, seg = res.path.numpy().copy(), res.seg.numpy().copy()
        res = host_shortcut_paths(SoftDiscs(), res.path, res.count, **_kw(partial, P, rounds=1, clearance_gain=gain, _record=rec,
                                                                          sampler=fixed(draws[t:t + 1])))
        _check_applied(rec, before, seg, partial, gain)
        assert_provenance(_worst, res.path, res.count, res.seg, gain, BAND)
        for r, p in enumerate(first):
            assert torch.equal(res.paths[r][0], p[0]) and torch.equal(res.paths[r][-1], p[-1]), (t, r)
        accepted += res.accepted
    res.accepted = accepted   # (every call counts from 0)
    return res, rec


@pytest.mark.parametrize("partial,P", CASES)
def test_rounds_applied_slots_provenance_and_coverage(partial, P):
    res, rec = _chained(partial, P)
    print("partial", partial, "slots", P, rec.seen, "counts", res.count.tolist(), "costs", res.costs.tolist())
    rec.assert_coverage(P)
    # T rounds in one call leave the same bits as T calls of one round: a call's own seg is the fresh sweep's, round after round
    ck = SoftDiscs()
    one = host_shortcut_paths(ck, _paths(), **_kw(partial, P, sampler=fixed(_draws(P)), rounds_per_call=5))
    assert one.route == "host"
    assert ck.batches == [sum(len(p) - 1 for p in _paths())] + [R * P * (3 if partial else 1)] * T   # ONE sweep per round, fixed
    assert_same_state(one, res)
    # shortcut_paths routes CPU tensors to the same composition
    again = shortcut_paths(SoftDiscs(), _paths(), **_kw(partial, P, sampler=fixed(_draws(P))))
    assert again.route == "host"
    assert_same_state(again, one)
    # costs never rise, and the result's sums are the contract's
    assert (one.costs <= one.costs_before).all() and (one.costs < one.costs_before).any()
    for r, n in enumerate(one.count.tolist()):
        assert bits(one.costs[r].numpy()) == bits(path_cost32(one.seg[r].numpy(), n))


@pytest.mark.parametrize("partial,P", CASES)
def test_all_free_stays_all_free_and_costs_what_clearance_cost_paths_says(partial, P):
    res = host_shortcut_paths(SoftDiscs(), _paths(), **_kw(partial, P, sampler=fixed(_draws(P))))
    assert torch.isfinite(res.costs_before).all()   # every initial segment is free
    cost, _, peak = clearance_cost_paths(SoftDiscs(), res.path, res.count, max_step=MAX_STEP, gain=GAIN, band=BAND,
                                         max_samples=MAX_SAMPLES)
    assert (peak <= 0).all(), peak
    assert bits(cost.numpy()).tolist() == bits(res.costs.numpy()).tolist()


@pytest.mark.parametrize("partial", [False, True])
def test_a_colliding_segment_is_repaired(partial):
    # the second segment runs through the large disc; the chord from waypoint 0 to waypoint 3 passes under it with room to spare
    p = torch.tensor([[-0.9, -0.9], [-0.5, -0.2], [0.5, -0.2], [0.9, -0.9]], dtype=torch.float32)
    u = torch.tensor([[[[0.0, 0.999]]]]) if not partial else torch.tensor([[[[0.01, 0.99]]]])
    ck = SoftDiscs(discs=((0.0, 0.0, 0.4),))
    res = host_shortcut_paths(ck, [p], **_kw(partial, 1, rounds=1, sampler=fixed(u), capacity=8 if partial else None))
    assert float(res.costs_before[0]) == float("inf") and torch.isfinite(res.costs[0])
    assert int(res.accepted[0]) == 1 and int(res.count[0]) == (4 if partial else 2)
    _, _, peak = clearance_cost_paths(ck, res.path, res.count, max_step=MAX_STEP, gain=GAIN, band=BAND, max_samples=MAX_SAMPLES)
    assert float(peak[0]) <= 0


def test_hand_built_corner_keeps_its_distance():
    """one disc, a three-waypoint path over it with room to spare.  The length mode pulls the corner down to the disc's edge; the
    clearance mode at gain 4 ends cheaper under the objective and stays at least half a band away.  Scene and seed chosen here
    on the CPU so that both hold for the referee."""
    ck = lambda: SoftDiscs(discs=((0.0, 0.0, 0.4),))
    p = [torch.tensor([[-0.9, -0.1], [0.0, 1.3], [0.9, -0.1]], dtype=torch.float32)]
    kw = dict(max_step=MAX_STEP, max_samples=MAX_SAMPLES, slots=4, rounds=48, partial=True, capacity=40, seed=1)
    length = host_shortcut_paths(ck(), p, **kw)
    clear = host_shortcut_paths(ck(), p, objective="clearance", clearance_gain=GAIN, clearance_band=BAND, **kw)
    cost = lambda res: clearance_cost_paths(ck(), res.path, res.count, max_step=MAX_STEP, gain=GAIN, band=BAND, max_samples=MAX_SAMPLES)
    (cl, ll, pl), (cc, lc, pc) = cost(length), cost(clear)
    print("length mode: cost, length, peak", float(cl), float(ll), float(pl), " clearance mode:", float(cc), float(lc), float(pc))
    assert -0.02 < float(pl) <= 0          # the length mode skims the disc
    assert float(cc) < float(cl)           # cheaper under the objective
    assert float(pc) <= -BAND / 2          # and at a distance
    assert bits(cc.numpy()) == bits(clear.costs.numpy())


@pytest.mark.parametrize("partial,P", [(False, 4), (True, 4)])
def test_gain_zero_applies_only_chords_that_shorten(partial, P):
    res, rec = _chained(partial, P, gain=0.0)   # (_check_applied: every applied chord has C == L < old)
    assert rec.seen["applied"] >= 1
    for rd in rec.rounds:
        on = rd["applied"]
        assert (rd["cost"][on] < rd["old"][on]).all()
    length = host_shortcut_paths(SoftDiscs(), _paths(), **_kw(partial, P, sampler=fixed(_draws(P)), objective="length"))
    assert length.seg is None and length.costs is None and length.costs_before is None
    # never lengthening: the cost of a free path IS its length at gain 0
    assert (res.costs <= res.costs_before).all()
    print("gain 0 lengths", res.costs.tolist(), "length mode", length.lengths.tolist())


def test_arguments():
    class NoWorst:
        def check_motions(self, *a, **k):
            raise AssertionError("not reached")

    with pytest.raises(TypeError, match="motion_worst"):
        host_shortcut_paths(NoWorst(), _paths(), **_kw(False, 1))
    with pytest.raises(ValueError, match="clearance_band"):
        shortcut_paths(SoftDiscs(), _paths(), max_step=MAX_STEP, objective="clearance")
    with pytest.raises(ValueError, match="clearance_gain"):
        shortcut_paths(SoftDiscs(), _paths(), max_step=MAX_STEP, objective="clearance", clearance_band=0.1, clearance_gain=-1.0)
    with pytest.raises(ValueError, match="objective"):
        host_shortcut_paths(SoftDiscs(), _paths(), max_step=MAX_STEP, objective="peak")
