"""CPU: the referee of RRT*'s device-side sampling (rrtstar.host_device_samples, rrtstar.philox4x32_10) and host_rrt_star drawing
from it.  Philox4x32-10 against the known answers of the Random123 distribution; on hand-made states of 2 and 7 coordinates the
goal rows carry the goals' bits, every informed sample lies in its problem's informed set under the torus metric, c = c_min
puts the samples on the segment, a draw depends on neither the chunking nor T, and seeds differ; then case S (rrtstar_helpers)
planned with sampling="informed": every state is a valid tree, no cost rises, and every sample drawn for a problem after it
first reached its goal lies in the informed set of the best cost the trace shows at that round's start."""
import functools

import pytest
import torch

from rrtstar_helpers import GOALS_S, STARTS_S, Discs, check_state, kwargs_s
from rrtstar_sample_helpers import (BAXTER_MASK, GOAL_BIAS, TRIES, assert_in_informed_set, best_cost, dist64, kinds,
                                    make_state, wrapped)

KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
SEED_INFORMED = 19   # chosen on the CPU against the referee's own trace: see test_case_s_informed


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    from diffco_amd.rrtstar import philox4x32_10
    assert " ".join("%08x" % int(w) for w in philox4x32_10(counter, key)) == want
    # as tensors, broadcast: the same words in every element
    c = [torch.full((3, 2), v, dtype=torch.int64) for v in counter]
    out = philox4x32_10(c, key)
    assert all(o.shape == (3, 2) and (o == int(w, 16)).all() for o, w in zip(out, want.split()))


def _draw(dof, mask, seed=7, g=3, P=16, mode="informed", R=24, **kw):
    from diffco_amd.rrtstar import host_device_samples
    st, goals, lim = make_state(R, dof, mask)
    return (st, goals, lim) + host_device_samples(st, goals, lim, seed, g, P, mode, kw.get("goal_bias", GOAL_BIAS),
                                                  kw.get("uniform_mix", 0.), TRIES, mask)


@pytest.mark.parametrize("dof,mask", [(2, 0), (2, 3), (7, 0), (7, BAXTER_MASK)])
def test_referee_rows_by_kind(dof, mask):
    st, goals, lim, smp, info, cand = _draw(dof, mask)
    kind = kinds(24)
    assert cand.shape == (TRIES, 24, 16, dof) and cand.dtype == torch.float64 and smp.dtype == torch.float32
    # not running: the start row
    idle = (kind == 1) | (kind == 2)
    assert bool((info[idle] == -1).all()) and torch.equal(smp[idle], st["nodes"][idle, 0][:, None, :].expand(-1, 16, -1))
    # without a goal node: goal rows with the goals' bits at about the bias, else uniform in the limits
    open_ = kind == 0
    assert set(info[open_].reshape(-1).tolist()) == {0, 1}
    rows = info == 1
    assert torch.equal(smp[rows].view(torch.int32), goals[:, None, :].expand(-1, 16, -1)[rows].view(torch.int32))
    assert 0.1 < float(rows[open_].float().mean()) < 0.45
    # with a goal node: no goal bias any more, informed draws, every one in the informed set
    solved = kind == 3
    assert bool((info[solved] >= 2).all())
    accepted = assert_in_informed_set(smp, info, st, goals, mask)
    assert accepted + int((info == 2 + TRIES).sum()) == int(solved.sum()) * 16 and accepted >= int(solved.sum() - 1) * 16
    assert bool(((lim[:, 0] <= smp) & (smp < lim[:, 1])).all())
    # the corner problem's ellipsoid pokes out of the limits: later tries and the info words say so (where every coordinate is
    # on the circle and the limits are the circle, the wrap brings every point back inside)
    corner = int(torch.nonzero(solved)[-1])
    assert int((info[corner] > 2).sum()) >= 1 or mask == (1 << dof) - 1
    # uniform mode never draws informed, and is the informed mode's draw where that one is not informed
    _, _, _, smp_u, info_u, _ = _draw(dof, mask, mode="uniform")
    assert set(info_u.reshape(-1).tolist()) <= {-1, 0, 1}
    assert torch.equal(smp_u[info < 2], smp[info < 2]) and torch.equal(info_u[info < 2], info[info < 2])
    # uniform_mix = 1: every draw of a solved problem is uniform
    _, _, _, _, info_m, _ = _draw(dof, mask, uniform_mix=1.0)
    assert bool((info_m[solved] == 0).all())


@pytest.mark.parametrize("dof,mask", [(2, 0), (7, BAXTER_MASK)])
def test_c_equal_c_min_gives_points_on_the_segment(dof, mask):
    st, goals, lim, smp, info, cand = _draw(dof, mask)
    r = 1   # the first solved problem: c = c_min exactly
    start = st["nodes"][r, 0].to(torch.float64)
    a = wrapped(goals[r].to(torch.float64) - start, mask)
    assert float(best_cost(st)[r]) == pytest.approx(float(a.norm()), rel=1e-6)
    x = cand[0, r]   # (before the float32 rounding)
    rel = wrapped(x - start, mask)
    along = (rel @ a) / (a @ a)
    # the draw's axis is the float32 delta (2^-24 relative per coordinate), this one the float64 difference: the residual off
    # the segment is at most that rounding times the distance walked, far below 1e-6 at these lengths of a few units
    assert bool((along > -1e-6).all()) and bool((along < 1 + 1e-6).all())
    assert float((rel - along[:, None] * a[None]).norm(dim=1).max()) < 1e-6
    assert float(along.max() - along.min()) > 0.2   # spread along it


def test_draw_depends_on_seed_round_and_slot_alone():
    from diffco_amd.rrtstar import host_device_samples
    st, goals, lim = make_state(12, 7, BAXTER_MASK)
    args = (GOAL_BIAS, 0.1, TRIES, BAXTER_MASK)
    a = host_device_samples(st, goals, lim, 11, 5, 16, "informed", *args)
    b = host_device_samples(st, goals, lim, 11, 5, 4, "informed", *args)       # fewer slots: the same leading slots
    assert torch.equal(a[0][:, :4], b[0]) and torch.equal(a[1][:, :4], b[1])
    sub = {k: v[:5] for k, v in st.items()}                                     # fewer problems: the same leading problems
    c = host_device_samples(sub, goals[:5], lim, 11, 5, 16, "informed", *args)
    assert torch.equal(a[0][:5], c[0]) and torch.equal(a[1][:5], c[1])
    other_round = host_device_samples(st, goals, lim, 11, 6, 16, "informed", *args)
    other_seed = host_device_samples(st, goals, lim, 12, 5, 16, "informed", *args)
    high_word = host_device_samples(st, goals, lim, 11 + (1 << 32), 5, 16, "informed", *args)
    running = st["status"] == 0
    for o in (other_round, other_seed, high_word):   # (two goal rows of one problem are the same row)
        same = (o[0] == a[0]).all(dim=-1) & ~((o[1] == 1) & (a[1] == 1))
        assert not bool(same[running].any())


@functools.lru_cache(maxsize=None)
def _case_s(chunk):
    from diffco_amd.rrtstar import host_rrt_star
    ck, trace = Discs(), []
    res = host_rrt_star(ck, STARTS_S, GOALS_S, sampling="informed", goal_bias=GOAL_BIAS, seed=SEED_INFORMED, record_samples=True,
                        _trace=trace, **kwargs_s(rounds_per_call=chunk))
    return res, trace, ck


def test_case_s_informed():
    res, trace, ck = _case_s(4)
    assert res.route == "host" and res.rounds == 24 and res.samples.shape == (24, 4, 4, 2) and res.sample_info.shape == (24, 4, 4)
    prev, informed, later_tries, fell_back = None, 0, 0, 0
    first = res.first_round.tolist()
    assert min(f for f in first if f >= 0) < 12, first   # a problem solved before round 12 (the seed was chosen for it)
    for g, ev in enumerate(trace):
        st = ev["state"]
        check_state(st, prev, ck if g % 6 == 5 else None, 0.05)   # (no cost rises: check_state holds cost <= prev's)
        before = trace[g - 1]["state"] if g else None
        smp, info = res.samples[g], res.sample_info[g]
        assert torch.equal(smp, ev["samples"]) and torch.equal(info, ev["sample_info"])
        for r in range(4):
            running = int(before["status"][r]) == 0 if g else int(res.status[r]) not in (1, 3)
            if not running:
                assert bool((info[r] == -1).all()) and torch.equal(smp[r], STARTS_S[r][None].expand(4, 2))
            elif 0 <= first[r] < g:
                # drawn after first_round: no goal row, every sample in the informed set of the best cost at the round's start
                assert bool((info[r] >= 2).all()), (g, r, info[r])
                c = float(best_cost(before)[r])
                total = dist64(STARTS_S[r][None], smp[r], 0) + dist64(smp[r], GOALS_S[r][None], 0)
                assert bool((total <= c * (1 + 1e-5)).all()), (g, r)
                informed += 4
                later_tries += int(((info[r] > 2) & (info[r] < 2 + 8)).sum())
                fell_back += int((info[r] == 2 + 8).sum())
            else:
                assert set(info[r].tolist()) <= {0, 1}
        prev = st
    print("case S informed: first_round", first, "informed draws", informed, "at a later try", later_tries, "fell back", fell_back)
    assert informed >= 16 and later_tries >= 1   # (the seed was chosen for a draw accepted at a try > 0)
    assert fell_back <= 0.01 * informed           # the ellipsoid of the hard problem lies almost inside the square


def test_case_s_does_not_depend_on_the_chunking():
    a, b, c = _case_s(4)[0], _case_s(1)[0], _case_s(24)[0]
    for o in (b, c):
        assert torch.equal(a.samples, o.samples) and torch.equal(a.sample_info, o.sample_info)
        for k, v in a.state().items():
            assert torch.equal(v, o.state()[k]), k


def test_options_are_checked():
    from diffco_amd.rrtstar import host_rrt_star
    kw = kwargs_s()
    with pytest.raises(ValueError, match="sampler"):
        host_rrt_star(Discs(), STARTS_S, GOALS_S, sampling="informed", sampler=lambda T, R, P: None, **kw)
    with pytest.raises(ValueError, match="sampling"):
        host_rrt_star(Discs(), STARTS_S, GOALS_S, sampling="gpu", **kw)
    with pytest.raises(ValueError, match="informed_tries"):
        host_rrt_star(Discs(), STARTS_S, GOALS_S, sampling="informed", informed_tries=17, **kw)
    with pytest.raises(ValueError, match="uniform_mix"):
        host_rrt_star(Discs(), STARTS_S, GOALS_S, sampling="informed", uniform_mix=1.5, **kw)
    kw.pop("limits")
    with pytest.raises(ValueError, match="limits"):
        host_rrt_star(Discs(), STARTS_S, GOALS_S, sampling="device", **kw)
    # the default is the host sampler, and it records what it was given
    res = host_rrt_star(Discs(), STARTS_S, GOALS_S, record_samples=True, **kwargs_s(max_rounds=4))
    assert res.samples.shape == (4, 4, 4, 2) and res.sample_info is None
    assert host_rrt_star(Discs(), STARTS_S, GOALS_S, **kwargs_s(max_rounds=4)).samples is None
