"""host_shortcut_paths (diffco_amd/shortcut.py) on CPU tensors with test_rrt_host's fake 2-D checker - a wall with a gap -
against a plain list-and-loop restatement of include/dcx.h's shortcut contract written here: equal path[:count] (bits), count
and accepted; the coverage of the draws asserted on the restatement's own record; the outcome (the zig-zag ends as three
waypoints through the gap); idle draws, chunking, subdivide and the argument errors.  No GPU."""
import numpy as np
import pytest
import torch

from motion_band_helpers import listed_points32
from test_rrt_host import Wall

from diffco_amd.shortcut import ShortcutResult, host_shortcut_paths, shortcut_paths

F = np.float32
ZIGZAG = [(-.8, -.8), (-.6, .6), (-.4, -.6), (-.3, .5), (-.2, 0), (.2, 0), (.3, -.5), (.4, .6), (.6, .7), (.8, -.8)]
MAX_STEP, P, T = 0.05, 4, 16


def _paths():
    z = torch.tensor(ZIGZAG, dtype=torch.float32)
    return [z.clone(), z.clone(), z.clone(), torch.stack([z[0], z[-1]])]


def _draws(seed):
    return torch.from_numpy(np.random.default_rng(seed).random((T, 4, P, 2), dtype=F))


def _fixed(draws):
    """a sampler that hands out the rounds of `draws` in order, whatever the chunking"""
    at = [0]

    def sampler(Tc, R, Pc):
        out = draws[at[0]:at[0] + Tc]
        at[0] += Tc
        return out
    return sampler


def _length(p):
    p = np.asarray(p, np.float64)
    return float(np.linalg.norm(p[1:] - p[:-1], axis=1).sum())


# ---- the contract in lists and loops, numpy float32 one operation at a time --------------------------------------------------
def restated(checker, paths, draws, max_step, max_samples):
    paths = [[np.array(w, F) for w in p] for p in paths]
    R, Pn = len(paths), draws.shape[2]
    accepted = [0] * R
    seen = dict(applied=0, lost=0, two=0, blocked=0, idle=0, batches=[])
    for t in range(len(draws)):
        picks = []
        for r in range(R):
            n = len(paths[r])
            row = []
            for p in range(Pn):
                u0, u1 = F(draws[t, r, p, 0]), F(draws[t, r, p, 1])
                if n < 3 or not (u0 >= 0 and u0 < 1) or not (u1 >= 0 and u1 < 1):
                    row.append(None)
                    continue
                i = min(int(F(u0 * F(n - 2))), n - 3)
                m = n - 2 - i
                j = i + 2 + min(int(F(u1 * F(m))), m - 1)
                assert 0 <= i and i + 2 <= j <= n - 1
                row.append((i, j))
            picks.append(row)
        # the fixed batch: an idle slot takes the zero-length edge on the path's first row
        qa = np.array([paths[r][pk[0]] if pk else paths[r][0] for r in range(R) for pk in picks[r]], F)
        qb = np.array([paths[r][pk[1]] if pk else paths[r][0] for r in range(R) for pk in picks[r]], F)
        seen["batches"].append(len(qa))
        first = checker.check_motions(torch.from_numpy(qa), torch.from_numpy(qb), max_step=max_step, wrap=None,
                                      max_samples=max_samples, return_first=True)[1].numpy().reshape(R, Pn)
        for r in range(R):
            applied = []
            for p in range(Pn):
                if picks[r][p] is None:
                    seen["idle"] += 1
                    continue
                if first[r, p] != -1:
                    seen["blocked"] += 1
                    continue
                i, j = picks[r][p]
                if all(j <= iq or jq <= i for iq, jq in applied):
                    applied.append((i, j))
                else:
                    seen["lost"] += 1
            seen["applied"] += len(applied)
            seen["two"] += len(applied) >= 2
            accepted[r] += len(applied)
            old, new = paths[r], [None] * len(paths[r])
            kept = 0
            for k, w in enumerate(old):
                if any(i < k < j for i, j in applied):
                    continue
                at = k - sum(j - i - 1 for i, j in applied if j <= k)
                assert at == kept and new[at] is None   # survivors keep their order
                new[at] = w
                kept += 1
            paths[r] = new[:kept]
    return paths, accepted, seen


def _same(res, paths, accepted):
    assert res.count.tolist() == [len(p) for p in paths]
    assert res.accepted.tolist() == accepted
    for r, p in enumerate(paths):
        got = res.path[r, :len(p)].numpy()
        assert got.tobytes() == np.array(p, F).reshape(len(p), 2).tobytes(), r


@pytest.fixture(scope="module")
def max_samples():
    return int(np.ceil(_length(ZIGZAG) / MAX_STEP)) + 2


def test_the_input_is_what_the_issue_says(max_samples):
    wall = Wall()
    z = torch.tensor(ZIGZAG, dtype=torch.float32)
    assert abs(_length(ZIGZAG) - 7.997) < 1e-3
    kw = dict(max_step=MAX_STEP, wrap=None, max_samples=max_samples, return_first=True)
    assert int(wall.check_motions(z[:1], z[-1:], **kw)[1][0]) != -1          # the direct motion is blocked
    assert wall.check_motions(z[:-1], z[1:], **kw)[1].tolist() == [-1] * 9   # every segment is free


@pytest.mark.parametrize("seed", [0, 3])
def test_host_equals_the_restated_contract(seed, max_samples):
    draws = _draws(seed)
    want, accepted, seen = restated(Wall(), [p.tolist() for p in _paths()], draws.numpy(), MAX_STEP, max_samples)
    # the draws exercise the contract: asserted on the restatement's own record
    assert seen["applied"] >= 8 and seen["lost"] >= 9 and seen["two"] >= 1 and seen["blocked"] >= 160 and seen["idle"] == 64, seen
    assert seen["batches"] == [4 * P] * T
    wall = Wall()
    res = host_shortcut_paths(wall, _paths(), max_step=MAX_STEP, slots=P, rounds=T, sampler=_fixed(draws))
    assert isinstance(res, ShortcutResult) and res.route == "host"
    assert wall.calls == T and wall.batches == {4 * P}   # ONE check_motions per round, on the fixed batch
    _same(res, want, accepted)
    # the outcome: three waypoints through the gap, less than half as long; the 2-point path as it was
    assert res.count.tolist() == [3, 3, 3, 2]
    assert all(float(v) < 0.5 * 7.997 for v in res.lengths[:3])
    assert torch.allclose(res.lengths_before[:3], torch.full((3,), 7.997), atol=1e-3)
    z = torch.tensor(ZIGZAG, dtype=torch.float32)
    for r in range(4):
        assert torch.equal(res.paths[r][0], z[0]) and torch.equal(res.paths[r][-1], z[-1])
    assert torch.equal(res.paths[3], torch.stack([z[0], z[-1]])) and int(res.accepted[3]) == 0
    # shortcut_paths routes CPU tensors to the same composition
    again = shortcut_paths(Wall(), _paths(), max_step=MAX_STEP, slots=P, rounds=T, sampler=_fixed(draws))
    assert again.route == "host"
    _same(again, want, accepted)


def test_nan_one_and_negative_draws_idle_a_slot(max_samples):
    draws = _draws(1)
    bad = draws.clone()
    bad[:, 0, 0, 0] = float("nan")
    bad[:, 0, 1, 1] = 1.0
    bad[:, 1, 2, 0] = -0.25
    bad[:, 1, 3, 1] = float("nan")
    bad[:, 2] = torch.tensor([1.0, -1e-9])
    want, accepted, seen = restated(Wall(), [p.tolist() for p in _paths()], bad.numpy(), MAX_STEP, max_samples)
    assert seen["idle"] >= 64 + 4 * T and accepted[2] == 0 and len(want[2]) == 10
    res = host_shortcut_paths(Wall(), _paths(), max_step=MAX_STEP, slots=P, rounds=T, sampler=_fixed(bad))
    _same(res, want, accepted)


def test_chunking_leaves_equal_state():
    draws = _draws(2)
    a = host_shortcut_paths(Wall(), _paths(), max_step=MAX_STEP, slots=P, rounds=T, rounds_per_call=1, sampler=_fixed(draws))
    b = host_shortcut_paths(Wall(), _paths(), max_step=MAX_STEP, slots=P, rounds=T, rounds_per_call=16, sampler=_fixed(draws))
    assert torch.equal(a.count, b.count) and torch.equal(a.accepted, b.accepted)
    for r, n in enumerate(a.count.tolist()):
        assert torch.equal(a.path[r, :n], b.path[r, :n])
    # the default sampler's stream does not depend on the chunking either
    c = host_shortcut_paths(Wall(), _paths(), max_step=MAX_STEP, slots=P, rounds=T, rounds_per_call=1, seed=5)
    d = host_shortcut_paths(Wall(), _paths(), max_step=MAX_STEP, slots=P, rounds=T, rounds_per_call=5, seed=5)
    assert torch.equal(c.count, d.count) and torch.equal(c.accepted, d.accepted)
    for r, n in enumerate(c.count.tolist()):
        assert torch.equal(c.path[r, :n], d.path[r, :n])


def test_subdivide_inserts_the_max_step_rule_points():
    step = 0.3
    z = np.array(ZIGZAG, F)
    short = torch.tensor([[0.5, 0.5], [0.6, 0.5], [0.6, 0.2]], dtype=torch.float32)   # no segment longer than the step
    res = host_shortcut_paths(Wall(), [torch.from_numpy(z), short, None], max_step=MAX_STEP, slots=P, rounds=0, subdivide=step)
    want = []
    for e in range(len(z) - 1):
        L = float(np.linalg.norm(z[e + 1].astype(np.float64) - z[e]))
        n = int(np.ceil(L / step)) + 1                      # the rule's samples: k = 0 .. n - 2 on the stride, then the target
        ks = list(range(n - 1))
        pts = listed_points32(z[:-1], z[1:], 0, [e] * len(ks), ks, max_step=step)
        assert pts[0].tobytes() == z[e].tobytes()
        want.extend(pts)
    want.append(z[-1])
    want = np.array(want, F)
    assert len(want) > len(z)
    assert int(res.count[0]) == len(want) and res.path[0, :len(want)].numpy().tobytes() == want.tobytes()
    assert res.path[0, 0].numpy().tobytes() == z[0].tobytes() and res.path[0, len(want) - 1].numpy().tobytes() == z[-1].tobytes()
    assert int(res.count[1]) == 3 and torch.equal(res.path[1, :3], short)
    assert int(res.count[2]) == 0 and res.paths[2] is None
    assert abs(float(res.lengths_before[0]) - 7.997) < 1e-3   # the inserted points lie on the segments
    # every inserted point is a waypoint a shortcut can land on: the run still ends through the gap
    done = host_shortcut_paths(Wall(), [torch.from_numpy(z)], max_step=MAX_STEP, slots=P, rounds=64, subdivide=step, seed=0)
    assert float(done.lengths[0]) < 0.5 * 7.997 and int(done.count[0]) < len(want)


def test_a_tensor_with_counts_is_the_same_input():
    draws = _draws(0)
    path = torch.zeros((4, 12, 2))
    counts = torch.tensor([10, 10, 10, 2])
    for r, p in enumerate(_paths()):
        path[r, :len(p)] = p
    a = host_shortcut_paths(Wall(), path, counts, max_step=MAX_STEP, slots=P, rounds=T, sampler=_fixed(draws))
    b = host_shortcut_paths(Wall(), _paths(), max_step=MAX_STEP, slots=P, rounds=T, sampler=_fixed(draws))
    assert a.path.shape == (4, 10, 2)
    assert torch.equal(a.count, b.count) and torch.equal(a.accepted, b.accepted)
    for r, n in enumerate(a.count.tolist()):
        assert torch.equal(a.path[r, :n], b.path[r, :n])
    assert torch.equal(path[0, :10], torch.tensor(ZIGZAG))   # the caller's tensor is not written


@pytest.mark.parametrize("kw", [dict(max_step=0.0), dict(max_step=float("nan")), dict(slots=0), dict(slots=17), dict(rounds=-1),
                                dict(subdivide=0.0), dict(max_samples=0), dict(counts=torch.tensor([10, 10, 10, 2])),
                                dict(sampler=lambda T, R, P: torch.zeros((T, R, P, 3)))])
def test_bad_arguments_raise(kw):
    args = dict(max_step=MAX_STEP, slots=P, rounds=4)
    args.update(kw)
    counts = args.pop("counts", None)
    with pytest.raises(ValueError):
        host_shortcut_paths(Wall(), _paths(), counts, **args)


def test_bad_paths_raise():
    with pytest.raises(ValueError):
        host_shortcut_paths(Wall(), torch.zeros((2, 5, 2)), max_step=MAX_STEP)                         # a tensor without counts
    with pytest.raises(ValueError):
        host_shortcut_paths(Wall(), torch.zeros((2, 5, 2)), torch.tensor([6, 0]), max_step=MAX_STEP)   # a count above W
    with pytest.raises(ValueError):
        host_shortcut_paths(Wall(), [torch.zeros((3, 2)), torch.zeros((3, 3))], max_step=MAX_STEP)     # two dofs
    with pytest.raises(ValueError):
        host_shortcut_paths(Wall(), [None, None], max_step=MAX_STEP)                                   # no dof to be had
