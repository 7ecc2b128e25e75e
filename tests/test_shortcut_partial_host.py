"""host_shortcut_paths(partial=True) (diffco_amd/shortcut.py) on CPU tensors with test_rrt_host's fake 2-D checker - a wall with
a gap - against a plain list-and-loop restatement of include/dcx.h's partial shortcut contract written here, numpy float32 one
operation at a time: equal path[:count] (bits), count and accepted; the coverage of the draws asserted on the restatement's own
record; the outcome (the corner the vertex mode cannot move is cut); chunking and the argument errors.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from test_rrt_host import Wall
from test_shortcut_host import ZIGZAG, _fixed, _length

from diffco_amd.shortcut import MAX_WAYPOINTS, ShortcutResult, host_shortcut_paths, shortcut_paths

F = np.float32
CORNER = [(-.8, -.8), (0, 0), (.8, -.8)]
MAX_STEP, MAX_SAMPLES, P, T, W = 0.05, 400, 4, 16, 12
CHUNK = 32   # DCX_RESAMPLE_CHUNK
SEEDS = [0, 3]
EVENTS = ("applied", "two", "lost", "blocked", "idle_draw", "idle_same", "grew", "capacity")


def _paths():
    z = torch.tensor(ZIGZAG, dtype=torch.float32)
    return [torch.tensor(CORNER, dtype=torch.float32), z.clone(), z.clone(), torch.stack([z[0], z[-1]])]


def _draws(seed):
    u = np.random.default_rng(seed).random((T, 4, P, 2), dtype=F)
    u[1, 0, 0, 0] = np.nan
    u[2, 3, 3, 1] = 1.0
    return torch.from_numpy(u)


# ---- the contract in lists and loops, numpy float32 one operation at a time --------------------------------------------------
def _fma(a, b, c):
    """float32 a * b + c rounded once: the exact rational, then the nearest float32 (ties to even) among its neighbours"""
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    near = F(float(x))
    cands = [near, np.nextafter(near, F(np.inf)), np.nextafter(near, F(-np.inf))]
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - x), int(np.array(v, F).view(np.uint32)) & 1))


def _arc(path):
    """(len_e, c_e) in the resampler's association: chunks of 32 added in order, the chunk totals added in order"""
    n = len(path)
    ln = []
    for e in range(n - 1):
        l2 = F(0)
        for j in range(len(path[e])):
            d = F(path[e + 1][j] - path[e][j])
            l2 = F(l2 + F(d * d))
        ln.append(F(np.sqrt(l2)))
    within, totals = [None] * n, []
    for g in range((n + CHUNK - 1) // CHUNK):
        p = F(0)
        for i in range(CHUNK):
            e = g * CHUNK + i
            if e < n:
                within[e] = p
            if e < n - 1:
                p = F(p + ln[e])
        totals.append(p)
    base, b = [], F(0)
    for t in totals:
        base.append(b)
        b = F(b + t)
    return ln, [F(base[e // CHUNK] + within[e]) for e in range(n)]


def _point(path, ln, c, s):
    n = len(path)
    e = max(k for k in range(n - 1) if c[k] <= s)
    a = F(s - c[e])
    if not a < ln[e]:
        return e, path[e + 1].copy()
    f = F(a / ln[e])
    return e, np.array([_fma(f, F(path[e + 1][j] - path[e][j]), path[e][j]) for j in range(len(path[e]))], F)


def restated(checker, paths, draws, cap):
    paths = [[np.array(w, F) for w in p] for p in paths]
    R, Pn = len(paths), draws.shape[2]
    accepted = [0] * R
    seen = dict.fromkeys(EVENTS, 0)
    seen["batches"] = []
    for t in range(len(draws)):
        picks = []
        for r in range(R):
            n = len(paths[r])
            row = [None] * Pn
            ln, c = _arc(paths[r]) if n >= 2 else ([], [F(0)])
            L = c[n - 1] if n else F(0)
            for p in range(Pn):
                if n < 3 or not (L > 0 and L < np.inf):
                    continue
                u0, u1 = F(draws[t, r, p, 0]), F(draws[t, r, p, 1])
                if not (u0 >= 0 and u0 < 1) or not (u1 >= 0 and u1 < 1):
                    seen["idle_draw"] += 1
                    continue
                s0, s1 = F(u0 * L), F(u1 * L)
                ea, xa = _point(paths[r], ln, c, min(s0, s1))
                eb, xb = _point(paths[r], ln, c, max(s0, s1))
                assert 0 <= ea <= eb <= n - 2
                if ea == eb:
                    seen["idle_same"] += 1
                    continue
                row[p] = (ea, eb, xa, xb)
            picks.append(row)
        # the fixed batch: an idle slot takes the zero-length edge on the path's first row
        qa = np.array([pk[2] if pk else paths[r][0] for r in range(R) for pk in picks[r]], F)
        qb = np.array([pk[3] if pk else paths[r][0] for r in range(R) for pk in picks[r]], F)
        seen["batches"].append(len(qa))
        first = checker.check_motions(torch.from_numpy(qa), torch.from_numpy(qb), max_step=MAX_STEP, wrap=None,
                                      max_samples=MAX_SAMPLES, return_first=True)[1].numpy().reshape(R, Pn)
        for r in range(R):
            old = paths[r]
            applied, cnt = [], len(old)
            for p in range(Pn):
                if picks[r][p] is None:
                    continue
                if first[r, p] != -1:
                    seen["blocked"] += 1
                    continue
                ea, eb, xa, xb = picks[r][p]
                if not all(eb < qa_ or qb_ < ea for qa_, qb_, _, _ in applied):
                    seen["lost"] += 1
                elif cnt + 2 - (eb - ea) > cap:
                    seen["capacity"] += 1
                else:
                    applied.append(picks[r][p])
                    cnt += 2 - (eb - ea)
                    seen["grew"] += eb == ea + 1
            seen["applied"] += len(applied)
            seen["two"] += len(applied) >= 2
            accepted[r] += len(applied)
            new, k = [], 0
            for ea, eb, xa, xb in sorted(applied, key=lambda s: s[0]):   # the applied slots in path order
                new += old[k:ea + 1] + [xa, xb]
                k = eb + 1
            paths[r] = new + old[k:]
            assert len(paths[r]) == cnt <= cap
    return paths, accepted, seen


def _same(res, paths, accepted):
    assert res.count.tolist() == [len(p) for p in paths]
    assert res.accepted.tolist() == accepted
    for r, p in enumerate(paths):
        got = res.path[r, :len(p)].numpy()
        assert got.tobytes() == np.array(p, F).reshape(len(p), 2).tobytes(), r


def _run(seed, **kw):
    args = dict(max_step=MAX_STEP, max_samples=MAX_SAMPLES, slots=P, rounds=T, partial=True, capacity=W, sampler=_fixed(_draws(seed)))
    args.update(kw)
    return host_shortcut_paths(Wall(), _paths(), **args)


@pytest.mark.parametrize("seed", SEEDS)
def test_host_equals_the_restated_contract(seed):
    draws = _draws(seed)
    want, accepted, seen = restated(Wall(), [p.tolist() for p in _paths()], draws.numpy(), W)
    # the draws exercise the contract: asserted on the restatement's own record
    print("seed", seed, seen, "counts", [len(p) for p in want], "accepted", accepted)
    for what in EVENTS:
        assert seen[what] >= 1, (what, seen)
    assert seen["batches"] == [4 * P] * T
    wall = Wall()
    res = host_shortcut_paths(wall, _paths(), max_step=MAX_STEP, max_samples=MAX_SAMPLES, slots=P, rounds=T, partial=True, capacity=W,
                              sampler=_fixed(draws))
    assert isinstance(res, ShortcutResult) and res.route == "host" and res.path.shape == (4, W, 2)
    assert wall.calls == T and wall.batches == {4 * P}   # ONE check_motions per round, on the fixed batch
    _same(res, want, accepted)
    # shortcut_paths routes CPU tensors to the same composition
    again = shortcut_paths(Wall(), _paths(), max_step=MAX_STEP, max_samples=MAX_SAMPLES, slots=P, rounds=T, partial=True, capacity=W,
                           sampler=_fixed(draws))
    assert again.route == "host"
    _same(again, want, accepted)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_corner_is_cut_where_vertex_shortcuts_cannot_move_it(seed):
    res = _run(seed)
    before = [_length(p.numpy()) for p in _paths()]
    after = [_length(res.paths[r].numpy()) for r in range(4)]
    print("seed", seed, "lengths", before, "->", after)
    assert abs(before[0] - 2.2627) < 1e-4 and after[0] < before[0] - 0.1      # the corner row is strictly shorter
    assert float(res.lengths[0]) < float(res.lengths_before[0])
    assert after[1] < before[1] and after[2] < before[2]                      # both zig-zag rows end shorter
    # the same row through the vertex mode keeps its three waypoints, bit for bit
    vertex = host_shortcut_paths(Wall(), _paths(), max_step=MAX_STEP, max_samples=MAX_SAMPLES, slots=P, rounds=T,
                                 sampler=_fixed(_draws(seed)))
    assert int(vertex.count[0]) == 3 and vertex.path[0, :3].numpy().tobytes() == np.array(CORNER, F).tobytes()
    # the two-point row is untouched, every endpoint keeps its bits
    assert int(res.count[3]) == 2 and int(res.accepted[3]) == 0
    for r, p in enumerate(_paths()):
        assert torch.equal(res.paths[r][0], p[0]) and torch.equal(res.paths[r][-1], p[-1]), r
    assert torch.equal(res.paths[3], _paths()[3])
    assert int(res.count.max()) <= W


@pytest.mark.parametrize("seed", SEEDS)
def test_every_final_segment_is_free(seed):
    """a property of this input, not of the contract (only the chord is checked): the wall is 0.2 thick against a 0.05 stride.
    It holds on the restatement alone for these seeds."""
    want, _, _ = restated(Wall(), [p.tolist() for p in _paths()], _draws(seed).numpy(), W)
    for r in range(3):
        p = torch.from_numpy(np.array(want[r], F))
        first = Wall().check_motions(p[:-1], p[1:], max_step=MAX_STEP, wrap=None, max_samples=MAX_SAMPLES, return_first=True)[1]
        assert first.tolist() == [-1] * (len(p) - 1), r


def test_chunking_leaves_equal_state():
    a, b = _run(2, rounds_per_call=1), _run(2, rounds_per_call=5)
    assert torch.equal(a.count, b.count) and torch.equal(a.accepted, b.accepted) and int(a.accepted.sum()) >= 1
    for r, n in enumerate(a.count.tolist()):
        assert torch.equal(a.path[r, :n], b.path[r, :n])


def test_capacity_defaults_to_the_longest_count_plus_the_slot_maximum():
    res = _run(0, capacity=None, rounds=2)
    assert res.path.shape == (4, 10 + 16, 2)


@pytest.mark.parametrize("capacity", [9, 0, MAX_WAYPOINTS + 1])
def test_capacity_outside_its_range_raises(capacity):
    with pytest.raises(ValueError, match="capacity"):
        _run(0, capacity=capacity)
    with pytest.raises(ValueError, match="capacity"):
        shortcut_paths(Wall(), _paths(), max_step=MAX_STEP, partial=True, capacity=capacity)


def test_capacity_without_partial_raises():
    with pytest.raises(ValueError, match="capacity"):
        _run(0, partial=False)
    with pytest.raises(ValueError, match="capacity"):
        shortcut_paths(Wall(), _paths(), max_step=MAX_STEP, capacity=W)
