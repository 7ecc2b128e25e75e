"""CPU: resample.host_resample_paths - the referee of dcx_path_resample - against the contract by hand and against the float64
polyline: the exact hand cases, the issue's error bound on random paths of every shape the contract distinguishes, the
endpoints' bits, paths without a result, unread rows, zero-length segments, the seam of a circular coordinate, and the two input
forms."""
import math

import pytest
import torch

from resample_helpers import DOFS, MIXED, NS, TS, batch, bits, worst_ratio

NAN = float("nan")


def _host(*a, **k):
    from diffco_amd.resample import host_resample_paths
    res = host_resample_paths(*a, **k)
    assert res.route == "host" and res.count.dtype == torch.int32 and res.path.dtype == res.lengths.dtype == torch.float32
    return res


def test_hand_case_is_exact():
    """five waypoints at x = 0 .. 4, T = 9: L = 4, step = 0.5, every s, a and f exact"""
    p = torch.zeros(5, 2)
    p[:, 0] = torch.arange(5.0)
    p[:, 1] = 0.25
    res = _host([p], n_waypoints=9)
    assert res.count.tolist() == [9] and res.lengths.tolist() == [4.0]
    assert res.path[0, :, 0].tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0]
    assert res.path[0, :, 1].tolist() == [0.25] * 9


@pytest.mark.parametrize("dof", DOFS)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "mixed-mask"])
def test_within_the_bound_of_the_float64_polyline(dof, T, masked):
    """|out[r, t] - the float64 point at arc length t L64 / (T - 1)| <= (n + 8) 2^-23 L64 + 2^-22 max|coord| sqrt(dof): n sequential
    fp32 adds plus the product, quotient and interpolation roundings.  Masked coordinates are compared on the circle.
    Measured on these batches: at most 0.1 of the bound (the test prints each case's worst)."""
    mask = MIXED[dof] if masked else 0
    path, count, rows = batch(dof, mask)
    res = _host(path, count, n_waypoints=T, wrap=mask)
    assert res.count.tolist() == [T] * len(NS)
    worst = 0.0
    for r, p in enumerate(rows):
        ratio, L = worst_ratio(res.path[r], p, T, mask)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (NS[r], T, dof, ratio)
        assert abs(float(res.lengths[r]) - L) <= (len(p) + 8) * 2.0 ** -23 * L
        assert torch.equal(bits(res.path[r, 0]), bits(p[0])) and torch.equal(bits(res.path[r, -1]), bits(p[-1]))
        if mask:
            on = torch.tensor([bool((mask >> j) & 1) for j in range(dof)])
            ang = res.path[r][:, on]
            pi32 = torch.tensor(math.pi, dtype=torch.float32)   # (wrap2pi's range in float32: [-pi32, pi32))
            assert bool((ang >= -pi32).all()) and bool((ang < pi32).all())
    print(f"dof {dof} T {T} mask {mask:#x}: worst distance / bound = {worst:.3f}")


def test_endpoints_keep_their_bits():
    p = torch.tensor([[-0.0, 1e-40, 3.0], [1.0, 2.0, 3.0], [0.1, -0.0, 1e18]])
    res = _host([p], n_waypoints=5)
    assert res.count.tolist() == [5]
    assert torch.equal(bits(res.path[0, 0]), bits(p[0])) and torch.equal(bits(res.path[0, 4]), bits(p[2]))
    two = _host([p[:2]], n_waypoints=2)
    assert torch.equal(bits(two.path[0]), bits(p[:2]))


def test_paths_without_a_result():
    line = torch.tensor([[0.0, 0.0], [3.0, 4.0]])
    bad = line.clone()
    bad[1, 0] = NAN
    far = line.clone()
    far[1, 1] = float("inf")
    path = torch.zeros(6, 3, 2)
    path[2, 0] = 1.5
    path[3, :2], path[4, :2], path[5, :2] = bad, far, line
    res = _host(path, torch.tensor([0, 0, 1, 2, 2, 2]), n_waypoints=4)
    assert res.count.tolist() == [0, 0, 0, 0, 0, 4]
    got = res.lengths.tolist()
    assert all(x != x for x in got[:4]) and got[4] == float("inf") and got[5] == 5.0
    assert bits(res.lengths[:4]).tolist() == [0x7fc00000] * 4   # every NaN is the one quiet NaN
    assert bool((res.path[:5] == 0).all())                      # rows without a result are left as they were: zeros
    assert torch.allclose(res.path[5], torch.tensor([[0.0, 0.0], [1.0, 4.0 / 3.0], [2.0, 8.0 / 3.0], [3.0, 4.0]]), rtol=5e-7, atol=0)
    # a list: None and a single waypoint are paths without a result too
    res = _host([None, line[:1], line], n_waypoints=3)
    assert res.count.tolist() == [0, 0, 3] and res.path[2, 1].tolist() == [1.5, 2.0]


def test_coincident_waypoints_give_copies():
    q = torch.tensor([0.3, -1.25, 2.0])
    res = _host([q.expand(7, 3).clone()], n_waypoints=6)
    assert res.count.tolist() == [6] and res.lengths.tolist() == [0.0]
    assert torch.equal(bits(res.path[0]), bits(q.expand(6, 3)))


@pytest.mark.parametrize("masked", [False, True])
def test_rows_beyond_count_are_never_read(masked):
    mask = MIXED[7] if masked else 0
    path, count, rows = batch(7, mask)
    assert bool(torch.isnan(path[0, 2:]).all())
    want = _host(path, count, n_waypoints=65, wrap=mask)
    other = torch.where(torch.isnan(path), torch.full_like(path, 123.0), path)
    got = _host(other, count, n_waypoints=65, wrap=mask)
    assert not bool(torch.isnan(want.path).any())
    assert torch.equal(bits(want.path), bits(got.path)) and torch.equal(bits(want.lengths), bits(got.lengths))
    # a count above W is read as W (the library's reading; the Python layer refuses it)
    from diffco_amd.resample import _host as contract
    a = contract(path[:, :200].contiguous(), torch.tensor([2, 3, 32, 33, 34, 65, 200, 2049], dtype=torch.int32), 9, mask)
    b = contract(path[:, :200].contiguous(), torch.tensor([2, 3, 32, 33, 34, 65, 200, 200], dtype=torch.int32), 9, mask)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_zero_length_segments_first_last_and_inside():
    x = torch.tensor([0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0])
    res = _host([x[:, None]], n_waypoints=5)
    assert res.lengths.tolist() == [2.0] and res.path[0, :, 0].tolist() == [0.0, 0.5, 1.0, 1.5, 2.0]
    res = _host([x[:, None]], n_waypoints=3)
    assert res.path[0, :, 0].tolist() == [0.0, 1.0, 2.0]


def test_masked_edge_crosses_the_seam_the_short_way():
    p = torch.tensor([[3.0, 0.0], [-3.0, 1.0]])
    res = _host([p], n_waypoints=5, wrap=0b01)
    arc = 2 * math.pi - 6.0
    assert abs(float(res.lengths[0]) - math.hypot(arc, 1.0)) < 1e-6
    ang = res.path[0, :, 0].double()
    walked = (ang - 3.0 + math.pi) % (2 * math.pi) - math.pi   # from the start, on the circle
    assert torch.allclose(walked, torch.linspace(0, arc, 5, dtype=torch.float64), atol=1e-6)
    pi32 = float(torch.tensor(math.pi, dtype=torch.float32))   # (the circle in float32 is [-pi32, pi32): wrap2pi's range)
    assert bool((ang.abs() >= 3.0 - 1e-6).all()) and bool((ang >= -pi32).all()) and bool((ang < pi32).all())
    assert torch.allclose(res.path[0, :, 1], torch.linspace(0, 1, 5), atol=1e-6)
    # without the mask the same edge is walked the long way, through 0
    plain = _host([p], n_waypoints=5)
    assert abs(float(plain.path[0, 2, 0])) < 1e-6 and abs(float(plain.lengths[0]) - math.hypot(6.0, 1.0)) < 1e-6
    # one bool per coordinate is the same mask
    flags = _host([p], n_waypoints=5, wrap=[True, False])
    assert torch.equal(bits(flags.path), bits(res.path))


def test_list_and_tensor_input_agree():
    mask = MIXED[2]
    path, count, rows = batch(2, mask)
    a = _host(path, count, n_waypoints=64, wrap=mask)
    b = _host(list(rows), n_waypoints=64, wrap=mask)
    c = _host(torch.nan_to_num(path, nan=0.0).double(), count.to(torch.int64), n_waypoints=64, wrap=mask)
    for other in (b, c):
        assert torch.equal(bits(a.path), bits(other.path)) and torch.equal(a.count, other.count)
        assert torch.equal(bits(a.lengths), bits(other.lengths))
    from diffco_amd import resample_paths
    d = resample_paths(path, count, n_waypoints=64, wrap=mask)   # CPU tensors: the host route
    assert d.route == "host" and torch.equal(bits(a.path), bits(d.path))
