"""GPU: dcx_knn against the numpy referee (knn_helpers.knn_ref), bit for bit: a table of shapes under the plan's own split and
three forced ones, ties across wave and split boundaries, NaNs, the radius' boundary, self exclusion, empty inputs, the seam of
the circle, the tie to the motion call's sample counts, graph capture and the Python route."""
import ctypes
import math

import numpy as np
import pytest
import torch

from knn_helpers import cloud, knn_ref, same, where_differs
from motion_wrap_helpers import F, fixture_model

pytestmark = pytest.mark.gpu

# the search keeps a query of up to 16 coordinates in registers and a longer one in LDS (csrc/knn_kernel.h kKnnRegDof):
# 1, 2, 7, 14 and 16 lie on the register side, 17, 23 and 64 on the other
REG_DOF = 16
DOFS, KS, NS, QS, MASKS = {1, 2, 7, 14, 23, 64}, {1, 5, 16, 64}, {1, 4, 63, 64, 65, 1000, 4097}, {1, 63, 65, 300}, {"none", "alt", "all"}
SPLITS = (0, 1, 2, 7)     # the plan's own, unsplit, two, and a count that divides neither 1000 nor 4097
#        dof  k    N    Q   mask
TABLE = [(1, 1, 1, 1, "none"), (1, 5, 4, 63, "all"), (2, 16, 63, 65, "alt"), (2, 64, 64, 300, "none"), (2, 5, 4097, 300, "all"),
         (7, 1, 65, 1, "all"), (7, 5, 1000, 300, "alt"), (7, 16, 4097, 65, "none"), (7, 64, 4097, 63, "all"), (7, 64, 1, 65, "alt"),
         (14, 64, 1000, 65, "alt"), (14, 5, 65, 63, "none"), (16, 16, 1000, 65, "all"), (17, 16, 1000, 65, "all"),
         (23, 1, 4097, 300, "none"), (23, 16, 64, 1, "alt"), (23, 64, 63, 65, "all"),
         (64, 5, 4097, 65, "all"), (64, 64, 1000, 63, "alt"), (64, 1, 4, 300, "none")]


def _mask(kind, dof):
    return {"none": 0, "all": (1 << dof) - 1, "alt": sum(1 << j for j in range(0, dof, 2))}[kind]


@pytest.fixture(scope="module")
def lib():
    from diffco_amd import _lib
    return _lib.require_gpu()


@pytest.fixture
def split(lib):
    from diffco_amd import _lib
    try:
        yield lambda n: _lib.check(lib.dcx_debug_set(b"knn_split", int(n)))
    finally:
        lib.dcx_debug_set(b"knn_split", 0)


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")


def _raw(lib, q, p, k, mask=0, max_dist2=math.inf, self_offset=-1, fill=True):
    """dcx_knn itself on device copies of q and p: (idx, dist2) device tensors (pre-filled with a value the call never writes)"""
    from diffco_amd import _lib
    q, p = _t(q), _t(p)
    Q, N, dof = len(q), len(p), q.shape[1]
    idx = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    d2 = torch.full((Q, k), -7.0, dtype=torch.float32, device="cuda")
    nbytes = int(lib.dcx_knn_work_bytes(Q, N, dof, k))
    assert nbytes > 0
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    opt = _lib.KnnOpts(k, 0, mask, max_dist2, 0, self_offset, (ctypes.c_int64 * 2)(0, 0))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else 0)   # noqa: E731
    _lib.check(lib.dcx_knn(0, ptr(q), Q, ptr(p), N, dof, ctypes.byref(opt), ptr(idx), ptr(d2), ptr(work), nbytes,
                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return idx, d2


def _all_splits(lib, split, q, p, k, want, **kw):
    for n in SPLITS:
        split(n)
        got = _raw(lib, q, p, k, **kw)
        assert same(got, want), (n, where_differs(got, want))


def test_the_table_covers_every_value_the_contract_names():
    have = [set(col) for col in zip(*TABLE)]
    for name, want, got in zip(("dof", "k", "N", "Q", "mask"), (DOFS, KS, NS, QS, MASKS), have):
        assert want <= got, f"the shape table lost {name} in {sorted(want - got)}"
    assert any(r[0] <= REG_DOF for r in TABLE) and any(r[0] > REG_DOF for r in TABLE), "no dof on one side of the register / LDS boundary"
    assert {REG_DOF, REG_DOF + 1} <= have[0], "the boundary's own two widths are gone"
    assert 4 in NS and any(r[2] < r[1] for r in TABLE), "no row with fewer points than k"
    assert 1000 % 7 and 4097 % 7 and {1000, 4097} <= have[2] and set(SPLITS) == {0, 1, 2, 7}, "no split count that divides no large N"


@pytest.mark.parametrize("dof,k,N,Q,kind", TABLE)
def test_shape_table_is_exact_under_every_split(lib, split, dof, k, N, Q, kind):
    mask = _mask(kind, dof)
    p = cloud(100 + dof + N, N, dof, mask)
    q = cloud(200 + dof + Q, Q, dof, mask)
    want = knn_ref(q, p, k, mask)
    _all_splits(lib, split, q, p, k, want, mask=mask)


def _boundaries(N, n_splits):
    """the first point of every wave's and block's share under n_splits splits (csrc/knn_kernels.hip: ceil(N / splits) per block,
    a quarter of that, rounded up, per wave)"""
    per = -(-N // n_splits)
    out = set()
    for s in range(n_splits):
        lo, hi = min(N, s * per), min(N, s * per + per)
        wper = -(-(hi - lo) // 4)
        out |= {min(hi, lo + w * wper) for w in range(4)}
    return sorted(b for b in out if 0 < b < N)


@pytest.mark.parametrize("dof,kind", [(7, "none"), (7, "all"), (23, "alt")])
def test_ties_come_in_index_order_across_waves_and_splits(lib, split, dof, kind):
    N, k = 1000, 16
    mask = _mask(kind, dof)
    p = cloud(7, N, dof, mask)
    g = np.random.default_rng(8)
    dup = g.choice(N, N // 5, replace=False)
    p[dup] = p[g.integers(0, N, len(dup))]
    edge = sorted({b for n in (1, 2, 7) for b in _boundaries(N, n)})
    assert len(edge) >= 4 + 8 + 20
    for b in edge:                       # the same point on both sides of every boundary ...
        p[b] = p[b - 1]
    q = np.concatenate([p[[b for b in edge]], cloud(9, 30, dof, mask)])   # ... and asked for: the pair ties at distance 0
    want = knn_ref(q, p, k, mask)
    ties = (want[1][:, 1:] == want[1][:, :-1]) & (want[0][:, 1:] >= 0)
    assert ties.sum() >= len(edge) and (want[0][:, 1:][ties] > want[0][:, :-1][ties]).all()
    for i, b in enumerate(edge):
        assert want[0][i, 0] <= b - 1 and want[1][i, 0] == 0.0
    _all_splits(lib, split, q, p, k, want, mask=mask)


def test_nan_points_and_nan_queries(lib, split):
    dof, N, k = 7, 500, 16
    p = cloud(12, N, dof)
    p[::9, 3] = np.nan
    p[5] = np.nan
    q = cloud(13, 70, dof)
    q[4, 0] = np.nan
    q[66] = np.nan
    for mask in (0, 0b1111111):
        want = knn_ref(q, p, k, mask)
        assert (want[0][[4, 66]] == -1).all() and np.isposinf(want[1][[4, 66]]).all()
        assert not np.isin(want[0], np.arange(0, N, 9)).any() and (want[0][0] >= 0).all()
        _all_splits(lib, split, q, p, k, want, mask=mask)
    # nothing but NaN points: every slot unfilled
    _all_splits(lib, split, q, np.full((40, dof), np.nan, F), 5, knn_ref(q, np.full((40, dof), np.nan, F), 5))


@pytest.mark.parametrize("mask", [0, 0b1111111])
def test_the_radius_admits_its_own_boundary(lib, split, mask):
    dof, N, k = 7, 1000, 16
    p, q = cloud(14, N, dof, mask), cloud(15, 65, dof, mask)
    free = knn_ref(q, p, k, mask)
    r2 = float(free[1][3, 7])                        # one of the referee's own values: row 3 keeps exactly eight
    want = knn_ref(q, p, k, mask, max_dist2=r2)
    assert want[0][3, 7] == free[0][3, 7] and want[0][3, 8] == -1 and (want[0] == -1).any() and (want[0][:, 0] >= 0).any()
    _all_splits(lib, split, q, p, k, want, mask=mask, max_dist2=r2)
    _all_splits(lib, split, q, p, k, knn_ref(q, p, k, mask, max_dist2=0.0), mask=mask, max_dist2=0.0)


@pytest.mark.parametrize("mask", [0, 0b101])
def test_self_exclusion(lib, split, mask):
    dof, N, k = 3, 700, 5
    p = cloud(16, N, dof, mask)
    p[100] = p[101]                                  # a duplicate of a query is a neighbour at distance 0; the query itself is not
    want = knn_ref(p, p, k, mask, self_offset=0)
    assert not (want[0] == np.arange(N)[:, None]).any() and want[0][100, 0] == 101 and want[0][101, 0] == 100
    _all_splits(lib, split, p, p, k, want, mask=mask, self_offset=0)
    want = knn_ref(p[90:390], p, k, mask, self_offset=90)
    assert not (want[0] == np.arange(90, 390)[:, None]).any()
    _all_splits(lib, split, p[90:390], p, k, want, mask=mask, self_offset=90)
    # an offset whose points do not exist excludes nothing
    _all_splits(lib, split, p[:70], p, k, knn_ref(p[:70], p, k, mask), mask=mask, self_offset=N)


def test_no_points_and_no_queries(lib, split):
    q = cloud(17, 65, 7)
    want = knn_ref(q, q[:0], 5)
    assert (want[0] == -1).all()
    _all_splits(lib, split, q, q[:0], 5, want)
    split(0)
    idx, d2 = _raw(lib, q[:0], q, 5)
    assert idx.shape == (0, 5) and d2.shape == (0, 5)


def test_points_at_the_seam_of_the_circle(lib, split):
    pi = F(np.pi)
    below, above = np.nextafter(pi, F(0)), np.nextafter(pi, F(4))
    seam = np.array([pi, -pi, below, -below, above, -above, 3.0, -3.0, 0.0, 2 * pi, -2 * pi], F)
    p = np.stack([np.repeat(seam, len(seam)), np.tile(seam, len(seam))], axis=1)
    q = np.concatenate([p, cloud(18, 30, 2, 0b11)])
    for mask in (0b11, 0b01, 0):
        want = knn_ref(q, p, 16, mask)
        _all_splits(lib, split, q, p, 16, want, mask=mask)
    masked, plain = knn_ref(p[6 * 11 + 8:][:1], p, 40, 0b11), knn_ref(p[6 * 11 + 8:][:1], p, 40, 0)   # the query (3, 0)
    far = 7 * 11 + 8                                                                                 # the point (-3, 0)
    assert far in masked[0][0] and masked[1][0][list(masked[0][0]).index(far)] < 0.1
    assert far not in plain[0][0][:20]


@pytest.mark.parametrize("name,mask", [("cfg1_planar2_rq", 0b11), ("cfg1_planar2_rq", 0), ("cfg2_baxter_rq", 0b0100101), ("cfg2_baxter_rq", 0)])
def test_dist2_is_the_length_the_motion_call_walks(lib, name, mask):
    """the sample counts dcx_check_motions_ex reports for (query, neighbour) edges are ceil(sqrt(dist2) * (1 / max_step)) + 1 in
    float32, as motion_prep.hip forms them from its own l2: dist2 holds those bits"""
    from diffco_amd import _ops
    d, desc, kern, sup, W = fixture_model(name)
    m = _ops.ScoreModel(desc, kern[0], kern[1], kern[2], _t(sup), _t(W))
    pts = np.asarray(d["q"][:400], F)
    assert len(pts) >= 100
    idx, d2 = _raw(lib, pts[:60], pts, 6, mask=mask, self_offset=0)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    assert same((idx, d2), knn_ref(pts[:60], pts, 6, mask, self_offset=0))
    qa, qb, l2 = np.repeat(pts[:60], 6, axis=0)[:300], pts[idx.reshape(-1)[:300]], d2.reshape(-1)[:300]
    max_step = F(np.median(np.sqrt(l2)) / 7.3)
    want = np.ceil((np.sqrt(l2).astype(F) * (F(1) / max_step)).astype(F)).astype(np.int64) + 1
    _, n = m.check_motions(_t(qa), _t(qb), max_step=float(max_step), max_samples=int(want.max()) + 1, wrap=mask)
    assert np.array_equal(n.cpu().numpy().astype(np.int64), want)
    assert len(set(want.tolist())) > 5


def test_one_call_captured_and_replayed(lib):
    from diffco_amd import _ops
    for Q, N, dof, k, mask in ((1, 5000, 7, 1, 0), (300, 1000, 7, 16, 0b1111111)):    # a split launch with its merge, and an unsplit one
        q, p = _t(cloud(19, Q, dof, mask)), _t(cloud(20, N, dof, mask))
        want = knn_ref(q.cpu().numpy(), p.cpu().numpy(), k, mask)
        assert same(_ops.knn(q, p, k, wrap=mask), want)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            warm = _ops.knn(q, p, k, wrap=mask)
        torch.cuda.current_stream().wait_stream(s)
        assert same(warm, want)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):      # one linear sequence on one stream
            out = _ops.knn(q, p, k, wrap=mask)
        for _ in range(2):
            out[0].fill_(-7)
            out[1].fill_(-7.0)
            g.replay()
            torch.cuda.synchronize()
            assert same(out, want)


@pytest.mark.parametrize("Q,N,dof,k,mask", [(130, 900, 7, 8, 0b0100101), (5, 4500, 23, 3, 0)])
def test_the_python_route_equals_the_host_composition(lib, Q, N, dof, k, mask):
    from diffco_amd import _ops
    from diffco_amd.roadmap import host_knn, knn, knn_edges
    q, p = _t(cloud(21, Q, dof, mask)), _t(cloud(22, N, dof, mask))
    want = knn_ref(q.cpu().numpy(), p.cpu().numpy(), k, mask)
    flags = [bool((mask >> j) & 1) for j in range(dof)]
    for got in (_ops.knn(q, p, k, wrap=mask), _ops.knn(q.double().cpu(), p, k, wrap=flags), knn(q, p, k, wrap=mask)):
        assert got[0].is_cuda and same(got, want), where_differs(got, want)
    host = host_knn(q, p, k, wrap=mask, chunk=333)
    assert host[0].is_cuda and same(host, want), where_differs(host, want)
    r = float(np.sqrt(want[1][0, -1]))
    assert same(_ops.knn(q, p, k, wrap=mask, max_dist=r), knn_ref(q.cpu().numpy(), p.cpu().numpy(), k, mask, max_dist2=F(r) * F(r)))
    assert same(_ops.knn(p[:200], p[:200], k, wrap=mask, exclude_self=True),
                knn_ref(p[:200].cpu().numpy(), p[:200].cpu().numpy(), k, mask, self_offset=0))
    assert same(_ops.knn(p[40:90], p, k, wrap=mask, self_offset=40), knn_ref(p[40:90].cpu().numpy(), p.cpu().numpy(), k, mask, self_offset=40))
    e_gpu, e_cpu = knn_edges(p[:300], k, wrap=mask), knn_edges(p[:300].cpu(), k, wrap=mask)
    assert e_gpu.is_cuda and e_gpu.dtype == torch.int64 and torch.equal(e_gpu.cpu(), e_cpu) and len(e_cpu) >= 300 * k // 2
    with pytest.raises(ValueError, match="exclude_self"):
        _ops.knn(q, p, k, exclude_self=True)
