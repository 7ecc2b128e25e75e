"""The referee of dcx_knn (include/dcx.h "k-nearest neighbours"): the contract restated in numpy float32, operation by operation,
from motion_wrap_helpers' wrap2pi32 / wrapped_delta.  Shared by the CPU and GPU tests; importable without a GPU.

The contract is exact, so every comparison against it is array_equal on idx and on dist2's bits (`same`)."""
import numpy as np

from motion_wrap_helpers import F, mask_bits, wrapped_delta

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def dist2_matrix(queries, points, mask):
    """[Q, N] float32: l2 = l2 + d_j * d_j over j in order from +0, d_j the (wrapped) rounded difference point_j - query_j"""
    q, p = np.asarray(queries, F), np.asarray(points, F)
    on = mask_bits(mask, q.shape[1])
    l2 = np.zeros((len(q), len(p)), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(q.shape[1]):
            d = wrapped_delta(q[:, None, j], p[None, :, j], on[j])
            l2 = (l2 + (d * d).astype(F)).astype(F)
    return l2


def knn_ref(queries, points, k, mask=0, max_dist2=None, self_offset=None):
    """(idx int32 [Q, k], dist2 float32 [Q, k]): per row the first k admissible points in the order of the 64-bit key
    bits(dist2) << 32 | index; unfilled slots -1 / +inf.  Not admissible: a NaN dist2, one above max_dist2, point self_offset + i."""
    q, p = np.asarray(queries, F), np.asarray(points, F)
    Q, N = len(q), len(p)
    idx = np.full((Q, k), -1, np.int32)
    dist2 = np.full((Q, k), np.inf, F)
    if Q == 0 or N == 0:
        return idx, dist2
    l2 = dist2_matrix(q, p, mask)
    keys = (l2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(N, dtype=np.uint64)[None, :]
    ok = ~np.isnan(l2)
    if max_dist2 is not None:
        with np.errstate(invalid="ignore"):
            ok &= l2 <= F(max_dist2)
    if self_offset is not None:
        ok &= np.arange(N)[None, :] != (np.arange(Q)[:, None] + int(self_offset))
    assert not (np.signbit(l2) & ok).any()   # never negative or -0: the bits order like the value
    keys = np.where(ok, keys, EMPTY)
    order = np.sort(keys, axis=1)[:, :k]
    n = order.shape[1]
    found = order != EMPTY
    idx[:, :n] = np.where(found, (order & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    d = (order >> np.uint64(32)).astype(np.uint32).view(F)
    dist2[:, :n] = np.where(found, d, F(np.inf))
    return idx, dist2


def same(got, want):
    """idx equal and dist2 equal bit for bit"""
    gi, gd = (np.asarray(x.cpu() if hasattr(x, "cpu") else x) for x in got)
    wi, wd = want
    return (gi.dtype == np.int32 and gd.dtype == np.float32 and np.array_equal(gi, wi)
            and np.array_equal(gd.view(np.uint32), np.asarray(wd, F).view(np.uint32)))


def where_differs(got, want):
    gi, gd = (np.asarray(x.cpu() if hasattr(x, "cpu") else x) for x in got)
    wi, wd = want
    bad = (gi != wi) | (gd.view(np.uint32) != np.asarray(wd, F).view(np.uint32))
    at = np.argwhere(bad)[:5]
    return [(tuple(a), int(gi[tuple(a)]), int(wi[tuple(a)]), float(gd[tuple(a)]), float(wd[tuple(a)])) for a in at]


def cloud(seed, n, dof, mask=0, span=3.0):
    """n random configurations: masked coordinates over the whole circle, plain ones in [-span, span]"""
    g = np.random.default_rng(seed)
    x = g.uniform(-span, span, (n, dof))
    on = mask_bits(mask, dof)
    x[:, on] = g.uniform(-np.pi, np.pi, (n, int(on.sum())))
    return x.astype(F)
