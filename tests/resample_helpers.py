"""What the path resampling tests share (test_resample_host.py on the CPU, test_gpu_resample.py on the GPU): the random batches
of the contract's shapes, the float64 polyline they are held to, and its error bound."""
import functools
import math

import numpy as np
import torch

# waypoints per path: below, at and above one chunk of 32 segments and its neighbours, several chunks, more than the 2048
# waypoints a block keeps in LDS;  output waypoints: the least, odd and even, more than a block's threads per coordinate
NS = (2, 3, 32, 33, 34, 65, 200, 2049)
TS = (2, 3, 64, 65, 257)
DOFS = (1, 2, 7)
MIXED = {1: 0b1, 2: 0b10, 7: 0b0101101}   # a mixed mask per dof


def random_path(g, n, dof, mask, dup=True):
    """[n, dof] float32: random waypoints (masked coordinates in [-pi, pi), steps of up to a few radians, so masked edges cross
    the seam), with repeated waypoints - the first, the last and a few inside - where there is room"""
    p = g.uniform(-3.0, 3.0, (n, dof))
    for j in range(dof):
        if (mask >> j) & 1:
            p[:, j] = g.uniform(-math.pi, math.pi, n)
    p = p.astype(np.float32)
    for j in range(dof):
        if (mask >> j) & 1:
            p[:, j] = np.clip(p[:, j], -np.float32(math.pi), np.nextafter(np.float32(math.pi), np.float32(0)))
    if dup and n >= 4:
        for k in {0, n - 2, *g.integers(0, n - 1, max(1, n // 16)).tolist()}:
            p[k + 1] = p[k]
    return torch.from_numpy(p)


@functools.lru_cache(maxsize=None)
def batch(dof, mask, ns=NS, seed=0):
    """(path [R, W, dof] with NaN rows beyond each count, count [R] int32, the paths as a list): one path per entry of ns"""
    g = np.random.default_rng(1000 * dof + seed)
    rows = [random_path(g, n, dof, mask) for n in ns]
    W = max(ns)
    path = torch.full((len(ns), W, dof), float("nan"))
    for r, p in enumerate(rows):
        path[r, :len(p)] = p
    return path, torch.tensor(ns, dtype=torch.int32), rows


def _wrap64(x):
    return (x + math.pi) % (2 * math.pi) - math.pi


def polyline64(p32, T, mask):
    """(points [T, dof], L) in float64: the point at arc length t L / (T - 1) of the polyline through p32, masked coordinates
    along their shortest arc (and left unwrapped: compare on the circle)"""
    p = p32.double().numpy()
    on = np.array([bool((mask >> j) & 1) for j in range(p.shape[1])])
    d = p[1:] - p[:-1]
    d[:, on] = _wrap64(d[:, on])
    seg = np.sqrt((d * d).sum(axis=1))
    c = np.concatenate([[0.0], np.cumsum(seg)])
    L = c[-1]
    s = np.arange(T) * (L / (T - 1))
    e = np.clip(np.searchsorted(c, s, side="right") - 1, 0, len(p) - 2)
    f = np.where(seg[e] > 0, (s - c[e]) / np.where(seg[e] > 0, seg[e], 1.0), 0.0)
    return p[e] + f[:, None] * d[e], L


def bound(n, L64, p32):
    """the issue's bound on |out[t] - the float64 point|: n sequential fp32 adds of lengths plus the product, quotient and
    interpolation roundings, relative to L, and the rounding of a coordinate itself"""
    dof = p32.shape[1]
    return (n + 8) * 2.0 ** -23 * L64 + 2.0 ** -22 * float(p32.abs().max()) * math.sqrt(dof)


def worst_ratio(out, p32, T, mask):
    """max over t of (distance of out[t] to the float64 point, masked coordinates on the circle) / bound"""
    pts, L = polyline64(p32, T, mask)
    diff = out.double().numpy() - pts
    on = np.array([bool((mask >> j) & 1) for j in range(p32.shape[1])])
    diff[:, on] = _wrap64(diff[:, on])
    return float(np.sqrt((diff * diff).sum(axis=1)).max() / bound(len(p32), L, p32)), L


def bits(t):
    return t.contiguous().view(torch.int32)
