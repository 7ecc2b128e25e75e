"""Batched path resampling: R piecewise-straight paths of uneven length brought to one waypoint count, equally spaced in arc
length under the motion calls' metric - the step between the planners (`rrt.rrt_connect(...).path_tensor()`,
`Roadmap.query_batch`, `shortcut.shortcut_paths`: one [R, W, dof] tensor with a count per path) and the trajectory optimisers
(`traj.DenseAdamRun`, `traj.optimize_paths`: rows of one fixed length).

`resample_paths` runs the fused call (dcx_path_resample: one launch, a block per path, nothing read back) for paths on the GPU
and `host_resample_paths` for paths on the CPU.  `host_resample_paths` is the same contract (include/dcx.h, "batched path
resampling") in torch ops, one rounded fp32 operation at a time and the arc length added in the contract's fixed association:
the referee of the fused call (equal path, count and lengths, bit for bit) and the baseline it is measured against.
"""
import torch

from . import _ops
from .rrt import _div, _f32
from .shortcut import MAX_WAYPOINTS, _arc_length, _arc_points, _path_rows, _path_tensor

__all__ = ["resample_paths", "host_resample_paths", "ResampleResult"]


class ResampleResult:
    """path [R, T, dof]: row r holds the T waypoints of path r where count[r] == T (a row with count 0 is zeros);  count [R]
    int32: T, or 0 for a path with fewer than two waypoints or a length that is NaN or infinite;  lengths [R]: the paths'
    lengths under the motion calls' metric (nan with fewer than two waypoints);  route: "fused" or "host"."""

    def __init__(self, route, path, count, lengths):
        self.route, self.path, self.count, self.lengths = route, path, count, lengths


def _batch(paths, counts, n_waypoints, wrap, transform):
    """(path [R, W, dof] float32, count [R] int32, T, mask) on the paths' device, or the ValueError of the mistake"""
    T = int(n_waypoints)
    if T < 2:
        raise ValueError(f"resample_paths: n_waypoints must be >= 2, got {n_waypoints}")
    if T > MAX_WAYPOINTS:
        raise ValueError(f"resample_paths: n_waypoints must be <= {MAX_WAYPOINTS}, got {n_waypoints}")
    first = paths if torch.is_tensor(paths) else next((p for p in paths if p is not None), None)
    dev = torch.as_tensor(first).device if first is not None else torch.device("cpu")
    if torch.is_tensor(paths):   # as it stands: no walk over the paths
        path, count = _path_tensor("resample_paths", paths, counts, dev)
        dof = int(path.shape[2])
        if dof < 1:
            raise ValueError("resample_paths: dof must be >= 1")
        if path.shape[1] < 1:
            path = torch.zeros((len(path), 1, dof), dtype=torch.float32, device=dev)
        path, count = path.contiguous(), count.to(torch.int32).contiguous()
    else:
        rows, dof = _path_rows("resample_paths", paths, counts, dev)
        W = max([1] + [len(p) for p in rows if p is not None])
        path = torch.zeros((len(rows), W, dof), dtype=torch.float32, device=dev)
        count = torch.tensor([0 if p is None else len(p) for p in rows], dtype=torch.int32).to(dev)
        for r, p in enumerate(rows):
            if p is not None and len(p):
                path[r, :len(p)] = p
    if path.shape[1] > MAX_WAYPOINTS:
        raise ValueError(f"resample_paths: a path has {path.shape[1]} waypoints, more than {MAX_WAYPOINTS}")
    return path, count, T, _ops.wrap_mask(wrap, dof, transform)


def _host(path, count, T, mask):
    """the contract on [R, W, dof] / [R]: (out [R, T, dof], out_count [R] int32, length [R])"""
    R, W, dof = path.shape
    dev = path.device
    out = torch.zeros((R, T, dof), dtype=torch.float32, device=dev)
    if R == 0:
        return out, torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.float32, device=dev)
    n = count.to(torch.int64).clamp(max=W)                                         # [R]
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    # the arc length at the waypoints in the fixed association (shortcut.py's _arc_length: the partial shortcut's referee shares it)
    arc = _arc_length(path, n, mask)
    L = arc[3].gather(1, (n - 1).clamp(min=0)[:, None])[:, 0]

    has = n >= 2
    ok = has & (L < float("inf"))
    length = torch.where(has & ~torch.isnan(L), L, torch.full_like(L, float("nan")))   # (every NaN the one quiet NaN)
    out_count = torch.where(ok, torch.full_like(n, T), torch.zeros_like(n)).to(torch.int32)

    # the output waypoints: the largest e in 0 .. n - 2 with c_e <= s, then the interpolation
    step = _div(torch.where(ok, L, zero), _f32(float(T - 1), dev))
    s = torch.arange(T, device=dev).to(torch.float32)[None, :] * step[:, None]     # [R, T]
    rows = _arc_points(path, n, arc, s, ok, mask)[1]
    rows[:, 0] = path[:, 0]
    rows[:, T - 1] = path.gather(1, (n - 1).clamp(min=0)[:, None, None].expand(R, 1, dof))[:, 0]
    out = torch.where(ok[:, None, None], rows, out)
    return out, out_count, length


def host_resample_paths(paths, counts=None, *, n_waypoints, wrap=None, transform=None):
    """resample_paths' contract in torch ops, on the device of the paths: a ResampleResult with route "host"."""
    path, count, T, mask = _batch(paths, counts, n_waypoints, wrap, transform)
    return ResampleResult("host", *_host(path, count, T, mask))


def resample_paths(paths, counts=None, *, n_waypoints, wrap=None, transform=None):
    """R piecewise-straight paths resampled to n_waypoints waypoints each, equally spaced in arc length: a ResampleResult.
    paths: a list of [W_r, dof] tensors or None, or a [R, W, dof] tensor with counts [R] (what shortcut_paths takes and what it,
    RRTResult.path_tensor() and Roadmap.query_batch return);  wrap (as check_motions: None, True, a bitmask, one bool per
    coordinate): the circular coordinates, measured and walked along their shortest arc (True: the mask of the robot whose fkine
    is `transform`).  The endpoints keep their bits; a path with fewer than two waypoints, or with a NaN or infinite length,
    gets count 0.  Paths on the GPU take the fused call (result.route == "fused": one launch, nothing read back), paths on the
    CPU host_resample_paths ("host")."""
    path, count, T, mask = _batch(paths, counts, n_waypoints, wrap, transform)
    if path.device.type != "cuda":
        return ResampleResult("host", *_host(path, count, T, mask))
    return ResampleResult("fused", *_ops.path_resample(path, count, T, mask))
