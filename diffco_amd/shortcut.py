"""Batched path shortcutting over a collision checker: R piecewise-straight paths simplified in lockstep, P attempts per path and
round - try the straight motion between two waypoints and cut out what lies between.

`shortcut_paths` runs the fused pass (dcx_path_shortcut_run: the pick and the in-place compaction in HIP, the edge checks through
the fused motion sweep, nothing read back between rounds) where the checker's own `check_motions` would take the fused route
and the paths are on the GPU, and `host_shortcut_paths` everywhere else.  `host_shortcut_paths` is the same contract
(include/dcx.h, "batched path shortcutting") composed of torch indexing and the checker's `check_motions(..., return_first=True)`
on the same fixed batch of R * P edges: the referee of the fused pass (equal path[:count], count and accepted, bit for bit, for
equal draws) and the baseline it is measured against.  It runs on CPU tensors with any checker that has such a `check_motions`.

`partial=True` is the second mode (include/dcx.h, "Partial shortcuts"; dcx_path_shortcut_partial_run): a slot draws two arc-length
positions on the path and tries the chord between the two points, inside segments, so corners are cut and not only vertices
removed.  A slot inside two neighbouring segments adds a waypoint: the state's W is then the `capacity` the paths may grow into.
Only the chord is checked; the two end pieces lie on segments the path already had (the header says what that does not promise).

`objective="clearance"` is both modes under rrt_star's clearance objective (include/dcx.h, "Path shortcuts under the clearance
objective"; dcx_path_shortcut_run_cost, dcx_path_shortcut_partial_run_cost): an edge with peak w of score - margin costs
C = L * (1 + gain * max(w + band, 0)), the state carries the segments' costs `seg`, and a slot is applied only where every piece
it inserts is free and together they cost less than the segments it removes - so the paths keep their distance where the length
modes skim the obstacle boundary, the partial mode's three pieces are all swept, and a segment that is not free (seg = +inf) is
repaired by any free chord across it.  The edge sweeps are `motion_worst`'s on either route.

The paths of `rrt.rrt_connect` come as one tensor from `RRTResult.path_tensor()`; what leaves here - one [R, W, dof] tensor with a
count per path - is what `resample.resample_paths` brings to one waypoint count and `traj.optimize_paths` optimises as R problems
at once (a single path, read back, is still a valid `init_solution` of `fused_adam_traj_optimize`).
"""
import math

import torch

from . import _ops
from .rrt import _Edges, _edge_plan, _f32, _div, _fma32, _fused_model, _length, _sample, _transform_of, _wrap
from .rrtstar import _FusedPeakEdges, _PeakEdges, _objective

__all__ = ["shortcut_paths", "host_shortcut_paths", "ShortcutResult"]

MAX_SLOTS = 16            # DCX_SHORTCUT_MAX_SLOTS
MAX_WAYPOINTS = 1 << 16   # DCX_SHORTCUT_MAX_WAYPOINTS
CHUNK = 32                # DCX_RESAMPLE_CHUNK


class ShortcutResult:
    """path [R, W, dof]: row k < count[r] is waypoint k of path r (rows beyond are unspecified);  count [R] int32;  accepted [R]
    int32: the shortcuts applied;  paths: per path a [count, dof] tensor or None where count < 2;  lengths_before, lengths [R]:
    the paths' lengths under the checks' metric before (after `subdivide`, which does not change them) and after (nan without a
    path);  route: "fused" or "host".  Under objective="clearance" (None under "length"): seg [R, W] float32: for
    k < count[r] - 1 the cost of segment k -> k + 1 (+inf where it is not free);  costs_before, costs [R] on the CPU: the paths'
    costs before and after, the serial float32 sum of seg[r, :count[r] - 1] from +0 (clearance_cost_paths' own sum)."""

    def __init__(self, route, path, count, accepted, lengths_before, lengths, seg=None, costs_before=None, costs=None):
        self.route, self.path, self.count, self.accepted = route, path, count, accepted
        self.lengths_before, self.lengths = lengths_before, lengths
        self.seg, self.costs_before, self.costs = seg, costs_before, costs
        self.paths = [path[r, :n] if n >= 2 else None for r, n in enumerate(count.tolist())]


def _lengths(path, count, mask):
    """[R] float32 on the CPU: the sum of the segments' lengths (the wrapped delta on masked coordinates), nan where count < 2"""
    R, W, _ = path.shape
    out = torch.full((R,), float("nan"), dtype=torch.float32)
    if R == 0 or W < 2:
        return out
    seg = _ops.wrapped_delta(path[:, :-1], path[:, 1:], mask).norm(dim=2)
    live = torch.arange(W - 1, device=path.device)[None, :] < (count.to(torch.int64)[:, None] - 1)
    total = torch.where(live, seg, torch.zeros_like(seg)).sum(dim=1).cpu()
    return torch.where(count.cpu() >= 2, total, out)


def _costs(seg, count):
    """[R] float32 on the CPU: seg[r, 0] + ... + seg[r, count[r] - 2] added to +0 in ascending order, one float32 sum at a time
    (a dead entry adds +0: the sum keeps its bits)"""
    seg, n = seg.cpu(), count.cpu().to(torch.int64)
    total = torch.zeros(len(seg), dtype=torch.float32)
    zero = torch.zeros((), dtype=torch.float32)
    for k in range(max(int(n.max()) - 1, 0) if len(n) else 0):
        total = total + torch.where(k < n - 1, seg[:, k], zero)
    return total


def _subdivide(p, step, mask):
    """the path p [n, dof] with, on every segment longer than `step`, the interior points of the max_step rule of stride `step`
    inserted (rrt.py's _edge_plan and _sample: the points the motion calls would sample on that segment)"""
    if len(p) < 2:
        return p
    qa, qb = p[:-1], p[1:]
    d, frac, _ = _edge_plan(qa, qb, step, 1, mask)
    n = (torch.ceil(_length(d) * _div(_f32(1.0, p.device), _f32(step, p.device))) + 1.0)
    n = torch.where(torch.isfinite(n), n, torch.full_like(n, 2.0)).to(torch.int64).tolist()
    rows = []
    for e in range(len(qa)):
        rows.append(qa[e:e + 1])
        if n[e] > 2:
            k = torch.arange(1, n[e] - 1, device=p.device)
            rows.append(_sample(qa[e][None].expand(len(k), -1), d[e][None].expand(len(k), -1), frac[e][None].expand(len(k)), k, mask))
    rows.append(qb[-1:])
    return torch.cat(rows)


def _path_tensor(who, paths, counts, dev):
    """(path [R, W, dof] float32, count [R]) on `dev` of a tensor of paths with its counts, or the ValueError of the mistake
    (one flag read back: whether every count lies in 0 .. W)"""
    if paths.dim() != 3 or counts is None:
        raise ValueError(f"{who}: a tensor of paths must be [R, W, dof] and come with `counts` [R]")
    path = paths.detach().to(device=dev, dtype=torch.float32)
    count = torch.as_tensor(counts).detach().to(device=dev).reshape(-1)
    if len(count) != len(path) or count.dtype.is_floating_point or bool(((count < 0) | (count > path.shape[1])).any()):
        raise ValueError(f"{who}: counts must be {len(path)} integers in [0, {path.shape[1]}]")
    return path, count


def _path_rows(who, paths, counts, dev):
    """(rows, dof) of the two forms a batch of paths comes in - a list of [W_r, dof] tensors or None, or a [R, W, dof] tensor
    with counts [R]: per path a float32 [n, dof] tensor on `dev`, or None.  `who` names the caller in the ValueErrors
    (shortcut_paths and resample.resample_paths take the same forms and refuse the same mistakes)."""
    if torch.is_tensor(paths):
        path, count = _path_tensor(who, paths, counts, dev)
        rows = [path[r, :n] if n else None for r, n in enumerate(count.tolist())]
        dof = int(path.shape[2])
    else:
        if counts is not None:
            raise ValueError(f"{who}: `counts` goes with a tensor of paths; a list carries its own lengths")
        rows = [None if p is None else torch.as_tensor(p).detach().to(device=dev, dtype=torch.float32) for p in paths]
        shaped = [p for p in rows if p is not None]
        if any(p.dim() != 2 for p in shaped) or len({int(p.shape[1]) for p in shaped}) > 1:
            raise ValueError(f"{who}: every path must be a [W_r, dof] tensor of the same dof")
        if not shaped:
            raise ValueError(f"{who}: a list of paths needs at least one path (its dof); pass a tensor with counts")
        dof = int(shaped[0].shape[1])
    if dof < 1:
        raise ValueError(f"{who}: dof must be >= 1")
    return rows, dof


class _Pass:
    """what both routes share: the arguments, the state, the draws, the loop"""

    def __init__(self, checker, paths, counts, dev, max_step, wrap, slots, rounds, rounds_per_call, sampler, seed, max_samples,
                 subdivide, partial=False, capacity=None, obj=None):
        self.obj = obj
        self.max_step = float(max_step)
        if not self.max_step > 0:
            raise ValueError("shortcut_paths: max_step must be > 0")
        self.P, self.rounds, self.chunk = int(slots), int(rounds), max(int(rounds_per_call), 1)
        if not 1 <= self.P <= MAX_SLOTS:
            raise ValueError(f"shortcut_paths: slots must be in [1, {MAX_SLOTS}], got {slots}")
        if self.rounds < 0:
            raise ValueError(f"shortcut_paths: rounds must be >= 0, got {rounds}")
        if subdivide is not None and not float(subdivide) > 0:
            raise ValueError("shortcut_paths: subdivide must be > 0")
        self.partial = bool(partial)
        if capacity is not None and not self.partial:
            raise ValueError("shortcut_paths: capacity goes with partial=True; vertex shortcuts never grow a path")
        self.dev = dev
        rows, self.dof = _path_rows("shortcut_paths", paths, counts, dev)
        self.mask = _ops.wrap_mask(wrap, self.dof, _transform_of(checker))
        if subdivide is not None:
            rows = [None if p is None else _subdivide(p, float(subdivide), self.mask) for p in rows]
        self.R = len(rows)
        W = max([1] + [len(p) for p in rows if p is not None])
        if W > MAX_WAYPOINTS:
            raise ValueError(f"shortcut_paths: a path has {W} waypoints, more than {MAX_WAYPOINTS}")
        if self.partial:   # W is also what a path may grow into: by default one round's worth of growth for any `slots`
            longest, W = W, min(W + MAX_SLOTS, MAX_WAYPOINTS) if capacity is None else int(capacity)
            if not longest <= W <= MAX_WAYPOINTS:
                raise ValueError(f"shortcut_paths: capacity must be in [{longest}, {MAX_WAYPOINTS}] (the longest path .. the "
                                 f"most rows of a path), got {capacity}")
        self.W = W
        self.st = dict(path=torch.zeros((self.R, W, self.dof), dtype=torch.float32, device=dev),
                       count=torch.zeros(self.R, dtype=torch.int32, device=dev),
                       accepted=torch.zeros(self.R, dtype=torch.int32, device=dev))
        for r, p in enumerate(rows):
            if p is not None and len(p):
                self.st["path"][r, :len(p)] = p
                self.st["count"][r] = len(p)
        self.lengths_before = _lengths(self.st["path"], self.st["count"], self.mask)   # (the one read-back before the loop)
        if max_samples is None:
            # a straight motion between two waypoints is never longer than the path between them
            known = self.lengths_before[torch.isfinite(self.lengths_before)]
            longest = float(known.max()) if len(known) else 0.0
            max_samples = min(_ops.MOTION_MAX_SAMPLES, int(math.ceil(longest / self.max_step)) + 2)
            if len(known) < int((self.st["count"] >= 2).sum()):   # a path of unknown length (NaN or infinite waypoints)
                max_samples = _ops.MOTION_MAX_SAMPLES
        self.max_samples = int(max_samples)
        if self.max_samples < 1:
            raise ValueError(f"shortcut_paths: max_samples must be >= 1, got {max_samples}")
        if sampler is None:
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(seed))

            def sampler(T, R, P):   # one draw per round: the stream of draws does not depend on rounds_per_call
                return torch.stack([torch.rand((R, P, 2), generator=gen, device=dev) for _ in range(T)]) \
                    if T else torch.zeros((0, R, P, 2), device=dev)
        self.sampler = sampler

    def loop(self, run_chunk):
        g = 0
        while g < self.rounds and self.R:
            T = min(self.chunk, self.rounds - g)
            draws = torch.as_tensor(self.sampler(T, self.R, self.P)).to(device=self.dev, dtype=torch.float32).contiguous()
            if tuple(draws.shape) != (T, self.R, self.P, 2):
                raise ValueError(f"shortcut_paths: the sampler returned {tuple(draws.shape)}, expected {(T, self.R, self.P, 2)}")
            run_chunk(draws)
            g += T

    def form_seg(self, peaks):
        """the state's seg [R, W] under the objective: ONE motion_worst call (`peaks`: the route's) on the consecutive waypoint
        pairs, priced by the objective, +inf where a segment is not free (w > 0, or NaN for one over max_samples)"""
        path, n = self.st["path"], self.st["count"].to(torch.int64)
        seg = torch.zeros((self.R, self.W), dtype=torch.float32, device=self.dev)
        live = torch.arange(self.W - 1, device=self.dev)[None, :] + 1 < n[:, None]   # segment k of path r: waypoints k -> k + 1
        qa, qb = path[:, :-1][live], path[:, 1:][live]
        if len(qa):
            w = peaks.worst(qa, qb, qa[:1].expand_as(qa))
            C = self.obj.price(_length(_ops.wrapped_delta(qa, qb, self.mask)), w)
            seg[:, :-1][live] = torch.where(w <= 0, C, torch.full_like(C, float("inf")))
        self.st["seg"] = seg
        self.costs_before = _costs(seg, self.st["count"])

    def result(self, route):
        st = self.st
        cost = () if self.obj is None else (st["seg"], self.costs_before, _costs(st["seg"], st["count"]))
        return ShortcutResult(route, st["path"], st["count"], st["accepted"], self.lengths_before,
                              _lengths(st["path"], st["count"], self.mask), *cost)


def _pick(count, u):
    """(i, j, live) [R, P] of include/dcx.h's pick for the draws u [R, P, 2]: float32, one rounded operation at a time"""
    n = count.to(torch.int64)[:, None]
    u0, u1 = u[..., 0], u[..., 1]
    live = (n >= 3) & (u0 >= 0) & (u0 < 1) & (u1 >= 0) & (u1 < 1)
    zero = torch.zeros_like(u0)
    u0, u1, n = torch.where(live, u0, zero), torch.where(live, u1, zero), n.clamp(min=3)
    i = torch.minimum((u0 * (n - 2).to(torch.float32)).to(torch.int64), n - 3)
    m = n - 2 - i
    j = i + 2 + torch.minimum((u1 * m.to(torch.float32)).to(torch.int64), m - 1)
    return i, j, live


def _host_round(ps, edges, u, record=None):
    """one round of the contract on the state tensors, in place"""
    st, R, P, W, dof = ps.st, ps.R, ps.P, ps.W, ps.dof
    path, dev = st["path"], ps.dev
    i, j, live = _pick(st["count"], u)
    r_all = torch.arange(R, device=dev)[:, None]
    root = path[:, :1].expand(R, P, dof)
    qa = torch.where(live[..., None], path[r_all, i], root)
    qb = torch.where(live[..., None], path[r_all, j], root)
    first = edges.first_hit(qa.reshape(-1, dof), qb.reshape(-1, dof), root.reshape(-1, dof))[0].reshape(R, P)
    free = live & (first == -1)
    applied = torch.zeros_like(free)
    for p in range(P):   # slot order: a free slot is applied iff it crosses none that was applied before it
        ok = free[:, p].clone()
        for q in range(p):
            ok &= ~applied[:, q] | (j[:, p] <= i[:, q]) | (j[:, q] <= i[:, p])
        applied[:, p] = ok
    if record is not None:
        record(live, first, free, applied)
    k = torch.arange(W, device=dev)[None, :, None]                                   # [1, W, 1]
    ia, ja, on = i[:, None, :], j[:, None, :], applied[:, None, :]                   # [R, 1, P]
    dead = (on & (ia < k) & (k < ja)).any(dim=2)                                     # [R, W]
    shift = torch.where(on & (ja <= k), ja - ia - 1, torch.zeros_like(ja)).sum(dim=2)
    keep = ~dead & (k[:, :, 0] < st["count"].to(torch.int64)[:, None])
    rr, kk = torch.nonzero(keep, as_tuple=True)
    moved = path[rr, kk]   # (a copy: read before anything is written)
    path[rr, kk - shift[rr, kk]] = moved
    st["count"].copy_(keep.sum(dim=1).to(torch.int32))
    st["accepted"] += applied.sum(dim=1).to(torch.int32)


def _arc_length(path, n, mask):
    """(nxt, d, seg, c) of include/dcx.h's arc length ("batched path resampling") for path [R, W, dof] and n [R] int64 <= W:
    the rows' successors, the segments' wrapped deltas [R, W, dof], their lengths len_e [R, W] (+0 where there is no segment)
    and the arc length at the waypoints c_e [R, W] in the fixed association - 32 steps inside every chunk, then the chunk
    totals in order.  Shared by resample.py's referee and the partial shortcut's."""
    R, W, _ = path.shape
    dev = path.device
    k = torch.arange(W, device=dev)[None, :]                                       # [1, W]
    # segment e = 0 .. W - 1 (the last one has no end: it is never live); rows at and beyond n are never read into a result
    nxt = torch.cat([path[:, 1:], path[:, -1:]], dim=1)
    d = _ops.wrapped_delta(path, nxt, mask)                                        # [R, W, dof]
    live = k < (n[:, None] - 1)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    seg = torch.where(live, _length(d), zero)                                      # [R, W]: +0 where there is no segment
    G = (W + CHUNK - 1) // CHUNK
    seg3 = torch.cat([seg, torch.zeros((R, G * CHUNK - W), dtype=torch.float32, device=dev)], dim=1).reshape(R, G, CHUNK)
    p = torch.zeros((R, G), dtype=torch.float32, device=dev)
    within = []
    for i in range(CHUNK):
        within.append(p)
        p = p + seg3[:, :, i]
    within = torch.stack(within, dim=2)                                            # [R, G, 32]: p_{g,i};  p is now t_g
    b = torch.zeros(R, dtype=torch.float32, device=dev)
    base = []
    for g in range(G):
        base.append(b)
        b = b + p[:, g]
    base = torch.stack(base, dim=1)                                                # [R, G]: b_g
    c = (base[:, :, None] + within).reshape(R, G * CHUNK)[:, :W]                   # [R, W]
    return nxt, d, seg, c


def _arc_points(path, n, arc, s, ok, mask):
    """(e [R, T], points [R, T, dof]) at the arc lengths s [R, T] of the paths with ok [R] (s must be 0 on the others), `arc`
    being _arc_length's: the largest e in 0 .. n - 2 with c_e <= s, then the contract's interpolation - the bits of
    path[r, e + 1] where !(s - c_e < len_e)"""
    nxt, d, seg, c = arc
    R, W, dof = path.shape
    T = s.shape[1]
    dev = path.device
    k = torch.arange(W, device=dev)[None, :]
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    keys = torch.where(ok[:, None] & (k <= (n[:, None] - 2)), c, torch.full_like(c, float("inf")))
    keys = torch.where(ok[:, None], keys, zero.expand_as(keys)).contiguous()
    e = (torch.searchsorted(keys, s.contiguous(), right=True) - 1).clamp(min=0)
    e = torch.minimum(e, (n[:, None] - 2).clamp(min=0))                            # [R, T]
    a = s - c.gather(1, e)
    ln = seg.gather(1, e)
    at = e[:, :, None].expand(R, T, dof)
    qa, qb, de = path.gather(1, at), nxt.gather(1, at), d.gather(1, at)
    f = _div(a, ln)[:, :, None]
    point = _fma32(f, de, qa)
    if mask:
        on = torch.tensor([bool((mask >> j) & 1) for j in range(dof)], device=dev)
        point = torch.where(on, _wrap(qa + f * de, mask), point)
    return e, torch.where((a < ln)[:, :, None], point, qb)


def _host_round_partial(ps, edges, u, record=None):
    """one round of the partial contract on the state tensors, in place"""
    st, R, P, W, dof = ps.st, ps.R, ps.P, ps.W, ps.dof
    path, dev = st["path"], ps.dev
    n = st["count"].to(torch.int64).clamp(min=0, max=W)
    arc = _arc_length(path, n, ps.mask)
    L = arc[3].gather(1, (n - 1).clamp(min=0)[:, None])[:, 0]
    has = (n >= 3) & (L > 0) & (L < float("inf"))                                    # (a NaN fails it)
    u0, u1 = u[..., 0], u[..., 1]
    drawn = has[:, None] & (u0 >= 0) & (u0 < 1) & (u1 >= 0) & (u1 < 1)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    Lz = torch.where(has, L, zero)[:, None]
    s0, s1 = torch.where(drawn, u0, zero) * Lz, torch.where(drawn, u1, zero) * Lz
    sa, sb = torch.minimum(s0, s1), torch.maximum(s0, s1)
    e, pts = _arc_points(path, n, arc, torch.cat([sa, sb], dim=1), has, ps.mask)
    ea, eb, xa, xb = e[:, :P], e[:, P:], pts[:, :P], pts[:, P:]
    live = drawn & (ea != eb)
    root = path[:, :1].expand(R, P, dof)
    qa = torch.where(live[..., None], xa, root)
    qb = torch.where(live[..., None], xb, root)
    first = edges.first_hit(qa.reshape(-1, dof), qb.reshape(-1, dof), root.reshape(-1, dof))[0].reshape(R, P)
    free = live & (first == -1)
    applied, apart, cnt = torch.zeros_like(free), torch.zeros_like(free), n.clone()
    grow = 2 - (eb - ea)
    for p in range(P):   # slot order: a free slot is applied iff it shares no segment with an applied one and the path has room
        ok = free[:, p].clone()
        for q in range(p):
            ok &= ~applied[:, q] | (eb[:, p] < ea[:, q]) | (eb[:, q] < ea[:, p])
        apart[:, p] = ok
        ok = ok & (cnt + grow[:, p] <= W)
        applied[:, p] = ok
        cnt = torch.where(ok, cnt + grow[:, p], cnt)
    if record is not None:
        record(live, first, free, applied, dict(drawn=drawn, ea=ea, eb=eb, apart=apart, has=has))
    k = torch.arange(W, device=dev)[None, :, None]                                   # [1, W, 1]
    a3, b3, on = ea[:, None, :], eb[:, None, :], applied[:, None, :]                 # [R, 1, P]
    dead = (on & (a3 < k) & (k <= b3)).any(dim=2)                                    # [R, W]
    shift = torch.where(on & (b3 < k), 2 - (b3 - a3), torch.zeros_like(b3)).sum(dim=2)
    keep = ~dead & (k[:, :, 0] < n[:, None])
    rr, kk = torch.nonzero(keep, as_tuple=True)
    moved = path[rr, kk]   # (a copy: read before anything is written; xa and xb are no views of the path either)
    ra, pa = torch.nonzero(applied, as_tuple=True)
    at = ea[ra, pa] + 1 + shift[ra, ea[ra, pa]]
    path[rr, kk + shift[rr, kk]] = moved
    path[ra, at] = xa[ra, pa]
    path[ra, at + 1] = xb[ra, pa]
    st["count"].copy_(cnt.to(torch.int32))
    st["accepted"] += applied.sum(dim=1).to(torch.int32)


def _span_cost(seg, a, b, live):
    """old [R, P]: seg[r, a] + seg[r, a + 1] + ... + seg[r, b] where `live` (a <= b there), ascending from seg[r, a], one float32
    sum at a time; +0 elsewhere (two read-backs: the columns the live spans cover)"""
    old = torch.zeros(a.shape, dtype=torch.float32, device=seg.device)
    if not bool(live.any()):
        return old
    lo, hi = int(a[live].min()), int(b[live].max())
    for k in range(lo, hi + 1):
        s = seg[:, k:k + 1].expand_as(old)
        old = torch.where(live & (a == k), s, torch.where(live & (a < k) & (k <= b), old + s, old))
    return old


def _host_round_cost(ps, peaks, u, record=None):
    """one round of the vertex contract under the objective on the state tensors, in place"""
    st, R, P, W, dof = ps.st, ps.R, ps.P, ps.W, ps.dof
    path, seg, dev = st["path"], st["seg"], ps.dev
    i, j, live = _pick(st["count"], u)
    r_all = torch.arange(R, device=dev)[:, None]
    root = path[:, :1].expand(R, P, dof)
    qa = torch.where(live[..., None], path[r_all, i], root)
    qb = torch.where(live[..., None], path[r_all, j], root)
    w = peaks.worst(qa.reshape(-1, dof), qb.reshape(-1, dof), root.reshape(-1, dof)).reshape(R, P)
    C = ps.obj.price(_length(_ops.wrapped_delta(qa, qb, ps.mask)), w)
    old = _span_cost(seg, i, j - 1, live)
    free = live & (w <= 0)
    gainful = free & (C < old)                                                       # (strict: a NaN fails it)
    applied = torch.zeros_like(free)
    for p in range(P):   # slot order: a gainful slot is applied iff it crosses none that was applied before it
        ok = gainful[:, p].clone()
        for q in range(p):
            ok &= ~applied[:, q] | (j[:, p] <= i[:, q]) | (j[:, q] <= i[:, p])
        applied[:, p] = ok
    if record is not None:
        record(live, w, free, applied, dict(i=i, j=j, cost=C, old=old, gainful=gainful))
    n = st["count"].to(torch.int64)[:, None]
    k = torch.arange(W, device=dev)[None, :, None]                                   # [1, W, 1]
    ia, ja, on = i[:, None, :], j[:, None, :], applied[:, None, :]                   # [R, 1, P]
    dead = (on & (ia < k) & (k < ja)).any(dim=2)                                     # [R, W]
    shift = torch.where(on & (ja <= k), ja - ia - 1, torch.zeros_like(ja)).sum(dim=2)
    keep = ~dead & (k[:, :, 0] < n)
    keep_seg = keep & ~(on & (ia == k)).any(dim=2) & (k[:, :, 0] < n - 1)            # both ends survive, and not an applied i
    rr, kk = torch.nonzero(keep, as_tuple=True)
    moved = path[rr, kk]   # (a copy: read before anything is written)
    rs, ks = torch.nonzero(keep_seg, as_tuple=True)
    moved_seg = seg[rs, ks]
    ra, pa = torch.nonzero(applied, as_tuple=True)
    path[rr, kk - shift[rr, kk]] = moved
    seg[rs, ks - shift[rs, ks]] = moved_seg
    seg[ra, i[ra, pa] - shift[ra, i[ra, pa]]] = C[ra, pa]
    st["count"].copy_(keep.sum(dim=1).to(torch.int32))
    st["accepted"] += applied.sum(dim=1).to(torch.int32)


def _host_round_partial_cost(ps, peaks, u, record=None):
    """one round of the partial contract under the objective on the state tensors, in place"""
    st, R, P, W, dof = ps.st, ps.R, ps.P, ps.W, ps.dof
    path, seg, dev = st["path"], st["seg"], ps.dev
    n = st["count"].to(torch.int64).clamp(min=0, max=W)
    arc = _arc_length(path, n, ps.mask)
    L = arc[3].gather(1, (n - 1).clamp(min=0)[:, None])[:, 0]
    has = (n >= 3) & (L > 0) & (L < float("inf"))                                    # (a NaN fails it)
    u0, u1 = u[..., 0], u[..., 1]
    drawn = has[:, None] & (u0 >= 0) & (u0 < 1) & (u1 >= 0) & (u1 < 1)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    Lz = torch.where(has, L, zero)[:, None]
    s0, s1 = torch.where(drawn, u0, zero) * Lz, torch.where(drawn, u1, zero) * Lz
    sa, sb = torch.minimum(s0, s1), torch.maximum(s0, s1)
    e, pts = _arc_points(path, n, arc, torch.cat([sa, sb], dim=1), has, ps.mask)
    ea, eb, xa, xb = e[:, :P], e[:, P:], pts[:, :P], pts[:, P:]
    live = drawn & (ea != eb)
    r_all = torch.arange(R, device=dev)[:, None]
    root = path[:, :1].expand(R, P, dof)
    wa, wb = path[r_all, ea], path[r_all, (eb + 1).clamp(max=W - 1)]
    # the three pieces of a slot: path[ea] -> xa, xa -> xb, xb -> path[eb + 1]
    qa = torch.where(live[..., None, None], torch.stack([wa, xa, xb], dim=2), root[:, :, None, :])   # [R, P, 3, dof]
    qb = torch.where(live[..., None, None], torch.stack([xa, xb, wb], dim=2), root[:, :, None, :])
    w = peaks.worst(qa.reshape(-1, dof), qb.reshape(-1, dof), root[:, :, None, :].expand(R, P, 3, dof).reshape(-1, dof)).reshape(R, P, 3)
    C = ps.obj.price(_length(_ops.wrapped_delta(qa, qb, ps.mask)), w)                # [R, P, 3]
    new = (C[..., 0] + C[..., 1]) + C[..., 2]
    old = _span_cost(seg, ea, eb, live)
    free = live & (w <= 0).all(dim=2)
    gainful = free & (new < old)                                                     # (strict: a NaN fails it)
    applied, apart, cnt = torch.zeros_like(free), torch.zeros_like(free), n.clone()
    grow = 2 - (eb - ea)
    for p in range(P):   # slot order: a gainful slot is applied iff it shares no segment with an applied one and the path has room
        ok = gainful[:, p].clone()
        for q in range(p):
            ok &= ~applied[:, q] | (eb[:, p] < ea[:, q]) | (eb[:, q] < ea[:, p])
        apart[:, p] = ok
        ok = ok & (cnt + grow[:, p] <= W)
        applied[:, p] = ok
        cnt = torch.where(ok, cnt + grow[:, p], cnt)
    if record is not None:
        record(live, w, free, applied, dict(drawn=drawn, ea=ea, eb=eb, apart=apart, has=has, xa=xa, xb=xb, cost=new, pieces=C, old=old,
                                               gainful=gainful))
    k = torch.arange(W, device=dev)[None, :, None]                                   # [1, W, 1]
    a3, b3, on = ea[:, None, :], eb[:, None, :], applied[:, None, :]                 # [R, 1, P]
    dead = (on & (a3 < k) & (k <= b3)).any(dim=2)                                    # [R, W]
    shift = torch.where(on & (b3 < k), 2 - (b3 - a3), torch.zeros_like(b3)).sum(dim=2)
    keep = ~dead & (k[:, :, 0] < n[:, None])
    keep_seg = ~(on & (a3 <= k) & (k <= b3)).any(dim=2) & (k[:, :, 0] < n[:, None] - 1)
    rr, kk = torch.nonzero(keep, as_tuple=True)
    moved = path[rr, kk]   # (a copy: read before anything is written; xa and xb are no views of the path either)
    rs, ks = torch.nonzero(keep_seg, as_tuple=True)
    moved_seg = seg[rs, ks]
    ra, pa = torch.nonzero(applied, as_tuple=True)
    at = ea[ra, pa] + shift[ra, ea[ra, pa]]   # the new index of waypoint ea
    path[rr, kk + shift[rr, kk]] = moved
    path[ra, at + 1] = xa[ra, pa]
    path[ra, at + 2] = xb[ra, pa]
    seg[rs, ks + shift[rs, ks]] = moved_seg
    for piece in range(3):
        seg[ra, at + piece] = C[ra, pa, piece]
    st["count"].copy_(cnt.to(torch.int32))
    st["accepted"] += applied.sum(dim=1).to(torch.int32)


def host_shortcut_paths(checker, paths, counts=None, *, max_step, wrap=None, slots=4, rounds=64, rounds_per_call=32, sampler=None,
                        seed=0, margin=0., max_samples=None, subdivide=None, partial=False, capacity=None, objective="length",
                        clearance_gain=1.0, clearance_band=None, _record=None):
    """shortcut_paths' contract as the loop a user would write from the library's other calls: per round the pick and the
    compaction as torch indexing, ONE `checker.check_motions(..., return_first=True)` call on the fixed batch of R * slots
    edges.  The state lives on the device of the paths.  `margin` is passed on to the checker's check_motions only where it is
    not 0.  partial, capacity: as shortcut_paths' (the partial contract in torch ops, one rounded fp32 operation at a time and
    the arc length in the resampler's association; `_record` then gets a fifth argument, the round's drawn, ea, eb, apart, has).
    objective, clearance_gain, clearance_band: as shortcut_paths'; under "clearance" the one call per round is
    `checker.motion_worst` (a TypeError for a checker without it) on the R * slots (partial: R * slots * 3) edges, every cost one
    rounded fp32 operation at a time, and `_record` gets (live, worst, free, applied, info): info holds the round's cost (C, or
    new = (C0 + C1) + C2), old and the gainful mask beside the picks."""
    obj = _objective("shortcut_paths", objective, clearance_gain, clearance_band)
    first = paths if torch.is_tensor(paths) else next((p for p in paths if p is not None), None)
    dev = torch.as_tensor(first).device if first is not None else torch.device("cpu")
    ps = _Pass(checker, paths, counts, dev, max_step, wrap, slots, rounds, rounds_per_call, sampler, seed, max_samples, subdivide,
               partial, capacity, obj)
    if obj is None:
        edges = _Edges(checker, ps.max_step, ps.max_samples, ps.mask, margin)
        one_round = _host_round_partial if ps.partial else _host_round
    else:
        edges = _PeakEdges("shortcut_paths", checker, ps.max_step, ps.max_samples, ps.mask, margin)
        ps.form_seg(edges)
        one_round = _host_round_partial_cost if ps.partial else _host_round_cost

    def run_chunk(draws):
        for u in draws:
            one_round(ps, edges, u, _record)

    ps.loop(run_chunk)
    return ps.result("host")


def shortcut_paths(checker, paths, counts=None, *, max_step, wrap=None, slots=4, rounds=64, rounds_per_call=32, sampler=None,
                   seed=0, margin=0., max_samples=None, subdivide=None, partial=False, capacity=None, objective="length",
                   clearance_gain=1.0, clearance_band=None):
    """Shorten R piecewise-straight paths under `checker` by random shortcuts - between waypoints, or with partial=True between
    points inside segments: a ShortcutResult.
    paths: a list of [W_r, dof] tensors or None, or a [R, W, dof] tensor with counts [R];  max_step: the stride of every edge
    check;  wrap (as check_motions: None, True, a bitmask, one bool per coordinate): the circular coordinates, walked along
    their shortest arc;  slots: attempts per path and round (1 .. 16);  rounds: how many;  sampler(T, R, P) -> [T, R, P, 2] in
    [0, 1) (default: uniform, seeded by `seed`);  margin: a sample collides where score - margin > 0, on top of the checker's
    own threshold;  max_samples: the most samples of one edge (default: from the longest path: one read-back before the loop);
    subdivide=step: first insert, on every segment longer than `step`, the max_step-rule points of stride `step`, so that vertex
    shortcuts have somewhere to land on long edges;  partial=True: a slot draws two arc-length positions on the path and tries
    the chord between the two points (it cuts corners; only the chord is checked, the end pieces lie on segments the path had);
    capacity (partial only): the rows W of a path, which a slot inside two neighbouring segments grows by one - at least the
    longest path, at most 65536, default the longest path + 16.
    objective="clearance" (with clearance_gain >= 0 and clearance_band > 0, rrt_star's names and meaning): an edge with peak w of
    score - margin costs L * (1 + clearance_gain * max(w + clearance_band, 0)), and a slot is applied only where every piece it
    inserts is free and together they cost less than the segments they replace (in the partial mode all three pieces are swept).
    The result then carries seg, costs_before and costs; a segment that is not free costs +inf, so any free chord across it
    repairs it.  clearance_gain=0 prices length alone but is not objective="length": that applies every free chord, this only
    those that shorten the path.  The checker needs `motion_worst`.
    The fused pass (result.route == "fused") runs for kernel_perceptrons.DiffCo, RBFDiffCo and ForwardKinematicsDiffCo whose
    transform fuses, on paths that are on the GPU; everything else goes through host_shortcut_paths ("host")."""
    first = paths if torch.is_tensor(paths) else next((p for p in paths if p is not None), None)
    dev0 = torch.as_tensor(first).device if first is not None else torch.device("cpu")
    got = _fused_model(checker, dev0) if dev0.type == "cuda" else None
    if got is None:
        return host_shortcut_paths(checker, paths, counts, max_step=max_step, wrap=wrap, slots=slots, rounds=rounds,
                                   rounds_per_call=rounds_per_call, sampler=sampler, seed=seed, margin=margin,
                                   max_samples=max_samples, subdivide=subdivide, partial=partial, capacity=capacity,
                                   objective=objective, clearance_gain=clearance_gain, clearance_band=clearance_band)
    obj = _objective("shortcut_paths", objective, clearance_gain, clearance_band)
    model, base = got
    if isinstance(base, (int, float)) and isinstance(margin, (int, float)):
        mg = float(base) + float(margin)
    else:   # one per class on either side
        mg = (torch.as_tensor(base, dtype=torch.float32).reshape(-1).to(model.dev)
              + torch.as_tensor(margin, dtype=torch.float32).reshape(-1).to(model.dev))
    ps = _Pass(checker, paths, counts, model.dev, max_step, wrap, slots, rounds, rounds_per_call, sampler, seed, max_samples, subdivide,
               partial, capacity, obj)
    mg_dev = model._motion_margin(mg)   # on the device once: no copy from the host per chunk
    cost_kw = {}
    if obj is not None:
        ps.form_seg(_FusedPeakEdges(model, ps.max_step, ps.max_samples, ps.mask, 0. if mg_dev is None else mg_dev))
        cost_kw = dict(cost=(obj.gain, obj.band), seg=ps.st["seg"])

    def run_chunk(draws):
        model.shortcut_run(ps.st, draws, ps.max_step, ps.max_samples, margin=0. if mg_dev is None else mg_dev, wrap=ps.mask,
                           partial=ps.partial, **cost_kw)

    ps.loop(run_chunk)
    return ps.result("fused")
