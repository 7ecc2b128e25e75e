"""Batched RRT-Connect over a collision checker: R planning problems grown in lockstep, P extensions per problem and round.

`rrt_connect` runs the fused planner (dcx_rrt_connect_run: the tree logic in HIP, the edge checks through the fused motion
sweep, one status read-back per chunk of rounds) where the checker's own `check_motions` would take the fused route, and
`host_rrt_connect` everywhere else.  `host_rrt_connect` is the same contract (include/dcx.h, "batched RRT-Connect") composed of
the calls a user has without it - `roadmap.knn` per tree, torch arithmetic for the steering and the partial advance, the
checker's `check_motions(..., return_first=True)` on the same fixed batch of R * P edges: the referee of the fused planner (equal
state, bit for bit, for equal samples) and the baseline it is measured against.  It runs on CPU tensors with any checker that
has such a `check_motions`.

The path of a solved problem is walked from `parent` on the host: start, ..., link node of tree 0, link node of tree 1, ...,
goal; it is what `fused_adam_traj_optimize` takes as `init_solution`.  `RRTResult.path_tensor` gives the same rows as one
[R, W, dof] tensor, written on the device for a state on the GPU (dcx_rrt_extract_paths): what `shortcut.shortcut_paths` takes.
"""
import math

import torch

from . import _ops
from .roadmap import knn

__all__ = ["rrt_connect", "host_rrt_connect", "RRTResult", "RUNNING", "SOLVED", "FULL", "BLOCKED"]

RUNNING, SOLVED, FULL, BLOCKED = 0, 1, 2, 3   # dcx_rrt_state's status values
_STATE = ("nodes", "parent", "count", "status", "link", "solved_round")


class RRTResult:
    """paths: per problem a [W, dof] tensor (start first, goal last) or None;  status [R] (0 still running at max_rounds, 1 solved,
    2 a tree is full, 3 an endpoint collides);  rounds [R]: the rounds a problem took (a solved one: solved_round + 1, 0 for a
    free direct motion; else the rounds that were run);  lengths [R]: the paths' lengths under the planner's metric (nan
    without a path);  route: "fused" or "host";  nodes, parent, count, link, solved_round: the raw state tensors."""

    def __init__(self, route, state, paths, rounds, lengths):
        self.route, self.paths, self.rounds, self.lengths = route, paths, rounds, lengths
        for name in _STATE:
            setattr(self, name, state[name])

    def state(self):
        return {name: getattr(self, name) for name in _STATE}

    def path_tensor(self, W=None):
        """(path [R, W, dof] float32, count [R] int32) on the state's device: the rows of `paths` as one tensor, what
        shortcut.shortcut_paths takes.  count[r] is the path's waypoints, 0 without a path, and -n where its n waypoints do
        not fit into W (that row is left as it is: zeros).  A state on the GPU goes through dcx_rrt_extract_paths (one launch,
        the parents never leave the device); W=None asks for the sizes first and reads their maximum back once.  A state on the
        CPU is walked on the host."""
        if self.nodes.device.type == "cuda":
            st = self.state()
            if W is None:
                sizes = _ops.rrt_extract_paths(st, 0)[1]
                W = int((-sizes).max()) if len(sizes) else 0
            return _ops.rrt_extract_paths(st, W)
        R, dof = len(self.status), self.nodes.shape[3]
        status, link = self.status.tolist(), self.link.tolist()
        rows = [_walk(self.nodes, self.parent, link[r], r) if status[r] == SOLVED else None for r in range(R)]
        if W is None:
            W = max([0] + [len(p) for p in rows if p is not None])
        path = torch.zeros((R, int(W), dof), dtype=torch.float32)
        count = torch.zeros(R, dtype=torch.int32)
        for r, p in enumerate(rows):
            if p is not None:
                count[r] = len(p) if len(p) <= W else -len(p)
                if len(p) <= W:
                    path[r, :len(p)] = p
        return path, count


# ---- fp32 arithmetic of the contract in torch ops, one rounded operation at a time ------------------------------------------
def _length(d):
    """|d| as the motion calls form an edge's length: the squares summed from +0 in coordinate order, then a correctly rounded
    square root (taken in float64 and rounded once more: for a square root and a quotient of float32 values that double
    rounding is exact, whatever the device's float32 sqrt / division are)"""
    l2 = torch.zeros(d.shape[:-1], dtype=torch.float32, device=d.device)
    for j in range(d.shape[-1]):
        l2 = l2 + d[..., j] * d[..., j]
    return torch.sqrt(l2.to(torch.float64)).to(torch.float32)


def _div(a, b):
    return (a.to(torch.float64) / b.to(torch.float64)).to(torch.float32)


def _f32(x, dev):
    return torch.tensor(float(x), dtype=torch.float32, device=dev)


def _wrap(pts, mask):
    from ._perceptron import _wrap_points
    return _wrap_points(pts, mask)


def _steer(near, s, rng, mask):
    """(qb, ok) of include/dcx.h's steering step for the edges near -> s ([..., dof] each)"""
    d = _ops.wrapped_delta(near, s, mask)
    L = _length(d)
    ok = L > 0
    f = _div(_f32(rng, near.device), L)
    far = _wrap(near + d * f[..., None], mask)
    return torch.where((L <= _f32(rng, near.device))[..., None], s, far), ok


def _edge_plan(qa, qb, max_step, max_samples, mask):
    """(d, frac, over) of the max_step rule as motion_prep.hip forms them: the wrapped delta, the step fraction (1 / L) *
    max_step and whether the edge needs more than max_samples samples (a NaN or infinite length does)"""
    d = _ops.wrapped_delta(qa, qb, mask)
    L = _length(d)
    one, ms = _f32(1.0, qa.device), _f32(max_step, qa.device)
    n = torch.ceil(L * _div(one, ms)) + 1.0
    return d, _div(one, L) * ms, ~(n <= float(max_samples))


def _fma32(a, b, c):
    """float32 a * b + c rounded once.  In float64 the product is exact and the sum is rounded to odd (the two-sum's error term
    says which neighbour the exact sum leans to), so the final rounding to float32 is the fused operation's."""
    a, b, c = (torch.broadcast_to(t, torch.broadcast_shapes(a.shape, b.shape, c.shape)).to(torch.float64) for t in (a, b, c))
    p = a * b
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    bits = s.clone().view(torch.int64)
    nudge = torch.isfinite(err) & (err != 0) & ((bits & 1) == 0)   # (an infinite or NaN sum stays what it is)
    away = (err > 0) == (s > 0)
    bits = torch.where(nudge, torch.where(away, bits + 1, bits - 1), bits)
    return bits.view(torch.float64).to(torch.float32)


def _sample(qa, d, frac, k, mask):
    """interior sample k of the edges as motion_kernel.h's motion_coord forms it: wrap2pi(qa + k * (d * frac)), every operation
    rounded alone, on the masked coordinates; on the others the compiled expression, whose last product and sum are one fused
    multiply-add: fma(k, d * frac, qa)"""
    kf, step = k.to(torch.float32)[..., None], d * frac[..., None]
    if not mask:
        return _fma32(kf, step, qa)
    on = torch.tensor([bool((mask >> j) & 1) for j in range(qa.shape[-1])], device=qa.device)
    return torch.where(on, _wrap(qa + kf * step, mask), _fma32(kf, step, qa))


# ---- the checker's motion check on the fixed batch -------------------------------------------------------------------------
class _Edges:
    def __init__(self, checker, max_step, max_samples, mask, margin):
        self.checker, self.max_step, self.max_samples, self.mask = checker, float(max_step), int(max_samples), int(mask)
        self.kw = {} if (isinstance(margin, (int, float)) and float(margin) == 0.0) else {"margin": margin}

    def first_hit(self, qa, qb, root):
        """(first_hit [E] int64, d, frac) of the edges qa -> qb; an edge over max_samples is answered -2 without being
        submitted (a facade raises for it): its place in the batch takes `root` -> `root`, as an idle slot's"""
        d, frac, over = _edge_plan(qa, qb, self.max_step, self.max_samples, self.mask)
        qa_s, qb_s = torch.where(over[:, None], root, qa), torch.where(over[:, None], root, qb)
        _, first = self.checker.check_motions(qa_s, qb_s, max_step=self.max_step, wrap=self.mask if self.mask else None,
                                              max_samples=self.max_samples, return_first=True, **self.kw)
        first = torch.as_tensor(first).to(device=qa.device, dtype=torch.int64).reshape(-1)
        return torch.where(over, torch.full_like(first, -2), first), d, frac


class _FusedEdges:
    """the same on a ScoreModel (the initial checks of the fused planner)"""

    def __init__(self, model, max_step, max_samples, mask, margin):
        self.model, self.max_step, self.max_samples, self.mask, self.margin = model, float(max_step), int(max_samples), int(mask), margin

    def first_hit(self, qa, qb, root):
        first, _ = self.model.check_motions(qa, qb, max_step=self.max_step, margin=self.margin, max_samples=self.max_samples,
                                            wrap=self.mask)
        return first.to(torch.int64), None, None


# ---- what both planners share: arguments, initial state, the loop, the paths -----------------------------------------------
def _limits_of(checker):
    for owner in (getattr(checker, "robot", None), getattr(getattr(checker, "transform", None), "__self__", None),
                  getattr(getattr(getattr(checker, "perceptron", None), "transform", None), "__self__", None)):
        for name in ("joint_limits", "limits"):
            lim = getattr(owner, name, None) if owner is not None else None
            if lim is not None:
                return torch.as_tensor(lim)
    return None


def _transform_of(checker):
    return getattr(checker, "transform", None) or getattr(getattr(checker, "perceptron", None), "transform", None)


class _Plan:
    def __init__(self, checker, starts, goals, dev, reach, max_step, wrap, slots, cap, max_rounds, rounds_per_call, sampler, limits,
                 seed, max_samples):
        self.starts = torch.as_tensor(starts).detach().to(device=dev, dtype=torch.float32).reshape(-1, torch.as_tensor(starts).shape[-1])
        self.goals = torch.as_tensor(goals).detach().to(device=dev, dtype=torch.float32).reshape(self.starts.shape)
        self.dev, self.R, self.dof = dev, len(self.starts), self.starts.shape[1]
        self.range, self.max_step = float(reach), float(max_step)
        if not self.range > 0 or not self.max_step > 0:
            raise ValueError("rrt_connect: range and max_step must be > 0")
        self.P, self.cap = int(slots), int(cap)
        if not 1 <= self.P <= 16:
            raise ValueError(f"rrt_connect: slots must be in [1, 16], got {slots}")
        if self.cap < 1:
            raise ValueError(f"rrt_connect: cap must be >= 1, got {cap}")
        self.max_rounds, self.chunk = int(max_rounds), max(int(rounds_per_call), 1)
        self.mask = _ops.wrap_mask(wrap, self.dof, _transform_of(checker))
        lim = limits if limits is not None else _limits_of(checker)
        self.limits = None if lim is None else torch.as_tensor(lim).detach().to(device=dev, dtype=torch.float32).reshape(self.dof, 2)
        if sampler is None:
            if self.limits is None:
                raise ValueError("rrt_connect: pass `limits` [dof, 2] or a `sampler`: the checker's robot has no joint limits")
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(seed))
            lo, span = self.limits[:, 0], self.limits[:, 1] - self.limits[:, 0]

            def sampler(T, R, P):   # one draw per round: the stream of samples does not depend on rounds_per_call
                return torch.stack([lo + span * torch.rand((R, P, self.dof), generator=gen, device=dev) for _ in range(T)]) \
                    if T else torch.zeros((0, R, P, self.dof), device=dev)
        self.sampler = sampler
        if max_samples is None:
            # the longest edge a tree can hold: the box's diagonal (a circular coordinate never runs further than pi)
            if self.limits is None:
                max_samples = _ops.MOTION_MAX_SAMPLES
            else:
                ext = (self.limits[:, 1] - self.limits[:, 0]).abs().to(torch.float64).cpu()
                on = torch.tensor([bool((self.mask >> j) & 1) for j in range(self.dof)])
                ext = torch.where(on, ext.clamp(max=math.pi), ext)
                max_samples = min(_ops.MOTION_MAX_SAMPLES, int(math.ceil(float(ext.norm()) / self.max_step)) + 2)
        self.max_samples = int(max_samples)

    def initial_state(self, edges):
        """both trees' roots, and the initial checks as ONE batch of 3 R edges: the zero-length edges on the starts and on the
        goals (one sample each: the point check under the planner's own margin) and the direct motions start -> goal"""
        R, cap, dof, dev = self.R, self.cap, self.dof, self.dev
        st = dict(nodes=torch.zeros((R, 2, cap, dof), dtype=torch.float32, device=dev),
                  parent=torch.full((R, 2, cap), -1, dtype=torch.int32, device=dev),
                  count=torch.ones((R, 2), dtype=torch.int32, device=dev),
                  status=torch.zeros(R, dtype=torch.int32, device=dev),
                  link=torch.full((R, 2), -1, dtype=torch.int32, device=dev),
                  solved_round=torch.full((R,), -1, dtype=torch.int32, device=dev))
        st["nodes"][:, 0, 0], st["nodes"][:, 1, 0] = self.starts, self.goals
        if R:
            qa, qb = torch.cat([self.starts, self.goals, self.starts]), torch.cat([self.starts, self.goals, self.goals])
            first = edges.first_hit(qa, qb, self.starts[:1].expand(3 * R, dof))[0]
            blocked = (first[:R] != -1) | (first[R:2 * R] != -1)
            direct = (first[2 * R:] == -1) & ~blocked
            st["status"][blocked] = BLOCKED
            st["status"][direct] = SOLVED
            st["link"][direct] = 0
        return st

    def loop(self, st, run_chunk):
        """chunks of rounds until no problem is running or max_rounds; one status read-back per chunk.  The rounds run."""
        g = 0
        while g < self.max_rounds and bool((st["status"] == RUNNING).any()):
            T = min(self.chunk, self.max_rounds - g)
            samples = torch.as_tensor(self.sampler(T, self.R, self.P)).to(device=self.dev, dtype=torch.float32).contiguous()
            if tuple(samples.shape) != (T, self.R, self.P, self.dof):
                raise ValueError(f"rrt_connect: the sampler returned {tuple(samples.shape)}, expected {(T, self.R, self.P, self.dof)}")
            run_chunk(samples, g)
            g += T
        return g

    def result(self, route, st, rounds_run):
        status, link, solved = st["status"].tolist(), st["link"].tolist(), st["solved_round"].tolist()
        parent, nodes = st["parent"].cpu(), st["nodes"]
        paths, rounds, lengths = [], [], []
        for r in range(self.R):
            if status[r] != SOLVED:
                paths.append(None)
                rounds.append(0 if status[r] == BLOCKED else rounds_run)
                lengths.append(float("nan"))
                continue
            p = _walk(nodes, parent, link[r], r)
            paths.append(p)
            rounds.append(solved[r] + 1)
            lengths.append(float(_ops.wrapped_delta(p[:-1], p[1:], self.mask).norm(dim=1).sum()))
        return RRTResult(route, st, paths, torch.tensor(rounds, dtype=torch.int64), torch.tensor(lengths, dtype=torch.float32))


def _walk(nodes, parent, link_r, r):
    """the path of solved problem r from `parent` (on the CPU): tree 0 from its root to the link node, tree 1 from its link node
    to its root"""
    walk = [[], []]
    for t in (0, 1):
        i = link_r[t]
        while i >= 0:
            walk[t].append(i)
            i = int(parent[r, t, i])
    i0 = torch.tensor(walk[0][::-1], dtype=torch.int64, device=nodes.device)
    i1 = torch.tensor(walk[1], dtype=torch.int64, device=nodes.device)
    return torch.cat([nodes[r, 0][i0], nodes[r, 1][i1]])


def _append(st, r_all, tree, app, pts, par, cap):
    """the commit of one phase: the slots `app` [R, P] append pts [R, P, dof] with parents par [R, P] to tree `tree` in slot
    order while count < cap.  (append index or -1 per slot [R, P], a slot did not fit [R])"""
    c0 = st["count"][:, tree].to(torch.int64)
    a64 = app.to(torch.int64)
    at = c0[:, None] + torch.cumsum(a64, dim=1) - a64
    fits = app & (at < cap)
    rr = r_all[:, None].expand_as(at)[fits]
    st["nodes"][rr, tree, at[fits]] = pts[fits]
    st["parent"][rr, tree, at[fits]] = par[fits].to(torch.int32)
    total = c0 + a64.sum(dim=1)
    st["count"][:, tree] = total.clamp(max=cap).to(torch.int32)
    return torch.where(fits, at, torch.full_like(at, -1)), total > cap


def _nearest(st, tree, queries, want, counts, mask):
    """[R, P] index of the node of tree `tree` nearest to each wanted query (roadmap.knn, k = 1), -1 elsewhere"""
    R, P = want.shape
    near = torch.full((R, P), -1, dtype=torch.int64, device=queries.device)
    rows = want.any(dim=1).tolist()
    for r in range(R):
        if rows[r]:
            idx, _ = knn(queries[r], st["nodes"][r, tree, :counts[r][tree]], 1, wrap=mask)
            near[r] = idx[:, 0].to(torch.int64)
    return torch.where(want, near, torch.full_like(near, -1))


def _host_round(pl, edges, st, s, g):
    """one round of the contract on the state tensors, in place (s [R, P, dof]: the round's samples)"""
    R, P, dof, cap, mask = pl.R, pl.P, pl.dof, pl.cap, pl.mask
    a, b = g & 1, 1 - (g & 1)
    r_all = torch.arange(R, device=pl.dev)
    running = st["status"] == RUNNING
    counts = st["count"].tolist()
    root = st["nodes"][:, 0, 0][:, None, :].expand(R, P, dof)

    def check(go, qa, qb):
        qa, qb = torch.where(go[..., None], qa, root), torch.where(go[..., None], qb, root)
        first, d, frac = edges.first_hit(qa.reshape(-1, dof), qb.reshape(-1, dof), root.reshape(-1, dof))
        return first.reshape(R, P), qa, d.reshape(R, P, dof), frac.reshape(R, P)

    # phase 1: extend tree a towards the samples
    near = _nearest(st, a, s, running[:, None].expand(R, P), counts, mask)
    nq = st["nodes"][r_all[:, None], a, near.clamp(min=0)]
    qb, ok = _steer(nq, s, pl.range, mask)
    go = (near >= 0) & ok
    first = check(go, nq, qb)[0]
    added, over1 = _append(st, r_all, a, go & (first == -1), qb, near, cap)

    # phase 2: connect tree b to the new nodes
    x = st["nodes"][r_all[:, None], a, added.clamp(min=0)]
    nb = _nearest(st, b, x, added >= 0, counts, mask)
    nbq = st["nodes"][r_all[:, None], b, nb.clamp(min=0)]
    go = nb >= 0
    first, qa, d, frac = check(go, nbq, x)
    joined = go & (first == -1)
    part = go & (first >= 2)
    _, over2 = _append(st, r_all, b, part, _sample(qa, d, frac, (first - 1).clamp(min=0), mask), nb, cap)

    solved = joined.any(dim=1)
    p0 = joined.to(torch.int64).argmax(dim=1)   # the joining slot with the lowest p
    st["link"][solved, a] = added[r_all, p0][solved].to(torch.int32)
    st["link"][solved, b] = nb[r_all, p0][solved].to(torch.int32)
    st["solved_round"][solved] = g
    st["status"][solved] = SOLVED
    st["status"][running & ~solved & (over1 | over2)] = FULL


def host_rrt_connect(checker, starts, goals, *, range, max_step, wrap=None, slots=4, cap=4096, max_rounds=1024, rounds_per_call=32,
                     sampler=None, limits=None, seed=0, margin=0., max_samples=None):
    """rrt_connect's contract as the loop a user would write from the library's other calls: per round and tree one `knn` per
    running problem, the steering in torch, ONE `checker.check_motions(..., return_first=True)` call per phase on the fixed
    batch of R * slots edges, the appends as indexed assignments.  The state lives on the device of `starts`.  `margin` is
    passed on to the checker's check_motions only where it is not 0."""
    dev = torch.as_tensor(starts).device
    pl = _Plan(checker, starts, goals, dev, range, max_step, wrap, slots, cap, max_rounds, rounds_per_call, sampler, limits, seed,
               max_samples)
    edges = _Edges(checker, pl.max_step, pl.max_samples, pl.mask, margin)
    st = pl.initial_state(edges)

    def run_chunk(samples, g0):
        for t, s in enumerate(samples):
            _host_round(pl, edges, st, s, g0 + t)

    return pl.result("host", st, pl.loop(st, run_chunk))


def _fused_model(checker, dev):
    """(ScoreModel, margin) where the checker's check_motions takes the fused route, else None"""
    fn = getattr(checker, "_rrt_model", None)
    return fn(dev) if fn is not None else None


def rrt_connect(checker, starts, goals, *, range, max_step, wrap=None, slots=4, cap=4096, max_rounds=1024, rounds_per_call=32,
                sampler=None, limits=None, seed=0, margin=0., max_samples=None):
    """Plan R motions starts[r] -> goals[r] ([R, dof] each) with batched RRT-Connect under `checker`: an RRTResult.
    range: the longest extension; max_step: the stride of every edge check; wrap (as check_motions: None, True, a bitmask, one
    bool per coordinate): the circular coordinates, measured and walked along their shortest arc; slots: extensions per problem
    and round (1 .. 16); cap: nodes per tree; sampler(T, R, P) -> [T, R, P, dof] (default: uniform in `limits` [dof, 2], taken
    from the checker's robot where it has them, seeded by `seed`); margin: a sample collides where score - margin > 0, on top
    of the checker's own threshold; max_samples: the most samples of one edge (default: from the limits' diagonal).
    The fused planner (result.route == "fused") runs for kernel_perceptrons.DiffCo, RBFDiffCo and ForwardKinematicsDiffCo whose
    transform fuses; every other checker is planned by host_rrt_connect ("host")."""
    dev0 = torch.as_tensor(starts).device
    got = _fused_model(checker, dev0 if dev0.type == "cuda" else None)
    if got is None:
        return host_rrt_connect(checker, starts, goals, range=range, max_step=max_step, wrap=wrap, slots=slots, cap=cap,
                                max_rounds=max_rounds, rounds_per_call=rounds_per_call, sampler=sampler, limits=limits, seed=seed,
                                margin=margin, max_samples=max_samples)
    model, base = got
    if isinstance(base, (int, float)) and isinstance(margin, (int, float)):
        mg = float(base) + float(margin)
    else:   # one per class on either side
        mg = (torch.as_tensor(base, dtype=torch.float32).reshape(-1).to(model.dev)
              + torch.as_tensor(margin, dtype=torch.float32).reshape(-1).to(model.dev))
    pl = _Plan(checker, starts, goals, model.dev, range, max_step, wrap, slots, cap, max_rounds, rounds_per_call, sampler, limits,
               seed, max_samples)
    st = pl.initial_state(_FusedEdges(model, pl.max_step, pl.max_samples, pl.mask, mg))
    mg_dev = model._motion_margin(mg)   # on the device once: no copy from the host per chunk

    def run_chunk(samples, g0):
        model.rrt_connect_run(st, samples, g0, pl.range, pl.max_step, pl.max_samples, pl.cap, margin=0. if mg_dev is None else mg_dev,
                              wrap=pl.mask)

    return pl.result("fused", st, pl.loop(st, run_chunk))

