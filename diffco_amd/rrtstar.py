"""Batched RRT* over a collision checker: R planning problems, one tree each, grown in lockstep with P extensions per problem
and round; every new node picks the cheapest free parent among its K nearest within a radius and then rewires those of them it
reaches more cheaply.  objective="length" (the default) optimises path length under the motion calls' metric;
objective="clearance" charges an edge its length times 1 + clearance_gain * max(w + clearance_band, 0), w the peak of score -
margin along it (include/dcx.h, "batched RRT*: clearance-weighted edge costs"): the tree then prefers motions that keep away
from the obstacle boundary, which no shortcutter can do.  `clearance_cost_paths` prices any piecewise-straight path under it.

`rrt_star` runs the fused planner (dcx_rrtstar_run: the tree logic in HIP, the three edge batches of a round through the fused
motion sweep, one status / goal read-back per chunk of rounds) where the checker's own `check_motions` would take the fused
route, and `host_rrt_star` everywhere else.  `host_rrt_star` is the same contract (include/dcx.h, "batched RRT*") composed of the
calls a user has without it - `roadmap.knn`, torch arithmetic one rounded operation at a time, the checker's
`check_motions(..., return_first=True)` on the same fixed batches of R * P, R * P * K and R * P * K edges: the referee of the
fused planner (equal state, bit for bit, for equal samples) and the baseline it is measured against.  It runs on CPU tensors
with any checker that has such a `check_motions`.

In lockstep RRT* the set of nodes does not depend on the parents: near = 0 (plain RRT with costs) grows the same nodes from the
same samples, and no node's cost with near > 0 is above its cost with near = 0.

sampling="device" / "informed" draws each round's samples where the trees live (include/dcx.h, "batched RRT*: samples drawn on
the device"; dcx_rrtstar_run_sampled), from the state as the round finds it: "informed" samples a problem that has reached its
goal inside the ellipsoid of points that can still shorten its path.  `host_device_samples` restates that draw in torch on CPU
tensors - the kernel's referee, and what host_rrt_star draws from in those modes.
"""
import builtins
import math

import torch

from . import _ops
from .roadmap import knn
from .rrt import (BLOCKED, FULL, RUNNING, _Edges, _FusedEdges, _Plan, _edge_plan, _fused_model, _length, _nearest, _steer)

__all__ = ["rrt_star", "host_rrt_star", "clearance_cost_paths", "host_device_samples", "philox4x32_10", "RRTStarResult", "RUNNING", "DIRECT", "FULL", "BLOCKED"]

DIRECT = 1   # dcx_rrtstar_state's status 1: the direct motion start -> goal is free (RUNNING, FULL, BLOCKED: as rrt.py's)
_STATE = ("nodes", "parent", "elen", "cost", "count", "status", "goal_node", "first_round")
_NO_KEY = torch.iinfo(torch.int64).max
_SAMPLING = {"host": None, "device": "uniform", "informed": "informed"}   # rrt_star's `sampling` -> the draw's mode


class RRTStarResult:
    """paths: per problem a [W, dof] tensor (start first, goal last) or None without a goal node;  costs [R]: the goal nodes'
    cost-to-come (nan without one);  first_round [R]: the round that first reached the goal (-1: none, or a free direct motion -
    under objective="clearance" also one that is penalised, which seeds the tree with status 0 and is improved on);
    status [R] (0 still running at max_rounds, 1 the direct motion is free, 2 full, 3 an endpoint collides);  rounds: the rounds
    that were run;  route: "fused" or "host";  nodes, parent, elen, cost, count, goal_node: the raw state tensors;  samples
    [rounds, R, P, dof] and sample_info [rounds, R, P] (record_samples=True, else None): what every round was given, and for the
    draws of sampling="device" / "informed" their info words (include/dcx.h: -1 not running, 0 uniform, 1 goal, 2 + t informed
    at try t, 2 + tries fallen back)."""

    def __init__(self, route, state, paths, costs, rounds, samples=None, sample_info=None):
        self.route, self.paths, self.costs, self.rounds = route, paths, costs, rounds
        self.samples, self.sample_info = samples, sample_info
        for name in _STATE:
            setattr(self, name, state[name])

    def state(self):
        return {name: getattr(self, name) for name in _STATE}

    def path_tensor(self, W=None):
        """(path [R, W, dof] float32, count [R] int32) on the state's device: the rows of `paths` as one tensor, what
        shortcut.shortcut_paths takes.  count[r] is the path's waypoints, 0 without a goal node, and -n where its n waypoints do
        not fit into W (that row is left as it is: zeros).  A state on the GPU goes through dcx_rrtstar_extract_paths (one
        launch, the parents never leave the device); W=None asks for the sizes first and reads their maximum back once.  A
        state on the CPU is walked on the host."""
        if self.nodes.device.type == "cuda":
            st = self.state()
            if W is None:
                sizes = _ops.rrtstar_extract_paths(st, 0)[1]
                W = int((-sizes).max()) if len(sizes) else 0
            return _ops.rrtstar_extract_paths(st, W)
        R, dof = len(self.status), self.nodes.shape[2]
        rows = _walk_all(self.nodes, self.parent, self.goal_node)
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


def _walk_all(nodes, parent, goal_node):
    """per problem the rows root .. goal node walked from `parent` on the host, None without a goal node"""
    parent, goal = parent.cpu(), goal_node.tolist()
    rows = []
    for r, i in enumerate(goal):
        walk = []
        while i >= 0:
            walk.append(i)
            i = int(parent[r, i])
        rows.append(nodes[r][torch.tensor(walk[::-1], dtype=torch.int64, device=nodes.device)] if walk else None)
    return rows


def _bits(x):
    """a float32 tensor's bit patterns as non-negative int64: they order like the values of floats that are not negative"""
    return x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _sqrt32(x):
    return torch.sqrt(x.to(torch.float64)).to(torch.float32)   # correctly rounded (rrt._length has the argument)


_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 in int64 arithmetic: the four output words (int64 tensors holding 32-bit values) of `counter` (four
    words) under `key` (two words); every word an int or an int64 tensor, broadcast together.  What csrc/philox_device.h
    computes, word for word."""
    c0, c1, c2, c3 = (torch.as_tensor(c, dtype=torch.int64) & _M32 for c in counter)
    k0, k1 = (torch.as_tensor(k, dtype=torch.int64) & _M32 for k in key)

    def mulhilo(m, b):   # the 64-bit product of two 32-bit words from 16-bit halves: nothing passes 2^63
        ph, lo = m * (b >> 16), m * (b & 0xFFFF)
        s = ((ph & 0xFFFF) << 16) + lo
        return (ph >> 16) + (s >> 32), s & _M32

    for _ in builtins.range(10):
        hi0, lo0 = mulhilo(0xD2511F53, c0)
        hi1, lo1 = mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def _u01(word):
    return (word >> 8).to(torch.float32) * 2.0 ** -24   # exact


def host_device_samples(state, goals, limits, seed, g, P, mode="informed", goal_bias=0.1, uniform_mix=0., tries=8, wrap=None):
    """Round g's samples as dcx_rrtstar_sample draws them (include/dcx.h, "batched RRT*: samples drawn on the device"), in torch
    ops on CPU tensors: (samples [R, P, dof] float32, info [R, P] int32, candidates [tries, R, P, dof] float64).  Philox in int64
    arithmetic; the goal rows and the uniform points in float32, one rounded operation at a time: the kernel's bits.  The
    informed draw in float64 from the same uniforms, the same float32 cost and c_min: every try's candidate is returned beside
    the chosen sample (the first try whose float32 rounding lies inside the limits), so a checker can hold the kernel's float32
    arithmetic to the candidate of the try the kernel names.  With circular coordinates (`wrap`) the ellipsoid is the one
    around the shortest-arc image of the goal; every point of it meets the bound under the torus metric.
    `state`: dcx_rrtstar_state's tensors, of which nodes, cost, status and goal_node are read; mode: "uniform" or "informed"."""
    if mode not in ("uniform", "informed"):
        raise ValueError(f"host_device_samples: mode must be 'uniform' or 'informed', got {mode!r}")
    nodes, cost = state["nodes"].detach().cpu().to(torch.float32), state["cost"].detach().cpu().to(torch.float32)
    status, gn = state["status"].cpu(), state["goal_node"].cpu().to(torch.int64)
    R, cap, dof = nodes.shape
    P, tries = int(P), int(tries)
    goals = torch.as_tensor(goals).detach().cpu().to(torch.float32).reshape(R, dof)
    lim = torch.as_tensor(limits).detach().cpu().to(torch.float32).reshape(dof, 2)
    mask = _ops.wrap_mask(wrap, dof)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    slot = (torch.arange(R, dtype=torch.int64)[:, None] * 16 + torch.arange(P, dtype=torch.int64)[None, :]) & _M32

    def block(t, b):
        return philox4x32_10((int(g), slot, t, b), (seed & _M32, seed >> 32))

    h0 = block(0, 0)
    u_bias, u_mix = _u01(h0[0]), _u01(h0[1])
    start = nodes[:, 0]
    running, has = (status == 0)[:, None], ((gn >= 0) & (gn < cap))[:, None]
    is_goal = running & (gn == -1)[:, None] & (u_bias < torch.tensor(float(goal_bias), dtype=torch.float32))
    # step 2's point: one rounded product, one rounded sum
    words = [block(0, 1 + b) for b in builtins.range((dof + 3) // 4)]
    u = torch.stack([_u01(words[j // 4][j % 4]) for j in builtins.range(dof)], dim=-1)
    lo, hi = lim[:, 0], lim[:, 1]
    uniform = lo + (hi - lo) * u
    # step 3 in float64
    a32 = _ops.wrapped_delta(start, goals, mask)
    cmin32 = _length(a32)
    informed = running & has & ~is_goal & (cmin32 > 0)[:, None] & \
        ~(u_mix < torch.tensor(float(uniform_mix), dtype=torch.float32)) & (mode == "informed")
    a, cmin = a32.to(torch.float64), cmin32.to(torch.float64)
    c = cost.gather(1, gn.clamp(0, cap - 1)[:, None])[:, 0].to(torch.float64)
    ah = a / torch.where(cmin > 0, cmin, torch.ones_like(cmin))[:, None]
    v = ah.clone()
    v[:, 0] += torch.where(a[:, 0] < 0, -1.0, 1.0).to(torch.float64)
    vv = (v * v).sum(dim=1)
    centre = start.to(torch.float64) + a / 2
    radii = (torch.sqrt(((c - cmin) * (c + cmin)).clamp(min=0)) / 2)[:, None].repeat(1, dof)
    radii[:, 0] = c / 2
    on = torch.tensor([bool((mask >> j) & 1) for j in builtins.range(dof)])
    cand = torch.zeros((tries, R, P, dof), dtype=torch.float64)
    chosen = torch.full((R, P), tries, dtype=torch.int64)
    for t in builtins.range(tries):
        z = torch.zeros((R, P, dof), dtype=torch.float64)
        for b in builtins.range((dof + 3) // 4):
            h = block(t, 10 + b)
            for i in (0, 1):
                rad = torch.sqrt(-2.0 * torch.log(((h[2 * i] >> 8) + 1).to(torch.float64) * 2.0 ** -24))
                ang = 2.0 * math.pi * _u01(h[2 * i + 1]).to(torch.float64)
                for j, val in ((4 * b + 2 * i, rad * torch.cos(ang)), (4 * b + 2 * i + 1, rad * torch.sin(ang))):
                    if j < dof:
                        z[..., j] = val
        n = z.norm(dim=-1, keepdim=True)
        ball = z / torch.where(n > 0, n, torch.ones_like(n)) * _u01(block(t, 9)[0]).to(torch.float64)[..., None] ** (1.0 / dof)
        y = radii[:, None, :] * ball
        x = centre[:, None, :] + y - 2.0 * v[:, None, :] * (v[:, None, :] * y).sum(dim=-1, keepdim=True) / vv[:, None, None]
        x = torch.where(on, torch.remainder(x + math.pi, 2 * math.pi) - math.pi, x)
        cand[t] = x
        x32 = x.to(torch.float32)
        inside = ((lo <= x32) & (x32 < hi)).all(dim=-1)
        chosen = torch.where((chosen == tries) & inside, torch.full_like(chosen, t), chosen)
    taken = cand.gather(0, chosen.clamp(max=tries - 1)[None, :, :, None].expand(1, R, P, dof))[0].to(torch.float32)
    samples = torch.where((informed & (chosen < tries))[..., None], taken, uniform)
    samples = torch.where(is_goal[..., None], goals[:, None, :].expand(R, P, dof), samples)
    samples = torch.where(running[..., None], samples, start[:, None, :].expand(R, P, dof))
    info = torch.where(informed, 2 + chosen, torch.zeros_like(chosen))
    info = torch.where(is_goal, torch.ones_like(info), info)
    info = torch.where(running, info, torch.full_like(info, -1))
    return samples.contiguous(), info.to(torch.int32), cand


class _Objective:
    """the clearance objective of include/dcx.h in torch ops, one rounded float32 operation at a time:
    C = L * (1 + gain * max(w + band, 0))"""

    def __init__(self, gain, band, submit_all=False):
        self.gain, self.band, self.submit_all = float(gain), float(band), bool(submit_all)

    def pen(self, w):
        return torch.clamp(w + torch.tensor(self.band, dtype=torch.float32, device=w.device), min=0)

    def price(self, L, w):
        f = 1 + torch.tensor(self.gain, dtype=torch.float32, device=w.device) * self.pen(w)
        return L * f


def _objective(name, objective, gain, band, submit_all=False):
    """None for objective="length", else the _Objective of "clearance" (its arguments checked)"""
    if objective == "length":
        return None
    if objective != "clearance":
        raise ValueError(f"{name}: objective must be 'length' or 'clearance', got {objective!r}")
    if band is None or not float(band) > 0:
        raise ValueError(f"{name}: objective='clearance' needs clearance_band > 0 (how far below the margin a peak starts to cost)")
    if not float(gain) >= 0:
        raise ValueError(f"{name}: clearance_gain must be >= 0")
    return _Objective(gain, band, submit_all)


class _PeakEdges:
    """the checker's motion_worst on the fixed batch, as rrt._Edges is its check_motions"""

    def __init__(self, name, checker, max_step, max_samples, mask, margin):
        if not callable(getattr(checker, "motion_worst", None)):
            raise TypeError(f"{name}: the clearance objective needs a checker with motion_worst(qa, qb, max_step=, max_samples=, wrap=)")
        self.checker, self.max_step, self.max_samples, self.mask = checker, float(max_step), int(max_samples), int(mask)
        self.kw = {} if (isinstance(margin, (int, float)) and float(margin) == 0.0) else {"margin": margin}

    def worst(self, qa, qb, root):
        """worst [E] float32 of the edges qa -> qb; an edge over max_samples is answered NaN without being submitted (a facade
        raises for it): its place in the batch takes `root` -> `root`, as an idle slot's"""
        over = _edge_plan(qa, qb, self.max_step, self.max_samples, self.mask)[2]
        qa_s, qb_s = torch.where(over[:, None], root, qa), torch.where(over[:, None], root, qb)
        w = self.checker.motion_worst(qa_s, qb_s, max_step=self.max_step, wrap=self.mask if self.mask else None,
                                      max_samples=self.max_samples, **self.kw)[0]
        w = torch.as_tensor(w).detach().to(device=qa.device, dtype=torch.float32).reshape(-1)
        return torch.where(over, torch.full_like(w, float("nan")), w)


class _FusedPeakEdges:
    """the same on a ScoreModel (the initial checks of the fused planner)"""

    def __init__(self, model, max_step, max_samples, mask, margin):
        self.model, self.max_step, self.max_samples, self.mask, self.margin = model, float(max_step), int(max_samples), int(mask), margin

    def worst(self, qa, qb, root):
        return self.model.motion_worst_raw(qa, qb, max_step=self.max_step, margin=self.margin, max_samples=self.max_samples,
                                           wrap=self.mask)[0]


class _StarPlan(_Plan):
    def __init__(self, checker, starts, goals, dev, reach, max_step, radius, near, wrap, slots, cap, max_rounds, rounds_per_call, sampler,
                 goal_bias, limits, seed, max_samples, sampling="host", uniform_mix=0., informed_tries=8, record_samples=False):
        if sampling not in _SAMPLING:
            raise ValueError(f"rrt_star: sampling must be one of {list(_SAMPLING)}, got {sampling!r}")
        if sampling != "host" and sampler is not None:
            raise ValueError(f"rrt_star: a `sampler` draws on the host: it cannot be combined with sampling={sampling!r}")
        self.mode, self.seed, self.goal_bias = _SAMPLING[sampling], int(seed), float(goal_bias)
        self.uniform_mix, self.tries = float(uniform_mix), int(informed_tries)
        self.kept = ([], []) if record_samples else None   # the rounds' samples and info words, chunk by chunk
        own = sampler is None
        super().__init__(checker, starts, goals, dev, reach, max_step, wrap, slots, cap, max_rounds, rounds_per_call,
                         (lambda T, R, P: None) if own else sampler, limits, seed, max_samples)
        self.K = int(near)
        if not 0 <= self.K <= 16:
            raise ValueError(f"rrt_star: near must be in [0, 16], got {near}")
        if not 2 <= self.cap <= 65536:
            raise ValueError(f"rrt_star: cap must be in [2, 65536], got {cap}")
        self.radius = self.range if radius is None else float(radius)
        if not self.radius >= 0:
            raise ValueError("rrt_star: radius must be >= 0")
        if self.mode is not None:
            if self.limits is None:
                raise ValueError(f"rrt_star: sampling={sampling!r} needs `limits` [dof, 2]: the checker's robot has no joint limits")
            if not 0 <= self.goal_bias <= 1 or not 0 <= self.uniform_mix <= 1:
                raise ValueError("rrt_star: goal_bias and uniform_mix must be in [0, 1]")
            if not 1 <= self.tries <= 16:
                raise ValueError(f"rrt_star: informed_tries must be in [1, 16], got {informed_tries}")
            self.limits = self.limits.contiguous()
        elif own:
            if self.limits is None:
                raise ValueError("rrt_star: pass `limits` [dof, 2] or a `sampler`: the checker's robot has no joint limits")
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(seed))
            lo, span, bias = self.limits[:, 0], self.limits[:, 1] - self.limits[:, 0], float(goal_bias)

            def default(T, R, P):   # one pair of draws per round: the stream of samples does not depend on rounds_per_call
                out = []
                for _ in range(T):
                    u = lo + span * torch.rand((R, P, self.dof), generator=gen, device=dev)
                    pick = torch.rand((R, P), generator=gen, device=dev) < bias
                    out.append(torch.where(pick[..., None], self.goals[:, None, :], u))
                return torch.stack(out) if T else torch.zeros((0, R, P, self.dof), device=dev)
            self.sampler = default

    def initial_state(self, edges, obj=None):
        """the roots, and the initial checks as ONE batch of 3 R edges: the zero-length edges on the starts and on the goals
        (the point checks under the planner's own margin) and the direct motions start -> goal.  A free direct motion is the
        optimum: node 1 is the goal.  Under an objective (`edges` then answers peaks) a free direct motion is node 1 with its
        cost C all the same, but the optimum (status 1) only where C has its length's bits; a penalised one keeps status 0
        and first_round -1, and the rounds improve on it"""
        R, cap, dof, dev = self.R, self.cap, self.dof, self.dev
        st = dict(nodes=torch.zeros((R, cap, dof), dtype=torch.float32, device=dev),
                  parent=torch.full((R, cap), -1, dtype=torch.int32, device=dev),
                  elen=torch.zeros((R, cap), dtype=torch.float32, device=dev),
                  cost=torch.zeros((R, cap), dtype=torch.float32, device=dev),
                  count=torch.ones(R, dtype=torch.int32, device=dev),
                  status=torch.zeros(R, dtype=torch.int32, device=dev),
                  goal_node=torch.full((R,), -1, dtype=torch.int32, device=dev),
                  first_round=torch.full((R,), -1, dtype=torch.int32, device=dev))
        st["nodes"][:, 0] = self.starts
        if R:
            qa, qb = torch.cat([self.starts, self.goals, self.starts]), torch.cat([self.starts, self.goals, self.goals])
            L = C = _length(_ops.wrapped_delta(self.starts, self.goals, self.mask))
            if obj is None:
                free = edges.first_hit(qa, qb, self.starts[:1].expand(3 * R, dof))[0] == -1
            else:
                w = edges.worst(qa, qb, self.starts[:1].expand(3 * R, dof))
                free = w <= 0
                C = obj.price(L, w[2 * R:])
            blocked = ~free[:R] | ~free[R:2 * R]
            direct = free[2 * R:] & ~blocked
            st["status"][blocked] = BLOCKED
            st["status"][direct & (_bits(C) == _bits(L))] = DIRECT
            st["nodes"][direct, 1] = self.goals[direct]
            st["parent"][direct, 1] = 0
            st["elen"][direct, 1] = C[direct]
            st["cost"][direct, 1] = C[direct]
            st["count"][direct] = 2
            st["goal_node"][direct] = 1
        return st

    def run(self, st, run_chunk, stop_on_first):
        """chunks of rounds until no problem is running or max_rounds (stop_on_first: or every running problem has a goal node);
        one status / goal_node read-back per chunk.  The rounds run."""
        g = 0
        while g < self.max_rounds:
            status, goal = torch.stack([st["status"], st["goal_node"]]).cpu()
            running = status == RUNNING
            if not bool(running.any()) or (stop_on_first and bool((goal[running] >= 0).all())):
                break
            T = min(self.chunk, self.max_rounds - g)
            if self.mode is not None:   # the chunk draws its own samples, round by round
                run_chunk(T, g)
                g += T
                continue
            samples = torch.as_tensor(self.sampler(T, self.R, self.P)).to(device=self.dev, dtype=torch.float32).contiguous()
            if tuple(samples.shape) != (T, self.R, self.P, self.dof):
                raise ValueError(f"rrt_star: the sampler returned {tuple(samples.shape)}, expected {(T, self.R, self.P, self.dof)}")
            if self.kept is not None:
                self.kept[0].append(samples)
            run_chunk(samples, g)
            g += T
        return g

    def star_result(self, route, st, rounds_run):
        paths = _walk_all(st["nodes"], st["parent"], st["goal_node"])
        goal = st["goal_node"].to(torch.int64)
        costs = st["cost"].gather(1, goal.clamp(min=0)[:, None])[:, 0] if self.R else st["cost"][:, 0]
        costs = torch.where(goal >= 0, costs, torch.full_like(costs, float("nan")))
        samples = info = None
        if self.kept is not None:
            samples = torch.cat(self.kept[0]) if self.kept[0] else torch.zeros((0, self.R, self.P, self.dof), device=self.dev)
            info = torch.cat(self.kept[1]) if self.kept[1] else None
        return RRTStarResult(route, st, paths, costs, rounds_run, samples, info)


def _host_round(pl, edges, st, s, g, trace=None, obj=None):
    """one round of the contract on the state tensors, in place (s [R, P, dof]: the round's samples).  `trace`: a dict that
    takes what the round did (the events the tests count).  `obj`: None, or the _Objective of the clearance round (`edges`
    then answers peaks): verdicts from w <= 0, every edge priced C = L * f(w), the places submitted on the lower bound L."""
    R, P, K, dof, cap, mask, dev = pl.R, pl.P, pl.K, pl.dof, pl.cap, pl.mask, pl.dev
    r_all = torch.arange(R, device=dev)
    r1, r2 = r_all[:, None], r_all[:, None, None]
    running = st["status"] == RUNNING
    counts = st["count"].tolist()   # the snapshot's
    nodes, cost = st["nodes"], st["cost"]
    root = nodes[:, 0][:, None, :].expand(R, P, dof)

    def check(go, qa, qb, rt, L):
        """(free, C) of the batch's edges: the verdicts and the edges' costs; the trace counts the free edges of `go` that cost
        more than their length"""
        qa, qb = torch.where(go[..., None], qa, rt), torch.where(go[..., None], qb, rt)
        if obj is None:
            return edges.first_hit(qa.reshape(-1, dof), qb.reshape(-1, dof), rt.reshape(-1, dof))[0].reshape(go.shape) == -1, L
        w = edges.worst(qa.reshape(-1, dof), qb.reshape(-1, dof), rt.reshape(-1, dof)).reshape(go.shape)
        if trace is not None:
            seen["penalised"] += int((go & (w <= 0) & (obj.pen(w) > 0)).sum())
        return w <= 0, obj.price(L, w)

    seen = dict(penalised=0, pruned_after=0, rewire_rejected_after=0)   # (counted for a trace only: each is a read-back)

    every = obj is not None and obj.submit_all   # (a test's: every near place submitted, the lower bounds ignored)

    # 1. extend: RRT-Connect's phase 1 on the one tree
    near = _nearest({"nodes": nodes[:, None]}, 0, s, running[:, None].expand(R, P), [[c] for c in counts], mask)
    nc = near.clamp(min=0)
    nq = nodes[r1, nc]
    x, ok = _steer(nq, s, pl.range, mask)
    go = (near >= 0) & ok
    L0 = _length(_ops.wrapped_delta(nq, x, mask))
    free, C0 = check(go, nq, x, root, L0)
    cand = go & free
    c0 = cost[r1, nc] + C0
    par, elen, cnew = near.clone(), C0, c0

    if K > 0:
        # 2. the near sets over the snapshot
        u = torch.full((R, P, K), -1, dtype=torch.int64, device=dev)
        d2 = torch.full((R, P, K), float("inf"), dtype=torch.float32, device=dev)
        for r in torch.nonzero(cand.any(dim=1)).reshape(-1).tolist():
            idx, dist2 = knn(x[r], nodes[r, :counts[r]], K, wrap=mask, max_dist=pl.radius)
            u[r], d2[r] = idx.to(torch.int64), dist2
        u = torch.where(cand[..., None], u, torch.full_like(u, -1))
        uc = u.clamp(min=0)
        un = nodes[r2, uc]
        rootk = root[:, :, None, :].expand(R, P, K, dof)
        xk = x[:, :, None, :].expand(R, P, K, dof)
        # 3. choose parent
        Lj = _length(_ops.wrapped_delta(un, xk, mask))
        key0 = ((_bits(c0) << 32) | nc)[..., None]
        submit = (u >= 0) & ((((_bits(cost[r2, uc] + Lj) << 32) | uc) < key0) | every)   # the lower bound: Cj >= Lj
        free, Cj = check(submit, un, xk, rootk, Lj)
        cj = cost[r2, uc] + Cj
        keyj = (_bits(cj) << 32) | uc
        free = submit & free
        if trace is not None:
            seen["pruned_after"] = int((free & ~(keyj < key0)).sum())
        free = free & (keyj < key0)
        keyj = torch.where(free, keyj, torch.full_like(keyj, _NO_KEY))
        jb = keyj.argmin(dim=2, keepdim=True)
        has = free.any(dim=2)
        par = torch.where(has, uc.gather(2, jb)[..., 0], near)
        elen = torch.where(has, Cj.gather(2, jb)[..., 0], C0)
        cnew = torch.where(has, cj.gather(2, jb)[..., 0], c0)

    # 4. append in slot order while count < cap
    n0 = st["count"].to(torch.int64)
    a64 = cand.to(torch.int64)
    at = n0[:, None] + torch.cumsum(a64, dim=1) - a64
    fits = cand & (at < cap)
    rr = r1.expand_as(at)[fits]
    st["nodes"][rr, at[fits]] = x[fits]
    st["parent"][rr, at[fits]] = par[fits].to(torch.int32)
    st["elen"][rr, at[fits]] = elen[fits]
    st["cost"][rr, at[fits]] = cnew[fits]
    total = n0 + a64.sum(dim=1)
    st["count"][:] = total.clamp(max=cap).to(torch.int32)
    over = total > cap
    added = torch.where(fits, at, torch.full_like(at, -1))
    is_goal = fits & (x.contiguous().view(torch.int32) == pl.goals.contiguous().view(torch.int32)[:, None, :]).all(dim=2)
    found = is_goal.any(dim=1) & (st["goal_node"] == -1)
    p0 = is_goal.to(torch.int64).argmax(dim=1)   # the lowest slot
    st["goal_node"][found] = added[r_all, p0][found].to(torch.int32)
    st["first_round"][found] = g
    st["status"][running & over] = FULL
    if trace is not None:
        trace.update(chose_other=int((fits & (par != near)).sum()), dropped=int((cand & ~fits).sum()), rewires=0, contested=0,
                     lowered_descendants=0, short_near=int((cand & (u[..., K - 1] < 0)).sum()) if K > 0 else 0,
                     **seen)
    if K == 0:
        return

    # 5. rewire: the new nodes against the snapshot's cost of their near nodes
    ac = added.clamp(min=0)
    Lp = _sqrt32(d2)
    cx = cost[r1, ac][..., None]
    submit = (added >= 0)[..., None] & (u >= 0) & (u != par[..., None]) & ((cx + Lp < cost[r2, uc]) | every)   # the lower bound
    free, Cp = check(submit, xk, un, rootk, Lp)
    cp = cx + Cp
    free = submit & free
    if trace is not None:
        seen["rewire_rejected_after"] = int((free & ~(cp < cost[r2, uc])).sum())
    free = (free & (cp < cost[r2, uc])).reshape(R, P * K)
    v = uc.reshape(R, P * K)
    key = ((_bits(cp) << 32) | torch.arange(P, device=dev)[None, :, None]).reshape(R, P * K)
    rival = free[:, :, None] & free[:, None, :] & (v[:, :, None] == v[:, None, :]) & (key[:, None, :] < key[:, :, None])
    win = free & ~rival.any(dim=2)
    rw = r1.expand_as(v)[win]
    st["parent"][rw, v[win]] = ac[:, :, None].expand(R, P, K).reshape(R, P * K)[win].to(torch.int32)
    st["elen"][rw, v[win]] = Cp.reshape(R, P * K)[win]

    # 6. refresh: the fixed point of cost = cost[parent] + elen from the roots' +0, where something was rewired
    rows = torch.nonzero(win.any(dim=1)).reshape(-1)
    before = st["cost"].clone() if trace is not None else None
    if len(rows):
        pr = st["parent"][rows].to(torch.int64)
        live = (pr >= 0) & (torch.arange(cap, device=dev)[None, :] < st["count"][rows].to(torch.int64)[:, None])
        while True:
            cur = st["cost"][rows]
            new = torch.where(live, cur.gather(1, pr.clamp(min=0)) + st["elen"][rows], cur)
            if torch.equal(_bits(new), _bits(cur)):
                break
            st["cost"][rows] = new
    if trace is not None:
        target = torch.zeros((R, cap), dtype=torch.bool, device=dev)
        target[rw, v[win]] = True
        trace.update(rewires=int(win.sum()), contested=int((win & (free[:, None, :] & (v[:, :, None] == v[:, None, :])).sum(dim=2).gt(1)).sum()),
                     lowered_descendants=int(((st["cost"] < before) & ~target).sum()), **seen)
        assert not bool((st["cost"] > before).any())


def host_rrt_star(checker, starts, goals, *, range, max_step, radius=None, near=8, wrap=None, slots=4, cap=4096, max_rounds=256,
                  rounds_per_call=32, sampler=None, goal_bias=0.1, limits=None, seed=0, margin=0., max_samples=None,
                  stop_on_first=False, sampling="host", uniform_mix=0., informed_tries=8, record_samples=False, objective="length",
                  clearance_gain=1.0, clearance_band=None, _trace=None, _submit_all=False):
    """rrt_star's contract as the loop a user would write from the library's other calls: per round one `knn` per running
    problem for the nearest nodes and one for the near sets, the steering, costs and selections in torch, ONE
    `checker.check_motions(..., return_first=True)` call per phase on the fixed batches of R * slots, R * slots * near and
    R * slots * near edges, the appends and rewires as indexed assignments.  The state lives on the device of `starts`.
    `margin` is passed on to the checker's check_motions only where it is not 0.  sampling="device" / "informed" (rrt_star has
    the options) draws every round from host_device_samples on the state as the round finds it.
    objective="clearance" (rrt_star has the arguments): the same round with ONE `checker.motion_worst(...)` call per phase on
    the same batches in place of check_motions; a checker without motion_worst is a TypeError.  `_trace` then also counts
    `penalised` (free edges that cost more than their length), `pruned_after` (places submitted on the lower bound and free,
    but no longer below the incumbent once priced) and `rewire_rejected_after` (the same for rewires)."""
    dev = torch.as_tensor(starts).device
    obj = _objective("host_rrt_star", objective, clearance_gain, clearance_band, _submit_all)
    pl = _StarPlan(checker, starts, goals, dev, range, max_step, radius, near, wrap, slots, cap, max_rounds, rounds_per_call, sampler,
                   goal_bias, limits, seed, max_samples, sampling, uniform_mix, informed_tries, record_samples)
    edges = _Edges(checker, pl.max_step, pl.max_samples, pl.mask, margin) if obj is None else \
        _PeakEdges("host_rrt_star", checker, pl.max_step, pl.max_samples, pl.mask, margin)
    st = pl.initial_state(edges, obj)

    def run_chunk(samples, g0):
        for t in builtins.range(samples if pl.mode is not None else len(samples)):
            ev = None if _trace is None else {"round": g0 + t}
            if pl.mode is not None:
                s, info, _ = host_device_samples(st, pl.goals, pl.limits, pl.seed, g0 + t, pl.P, pl.mode, pl.goal_bias, pl.uniform_mix,
                                                 pl.tries, pl.mask)
                s, info = s.to(dev), info.to(dev)
                if pl.kept is not None:
                    pl.kept[0].append(s[None])
                    pl.kept[1].append(info[None])
                if ev is not None:
                    ev["samples"], ev["sample_info"] = s, info
            else:
                s = samples[t]
            _host_round(pl, edges, st, s, g0 + t, ev, obj)
            if _trace is not None:
                ev["state"] = {k: v.clone() for k, v in st.items()}
                _trace.append(ev)

    return pl.star_result("host", st, pl.run(st, run_chunk, stop_on_first))


def rrt_star(checker, starts, goals, *, range, max_step, radius=None, near=8, wrap=None, slots=4, cap=4096, max_rounds=256,
             rounds_per_call=32, sampler=None, goal_bias=0.1, limits=None, seed=0, margin=0., max_samples=None, stop_on_first=False,
             sampling="host", uniform_mix=0., informed_tries=8, record_samples=False, objective="length", clearance_gain=1.0,
             clearance_band=None):
    """Plan R motions starts[r] -> goals[r] ([R, dof] each) with batched RRT* under `checker`: an RRTStarResult.  Anytime: a
    problem keeps improving its tree until max_rounds (stop_on_first: the loop ends at the first chunk after which every
    running problem has reached its goal).
    range: the longest extension; max_step: the stride of every edge check; radius: the near set's radius (None: range); near:
    K, the most near nodes a new node looks at (0 .. 16; 0: plain RRT with costs); wrap (as check_motions): the circular
    coordinates; slots: extensions per problem and round (1 .. 16); cap: nodes per tree (2 .. 65536); sampler(T, R, P) ->
    [T, R, P, dof] (default: uniform in `limits` [dof, 2], taken from the checker's robot where it has them, and with probability
    `goal_bias` the goal row itself, both drawn from one generator seeded by `seed`); margin: a sample collides where
    score - margin > 0, on top of the checker's own threshold; max_samples: the most samples of one edge.
    sampling: "host" (the default: `sampler`, a whole chunk of rounds drawn before the chunk runs), "device" (uniform in `limits`
    with the goal bias, drawn on the device at the start of every round: Philox4x32-10 keyed by `seed`, no launch of torch's per
    chunk) or "informed" (as "device" until a problem has a goal node of cost c; from then on its samples are uniform in the
    ellipsoid d(start, x) + d(x, goal) <= c, the only points that can still shorten its path, `informed_tries` (1 .. 16) draws
    before the uniform point is taken where the ellipsoid leaves the limits, and with probability `uniform_mix` a uniform sample
    all the same).  With circular coordinates the ellipsoid is the one around the shortest-arc image of the goal: every point
    of it meets the bound under the torus metric, and routes through other images of the goal are left to uniform_mix.  The
    goal bias is off once a problem has a goal node.  Both need `limits`; a `sampler` together with either is a ValueError.
    record_samples: keep every round's samples (and, for the device draws, their info words) on the result.
    objective: "length" (the default) or "clearance": an edge then costs C = L * (1 + clearance_gain * max(w + clearance_band,
    0)), L its length and w the peak of score - margin over its samples (motion_worst's), every operation fp32 and rounded
    alone - a hinge, so that the fused planner and host_rrt_star agree bit for bit.  clearance_band > 0 (required; in score
    units) is how far below the margin a peak starts to cost, clearance_gain >= 0 the slope.  costs, cost and elen then hold
    these costs (never below the lengths); clearance_cost_paths prices other paths the same way.  A free direct motion is final
    (status 1) only where it is not penalised; otherwise it seeds the tree (first_round stays -1) and the rounds improve on it.
    clearance_gain = 0 plans exactly as objective="length".
    The fused planner (result.route == "fused") runs for kernel_perceptrons.DiffCo, RBFDiffCo and ForwardKinematicsDiffCo whose
    transform fuses; every other checker is planned by host_rrt_star ("host")."""
    dev0 = torch.as_tensor(starts).device
    obj = _objective("rrt_star", objective, clearance_gain, clearance_band)
    got = _fused_model(checker, dev0 if dev0.type == "cuda" else None)
    if got is None:
        return host_rrt_star(checker, starts, goals, range=range, max_step=max_step, radius=radius, near=near, wrap=wrap, slots=slots,
                             cap=cap, max_rounds=max_rounds, rounds_per_call=rounds_per_call, sampler=sampler, goal_bias=goal_bias,
                             limits=limits, seed=seed, margin=margin, max_samples=max_samples, stop_on_first=stop_on_first,
                             sampling=sampling, uniform_mix=uniform_mix, informed_tries=informed_tries, record_samples=record_samples,
                             objective=objective, clearance_gain=clearance_gain, clearance_band=clearance_band)
    model, base = got
    if isinstance(base, (int, float)) and isinstance(margin, (int, float)):
        mg = float(base) + float(margin)
    else:   # one per class on either side
        mg = (torch.as_tensor(base, dtype=torch.float32).reshape(-1).to(model.dev)
              + torch.as_tensor(margin, dtype=torch.float32).reshape(-1).to(model.dev))
    pl = _StarPlan(checker, starts, goals, model.dev, range, max_step, radius, near, wrap, slots, cap, max_rounds, rounds_per_call,
                   sampler, goal_bias, limits, seed, max_samples, sampling, uniform_mix, informed_tries, record_samples)
    st = pl.initial_state((_FusedEdges if obj is None else _FusedPeakEdges)(model, pl.max_step, pl.max_samples, pl.mask, mg), obj)
    mg_dev = model._motion_margin(mg)   # on the device once: no copy from the host per chunk
    cost_kw = {} if obj is None else dict(gain=obj.gain, band=obj.band)

    def run_chunk(samples, g0):
        if pl.mode is not None:   # (samples: T)
            keep = info = None
            if pl.kept is not None:
                keep = torch.empty((samples, pl.R, pl.P, pl.dof), dtype=torch.float32, device=pl.dev)
                info = torch.empty((samples, pl.R, pl.P), dtype=torch.int32, device=pl.dev)
                pl.kept[0].append(keep)
                pl.kept[1].append(info)
            run = model.rrtstar_run_sampled if obj is None else model.rrtstar_run_sampled_cost
            return run(st, pl.goals, pl.limits, pl.seed, samples, pl.P, g0, pl.range, pl.max_step, pl.radius, pl.K, pl.max_samples,
                       mode=pl.mode, goal_bias=pl.goal_bias, uniform_mix=pl.uniform_mix, tries=pl.tries,
                       margin=0. if mg_dev is None else mg_dev, wrap=pl.mask, samples_out=keep, info_out=info, **cost_kw)
        run = model.rrtstar_run if obj is None else model.rrtstar_run_cost
        run(st, pl.goals, samples, g0, pl.range, pl.max_step, pl.radius, pl.K, pl.max_samples,
            margin=0. if mg_dev is None else mg_dev, wrap=pl.mask, **cost_kw)

    return pl.star_result("fused", st, pl.run(st, run_chunk, stop_on_first))


def clearance_cost_paths(checker, paths, counts, *, max_step, gain=1.0, band, wrap=None, margin=0., max_samples=None):
    """(cost [R], length [R], peak [R]) float32 of R piecewise-straight paths under rrt_star's clearance objective, whatever made
    them (RRTStarResult.path_tensor(), shortcut_paths, query_batch): paths [R, W, dof], counts [R] the waypoints of each (a row
    with fewer than two has cost and length 0 and peak nan).  ONE `checker.motion_worst` call on the consecutive pairs; a
    segment costs C = L * (1 + gain * max(w + band, 0)), L the motion calls' length bits and w its peak of score - margin, and a
    path's cost is the sum of its segments' from the root on, one float32 sum per segment - the goal node's cost of a tree that
    holds these edges, to the bits of w.  length sums the L the same way; peak is the largest w (> 0: the path collides).
    max_samples=None: from the longest segment."""
    obj = _objective("clearance_cost_paths", "clearance", gain, band)
    paths = torch.as_tensor(paths).detach().to(torch.float32)
    if paths.dim() != 3:
        raise ValueError("clearance_cost_paths: paths must be [R, W, dof]")
    R, W, dof = paths.shape
    dev = paths.device
    n = torch.as_tensor(counts).to(device=dev, dtype=torch.int64).reshape(R)
    cost = torch.zeros(R, dtype=torch.float32, device=dev)
    length = torch.zeros(R, dtype=torch.float32, device=dev)
    peak = torch.full((R,), float("nan"), dtype=torch.float32, device=dev)
    if R == 0 or W < 2:
        return cost, length, peak
    mask = _ops.wrap_mask(wrap, dof, getattr(checker, "transform", None) or
                          getattr(getattr(checker, "perceptron", None), "transform", None))
    live = torch.arange(W - 1, device=dev)[None, :] + 1 < n[:, None]   # segment s of path r: waypoints s -> s + 1
    qa, qb = paths[:, :-1][live], paths[:, 1:][live]
    if len(qa) == 0:
        return cost, length, peak
    L = _length(_ops.wrapped_delta(qa, qb, mask))
    if max_samples is None:
        max_samples = min(_ops.MOTION_MAX_SAMPLES, int(math.ceil(float(L.max()) / float(max_step))) + 2)
    edges = _PeakEdges("clearance_cost_paths", checker, max_step, max_samples, mask, margin)
    w = edges.worst(qa, qb, qa[:1].expand_as(qa))
    Cs, Ls, ws = (torch.zeros((R, W - 1), dtype=torch.float32, device=dev) for _ in builtins.range(3))
    Cs[live], Ls[live] = obj.price(L, w), L
    ws = torch.full_like(ws, -float("inf"))
    ws[live] = torch.where(torch.isnan(w), torch.full_like(w, float("inf")), w)   # (a segment over max_samples: not priced)
    for k in builtins.range(W - 1):   # (a dead segment adds +0: the sum keeps its bits)
        cost, length = cost + Cs[:, k], length + Ls[:, k]
    has = live.any(dim=1)
    peak = torch.where(has, ws.max(dim=1).values, peak)
    return cost, length, peak
