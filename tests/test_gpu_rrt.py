"""GPU: batched RRT-Connect (dcx_rrt_connect_run, ScoreModel.rrt_connect_run, rrt.rrt_connect) against its referee
rrt.host_rrt_connect - the same contract composed of roadmap.knn, torch arithmetic and the checker's check_motions - bit for bit
on every state tensor for identical samples: a DiffCo on the 2-DoF planar arm with both joints on the circle, a 7-DoF Baxter
fixture without a mask, and a five-class one with per-class margins.  Then every node's provenance restated in numpy float32, the
returned paths, one call of T rounds against T calls of one, graph capture, and the routing of rrt_connect."""
import functools

import numpy as np
import pytest
import torch

from helpers import CASE_ROBOT, case_kernel, load, make_robot
from motion_wrap_helpers import fixture_model, mixed_margin, motion_samples_wrapped, wrap2pi32

pytestmark = pytest.mark.gpu

F = np.float32
STATE = ("nodes", "parent", "count", "status", "link", "solved_round")
# case (a): chosen on the GPU against host_rrt_connect so that the coverage conditions of test_case_a_covers_the_contract hold
SEED_A = 20
CUT_START_A = 2   # which of the four hard pairs lends its start to the problem with the cut-off goal
A = dict(R=6, P=3, cap=48, range=0.5, max_step=0.1, rounds=48, chunk=4)
B = dict(R=4, P=2, cap=64, range=1.5, max_step=0.25, rounds=24, chunk=4)


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")


def _fixed(samples):
    at = [0]

    def sampler(T, R, P):
        out = samples[at[0]:at[0] + T]
        at[0] += T
        return out
    return sampler


class Recorder:
    """a checker's check_motions with every batch kept (edges and first hits): what the planner asked and was told"""

    def __init__(self, checker):
        self.checker, self.calls = checker, []

    def check_motions(self, qa, qb, **kw):
        hit, first = self.checker.check_motions(qa, qb, **kw)
        self.calls.append((qa.clone(), qb.clone(), first.clone()))
        return hit, first


class ModelChecker:
    """a ScoreModel with per-class margins as a checker: check_motions for the host planner, _rrt_model for the fused one"""

    def __init__(self, model, margin):
        self.model, self.margin = model, margin

    def check_motions(self, qa, qb, max_step=None, wrap=None, max_samples=None, return_first=False):
        first, _ = self.model.check_motions(qa, qb, max_step=max_step, margin=self.margin, max_samples=max_samples, wrap=wrap)
        return first >= 0, first

    def _rrt_model(self, device=None):
        return self.model, self.margin


def _pairs(check, nodes, n, hard=True):
    """tests/test_gpu_roadmap.py's _hard_pair for n pairs: of 40 sampled nodes, the n farthest pairs whose direct motion the
    checker refuses (hard=False: the nearest pair it accepts)"""
    pick = torch.as_tensor(np.random.default_rng(0).choice(len(nodes), 40, replace=False), device=nodes.device)
    a, b = torch.triu_indices(40, 40, 1, device=nodes.device)
    hit = check(nodes[pick[a]], nodes[pick[b]])
    dist = (nodes[pick[a]] - nodes[pick[b]]).norm(dim=1)
    if not hard:
        i = int(torch.where(hit, torch.full_like(dist, float("inf")), dist).argmin())
        assert not bool(hit[i])
        return [(int(pick[a[i]]), int(pick[b[i]]))]
    assert int(hit.sum()) >= n
    order = torch.argsort(dist * hit, descending=True)[:n].tolist()
    return [(int(pick[a[i]]), int(pick[b[i]])) for i in order]


def _planar_checker():
    from diffco_amd import _lib, kernel
    from diffco_amd.kernel_perceptrons import DiffCo
    _lib.require_gpu()
    name = "cfg1_planar2_rq"
    d = load(name)
    kind, p0, p1 = case_kernel(d)
    rob = make_robot(CASE_ROBOT[name])
    dc = DiffCo(kernel_func=kernel.RQKernel(p0, p1), transform=rob.fkine)
    dc.support_points = _t(d["sup_q"])
    dc.support_transformed = rob.fkine(dc.support_points)
    dc.gains = _t(d["weights"][:, 0])
    return d, dc, rob


@functools.lru_cache(maxsize=None)
def problem_a(which=None):
    """(fixture, checker, robot, starts [6, 2], goals): a colliding start; a pair whose direct motion is free; three pairs found
    as tests/test_gpu_roadmap.py's _hard_pair finds its one (nodes of the roadmap's largest component whose direct motion the
    checker refuses, the farthest of a sample); and one whose goal the roadmap leaves cut off from that component - a free
    pocket no motion leaves - so that its trees can only fill"""
    from scipy.sparse.csgraph import connected_components
    from diffco_amd.roadmap import Roadmap
    d, dc, rob = _planar_checker()
    g = torch.Generator().manual_seed(3)
    nodes = ((torch.rand(512, 2, generator=g) * 2 - 1) * np.pi).float().cuda()
    hit = dc.is_collision(nodes).reshape(-1)
    rm = Roadmap.build(dc, nodes, 8, A["max_step"], wrap=True)
    _, label = connected_components(rm.graph, directed=False)
    big = label == np.bincount(label).argmax()
    free = rm.nodes[torch.as_tensor(np.flatnonzero(big), device="cuda")]
    cut = rm.nodes[torch.as_tensor(np.flatnonzero(~big), device="cuda")]
    assert len(free) >= 40 and len(cut) >= 1
    check = lambda a, b: torch.as_tensor(dc.check_motions(a, b, max_step=A["max_step"], wrap=True)).cuda()   # noqa: E731
    easy = _pairs(check, free, 1, hard=False)[0]
    hard = _pairs(check, free, 4)
    which = CUT_START_A if which is None else which
    rest = [h for k, h in enumerate(hard) if k != which]
    starts = torch.stack([nodes[hit][0], free[easy[0]]] + [free[i] for i, _ in rest] + [free[hard[which][0]]])
    goals = torch.stack([free[0], free[easy[1]]] + [free[j] for _, j in rest] + [cut[0]])
    return d, dc, rob, starts, goals


def samples_a(seed):
    gs = torch.Generator().manual_seed(seed)
    return ((torch.rand(A["rounds"], A["R"], A["P"], 2, generator=gs) * 2 - 1) * np.pi).float().cuda()


def kwargs_a(rob):
    return dict(range=A["range"], max_step=A["max_step"], wrap=rob.wrap_mask, slots=A["P"], cap=A["cap"], max_rounds=A["rounds"],
                rounds_per_call=A["chunk"], limits=[[-np.pi, np.pi]] * 2)


@functools.lru_cache(maxsize=None)
def case_a():
    """(fixture, checker, starts, goals, samples, kwargs, host result, recorder, fused result)"""
    from diffco_amd.rrt import host_rrt_connect, rrt_connect
    d, dc, rob, starts, goals = problem_a()
    samples, kw = samples_a(SEED_A), kwargs_a(rob)
    rec = Recorder(dc)
    host = host_rrt_connect(rec, starts, goals, sampler=_fixed(samples), **kw)
    fused = rrt_connect(dc, starts, goals, sampler=_fixed(samples), **kw)
    return d, dc, starts, goals, samples, kw, host, rec, fused


def _assert_same_state(a, b):
    for name in STATE:
        x, y = getattr(a, name), getattr(b, name)
        if name == "nodes":
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), (name, int((x != y).sum()))


def test_case_a_fused_equals_host_bit_for_bit():
    *_, host, rec, fused = case_a()
    assert fused.route == "fused" and host.route == "host"
    _assert_same_state(fused, host)
    assert fused.rounds.tolist() == host.rounds.tolist()
    for p, q in zip(fused.paths, host.paths):
        assert (p is None) == (q is None) and (p is None or torch.equal(p, q))
    # the host planner submitted the initial batch and then the fixed batch, twice a round
    assert len(rec.calls[0][0]) == 3 * A["R"] and {len(c[0]) for c in rec.calls[1:]} == {A["R"] * A["P"]}


def test_case_a_covers_the_contract():
    *_, host, rec, fused = case_a()
    status = fused.status.tolist()
    print("case a: status", status, "counts", fused.count.tolist(), "solved_round", fused.solved_round.tolist())
    assert status[0] == 3 and status[1] == 1 and int(fused.solved_round[1]) == -1 and len(fused.paths[1]) == 2
    assert any(s == 1 and len(p) > 2 for s, p in zip(status, fused.paths) if p is not None)
    assert 2 in status
    # phase 1 is every second batch after the initial one: a rejected edge is a real edge (qa != qb) with a hit
    rejected = sum(int((((qa != qb).any(dim=1)) & (first != -1)).sum()) for qa, qb, first in rec.calls[1::2])
    partial = sum(int((first >= 2).sum()) for qa, qb, first in rec.calls[2::2])
    print("case a: rejected phase-1 edges", rejected, "partial advances", partial)
    assert rejected >= 1 and partial >= 1


def _steer32(near, s, rng, on):
    """include/dcx.h's steering step for one node and many samples, numpy float32 one operation at a time"""
    d = (s - near[None]).astype(F)
    d = np.where(on[None], wrap2pi32(d), d).astype(F)
    l2 = np.zeros(len(s), F)
    for j in range(s.shape[1]):
        l2 = (l2 + (d[:, j] * d[:, j]).astype(F)).astype(F)
    L = np.sqrt(l2).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):   # (a sample on the node itself: L = 0, no edge)
        f = (F(rng) / L).astype(F)
        far = (near[None] + (d * f[:, None]).astype(F)).astype(F)
        far = np.where(on[None], wrap2pi32(far), far).astype(F)
    return np.where((L <= F(rng))[:, None], s, far).astype(F), L > 0


def test_case_a_node_provenance():
    """every non-root node is the steering formula applied to its parent and one of the problem's samples, or sample h - 1
    (h >= 2) of the edge parent -> x for a node x of the other tree - restated in numpy float32"""
    d, dc, starts, goals, samples, kw, host, rec, fused = case_a()
    nodes, parent, count = fused.nodes.cpu().numpy(), fused.parent.cpu().numpy(), fused.count.cpu().numpy()
    smp = samples.cpu().numpy()
    on = np.array([True, True])
    bits = lambda x: np.ascontiguousarray(x, F).view(np.uint32)   # noqa: E731
    n_steer = n_part = 0
    for r in range(A["R"]):
        s_r = smp[:, r].reshape(-1, 2)
        for t in (0, 1):
            for i in range(1, count[r, t]):
                node, par = nodes[r, t, i], nodes[r, t, parent[r, t, i]]
                assert 0 <= parent[r, t, i] < i
                qb, ok = _steer32(par, s_r, A["range"], on)
                if bool(((bits(qb) == bits(node)[None]).all(axis=1) & ok).any()):
                    n_steer += 1
                    continue
                found = False
                for x in nodes[r, 1 - t, :count[r, 1 - t]]:
                    p = motion_samples_wrapped(par[None], x[None], 0b11, max_step=A["max_step"])[0][0]
                    if len(p) > 2 and bool((bits(p[1:-1]) == bits(node)[None]).all(axis=1).any()):
                        found = True
                        break
                assert found, (r, t, i)
                n_part += 1
    print("case a: steered nodes", n_steer, "partial-advance nodes", n_part)
    assert n_steer > 20 and n_part >= 1
    # untouched slots stay as initialised
    for r in range(A["R"]):
        for t in (0, 1):
            assert (parent[r, t, count[r, t]:] == -1).all() and (nodes[r, t, count[r, t]:] == 0).all()


def test_case_a_paths():
    d, dc, starts, goals, samples, kw, host, rec, fused = case_a()
    tol = 1e-5 * float(np.abs(d["score64"]).max())   # tests/test_gpu_motion_worst.py: worst against fp64 within 1e-5 max|s|
    seen = 0
    for r, p in enumerate(fused.paths):
        if p is None:
            continue
        assert torch.equal(p[0], starts[r]) and torch.equal(p[-1], goals[r])
        i, j = fused.link[r].tolist()
        chain0, chain1 = [i], [j]
        while int(fused.parent[r, 0, chain0[-1]]) >= 0:
            chain0.append(int(fused.parent[r, 0, chain0[-1]]))
        while int(fused.parent[r, 1, chain1[-1]]) >= 0:
            chain1.append(int(fused.parent[r, 1, chain1[-1]]))
        want = torch.cat([fused.nodes[r, 0][chain0[::-1]], fused.nodes[r, 1][chain1]])
        assert torch.equal(p, want)
        worst, _, _ = dc.motion_worst(p[:-1], p[1:], max_step=A["max_step"], wrap=kw["wrap"])
        print("case a: path", r, "waypoints", len(p), "peak", float(worst.max()), "tol", tol)
        assert float(worst.max()) <= tol
        assert float(fused.lengths[r]) > 0
        seen += 1
    assert seen >= 2


@functools.lru_cache(maxsize=None)
def _baxter(name):
    from diffco_amd import _lib, _ops
    _lib.require_gpu()
    d, desc, kern, sup, W = fixture_model(name)
    m = _ops.ScoreModel(desc, kern[0], kern[1], kern[2], _t(sup), _t(W))
    mg = mixed_margin(d)
    ck = ModelChecker(m, mg if W.shape[1] > 1 else mg[0])
    q = _t(d["q"])
    s = m.score_raw(q)
    free = q[((s - _t(mg)[None]) <= 0).all(dim=1)]
    assert len(free) >= 40
    check = lambda a, b: ck.check_motions(a, b, max_step=B["max_step"], max_samples=200)[0]   # noqa: E731
    pairs = _pairs(check, free, B["R"])
    starts, goals = torch.stack([free[i] for i, _ in pairs]), torch.stack([free[j] for _, j in pairs])
    lim = make_robot(CASE_ROBOT[name]).limits
    return ck, starts, goals, torch.as_tensor(lim, dtype=torch.float32)


@pytest.mark.parametrize("name", ["cfg2_baxter_rq", "cfg3_baxter_rq_c5"])
def test_baxter_fused_equals_host_bit_for_bit(name):
    """cases (b) and (c): 7 DoF, no mask - the partial advance takes motion_coord's fused multiply-add form - one class with a
    margin and five classes with a margin each"""
    from diffco_amd.rrt import host_rrt_connect, rrt_connect
    ck, starts, goals, lim = _baxter(name)
    g = torch.Generator().manual_seed(11)
    lo, span = lim[:, 0], lim[:, 1] - lim[:, 0]
    samples = (lo + span * torch.rand(B["rounds"], B["R"], B["P"], 7, generator=g)).float().cuda()
    kw = dict(range=B["range"], max_step=B["max_step"], slots=B["P"], cap=B["cap"], max_rounds=B["rounds"], rounds_per_call=B["chunk"],
              limits=lim)
    rec = Recorder(ck)
    host = host_rrt_connect(rec, starts, goals, sampler=_fixed(samples), **kw)
    fused = rrt_connect(ck, starts, goals, sampler=_fixed(samples), **kw)
    assert fused.route == "fused" and host.route == "host"
    _assert_same_state(fused, host)
    partial = sum(int((first >= 2).sum()) for qa, qb, first in rec.calls[2::2])
    print(name, "status", fused.status.tolist(), "counts", fused.count.tolist(), "partial advances", partial)
    assert int(fused.count.sum()) > 4 * B["R"] and partial >= 1
    for r, p in enumerate(fused.paths):
        if p is not None:
            assert torch.equal(p[0], starts[r]) and torch.equal(p[-1], goals[r])


def _raw_setup():
    """case (a)'s model, margin, initial state and samples for the raw call"""
    from diffco_amd.rrt import rrt_connect
    d, dc, starts, goals, samples, kw, *_ = case_a()
    init = rrt_connect(dc, starts, goals, sampler=_fixed(samples), **dict(kw, max_rounds=0))
    assert init.status.tolist()[:2] == [3, 1] and init.count.tolist() == [[1, 1]] * A["R"]
    model, margin = dc._rrt_model(torch.device("cuda"))
    run = lambda st, smp, g0: model.rrt_connect_run(st, smp, g0, A["range"], A["max_step"], 47, A["cap"], margin=margin,   # noqa: E731
                                                    wrap=kw["wrap"])
    return init.state(), samples, run


def test_one_call_of_eight_rounds_equals_eight_calls_of_one():
    init, samples, run = _raw_setup()
    one = {k: v.clone() for k, v in init.items()}
    run(one, samples[:8].contiguous(), 0)
    many = {k: v.clone() for k, v in init.items()}
    for t in range(8):
        run(many, samples[t:t + 1].contiguous(), t)
    again = {k: v.clone() for k, v in init.items()}
    run(again, samples[:8].contiguous(), 0)
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(one[k], many[k]) and torch.equal(one[k], again[k]), k
    assert int(one["count"].sum()) > 2 * A["R"] + 8
    # R = 0 and T = 0 launch nothing and change nothing
    run(one, samples[:0].contiguous(), 8)
    for k in STATE:
        assert torch.equal(one[k], again[k]), k


def test_a_captured_call_replays_to_the_eager_result():
    init, samples, run = _raw_setup()
    smp = samples[:4].contiguous()
    want = {k: v.clone() for k, v in init.items()}
    run(want, smp, 0)
    st = {k: v.clone() for k, v in init.items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(st, smp, 0)
    torch.cuda.current_stream().wait_stream(s)
    for k in STATE:
        assert torch.equal(st[k], want[k]), k
    for k in STATE:
        st[k].copy_(init[k])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run(st, smp, 0)
    for _ in range(2):
        for k in STATE:
            st[k].copy_(init[k])
        g.replay()
        torch.cuda.synchronize()
        for k in STATE:
            assert torch.equal(st[k], want[k]), k


def test_routing():
    """DiffCo on the planar arm plans fused; the hybrid facade plans through its own check_motions; where both can run - the
    hybrid with a zero band answers as ForwardKinematicsDiffCo on the same perceptron - the results are equal"""
    from diffco_amd import kernel
    from diffco_amd.collision_checkers import ForwardKinematicsDiffCo, HybridForwardKinematicsDiffCo
    from diffco_amd.rrt import rrt_connect
    from helpers import urdf_robot
    assert case_a()[-1].route == "fused"
    rob = urdf_robot("urdf_panda_nogripper")
    d = load("cfg2_panda_rq")
    w = torch.as_tensor(d["weights"][:300, 0], dtype=torch.float32)

    def facade(cls, **extra):
        ck = cls(robot=rob, gamma=10, **extra)
        p = ck.perceptron
        p.support_points = torch.as_tensor(d["sup_q"][:300], dtype=torch.float32).cuda()
        p.support_transformed = rob.fkine(p.support_points)
        p.rbf_kernel = kernel.Polyharmonic(1, 1.0)
        p.rbf_nodes = (w - w.mean()).cuda()
        ck.safety_bias = 0.0
        return ck

    plain = facade(ForwardKinematicsDiffCo)
    hybrid = facade(HybridForwardKinematicsDiffCo, gt_check_func=lambda q: torch.as_tensor(q).reshape(-1, 7)[:, 0] > 0)
    torch.manual_seed(6)
    q = rob.rand_configs(400).cuda()
    free = q[~plain.collision(q).reshape(len(q), -1).any(dim=1)]
    assert len(free) >= 40
    pairs = _pairs(lambda a, b: plain.check_motions(a, b, max_step=0.25), free, 3)
    starts, goals = torch.stack([free[i] for i, _ in pairs]), torch.stack([free[j] for _, j in pairs])
    out = {}
    for name, ck in (("plain", plain), ("hybrid", hybrid)):
        out[name] = rrt_connect(ck, starts, goals, range=1.5, max_step=0.25, slots=2, cap=32, max_rounds=8, rounds_per_call=4, seed=4)
    assert out["plain"].route == "fused" and out["hybrid"].route == "host"
    _assert_same_state(out["plain"], out["hybrid"])
    assert int(out["plain"].count.sum()) > 2 * 3 and hybrid.last_gt_checks == 0
