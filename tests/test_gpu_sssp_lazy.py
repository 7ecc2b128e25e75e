"""GPU: the fused lazy roadmap queries (dcx_sssp_mark_routes, dcx_graph_apply_checks) against the numpy referee bit for bit -
pending, list, qa, qb, n_out, the edges' state, the weights - over the lane tail and both sides of a query-block boundary, every
graph of the referee, capacities 1, 2 and M, with garbage in whatever the calls must set; whole relax - mark - check - apply loops;
a captured pass; and Roadmap.build(lazy=True).query_batch end to end on a DiffCo and on the hybrid Panda checker."""
import numpy as np
import pytest
import torch

from sssp_helpers import case, same_bits
from sssp_lazy_helpers import LAZY_GRAPHS, apply_ref, lazy_graph, loop_case, mark_ref, verdicts

pytestmark = pytest.mark.gpu

QS = (1, 3, 64, 65, 130)


def _d(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _graph(g, weight=None, state=None):
    """the CSR and the edges' arrays of a referee graph on the GPU: ((rowptr, col, weight), (eid, ent, ends, state))"""
    weight = g["weight"] if weight is None else weight
    state = np.zeros(g["M"], np.uint8) if state is None else state
    return tuple(_d(g["rowptr"], g["col"], weight.copy())), tuple(_d(g["eid"], g["ent"], g["ends"], state.copy()))


def _state(c, rounds_done):
    """dist [2, N, Q] with the referee's distances in the buffer the last round wrote and garbage in the other, and pred"""
    dist = torch.full((2,) + c["dist"].shape, -3.0, device="cuda")
    dist[(rounds_done - 1) & 1] = _d(c["dist"])[0]
    return dist, _d(c["pred"])[0]


def _garbage(Q, cap, dof=3):
    return (torch.full((Q,), 77, dtype=torch.int32, device="cuda"), torch.full((cap,), -5, dtype=torch.int32, device="cuda"),
            torch.full((cap, dof), 9.0, device="cuda"), torch.full((cap, dof), -9.0, device="cuda"),
            torch.full((2,), -3, dtype=torch.int32, device="cuda"))


def _np(tensors):
    return [t.cpu().numpy() for t in tensors]


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("name", LAZY_GRAPHS)
def test_fused_pass_equals_the_referee(name, Q):
    from diffco_amd import _lib, _ops
    c, g = case(name, Q), lazy_graph(name)                       # every mode, the relaxation's fixed point
    M = g["M"]
    state = np.array([1 if m % 5 == 3 else 0 for m in range(M)], np.uint8)
    nodes, mode, gi, gl = _d(c["nodes"], c["mode"], c["goal_idx"], c["goal_len"])
    work = torch.full((int(_lib.load().dcx_sssp_mark_routes_work_bytes(M)),), 0xAB, dtype=torch.uint8, device="cuda")
    for rounds_done, cap in zip((c["rounds"], c["rounds"] + 1, c["rounds"]), sorted({1, 2, M})):
        csr, lz = _graph(g, state=state)
        dist, pred = _state(c, rounds_done)
        before = _garbage(Q, cap)
        want = mark_ref(g, state, c["nodes"], c["dist"], c["pred"], c["mode"], c["goal_idx"], c["goal_len"], cap,
                        before=_np(before[1:4]))
        got = _ops.sssp_mark_routes(*csr, lz, nodes, dist, pred, rounds_done, mode, gi, gl, cap, out=before, work=work)
        assert all(a is b for a, b in zip(got, before))
        assert all(same_bits(a, b) for a, b in zip(_np(got), want)), (cap, _np(got)[4], want[4])
        assert same_bits(lz[3].cpu().numpy(), state) and same_bits(csr[2].cpu().numpy(), g["weight"])   # a mark pass writes neither
        total, n = want[4]
        hit = np.ones(cap, np.uint8)                             # (beyond n: verdicts nobody may read)
        hit[:n] = verdicts(want[1][:n])
        w_want, s_want, any_want = apply_ref(g, g["weight"], state, want[1], want[4], hit)
        flag = torch.full((1,), 5, dtype=torch.int32, device="cuda")
        assert _ops.graph_apply_checks(*csr, lz, got[1], got[4], _d(hit)[0], any_blocked=flag) is flag
        assert same_bits(csr[2].cpu().numpy(), w_want) and same_bits(lz[3].cpu().numpy(), s_want)
        assert same_bits(flag.cpu().numpy(), any_want)
        assert int((s_want != state).sum()) == n                 # truncation: the first ids are settled, the rest stay unknown
    # fresh outputs, a bool hit, and the workspace the wrapper takes itself
    csr, lz = _graph(g, state=state)
    dist, pred = _state(c, c["rounds"])
    fresh = _ops.sssp_mark_routes(*csr, lz, nodes, dist, pred, c["rounds"], mode, gi, gl, M)
    want = mark_ref(g, state, c["nodes"], c["dist"], c["pred"], c["mode"], c["goal_idx"], c["goal_len"], M)
    assert all(same_bits(a, b) for a, b in zip(_np(fresh), want))
    _ops.graph_apply_checks(*csr, lz, fresh[1], fresh[4], torch.zeros(M, dtype=torch.bool, device="cuda"))
    assert int((lz[3] == 1).sum()) == int((state == 1).sum()) + int(want[4][1]) and not bool(torch.isinf(csr[2]).any())


def _fused_loop(name, Q, cap):
    """the loop of Roadmap.query_batch's fused route on the referee's graph, the verdict rule in the checker's place"""
    from diffco_amd import _ops
    g = lazy_graph(name)
    c = loop_case(name, Q, False, None if cap == g["M"] else cap)
    csr, lz = _graph(g)
    nodes, si, sl, gi, gl, mode = _d(c["nodes"], c["start_idx"], c["start_len"], c["goal_idx"], c["goal_len"], c["mode"])
    N = g["n"]
    dist = torch.full((2, N, Q), -3.0, device="cuda")
    pred = torch.full((N, Q), 77, dtype=torch.int32, device="cuda")
    out = _garbage(Q, cap)
    hit = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    iters = checked = 0
    while True:
        done = 0
        while True:
            flags = _ops.sssp_run(*csr, si, sl, dist, pred, done, 8).tolist()
            done += 8
            if 0 in flags:
                break
        pending, lst, _, _, n_out = _ops.sssp_mark_routes(*csr, lz, nodes, dist, pred, done, mode, gi, gl, cap, out=out)
        want = c["passes"][iters]
        total, n = n_out.tolist()
        assert same_bits(pending.cpu().numpy(), want[0]) and [total, n] == want[2].tolist()
        assert same_bits(lst[:n].cpu().numpy(), want[1][:n])
        iters += 1
        if total == 0:
            break
        hit[:n] = _d(verdicts(want[1][:n]))[0]
        _ops.graph_apply_checks(*csr, lz, lst, n_out, hit)
        checked += n
    assert iters == c["iters"] and checked == c["checked"]
    assert same_bits(csr[2].cpu().numpy(), c["weight"]) and same_bits(lz[3].cpu().numpy(), c["state"])
    got = _ops.sssp_extract_paths(*csr, nodes, dist, pred, done, mode, *_d(c["starts"], c["goals"]), gi, gl, _d(c["direct_len"])[0], c["W"])
    assert all(same_bits(a, b) for a, b in zip(_np(got), (c["path"], c["count"], c["length"])))


@pytest.mark.parametrize("name", LAZY_GRAPHS)
def test_whole_fused_loops_equal_the_referee(name):
    M = lazy_graph(name)["M"]
    _fused_loop(name, 65, M)
    if M <= 300:                                                 # (a pass per edge: the small graphs)
        for cap in (1, 2):
            _fused_loop(name, 3, cap)


def test_a_captured_pass_replays():
    from diffco_amd import _lib, _ops
    name, Q = "duplicates300", 65
    c, g = loop_case(name, Q), lazy_graph(name)
    M = g["M"]
    # the first pass of the loop: every edge unknown, the relaxation's fixed point over all candidates
    first = case(name, Q, False)
    want = mark_ref(g, np.zeros(M, np.uint8), first["nodes"], first["dist"], first["pred"], first["mode"], first["goal_idx"],
                    first["goal_len"], M, before=[np.full(M, -5, np.int32), np.full((M, 3), 9.0, np.float32), np.full((M, 3), -9.0, np.float32)])
    assert same_bits(want[1][:want[4][1]], c["passes"][0][1][:want[4][1]]) and want[4][0] > 50
    hit_np = np.ones(M, np.uint8)
    hit_np[:want[4][1]] = verdicts(want[1][:want[4][1]])
    w_want, s_want, any_want = apply_ref(g, g["weight"], np.zeros(M, np.uint8), want[1], want[4], hit_np)
    csr, lz = _graph(g)
    nodes, mode, gi, gl, hit = _d(first["nodes"], first["mode"], first["goal_idx"], first["goal_len"], hit_np)
    dist, pred = _state(first, first["rounds"])
    out = _garbage(Q, M)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    work = torch.empty(int(_lib.load().dcx_sssp_mark_routes_work_bytes(M)), dtype=torch.uint8, device="cuda")

    def one_pass():
        _ops.sssp_mark_routes(*csr, lz, nodes, dist, pred, first["rounds"], mode, gi, gl, M, out=out, work=work)
        _ops.graph_apply_checks(*csr, lz, out[1], out[4], hit, any_blocked=flag)

    def reset():
        csr[2].copy_(_d(g["weight"])[0])
        lz[3].zero_()
        for t, v in zip(out, (77, -5, 9.0, -9.0, -3)):
            t.fill_(v)
        work.fill_(0xAB)
        flag.fill_(5)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        one_pass()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        one_pass()
    for _ in range(2):
        reset()
        graph.replay()
        torch.cuda.synchronize()
        assert all(same_bits(a, b) for a, b in zip(_np(out), want))
        assert same_bits(csr[2].cpu().numpy(), w_want) and same_bits(lz[3].cpu().numpy(), s_want)
        assert same_bits(flag.cpu().numpy(), any_want) and any_want[0] == 1


def test_wrappers_refuse_what_does_not_fit():
    from diffco_amd import _ops
    c, g = case("pair", 3), lazy_graph("pair")
    csr, lz = _graph(g)
    nodes, mode, gi, gl = _d(c["nodes"], c["mode"], c["goal_idx"], c["goal_len"])
    dist, pred = _state(c, c["rounds"])
    args = (nodes, dist, pred, c["rounds"], mode, gi, gl)
    with pytest.raises(ValueError, match="ent must be"):
        _ops.sssp_mark_routes(*csr, (lz[0], lz[1].long(), lz[2], lz[3]), *args, 1)
    with pytest.raises(ValueError, match="the edges' state must be"):
        _ops.sssp_mark_routes(*csr, (lz[0], lz[1], lz[2], lz[3].int()), *args, 1)
    with pytest.raises(ValueError, match="capacity must be >= 0"):
        _ops.sssp_mark_routes(*csr, lz, *args, -1)
    with pytest.raises(ValueError, match="work must be"):
        _ops.sssp_mark_routes(*csr, lz, *args, 1, work=torch.zeros(8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="list must be"):
        _ops.sssp_mark_routes(*csr, lz, *args, 1, out=_garbage(3, 2))
    out = _ops.sssp_mark_routes(*csr, lz, *args, 1)
    with pytest.raises(ValueError, match="hit must be"):
        _ops.graph_apply_checks(*csr, lz, out[1], out[4], torch.zeros(2, dtype=torch.uint8, device="cuda"))
    # a capacity of 0 counts alone
    counted = _ops.sssp_mark_routes(*csr, lz, *args, 0)
    assert counted[4].tolist() == [out[4].tolist()[0], 0] and counted[1].shape == (0,)


# ------------------------------------------------------------------------------------------------ end to end
class _Counting:
    """a checker as a roadmap sees it, with what its calls cost: the edges checked and the ground-truth samples"""

    def __init__(self, ck):
        self.ck = ck
        self.transform, self.perceptron = getattr(ck, "transform", None), getattr(ck, "perceptron", None)
        self.motion_calls = self.edges = self.gt = 0

    def collision(self, q):
        hit = (getattr(self.ck, "is_collision", None) or self.ck.collision)(q)
        self.gt += getattr(self.ck, "last_gt_checks", 0)
        return hit

    def check_motions(self, a, b, **kw):
        hit = self.ck.check_motions(a, b, **kw)
        self.motion_calls += 1
        self.edges += len(a)
        self.gt += getattr(self.ck, "last_gt_checks", 0)
        return hit


def _route_edges(rm, res):
    ids = {tuple(e): m for m, e in enumerate(rm.edges.cpu().tolist())}
    out = []
    for p in res.paths():
        if p is not None and len(p) > 2:
            inner = [int((rm.nodes == w).all(dim=1).nonzero()[0, 0]) for w in p[1:-1]]
            out += [ids[(min(a, b), max(a, b))] for a, b in zip(inner, inner[1:])]
    return out


@pytest.mark.parametrize("which", ["planar2_diffco", "panda_hybrid"])
def test_lazy_query_batch_end_to_end(which):
    from test_gpu_sssp import K, Q_PAIRS, _hybrid, _planar
    from diffco_amd.roadmap import Roadmap
    ck, _, _, nodes, step = (_planar if which == "planar2_diffco" else _hybrid)()
    lazy_ck, eager_ck = _Counting(ck), _Counting(ck)
    lazy = Roadmap.build(lazy_ck, nodes, K, step, wrap=True, lazy=True)
    M = len(lazy.edges)
    assert lazy_ck.motion_calls == 0 and lazy.lazy and lazy.edge_state.is_cuda and not lazy.edge_state.any()
    n = len(lazy.nodes)
    pick = torch.randint(0, n, (2, Q_PAIRS), generator=torch.Generator().manual_seed(11)).cuda()
    starts, goals = lazy.nodes[pick[0]] + 1e-3, lazy.nodes[pick[1]] - 1e-3

    res = lazy.query_batch(starts, goals)
    assert res.route == "fused" and bool(res.settled.all()) and res.iters > 1
    assert 0 < res.checked == int((lazy.edge_state != 0).sum()) < M
    assert lazy_ck.edges == res.checked + Q_PAIRS + 2 * Q_PAIRS * K and lazy_ck.motion_calls == 2 + res.iters - 1
    # the host route on a roadmap of its own learns the same and answers the same
    other = Roadmap.build(ck, nodes, K, step, wrap=True, lazy=True)
    host = other.query_batch(starts, goals, route="host")
    assert (host.iters, host.checked) == (res.iters, res.checked) and torch.equal(other.edge_state, lazy.edge_state)
    assert torch.equal(other.csr()[2].view(torch.int32), lazy.csr()[2].view(torch.int32))
    for a, b in ((res.path, host.path), (res.count, host.count), (res.length, host.length), (res.settled, host.settled)):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    # (i), (ii): everything checked changes no length, and then the roadmap answers as the eager one, bit for bit
    eager = Roadmap.build(eager_ck, nodes, K, step, wrap=True)
    want = eager.query_batch(starts, goals)
    assert other.validate() == M - res.checked and torch.equal(other.edges[other.edge_state == 1], eager.edges)
    after = other.query_batch(starts, goals)
    assert (after.iters, after.checked) == (1, 0)
    assert torch.equal(res.length.view(torch.int32), after.length.view(torch.int32))
    for a, b in ((after.path, want.path), (after.count, want.count), (after.length, want.length), (res.path, want.path)):
        assert torch.equal(a, b)
    assert int((res.count > 2).sum()) >= 10
    # (iii), (iv): the routes stand on edges known free, and no state contradicts the checker
    used = _route_edges(lazy, res)
    assert len(used) > 20 and bool((lazy.edge_state[used] == 1).all())
    known = (lazy.edge_state != 0).nonzero().reshape(-1)
    hit = torch.as_tensor(ck.check_motions(lazy.nodes[lazy.edges[known, 0]], lazy.nodes[lazy.edges[known, 1]], max_step=step, wrap=True))
    assert torch.equal(lazy.edge_state[known] == 2, hit.to("cuda").reshape(-1))
    # what it saves: the edges an eager build checks and these queries never touch, and the ground-truth samples on them
    print(f"{which}: {res.checked} of {M} edges checked in {res.iters} passes; ground-truth samples lazy {lazy_ck.gt}, eager {eager_ck.gt}")
    assert eager_ck.edges == M + Q_PAIRS + 2 * Q_PAIRS * K and lazy_ck.edges < eager_ck.edges
    assert lazy_ck.gt <= eager_ck.gt
    if which == "panda_hybrid":
        assert eager_ck.gt > 0
    # forgetting and asking again gives the same answers for the same checks
    lazy.invalidate()
    assert not lazy.edge_state.any() and not bool(torch.isinf(lazy.csr()[2]).any())
    again = lazy.query_batch(starts, goals)
    assert torch.equal(again.path, res.path) and (again.iters, again.checked) == (res.iters, res.checked)
