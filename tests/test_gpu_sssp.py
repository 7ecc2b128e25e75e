"""GPU: the fused roadmap queries (dcx_sssp_run, dcx_sssp_extract_paths) against the numpy referee bit for bit - dist, pred,
changed, path, count, length - over the lane tail and both sides of a query-block boundary, graphs of 1 to 300 nodes (a chain,
a grid of equal weights, a hub and empty rows, two components, duplicated nodes, extreme weights), every split of the rounds
over calls, a captured chunk, and Roadmap.query_batch end to end on a DiffCo and on the hybrid Panda checker."""
import numpy as np
import pytest
import torch

from helpers import CASE_ROBOT, case_kernel, load, make_robot, urdf_robot
from sssp_helpers import case, extract_ref, same_bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
CASES = [("single", 3), ("pair", 3), ("pair", 65), ("chain40", 65), ("grid12", 65), ("hub", 65), ("two_components", 130),
         ("extremes70", 64), ("duplicates300", 1), ("duplicates300", 3), ("duplicates300", 64), ("duplicates300", 65),
         ("duplicates300", 130), ("knn300", 65)]


def _d(c, *names):
    return [torch.from_numpy(c[n]).cuda() for n in names]


def _state(c, Q):
    # (garbage, not zeros: round 0 must set all of it)
    return (torch.full((2, c["n"], Q), -3.0, device="cuda"), torch.full((c["n"], Q), 77, dtype=torch.int32, device="cuda"))


def _relax(c, total, rounds_per_call, links=None):
    """`total` rounds in calls of `rounds_per_call`: (dist [2, N, Q], pred, changed [total])"""
    from diffco_amd import _ops
    g = _d(c, "rowptr", "col", "weight")
    si, sl = _d(c, "start_idx", "start_len") if links is None else links
    dist, pred = _state(c, len(si))
    flags, done = [], 0
    while done < total:
        m = min(rounds_per_call, total - done)
        flags.append(_ops.sssp_run(*g, si, sl, dist, pred, done, m))
        done += m
    return dist, pred, torch.cat(flags)


def _extract(c, dist, pred, done, W, out=None, mode=None):
    from diffco_amd import _ops
    g = _d(c, "rowptr", "col", "weight")
    m = _d(c, "mode")[0] if mode is None else mode
    return _ops.sssp_extract_paths(*g, *_d(c, "nodes"), dist, pred, done, m, *_d(c, "starts", "goals", "goal_idx", "goal_len",
                                                                                "direct_len"), W, out=out)


def _same(got, want):
    return all(same_bits(a.cpu().numpy(), b) for a, b in zip(got, want))


@pytest.mark.parametrize("name,Q", CASES)
def test_fused_equals_the_referee(name, Q):
    c = case(name, Q)
    R = c["rounds"]
    total = R + 3                                               # extra rounds after the fixed point change nothing
    dist, pred, changed = _relax(c, total, total)
    want_changed = np.concatenate([c["changed"], np.zeros(3, np.int32)])
    assert same_bits(changed.cpu().numpy(), want_changed)
    assert same_bits(dist[(total - 1) & 1].cpu().numpy(), c["dist"]) and same_bits(pred.cpu().numpy(), c["pred"])
    assert torch.equal(dist[0].view(torch.int32), dist[1].view(torch.int32))
    # the routes: sized by the longest, the sizes alone, and a W some do not fit (their rows stay as they are)
    assert _same(_extract(c, dist, pred, total, c["W"]), (c["path"], c["count"], c["length"]))
    sizes = _extract(c, dist, pred, total, 0)
    assert sizes[0].shape == (Q, 0, 3) and same_bits(sizes[1].cpu().numpy(), c["sizes"]) and same_bits(sizes[2].cpu().numpy(), c["length"])
    small = max(c["W"] - 1, 1)
    before = torch.full((Q, small, 3), 7.0, device="cuda")
    got = _extract(c, dist, pred, total, small, out=before.clone())
    want = extract_ref(c["nodes"], c["dist"], c["pred"], c["mode"], c["starts"], c["goals"], c["goal_idx"], c["goal_len"],
                       c["direct_len"], small, path=before.cpu().numpy())
    assert _same(got, want)
    if c["n"] > 2 and Q >= 64:
        assert (want[1] < 0).any() and (want[1] > 0).any() and set(c["mode"].tolist()) == {0, 1, 2}
    # short of the fixed point: the state after a round is the referee's after that round
    if R > 3:
        from sssp_helpers import sssp_ref
        few = R // 2
        d2, p2, ch2 = _relax(c, few, few)
        want = sssp_ref(c["rowptr"], c["col"], c["weight"], c["start_idx"], c["start_len"], few)
        assert _same((d2[(few - 1) & 1], p2, ch2), want)


@pytest.mark.parametrize("rounds_per_call", [1, 3, 64])
def test_rounds_split_over_calls_give_the_same(rounds_per_call):
    c = case("chain40", 65)
    assert c["rounds"] == 41                                    # a round per hop, and the one that changes nothing
    dist, pred, changed = _relax(c, 64, rounds_per_call)
    assert changed.tolist() == [1] * 40 + [0] * 24
    assert same_bits(dist[1].cpu().numpy(), c["dist"]) and same_bits(dist[0].cpu().numpy(), c["dist"])
    assert same_bits(pred.cpu().numpy(), c["pred"])
    assert _same(_extract(c, dist, pred, 64, c["W"]), (c["path"], c["count"], c["length"]))


def test_no_start_link_at_all():
    c = case("knn300", 65)
    none = torch.full((65, 4), -1, dtype=torch.int32, device="cuda")
    for per_call in (6, 1):
        dist, pred, changed = _relax(c, 6, per_call, links=(none, _d(c, "start_len")[0]))
        assert changed.tolist() == [0] * 6 and bool(torch.isinf(dist).all()) and bool((dist > 0).all()) and bool((pred == -1).all())
    path, count, length = _extract(c, dist, pred, 6, 4, mode=torch.full((65,), 2, dtype=torch.int32, device="cuda"))
    assert not count.any() and bool(torch.isinf(length).all()) and not path.any()


def test_a_captured_chunk_replays():
    from diffco_amd import _ops
    c = case("duplicates300", 65)
    total = c["rounds"] + 1
    g = _d(c, "rowptr", "col", "weight")
    si, sl = _d(c, "start_idx", "start_len")
    ex = _d(c, "mode", "starts", "goals", "goal_idx", "goal_len", "direct_len")
    nodes = _d(c, "nodes")[0]
    dist, pred = _state(c, 65)
    changed = torch.zeros(total, dtype=torch.int32, device="cuda")
    out = torch.zeros((65, c["W"], 3), device="cuda")

    def chunk():
        _ops.sssp_run(*g, si, sl, dist, pred, 0, total, changed=changed)
        return _ops.sssp_extract_paths(*g, nodes, dist, pred, total, *ex, c["W"], out=out)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chunk()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        _, count, length = chunk()
    for _ in range(2):
        dist.fill_(-3.0)
        pred.fill_(77)
        changed.fill_(5)
        out.fill_(9.0)
        count.fill_(-9)
        length.fill_(-9.0)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(changed.cpu().numpy(), np.concatenate([c["changed"], np.zeros(1, np.int32)]))
        assert same_bits(dist[(total - 1) & 1].cpu().numpy(), c["dist"]) and same_bits(pred.cpu().numpy(), c["pred"])
        want = extract_ref(c["nodes"], c["dist"], c["pred"], c["mode"], c["starts"], c["goals"], c["goal_idx"], c["goal_len"],
                           c["direct_len"], c["W"], path=np.full((65, c["W"], 3), 9.0, np.float32))
        assert _same((out, count, length), want)


def test_wrappers_refuse_what_does_not_fit():
    from diffco_amd import _ops
    c = case("pair", 3)
    g = _d(c, "rowptr", "col", "weight")
    si, sl = _d(c, "start_idx", "start_len")
    dist, pred = _state(c, 3)
    with pytest.raises(ValueError, match="pred must be"):
        _ops.sssp_run(*g, si, sl, dist, pred[:, :2], 0, 1)
    with pytest.raises(ValueError, match="link_len must be"):
        _ops.sssp_run(*g, si, sl.double(), dist, pred, 0, 1)
    with pytest.raises(ValueError, match="rowptr must be"):
        _ops.sssp_run(g[0].cpu(), g[1], g[2], si, sl, dist, pred, 0, 1)
    with pytest.raises(ValueError, match="round0 and n_rounds"):
        _ops.sssp_run(*g, si, sl, dist, pred, -1, 1)
    with pytest.raises(ValueError, match="rounds_done >= 1"):
        _extract(c, dist, pred, 0, 2)


# ------------------------------------------------------------------------------------------------ end to end
N_NODES, K, Q_PAIRS = 512, 8, 70


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")


def _planar():
    from diffco_amd import _lib, kernel
    from diffco_amd.kernel_perceptrons import DiffCo
    _lib.require_gpu()
    name = "cfg1_planar2_rq"
    d = load(name)
    kind, p0, p1 = case_kernel(d)
    assert kind == 0
    rob = make_robot(CASE_ROBOT[name])
    dc = DiffCo(kernel_func=kernel.RQKernel(p0, p1), transform=rob.fkine)
    dc.support_points = _t(d["sup_q"])
    dc.support_transformed = rob.fkine(dc.support_points)
    dc.gains = _t(d["weights"][:, 0])
    g = torch.Generator().manual_seed(3)
    nodes = ((torch.rand(N_NODES, 2, generator=g) * 2 - 1) * np.pi).float().cuda()
    return dc, dc.is_collision, rob.wrap_mask, nodes, 0.1


def _hybrid():
    from diffco_amd import _lib, kernel
    from diffco_amd.collision_checkers import HybridForwardKinematicsDiffCo
    _lib.require_gpu()
    rob = urdf_robot("urdf_panda_nogripper")
    d = load("cfg2_panda_rq")
    ck = HybridForwardKinematicsDiffCo(robot=rob, gamma=10, gt_check_func=lambda q: torch.as_tensor(q).reshape(-1, 7)[:, 0] > 0)
    p = ck.perceptron
    w = torch.as_tensor(d["weights"][:300, 0], dtype=torch.float32)
    p.support_points = torch.as_tensor(d["sup_q"][:300], dtype=torch.float32).cuda()
    p.support_transformed = rob.fkine(p.support_points)
    p.rbf_kernel = kernel.Polyharmonic(1, 1.0)
    p.rbf_nodes = (w - w.mean()).cuda()
    torch.manual_seed(5)
    ck.safety_bias = float(ck._calculate_safety_bias(rob.rand_configs(600).cuda()))
    torch.manual_seed(6)
    return ck, ck.collision, rob.wrap_mask, rob.rand_configs(N_NODES).cuda(), 0.25


def _hard_pair(check, nodes, graph):
    """two nodes of the roadmap's largest component whose direct motion the checker refuses, the farthest such pair of a sample"""
    from scipy.sparse.csgraph import connected_components
    _, label = connected_components(graph, directed=False)
    big = np.flatnonzero(label == np.bincount(label).argmax())
    assert len(big) >= 40
    pick = torch.as_tensor(big[np.random.default_rng(0).choice(len(big), 40, replace=False)], device=nodes.device)
    a, b = torch.triu_indices(40, 40, 1, device=nodes.device)
    hit = check(nodes[pick[a]], nodes[pick[b]])
    assert bool(hit.any())
    far = (nodes[pick[a]] - nodes[pick[b]]).norm(dim=1) * hit
    i = int(far.argmax())
    return int(pick[a[i]]), int(pick[b[i]])


@pytest.mark.parametrize("make", [_planar, _hybrid], ids=["planar2_diffco", "panda_hybrid"])
def test_query_batch_end_to_end(make):
    from diffco_amd import _ops
    from diffco_amd.roadmap import Roadmap
    from diffco_amd.shortcut import shortcut_paths
    ck, collides, mask, nodes, step = make()
    check = lambda a, b: torch.as_tensor(ck.check_motions(a, b, max_step=step, wrap=True)).to("cuda")   # noqa: E731
    rm = Roadmap.build(ck, nodes, K, step, wrap=True)
    n = len(rm.nodes)
    # the pairs: two free configurations beside two roadmap nodes whose direct motion collides, a colliding endpoint, the two
    # ends of a roadmap edge (their direct motion is free), and nodes of the roadmap moved a little
    ia, ib = _hard_pair(check, rm.nodes, rm.graph)
    ends = None
    for eps in (1e-3, -1e-3, 2e-3, -2e-3):
        cand_ends = rm.nodes[[ia, ib]] + eps
        if not bool(collides(cand_ends).any()) and bool(check(cand_ends[:1], cand_ends[1:])[0]):
            ends = cand_ends
            break
    assert ends is not None
    free = ~collides(nodes).reshape(N_NODES, -1).any(dim=1)
    bad = nodes[(~free).nonzero()[0, 0]]
    g = torch.Generator().manual_seed(11)
    pick = torch.randint(0, n, (2, Q_PAIRS), generator=g).cuda()
    starts, goals = rm.nodes[pick[0]] + 1e-3, rm.nodes[pick[1]] - 1e-3
    starts[0], goals[0] = ends[0], ends[1]
    starts[1] = bad
    goals[2] = bad
    starts[3], goals[3] = rm.nodes[rm.edges[0, 0]], rm.nodes[rm.edges[0, 1]]

    res = rm.query_batch(starts, goals)
    assert res.route == "fused" and res.path.dtype == torch.float32 and res.path.is_cuda
    assert res.mode.tolist()[:4] == [2, 0, 0, 1] and 2 <= res.rounds <= n
    host = rm.query_batch(starts, goals, route="host")
    assert host.route == "host" and host.rounds == res.rounds
    for a, b in ((res.path, host.path), (res.count, host.count), (res.length, host.length), (res.mode, host.mode)):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the split of the rounds over calls and a given W change nothing
    again = rm.query_batch(starts, goals, rounds_per_call=1, max_waypoints=res.path.shape[1])
    assert torch.equal(again.path, res.path) and torch.equal(again.count, res.count) and again.rounds == res.rounds

    paths = res.paths()
    have = {tuple(x) for x in rm.edges.cpu().tolist()}
    routed, seg = 0, []
    for q in range(Q_PAIRS):
        single = rm.query(starts[q], goals[q])
        if single is None:
            assert paths[q] is None and int(res.count[q]) == 0 and bool(torch.isinf(res.length[q])), q
            continue
        p1, l1 = single
        p = paths[q]
        assert p is not None and len(p) == int(res.count[q]) and torch.equal(p[0], starts[q]) and torch.equal(p[-1], goals[q])
        assert (len(p) == 2) == (len(p1) == 2) == (int(res.mode[q]) == 1)
        hops = max(len(p), len(p1)) - 1
        assert hops < 100
        assert abs(float(res.length[q]) - l1) <= (hops + 1) * U * l1, (q, float(res.length[q]), l1)
        if len(p) > 2:
            routed += 1
            inner = [int((rm.nodes == w).all(dim=1).nonzero()[0, 0]) for w in p[1:-1]]
            assert all((min(a, b), max(a, b)) in have for a, b in zip(inner, inner[1:]))
            seg += [(starts[q], p[1]), (goals[q], p[-2])]
            seg += [(rm.nodes[min(a, b)], rm.nodes[max(a, b)]) for a, b in zip(inner, inner[1:])]
        else:
            seg.append((starts[q], goals[q]))
    assert routed >= 10 and paths[0] is not None and len(paths[0]) > 2 and paths[1] is None and paths[2] is None and len(paths[3]) == 2
    # every segment of every route passes the checker, in one call: each in the direction the roadmap checked it (the samples
    # of a motion are laid from its first end, so the two directions of an edge are two checks)
    assert not bool(check(torch.stack([s[0] for s in seg]), torch.stack([s[1] for s in seg])).any())
    # the result goes into the shortcutter as it is
    short = shortcut_paths(ck, res.path, res.count, max_step=step, wrap=mask, rounds=8)
    assert all(0 <= a <= b for a, b in zip(short.count.tolist(), res.count.tolist()))
    for q in range(Q_PAIRS):
        m = int(short.count[q])
        if m:
            assert torch.equal(short.path[q, 0].cpu(), res.path[q, 0].cpu())
            assert torch.equal(short.path[q, m - 1].cpu(), res.path[q, int(res.count[q]) - 1].cpu())
