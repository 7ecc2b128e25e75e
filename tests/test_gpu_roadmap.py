"""GPU: Roadmap end to end on real checkers - a DiffCo on the 2-DoF planar arm's fixture (every joint on the circle: wrap=True)
and a HybridForwardKinematicsDiffCo on the URDF Panda arm whose ground truth is a Python function.  The kept edges are those of
knn_edges and check_motions composed by hand, every segment of a returned path passes check_motions, and the path's length is
that of the test's own Dijkstra."""
import numpy as np
import pytest
import torch

from helpers import CASE_ROBOT, case_kernel, load, make_robot, urdf_robot

pytestmark = pytest.mark.gpu

N_NODES, K = 512, 8


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
def test_roadmap_end_to_end(make):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    from diffco_amd import _ops
    from diffco_amd.roadmap import Roadmap, knn_edges
    ck, collides, mask, nodes, step = make()
    check = lambda a, b: torch.as_tensor(ck.check_motions(a, b, max_step=step, wrap=True)).to("cuda")   # noqa: E731
    rm = Roadmap.build(ck, nodes, K, step, wrap=True)
    assert rm.wrap_mask == mask

    # by hand: the free nodes, their candidate edges, one check_motions call
    free = ~collides(nodes).reshape(N_NODES, -1).any(dim=1)
    kept = free.nonzero().reshape(-1)
    assert 100 < len(kept) < N_NODES and torch.equal(rm.kept, kept) and torch.equal(rm.nodes, nodes[kept])
    cand = knn_edges(nodes[kept], K, wrap=mask)
    hit = check(nodes[kept][cand[:, 0]], nodes[kept][cand[:, 1]])
    assert 0 < int(hit.sum()) < len(cand)
    assert torch.equal(rm.edges, cand[~hit])
    lengths = _ops.wrapped_delta(rm.nodes[rm.edges[:, 0]], rm.nodes[rm.edges[:, 1]], mask).norm(dim=1)
    assert torch.equal(rm.lengths, lengths)
    n = len(rm.nodes)
    assert rm.graph.shape == (n, n) and rm.graph.nnz == 2 * len(rm.edges) and abs(rm.graph - rm.graph.T).sum() == 0

    # a query between two free configurations just beside two roadmap nodes whose direct motion collides
    ia, ib = _hard_pair(check, rm.nodes, rm.graph)
    ends = None
    for eps in (1e-3, -1e-3, 2e-3, -2e-3):
        cand_ends = rm.nodes[[ia, ib]] + eps
        if not bool(collides(cand_ends).any()) and bool(check(cand_ends[:1], cand_ends[1:])[0]):
            ends = cand_ends
            break
    assert ends is not None
    out = rm.query(ends[0], ends[1])
    assert out is not None
    path, length = out
    assert torch.equal(path[0], ends[0]) and torch.equal(path[-1], ends[1]) and len(path) > 2
    assert not bool(check(path[:-1], path[1:]).any())
    seg = _ops.wrapped_delta(path[:-1], path[1:], mask).norm(dim=1)
    assert length == pytest.approx(float(seg.double().sum()), rel=1e-6)
    # the test's own Dijkstra: the roadmap's edges, and each endpoint's free edges to its K nearest nodes
    idx, _ = _ops.knn(ends, rm.nodes, K, wrap=mask)
    e = torch.arange(2, device="cuda").repeat_interleave(K)
    j = idx.reshape(-1).long()
    ok = ~check(ends[e], rm.nodes[j])
    w = _ops.wrapped_delta(ends[e], rm.nodes[j], mask).norm(dim=1)[ok].double().cpu().numpy()
    ii = np.concatenate([rm.edges[:, 0].cpu().numpy(), n + e[ok].cpu().numpy()])
    jj = np.concatenate([rm.edges[:, 1].cpu().numpy(), j[ok].cpu().numpy()])
    ww = np.concatenate([rm.lengths.double().cpu().numpy(), w])
    own = dijkstra(csr_matrix((ww, (ii, jj)), shape=(n + 2, n + 2)), directed=False, indices=n)[n + 1]
    assert np.isfinite(own) and length == pytest.approx(float(own), rel=1e-9)
    # the inner waypoints are roadmap nodes, consecutive ones joined by roadmap edges
    inner = [int((rm.nodes == p).all(dim=1).nonzero()[0, 0]) for p in path[1:-1]]
    have = {tuple(x) for x in rm.edges.cpu().tolist()}
    assert all((min(a, b), max(a, b)) in have for a, b in zip(inner, inner[1:]))

    # a colliding endpoint: nothing; the nearest node of a batch: knn with k = 1
    bad = nodes[(~free).nonzero()[0, 0]]
    assert rm.query(bad, ends[1]) is None and rm.query(ends[0], bad) is None
    i1, d1 = rm.nearest(ends)
    assert i1.tolist() == [ia, ib] and torch.equal(i1, idx[:, 0])
