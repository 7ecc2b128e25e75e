"""GPU: differentiable motion costs (dcx_motion_cost, ScoreModel.motion_cost_raw / motion_cost / path_cost and the facades')
against the fp64 oracle with the chain rule formed on the host, against score_hinge_grad_raw on the same fp32 points, over
edge shapes (tiles spanning edges, zero-length edges, edges over max_samples, launch forms), several classes, autograd through
utils.dense_path, check_motions, determinism, graph capture and the host route of a foreign transform."""
import numpy as np
import pytest
import torch

from helpers import CASE_ROBOT, case_kernel, desc_for, load, make_robot
from helpers import motion_chain as _chain
from helpers import motion_oracle_cost as _oracle
from helpers import motion_samples as _samples

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def ops():
    from diffco_amd import _lib, _ops
    _lib.require_gpu()
    return _ops


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")


def _case(ops, name, weights=None):
    d = load(name)
    kind, p0, p1 = case_kernel(d)
    desc = desc_for(CASE_ROBOT[name], dof=d["q"].shape[1])
    sup = d["sup_x32"].reshape(len(d["sup_x32"]), -1) if "sup_x32" in d.files and CASE_ROBOT[name] else d["sup_q"]
    sup = np.asarray(sup, dtype=F).reshape(len(sup), -1)
    W = np.asarray(d["weights"] if weights is None else weights, F)
    m = ops.ScoreModel(desc, kind, p0, p1, _t(sup), _t(W))
    return d, m, desc, (kind, p0, p1), sup, W


def _edges(q, E, seed, scale=1.0):
    g = np.random.default_rng(seed)
    i, j = g.integers(0, len(q), E), g.integers(0, len(q), E)
    qa = q[i].astype(F)
    qb = (qa + scale * (q[j] - qa)).astype(F)
    return qa, qb


def _mixed_margin(d):
    C = d["score64"].shape[1]
    return np.percentile(d["score64"], 70 if C == 1 else 95, axis=0).astype(F).tolist()


def _kw(rule, qa, qb):
    if rule == "res":
        return dict(res=11)
    span = float(np.median(np.linalg.norm(qb - qa, axis=1)))
    return dict(max_step=max(span / 12, 1e-3), open_end=(rule == "open"))


def _check(got, ref, tie, what):
    cost, ga, gb = (x.cpu().numpy().astype(np.float64) for x in got[:3])
    rc, rga, rgb, = ref
    keep = ~tie
    assert keep.sum() >= 0.5 * len(keep), what
    scale = max(np.abs(rc).max(), 1e-30)
    assert np.abs(cost - rc).max() <= 1e-5 * scale, (what, np.abs(cost - rc).max(), scale)
    gs = max(np.abs(rga).max(), np.abs(rgb).max(), 1e-30)
    assert np.abs(ga[keep] - rga[keep]).max(initial=0) <= 1e-4 * gs, (what, np.abs(ga[keep] - rga[keep]).max(), gs)
    assert np.abs(gb[keep] - rgb[keep]).max(initial=0) <= 1e-4 * gs, (what, np.abs(gb[keep] - rgb[keep]).max(), gs)


CASES = [("cfg2_baxter_rq", 0.0), ("cfg2_baxter_poly1", "mixed"), ("cfg1_planar2_rq", 0.0), ("cfg2_panda_rq", 0.0),
         ("cfg2_panda_poly1", "mixed")]


@pytest.mark.parametrize("name,margin", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("rule", ["res", "closed", "open"])
def test_cost_and_gradients_match_fp64_oracle(ops, name, margin, rule):
    d, m, desc, kern, sup, W = _case(ops, name)
    if margin == "mixed":
        margin = _mixed_margin(d)
    qa, qb = _edges(d["q"], 200, 1)
    kw = _kw(rule, qa, qb)
    got = m.motion_cost_raw(_t(qa), _t(qb), margin=margin, weight=0.7, max_samples=5000 if rule != "res" else None, **kw)
    smp = _samples(qa, qb, kw.get("res"), kw.get("max_step"), kw.get("open_end", False))
    assert got[3].cpu().numpy().tolist() == [len(p) for p, *_ in smp]
    rc, rga, rgb, tie = _oracle(desc, kern, sup, W, smp, margin, 0.7)
    assert (rc[~tie] > 0).any() and (rc[~tie] == 0).any()
    _check(got, (rc, rga, rgb), tie, (name, rule))


def test_matches_score_hinge_grad_on_materialised_points(ops):
    d, m, desc, kern, sup, W = _case(ops, "cfg2_baxter_poly1")
    mg = _mixed_margin(d)[0]
    qa, qb = _edges(d["q"], 500, 2)
    for rule in ("res", "closed", "open"):
        kw = _kw(rule, qa, qb)
        got = m.motion_cost_raw(_t(qa), _t(qb), margin=mg, weight=1.5, max_samples=5000 if rule != "res" else None, **kw)
        smp = _samples(qa, qb, kw.get("res"), kw.get("max_step"), kw.get("open_end", False))
        flat = np.concatenate([p for p, *_ in smp])
        s, g = m.score_hinge_grad_raw(_t(flat), mg, 1.5)
        h = np.clip(s.cpu().numpy().astype(np.float64)[:, 0] - mg, 0, None)
        rc, rga, rgb = _chain(smp, h, g.cpu().numpy().astype(np.float64), 1.5)
        sv = s.cpu().numpy()[:, 0] - mg
        tie, i = [], 0
        for p, *_ in smp:
            tie.append(bool((np.abs(sv[i:i + len(p)]) <= 1e-4 * np.abs(sv).max()).any()))
            i += len(p)
        _check(got, (rc, rga, rgb), np.array(tie), rule)


def test_edge_shapes(ops):
    d, m, desc, kern, sup, W = _case(ops, "cfg2_baxter_rq")
    q = d["q"].astype(F)
    s = d["score64"][:, 0]
    inside, free = q[s > 0], q[s < 0]
    g = np.random.default_rng(5)
    qa, qb = [inside[0], free[0], inside[1], free[1]], [inside[0], free[0], free[2], inside[2]]   # L = 0 edges first
    step = 0.02
    for n in list(range(1, 70)) + [127, 128, 129, 640, 2000]:
        a = q[g.integers(len(q))]
        dirn = g.normal(size=q.shape[1]).astype(F)
        dirn /= np.linalg.norm(dirn)
        qa.append(a); qb.append((a + dirn * step * (n - 1.5)).astype(F))
    qa, qb = np.stack(qa).astype(F), np.stack(qb).astype(F)
    for open_end in (False, True):
        got = m.motion_cost_raw(_t(qa), _t(qb), max_step=step, open_end=open_end, max_samples=3000)
        smp = _samples(qa, qb, max_step=step, open_end=open_end)
        n = got[3].cpu().numpy()
        assert n.tolist() == [len(p) for p, *_ in smp]
        rc, rga, rgb, tie = _oracle(desc, kern, sup, W, smp, 0.0, 1.0)
        _check(got, (rc, rga, rgb), tie, open_end)
        cost, ga, gb = (x.cpu().numpy() for x in got[:3])
        if open_end:   # zero-length edges: no sample, cost 0
            assert n[0] == 0 and cost[0] == 0 and (ga[0] == 0).all() and (gb[0] == 0).all()
        else:          # the one sample is qb: grad_a 0, grad_b the hinge gradient at qb
            assert n[0] == 1 and cost[0] > 0 and (ga[0] == 0).all() and np.abs(gb[0]).max() > 0 and cost[1] == 0
    # edges over max_samples: NaN (and the counts they would need); the facade raises
    got = m.motion_cost_raw(_t(qa), _t(qb), max_step=step, max_samples=100)
    lens = np.array([len(p) for p, *_ in _samples(qa, qb, max_step=step)])
    cost, ga, gb = (x.cpu().numpy() for x in got[:3])
    assert np.isnan(cost[lens > 100]).all() and np.isnan(ga[lens > 100]).all() and np.isnan(gb[lens > 100]).all()
    assert np.isfinite(cost[lens <= 100]).all() and (got[3].cpu().numpy() == lens).all()
    _, dc, _ = _new_api("cfg2_baxter_rq")
    with pytest.raises(ValueError, match="max_samples"):
        dc.motion_cost(_t(qa), _t(qb), max_step=step, max_samples=100)


@pytest.mark.parametrize("E", [0, 1, 63, 64, 65, 10000])
def test_batch_sizes_and_launch_forms(ops, knob, E):
    d, m, desc, kern, sup, W = _case(ops, "cfg2_baxter_poly1")
    mg = _mixed_margin(d)
    qa, qb = _edges(d["q"], E, 7 + E)
    runs = {}
    for ys, nw in ((-1, -1), (1, 16), (1, 8), (4, 16), (2, 8)):
        knob("ys", ys)
        knob("nw", nw)
        runs[(ys, nw)] = [x.cpu().numpy() for x in m.motion_cost_raw(_t(qa), _t(qb), res=9, margin=mg)[:3]]
    if E == 0:
        assert all(len(v[0]) == 0 for v in runs.values())
        return
    sl = slice(0, E) if E <= 65 else slice(E - 300, E)
    smp = _samples(qa[sl], qb[sl], res=9)
    rc, rga, rgb, tie = _oracle(desc, kern, sup, W, smp, mg, 1.0)
    base = runs[(-1, -1)]
    _check([torch.as_tensor(x[sl]) for x in base], (rc, rga, rgb), tie, E)
    smp = _samples(qa, qb, res=9)
    s = m.score(_t(np.concatenate([p for p, *_ in smp]))).cpu().numpy()[:, 0].reshape(-1, 9) - mg[0]
    tie = (np.abs(s) <= 1e-4 * np.abs(s).max()).any(axis=1)
    for k, v in runs.items():
        sc = max(np.abs(base[0]).max(), 1e-30)
        assert np.abs(v[0][~tie] - base[0][~tie]).max() <= 1e-5 * sc, k
        gs = max(np.abs(base[1]).max(), np.abs(base[2]).max(), 1e-30)
        assert np.abs(v[1][~tie] - base[1][~tie]).max() <= 1e-4 * gs, k
        assert np.abs(v[2][~tie] - base[2][~tie]).max() <= 1e-4 * gs, k


@pytest.mark.parametrize("C", [2, 5, 8])
def test_several_classes(ops, C):
    d5 = load("cfg3_baxter_rq_c5")
    W5 = np.asarray(d5["weights"], F)
    W = np.concatenate([W5] * 2, axis=1)[:, :C] * np.linspace(1.0, 0.6, C, dtype=F)[None]
    d, m, desc, kern, sup, W = _case(ops, "cfg3_baxter_rq_c5", weights=W)
    qa, qb = _edges(d["q"], 300, 21)
    s = m.score(_t(d["q"])).cpu().numpy()
    margin = np.percentile(s, 93, axis=0).astype(F).tolist()
    for rule in ("res", "closed"):
        kw = _kw(rule, qa, qb)
        got = m.motion_cost_raw(_t(qa), _t(qb), margin=margin, weight=2.0, max_samples=5000 if rule != "res" else None, **kw)
        smp = _samples(qa, qb, kw.get("res"), kw.get("max_step"))
        rc, rga, rgb, tie = _oracle(desc, kern, sup, W, smp, margin, 2.0)
        assert (rc[~tie] > 0).any() and (rc[~tie] == 0).any()
        _check(got, (rc, rga, rgb), tie, (C, rule))
    # a free edge set: every tile skips the gradient pass, cost 0 and gradients exactly 0
    big = (np.abs(s).max(axis=0) * 10 + 1).tolist()
    cost, ga, gb, _ = m.motion_cost_raw(_t(qa), _t(qb), res=16, margin=big)
    assert (cost == 0).all() and (ga == 0).all() and (gb == 0).all()


def test_old_api_multidiffco_per_class_margins(ops):
    from diffco_amd import kernel
    from diffco_amd.deprecated import MultiDiffCo
    d, m, desc, kern, sup, W = _case(ops, "cfg3_baxter_rq_c5")
    rob = make_robot(CASE_ROBOT["cfg3_baxter_rq_c5"])
    dc = MultiDiffCo(None)
    dc.support_points = _t(d["sup_q"])
    dc.fkine = rob.fkine
    dc.support_fkine = rob.fkine(dc.support_points)
    dc.rbf_kernel = kernel.RQKernel(kern[1], kern[2])
    dc.rbf_nodes = _t(W)
    qa, qb = _edges(d["q"], 200, 23)
    s = m.score(_t(d["q"])).cpu().numpy()
    margin = np.percentile(s, 93, axis=0).astype(F).tolist()
    cost = dc.motion_cost(_t(qa), _t(qb), res=10, margin=margin)
    assert dc.last_route == "fused"
    ref = m.motion_cost_raw(_t(qa), _t(qb), res=10, margin=margin)[0]
    assert float((cost - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    hit = dc.check_motions(_t(qa), _t(qb), res=10, margin=margin)
    assert int(((cost > 0) != hit).sum()) <= 2 and bool(hit.any()) and not bool(hit.all())


def _new_api(name):
    from diffco_amd import kernel
    from diffco_amd.kernel_perceptrons import DiffCo
    d = load(name)
    kind, p0, p1 = case_kernel(d)
    rob = make_robot(CASE_ROBOT[name])
    kf = kernel.Polyharmonic(int(p0), p1) if kind == 1 else kernel.RQKernel(p0, p1)
    dc = DiffCo(kernel_func=kf, transform=rob.fkine)
    dc.support_points = _t(d["sup_q"])
    dc.support_transformed = rob.fkine(dc.support_points)
    dc.gains = _t(d["weights"][:, 0])
    return d, dc, rob


def test_autograd_and_path_cost(ops):
    from diffco_amd import utils
    d, dc, rob = _new_api("cfg2_baxter_rq")
    qa, qb = _edges(d["q"], 150, 31)
    m = dc._score_fused.model(dc.transform, dc.kernel_func, dc.support_transformed, dc.gains, torch.device("cuda"))
    a, b = _t(qa).requires_grad_(True), _t(qb).requires_grad_(True)
    w = torch.rand(len(qa), device="cuda")
    cost = dc.motion_cost(a, b, max_step=0.1, margin=-0.5, max_samples=5000)
    ga, gb = torch.autograd.grad(cost.mul(w).sum(), (a, b))
    _, rga, rgb, _ = m.motion_cost_raw(_t(qa), _t(qb), max_step=0.1, margin=-0.5, max_samples=5000)
    assert torch.equal(ga, w[:, None] * rga) and torch.equal(gb, w[:, None] * rgb)
    with pytest.raises(RuntimeError):   # no second derivatives
        c = dc.motion_cost(a, b, max_step=0.1, max_samples=5000)
        (g1,) = torch.autograd.grad(c.sum(), (a,), create_graph=True)
        torch.autograd.grad(g1.sum(), (a,))
    # path_cost against autograd through utils.dense_path and the score
    g = np.random.default_rng(3)
    T, Wp = 6, 5
    paths = d["q"][g.integers(0, len(d["q"]), (T, Wp))].astype(F)
    p = _t(paths).requires_grad_(True)
    got = dc.path_cost(p, max_step=0.15, margin=-0.3, weight=0.5)
    (gp,) = torch.autograd.grad(got.sum(), (p,))
    ref, ref_g, checked = [], [], 0
    for i in range(T):
        pi = _t(paths[i]).requires_grad_(True)
        pts = utils.dense_path(pi, max_step=0.15)
        s = dc.score(pts).reshape(-1)
        c = 0.5 * (s + 0.3).clamp(min=0).sum()
        (gi,) = torch.autograd.grad(c, (pi,))
        ref.append(float(c.detach()))
        ref_g.append(gi)
        tie = bool(((s + 0.3).abs() <= 1e-4 * s.abs().max()).any())
        if not tie:
            scale = float(gi.abs().max()) + 1e-12
            assert float((gp[i] - gi).abs().max()) <= 1e-4 * scale, i
            checked += 1
    ref = np.array(ref)
    assert np.abs(got.detach().cpu().numpy() - ref).max() <= 1e-5 * np.abs(ref).max()
    assert checked >= 3 and (ref > 0).any()


def test_consistent_with_check_motions(ops):
    d, m, *_ = _case(ops, "cfg2_baxter_poly1")
    mg = _mixed_margin(d)
    qa, qb = _edges(d["q"], 2000, 41)
    for kw in (dict(res=12), dict(max_step=0.1, max_samples=4000)):
        cost = m.motion_cost_raw(_t(qa), _t(qb), margin=mg, weight=3.0, **kw)[0]
        first = m.check_motions(_t(qa), _t(qb), margin=mg, **kw)[0]
        smp = _samples(qa, qb, kw.get("res"), kw.get("max_step"))
        s = m.score(_t(np.concatenate([p for p, *_ in smp]))).cpu().numpy()[:, 0] - mg[0]
        tie, i = [], 0
        for p, *_ in smp:
            tie.append(bool((np.abs(s[i:i + len(p)]) <= 1e-4 * np.abs(s).max()).any()))
            i += len(p)
        keep = torch.as_tensor(~np.array(tie), device="cuda")
        assert torch.equal((cost > 0)[keep], (first >= 0)[keep])
        assert bool((cost > 0).any()) and bool((cost == 0).any())


def test_deterministic_current_stream_and_graph_capture(ops):
    d, m, *_ = _case(ops, "cfg3_baxter_rq_c5")
    qa, qb = _edges(d["q"], 500, 11)
    qa_t, qb_t = _t(qa), _t(qb)
    margin = _t(np.percentile(d["score64"], 90, axis=0).astype(F))
    kw = dict(max_step=0.1, margin=margin, max_samples=4096)
    ref = [x.clone() for x in m.motion_cost_raw(qa_t, qb_t, **kw)]
    again = m.motion_cost_raw(qa_t, qb_t, **kw)
    for x, y in zip(ref, again):
        assert torch.equal(x, y)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = m.motion_cost_raw(qa_t, qb_t, **kw)
    torch.cuda.current_stream().wait_stream(side)
    for x, y in zip(ref, got):
        assert torch.equal(x, y)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.motion_cost_raw(qa_t, qb_t, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = m.motion_cost_raw(qa_t, qb_t, **kw)
    for x in out[:3]:
        x.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(ref, out):
        assert torch.equal(x, y)
    assert 0 < int((ref[0] > 0).sum()) < len(ref[0])


def test_foreign_transform_takes_host_route(ops):
    d, dc, rob = _new_api("cfg2_baxter_rq")
    qa, qb = _edges(d["q"], 80, 13)
    fused = dc.motion_cost(_t(qa), _t(qb), max_step=0.2, margin=-0.5)
    assert dc.last_route == "fused"
    dc.transform = lambda q: rob.fkine(q) * 1.0   # same map, not a diffco_amd robot's fkine: not fusable
    a, b = _t(qa).requires_grad_(True), _t(qb).requires_grad_(True)
    host = dc.motion_cost(a, b, max_step=0.2, margin=-0.5)
    assert dc.last_route == "host"
    assert float((host.detach() - fused).abs().max()) <= 1e-4 * float(fused.abs().max())
    ga, gb = torch.autograd.grad(host.sum(), (a, b))
    dc.transform = rob.fkine
    a2, b2 = _t(qa).requires_grad_(True), _t(qb).requires_grad_(True)
    ga2, gb2 = torch.autograd.grad(dc.motion_cost(a2, b2, max_step=0.2, margin=-0.5).sum(), (a2, b2))
    assert dc.last_route == "fused"
    gs = float(torch.cat([ga2, gb2]).abs().max())
    assert float((ga - ga2).abs().max()) <= 1e-3 * gs and float((gb - gb2).abs().max()) <= 1e-3 * gs
