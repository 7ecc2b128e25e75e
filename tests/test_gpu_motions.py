"""GPU: batched motion checks (dcx_check_motions, ScoreModel.check_motions and the facades' check_motions) against the point
queries they replace (line_predict, dense_path + is_collision), against the fp64 oracle on the same fp32 points, over edge
shapes that make tiles span edges and edges span tiles, split and unsplit launches, both block sizes, graph capture and the
host route of a foreign transform."""
import numpy as np
import pytest
import torch

from helpers import CASE_ROBOT, case_kernel, desc_for, load, make_robot
from helpers import motion_oracle_first as _oracle_first
from helpers import motion_points as _points

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def ops():
    from diffco_amd import _lib, _ops
    _lib.require_gpu()
    return _ops


@pytest.fixture
def early_exit():
    from diffco_amd import _lib
    lib = _lib.load()
    yield lambda v: _lib.check(lib.dcx_debug_set(b"motion_early_exit", int(v)))
    lib.dcx_debug_set(b"motion_early_exit", -1)


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")


def _case(ops, name):
    d = load(name)
    kind, p0, p1 = case_kernel(d)
    desc = desc_for(CASE_ROBOT[name], dof=d["q"].shape[1])
    sup = d["sup_x32"].reshape(len(d["sup_x32"]), -1) if "sup_x32" in d.files and CASE_ROBOT[name] else d["sup_q"]
    sup = np.asarray(sup, dtype=F).reshape(len(sup), -1)
    m = ops.ScoreModel(desc, kind, p0, p1, _t(sup), _t(d["weights"]))
    return d, m, desc, (kind, p0, p1), sup


def _edges(q, E, seed, scale=1.0):
    g = np.random.default_rng(seed)
    i, j = g.integers(0, len(q), E), g.integers(0, len(q), E)
    qa = q[i].astype(F)
    qb = (qa + scale * (q[j] - qa)).astype(F)
    return qa, qb


def _mixed_margin(d):
    """per-class margins at the 70th percentile of the fixture's scores: a mix of free and colliding edges (the Polyharmonic
    fixtures score every configuration positive)"""
    C = d["score64"].shape[1]
    return np.percentile(d["score64"], 70 if C == 1 else 95, axis=0).astype(F).tolist()


CASES = [("cfg1_planar2_rq", 0.0), ("cfg2_baxter_poly1", "mixed"), ("cfg2_baxter_rq", 0.0), ("cfg2_panda_poly1", "mixed"),
         ("cfg2_panda_rq", 0.0), ("cfg4_se3_nofk_rq", 0.0), ("cfg3_baxter_rq_c5", [3.0, 2.5, 2.8, 2.7, 2.9]),
         ("cfg3_baxter_rq_c5", "mixed")]


@pytest.mark.parametrize("name,margin", CASES, ids=[f"{c[0]}-{'mixed' if c[1] == 'mixed' else 'fixed'}" for c in CASES])
@pytest.mark.parametrize("rule", ["res", "max_step"])
def test_first_hit_matches_fp64_oracle(ops, name, margin, rule):
    d, m, desc, kern, sup = _case(ops, name)
    if margin == "mixed":
        margin = _mixed_margin(d)
    q = d["q"]
    qa, qb = _edges(q, 300, 1)
    if rule == "res":
        kw = dict(res=13)
    else:
        span = float(np.median(np.linalg.norm(qb - qa, axis=1)))
        kw = dict(max_step=max(span / 20, 1e-3), max_samples=100000)
    first, n = m.check_motions(_t(qa), _t(qb), margin=margin, **kw)
    pts = _points(qa, qb, kw.get("res"), kw.get("max_step"))
    assert n.cpu().numpy().tolist() == [len(p) for p in pts]
    ref, tie = _oracle_first(desc, kern, sup, d["weights"], pts, margin if isinstance(margin, list) else [margin] * m.C)
    got = first.cpu().numpy()
    keep = ~tie
    assert keep.sum() > 200
    assert (got[keep] == ref[keep]).all(), np.nonzero(got[keep] != ref[keep])
    assert (got >= -1).all() and (ref[keep] == -1).any() and (ref[keep] >= 0).any()


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


def test_res_rule_equals_line_predict(ops):
    d, dc, _ = _new_api("cfg2_baxter_rq")
    qa, qb = _edges(d["q"], 96, 2)
    hit, first = dc.check_motions(_t(qa), _t(qb), res=17, return_first=True)
    assert dc.last_route == "fused"
    ref = [dc.line_predict(_t(a), _t(b), 17) for a, b in zip(qa, qb)]
    assert hit.cpu().tolist() == ref
    assert 0 < sum(ref) < len(ref)
    assert ((first >= 0) == hit).all()


def test_max_step_rule_equals_dense_path(ops):
    from diffco_amd import utils
    d, dc, _ = _new_api("cfg2_panda_rq")
    qa, qb = _edges(d["q"], 64, 3)
    step = 0.15
    hit, first = dc.check_motions(_t(qa), _t(qb), max_step=step, return_first=True)
    got = first.cpu().tolist()
    agree = 0
    for e, (a, b) in enumerate(zip(qa, qb)):
        pts = utils.dense_path(torch.stack([_t(a), _t(b)]), max_step=step)
        s = dc.score(pts)
        if (s.abs() <= 1e-4 * s.abs().max()).any():
            continue   # a tie: the two point sets may differ by an ulp
        col = (s > 0).cpu()
        ref = int(col.nonzero()[0]) if col.any() else -1
        assert got[e] == ref, (e, got[e], ref)
        agree += 1
    assert agree > 48


def test_edge_shapes(ops, early_exit):
    d, m, desc, kern, sup = _case(ops, "cfg2_baxter_rq")
    q = d["q"].astype(F)
    s = d["score64"][:, 0]
    inside, free = q[s > 0], q[s < 0]
    assert len(inside) > 8 and len(free) > 8
    far = free[np.argsort(s[s < 0])[:8]]     # well outside
    g = np.random.default_rng(5)
    qa, qb = [], []
    qa.append(inside[0]); qb.append(far[0])          # starts in collision: first_hit 0
    qa.append(far[1]); qb.append(inside[1])          # hits only near its end (the target, under res: not sampled)
    qa.append(far[2]); qb.append(far[2])             # zero length: one sample, qb
    qa.append(inside[2]); qb.append(inside[2])       # zero length, in collision
    # lengths from 1 to 5000 samples under max_step: tiles span edges and edges span tiles
    step = 0.01
    for n in list(range(1, 70)) + [127, 128, 129, 640, 2000, 4999]:
        a = q[g.integers(len(q))]
        dirn = g.normal(size=q.shape[1]).astype(F)
        dirn /= np.linalg.norm(dirn)
        qa.append(a); qb.append((a + dirn * step * (n - 1.5)).astype(F))
    # edges whose ONLY colliding sample is the last (the target): short edges from just outside onto a shallow inside point
    cand_a, cand_b = [], []
    shallow = inside[np.argsort(s[s > 0])[:200]]
    for b in shallow:   # from a free configuration towards b, starting a few steps before b
        for a in free[g.integers(0, len(free), 8)]:
            u = (a - b) / np.linalg.norm(a - b)
            for r in (0.03, 0.06, 0.1):
                cand_a.append((b + r * u).astype(F))
                cand_b.append(b)
    cp = _points(cand_a, cand_b, max_step=step)
    cf, ct = _oracle_first(desc, kern, sup, d["weights"], cp, [0.0])
    last_only = [i for i in range(len(cp)) if not ct[i] and len(cp[i]) > 1 and cf[i] == len(cp[i]) - 1]
    assert len(last_only) >= 1
    n_fixed = len(qa)
    for i in last_only[:8]:
        qa.append(cand_a[i]); qb.append(cand_b[i])
    qa, qb = np.stack(qa).astype(F), np.stack(qb).astype(F)
    pts = _points(qa, qb, max_step=step)
    assert max(len(p) for p in pts) <= 5000
    ref, tie = _oracle_first(desc, kern, sup, d["weights"], pts, [0.0])
    for ee in (1, 0):
        early_exit(ee)
        first, n = m.check_motions(_t(qa), _t(qb), max_step=step, max_samples=5000)
        got = first.cpu().numpy()
        assert n.cpu().numpy().tolist() == [len(p) for p in pts]
        assert got[0] == 0 and got[3] == 0 and got[2] == -1 and n[2] == 1
        assert (got[~tie] == ref[~tie]).all()
    # the last sample of the max_step rule is the target itself: an edge into an obstacle hits at its last sample at the latest
    assert 0 <= got[1] <= len(pts[1]) - 1
    for e in range(n_fixed, n_fixed + min(len(last_only), 8)):
        assert got[e] == len(pts[e]) - 1
    # over max_samples: -2, and the facade raises
    first, n = m.check_motions(_t(qa), _t(qb), max_step=step, max_samples=100)
    got = first.cpu().numpy()
    lens = np.array([len(p) for p in pts])
    assert (got[lens > 100] == -2).all() and (got[lens <= 100] >= -1).all()
    assert (n.cpu().numpy() == lens).all()
    _, dc, _ = _new_api("cfg2_baxter_rq")
    with pytest.raises(ValueError, match="max_samples"):
        dc.check_motions(_t(qa), _t(qb), max_step=step, max_samples=100)


@pytest.mark.parametrize("E", [1, 63, 64, 65, 10000])
def test_batch_sizes_and_launch_forms(ops, knob, E):
    d, m, desc, kern, sup = _case(ops, "cfg2_baxter_poly1")
    mg = _mixed_margin(d)
    qa, qb = _edges(d["q"], E, 7 + E)
    runs = {}
    for ys, nw in ((-1, -1), (1, 16), (1, 8), (4, 16), (2, 8)):
        knob("ys", ys)
        knob("nw", nw)
        runs[(ys, nw)] = m.check_motions(_t(qa), _t(qb), res=9, margin=mg)[0].cpu().numpy()
    base = runs[(-1, -1)]
    # against the fp64 oracle: every edge of the small batches, a slice of the large one
    sl = slice(0, E) if E <= 65 else slice(E - 400, E)
    pts = _points(qa[sl], qb[sl], res=9)
    ref, tie = _oracle_first(desc, kern, sup, d["weights"], pts, mg)
    assert (base[sl][~tie] == ref[~tie]).all()
    if E > 65:
        assert (ref[~tie] == -1).any() and (ref[~tie] >= 0).any()
    # the forms sum the same terms in other orders: answers agree away from ties (the sample scores of other forms are fp32 close)
    s = m.score(_t(np.concatenate(_points(qa[:2000], qb[:2000], res=9)))).cpu().numpy()[:, 0].reshape(-1, 9) - mg[0]
    tie = (np.abs(s) <= 1e-4 * np.abs(s).max()).any(axis=1)
    for k, v in runs.items():
        assert (v[:2000][~tie] == base[:2000][~tie]).all(), k


def test_current_stream_and_graph_capture(ops):
    d, m, *_ = _case(ops, "cfg3_baxter_rq_c5")
    qa, qb = _edges(d["q"], 500, 11)
    qa_t, qb_t = _t(qa), _t(qb)
    margin = _t(_mixed_margin(d))   # on the device: nothing crosses from the host while the stream is captured
    ref = m.check_motions(qa_t, qb_t, max_step=0.1, margin=margin, max_samples=4096)[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = m.check_motions(qa_t, qb_t, max_step=0.1, margin=margin, max_samples=4096)[0]
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(got, ref)
    # warm-up on the capture stream, capture once, replay once
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.check_motions(qa_t, qb_t, max_step=0.1, margin=margin, max_samples=4096)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out, _ = m.check_motions(qa_t, qb_t, max_step=0.1, margin=margin, max_samples=4096)
    out.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert 0 < int((ref >= 0).sum()) < len(ref)


def test_foreign_transform_takes_host_route(ops):
    d, dc, rob = _new_api("cfg2_baxter_rq")
    qa, qb = _edges(d["q"], 80, 13)
    fused_hit, fused_first = dc.check_motions(_t(qa), _t(qb), max_step=0.2, return_first=True)
    assert dc.last_route == "fused"
    dc.transform = lambda q: rob.fkine(q) * 1.0   # same map, not a diffco_amd robot's fkine: not fusable
    host_hit, host_first = dc.check_motions(_t(qa), _t(qb), max_step=0.2, return_first=True)
    assert dc.last_route == "host"
    # (torch's norm may round an edge's length differently from the kernel's: at most a tie-level disagreement)
    mismatch = (host_first != fused_first).nonzero().reshape(-1).tolist()
    assert len(mismatch) <= 1, mismatch
    assert 0 < int(fused_hit.sum()) < len(qa)


def test_old_api_multiclass_margins(ops):
    from diffco_amd import kernel
    from diffco_amd.deprecated import MultiDiffCo
    d = load("cfg3_baxter_rq_c5")
    rob = make_robot("baxter_left")
    kind, p0, p1 = case_kernel(d)
    mc = MultiDiffCo(None)
    mc.support_points = _t(d["sup_q"])
    mc.fkine = rob.fkine
    mc.support_fkine = rob.fkine(mc.support_points)
    mc.rbf_kernel = kernel.RQKernel(p0, p1)
    mc.rbf_nodes = _t(d["weights"])
    margin = _mixed_margin(d)
    qa, qb = _edges(d["q"], 120, 17)
    hit, first = mc.check_motions(_t(qa), _t(qb), res=11, margin=margin, return_first=True)
    pts = torch.cat([torch.as_tensor(p, device="cuda") for p in _points(qa, qb, res=11)])
    s = (mc.rbf_score(pts) - _t(margin)).reshape(len(qa), 11, -1)
    tie = (s.abs() <= 1e-4 * s.abs().max()).any(-1).any(-1)
    col = (s > 0).any(-1)
    ref = torch.where(col.any(-1), col.int().argmax(-1), torch.full_like(col[:, 0], -1, dtype=torch.int64))
    assert (first.long()[~tie] == ref[~tie]).all()
    assert 0 < int(hit.sum()) < len(qa)


def test_urdf_panda_facade(ops):
    from diffco_amd.collision_checkers import ForwardKinematicsDiffCo
    from helpers import urdf_robot
    rob = urdf_robot("urdf_panda")
    k_tip = rob.unique_position_link_names.index("panda_virtual_ee_link")
    centre = torch.tensor([0.35, 0.0, 0.55])

    def ground_truth(q):
        return ((rob.fkine(q.cuda()).cpu()[:, :, k_tip] - centre).norm(dim=1) < 0.35).float()

    torch.manual_seed(0)
    fk = ForwardKinematicsDiffCo(robot=rob, gamma=10, gt_check_func=ground_truth)
    fk.fit(num_samples=800, verify_ratio=0.2, fix_joints=[7], fix_joint_values=[0.04])
    qa, qb = rob.rand_configs(200).cuda(), rob.rand_configs(200).cuda()
    hit, first = fk.check_motions(qa, qb, max_step=0.3, return_first=True)
    assert fk.last_route == "fused"
    from diffco_amd import utils
    agree = 0
    for e in range(40):
        pts = utils.dense_path(torch.stack([qa[e], qb[e]]), max_step=0.3)
        s = fk.collision_score(pts)[:, 0]
        if (s.abs() <= 1e-4 * s.abs().max()).any():
            continue
        ref = int((s > 0).nonzero()[0]) if (s > 0).any() else -1
        assert int(first[e]) == ref, e
        agree += 1
    assert agree > 25
    # the bias moves the predicate: a bias far below every score frees every edge
    assert not fk.check_motions(qa, qb, res=8, bias=-1e6).any()


def test_max_step_bound_default_and_loose(ops):
    """max_samples=None derives the grid's bound from the longest edge; a tight, the derived and a loose bound give the
    same answers (the bound only sizes the grid and rejects longer edges)"""
    from diffco_amd import _ops
    d, m, desc, kern, sup = _case(ops, "cfg2_panda_rq")
    qa, qb = _edges(d["q"], 700, 23)
    step = 0.1
    lens = np.array([len(p) for p in _points(qa, qb, max_step=step)])
    b = _ops.motion_bound(_t(qa), _t(qb), step)
    assert lens.max() <= b <= lens.max() + 2
    runs = [m.check_motions(_t(qa), _t(qb), max_step=step, max_samples=ms)[0].cpu().numpy()
            for ms in (None, int(lens.max()), 10000)]
    assert (runs[0] == runs[1]).all() and (runs[0] == runs[2]).all()
    assert (runs[0] >= -1).all() and (runs[0] == -1).any() and (runs[0] >= 0).any()
    # the default limit still rejects an edge that needs more samples than it
    far = qa[:1] + np.float32(step * (_ops.MOTION_MAX_SAMPLES + 5)) * np.eye(1, qa.shape[1], dtype=F)
    first, n = m.check_motions(_t(np.concatenate([qa[:3], qa[:1]])), _t(np.concatenate([qb[:3], far])), max_step=step)
    assert first.cpu().tolist()[3] == -2 and n.cpu().tolist()[3] > _ops.MOTION_MAX_SAMPLES
    assert (first.cpu().numpy()[:3] == runs[0][:3]).all()
