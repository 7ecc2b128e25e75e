"""dcx_geom_clearance and diffco_amd.geometry on the GPU against the fp64 referee (the oracle's fkine on the sphere descriptions,
then host_clearance_points): clearances to 1e-5 * s absolute (s = max(1, largest |coordinate| of the case)), labels, witnesses and
gradients wherever the referee says they are determined (test_geometry_host.py caps what that leaves out at 1 %)."""
import ctypes as C

import numpy as np
import pytest
import torch

import geometry_cases as gc
from diffco_amd import _lib, _ops, geometry
from oracle import oracle

pytestmark = pytest.mark.gpu


def _run(spheres, world, q, G, want_grad=True):
    checker = geometry.SphereWorldChecker(spheres, world)
    q32 = torch.as_tensor(q, dtype=torch.float32).cuda()
    clear, wit, grad = checker._run(q32, G, want_witness=True, want_grad=want_grad)
    torch.cuda.synchronize()
    return clear.cpu().double(), wit.cpu().long(), None if grad is None else grad.cpu().double()


def _compare(name, clear, wit, grad, ref):
    fin = torch.isfinite(ref.clear)
    assert torch.equal(torch.isinf(clear) & (clear > 0), ~fin), name
    err = float((clear[fin] - ref.clear[fin]).abs().max()) if bool(fin.any()) else 0.0
    print(f"{name}: s = {ref.s:.3f}, clearance err {err:.3e} (tol {ref.tol:.3e})")
    assert err <= ref.tol, (name, err, ref.tol)
    labels, want = clear < ref.margin, ref.clear < ref.margin
    assert torch.equal(labels[ref.label_ok], want[ref.label_ok]), name
    assert torch.equal(wit[ref.wit_ok], ref.wit[ref.wit_ok]), name
    if grad is not None:
        assert bool(torch.isfinite(grad).all()), name
        want_g = torch.from_numpy(ref.grad())
        ok = ref.grad_ok
        gerr = float((grad[ok] - want_g[ok]).abs().max()) if bool(ok.any()) else 0.0
        bound = 1e-5 * max(1.0, float(want_g[ok].abs().max()) if bool(ok.any()) else 0.0)
        print(f"{name}: gradient err {gerr:.3e} (bound {bound:.3e})")
        assert gerr <= bound, (name, gerr, bound)


@pytest.mark.parametrize("name", gc.CASE_NAMES)
def test_clearance_labels_witnesses_and_gradients_against_fp64(name):
    spheres, world, q, ref = gc.case(name)
    clear, wit, grad = _run(spheres, world, q, ref.G)
    _compare(name, clear, wit, grad, ref)
    if len(world) == 0:
        assert bool(torch.isinf(clear).all()) and bool((wit == -1).all()) and bool((grad == 0).all())
    if ref.G == 3:   # the group left empty
        assert bool(torch.isinf(clear[:, 1]).all()) and bool((wit[:, 1] == -1).all())


def test_the_referees_gradient_is_the_central_difference_of_its_clearance():
    spheres, world, q, ref = gc.case("baxter_m5_o4")
    g = ref.grad()
    b = int(torch.nonzero(ref.grad_ok & (ref.n_margin > 0.01))[0])
    h, one = 1e-6, world.merged()
    for j in range(spheres.dof):
        vals = []
        for sgn in (+1, -1):
            qq = np.asarray(q[b:b + 1], dtype=np.float64).copy()
            qq[0, j] += sgn * h
            X = torch.from_numpy(gc.centres64(spheres, qq))
            vals.append(float(geometry.host_clearance_points(X, spheres.radii.double(), one, 1)[0][0, 0]))
        assert abs((vals[0] - vals[1]) / (2 * h) - g[b, j]) < 1e-6, (j, vals, g[b, j])


def test_public_checker_matches_the_kernel_outputs():
    spheres, world, q, ref = gc.case("se3_m5_o37_g3")
    checker = geometry.SphereWorldChecker(spheres, world)
    qc = torch.from_numpy(q)                                     # CPU in, CPU out
    c = checker.clearance(qc)
    assert c.device.type == "cpu" and c.shape == (len(q),)
    assert float((c.double() - ref.all).abs().max()) <= ref.tol
    hit = checker(qc)
    assert hit.dtype == torch.bool and hit.device.type == "cpu"
    ok = (ref.all - 0.0).abs() > ref.tol
    assert torch.equal(hit[ok], (ref.all < 0)[ok])
    lab = checker.labels(qc.cuda())
    assert lab.is_cuda and lab.shape == (len(q), 3)
    assert torch.equal(lab.cpu()[ref.label_ok], torch.where(ref.clear < 0, 1.0, -1.0)[ref.label_ok].float())
    cg, wg = checker.clearance(qc.reshape(2, -1, 6), per_group=True, return_witness=True)     # leading batch dims are kept
    assert cg.shape == (2, len(q) // 2, 3) and wg.shape == (2, len(q) // 2, 3, 2)
    assert torch.equal(wg.reshape(-1, 3, 2).long()[ref.wit_ok], ref.wit[ref.wit_ok])
    shifted = geometry.SphereWorldChecker(spheres, world, margin=0.25)
    ok = (ref.all - 0.25).abs() > ref.tol
    assert torch.equal(shifted(qc)[ok], (ref.all < 0.25)[ok])


def test_autograd_is_the_kernels_gradient():
    spheres, world, q, ref = gc.case("tree_m40_o37_g3")
    checker = geometry.SphereWorldChecker(spheres, world)
    q32 = torch.from_numpy(q).cuda()
    _, _, grad = geometry.SphereWorldChecker(spheres, world.merged())._run(q32, 1, want_witness=False, want_grad=True)
    qt = torch.from_numpy(q).cuda().requires_grad_(True)
    c = checker.clearance(qt)
    up = torch.linspace(-1, 2, len(q), device="cuda")
    (g,) = torch.autograd.grad(c, qt, up)
    assert torch.equal(g, grad * up[:, None])      # the kernel's grad times the upstream, in float32
    assert float((c.detach().cpu().double() - ref.all).abs().max()) <= ref.tol


def test_degenerate_points_give_finite_outputs_and_collide():
    """a sphere centre exactly on an obstacle sphere's centre, on a capsule's axis, on a cylinder's axis and at a box's centre"""
    from diffco_amd import model
    body = model.RigidBody(keypoints=[[0.0, 0.0, 0.0]])
    spheres = geometry.RobotSpheres(body, [(None, (0, 0, 0), 0.05)])
    T = np.eye(4)
    T[:3, 3] = (1, 2, 3)
    q = torch.tensor([[1, 2, 3, 0.3, -0.2, 0.1], [1, 2, 3.25, 0, 0, 0]], dtype=torch.float32)
    for add in ("sphere", "capsule", "cylinder", "box"):
        w = geometry.World()
        {"sphere": lambda: w.add_sphere("o", 0.5, T), "capsule": lambda: w.add_capsule("o", 0.5, 1.0, T),
         "cylinder": lambda: w.add_cylinder("o", 0.5, 1.0, T), "box": lambda: w.add_box("o", [1, 1, 1], T)}[add]()
        clear, wit, grad = _run(spheres, w, q, 1)
        assert bool(torch.isfinite(clear).all()) and bool(torch.isfinite(grad).all()), add
        assert bool((clear < 0).all()), add
        assert abs(float(clear[0, 0]) - (-0.55)) < 1e-6, (add, clear)
        assert wit.tolist() == [[[0, 0]], [[0, 0]]]
        if add in ("sphere", "capsule"):
            assert bool((grad[0] == 0).all()), (add, grad)      # the normal is undefined: zero, not NaN
        checker = geometry.SphereWorldChecker(spheres, w)
        assert checker(q).tolist() == [True, True]


def test_chunks_accumulate_and_the_first_chunk_is_a_call_of_its_own():
    spheres, world, q, ref = gc.case("baxter_m40_o37_g3")
    clear, wit, grad = _run(spheres, world, q, ref.G)
    assert int(wit[..., 1].max()) >= 32                         # the second chunk's spheres, offset by sphere_base
    # the first 32 spheres alone: the one-call result, bit for bit, and what the chunked run holds where they win
    first = geometry.RobotSpheres(spheres.robot, spheres.spheres[:32])
    c1, w1, g1 = _run(first, world, q, ref.G)
    q32 = torch.from_numpy(q).cuda()
    rows = world.device_rows(q32.device)
    c_one, w_one, g_one = _ops.geom_clearance(spheres.descs[0], spheres.radii_on(q32.device)[0], rows, q32, n_groups=ref.G,
                                              want_grad=True)
    assert torch.equal(c1, c_one.cpu().double()) and torch.equal(w1, w_one.cpu().long()) and torch.equal(g1, g_one.cpu().double())
    low = wit[..., 1] < 32
    assert torch.equal(clear[low], c1[low]) and torch.equal(wit[low], w1[low])
    assert bool((clear <= c1).all())
    # a chunk that does not improve a row leaves the row alone: accumulate the same chunk twice
    c2, w2, g2 = c_one.clone(), w_one.clone(), g_one.clone()
    _ops.geom_clearance(spheres.descs[0], spheres.radii_on(q32.device)[0], rows, q32, n_groups=ref.G, accumulate=True,
                        clearance=c2, witness=w2, grad=g2)
    assert torch.equal(c2, c_one) and torch.equal(w2, w_one) and torch.equal(g2, g_one)


def test_moving_an_obstacle_reuses_the_device_rows():
    spheres, world, q, ref = gc.case("baxter_m5_o4")
    w = geometry.World.from_shape_dict(world.to_shape_dict())
    checker = geometry.SphereWorldChecker(spheres, w)
    qc = torch.from_numpy(q).cuda()
    before = checker.clearance(qc)
    ptr = w.device_rows(qc.device).data_ptr()
    T = np.eye(4)
    T[:3, 3] = (50, 50, 50)
    w.update_transform(w.names[0], T)
    after = checker.clearance(qc)
    assert w.device_rows(qc.device).data_ptr() == ptr
    assert float(after[0]) > float(before[0]) and float(before[0]) < 0     # configuration 0 sat inside that obstacle
    with pytest.raises(ValueError, match="coordinates"):
        checker.clearance(torch.zeros(3, 5))


def test_the_call_is_captured_in_a_hip_graph():
    """no allocation and no synchronisation inside dcx_geom_clearance: after one warm-up call (the program's upload) the call
    with a gradient replays identically"""
    spheres, world, q, ref = gc.case("tree_m32_o4")
    lib = _lib.require_gpu()
    q32 = torch.from_numpy(q).cuda()
    B, dof, G = len(q), spheres.dof, 1
    rows, rad, desc = world.device_rows(q32.device), spheres.radii_on(q32.device)[0], spheres.descs[0]
    clear = torch.empty((B, G), device="cuda")
    wit = torch.empty((B, G, 2), device="cuda", dtype=torch.int32)
    grad = torch.empty((B, dof), device="cuda")
    opt = _lib.GeomOpts(G, 0, 0, 0)

    def enqueue(st):
        _lib.check(lib.dcx_geom_clearance(0, C.byref(desc), _ops._ptr(rad), _ops._ptr(rows), len(rows), _ops._ptr(q32), B,
                                          C.byref(opt), _ops._ptr(clear), _ops._ptr(wit), _ops._ptr(grad), C.c_void_p(st.cuda_stream)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enqueue(side)
        side.synchronize()
        want = clear.clone(), wit.clone(), grad.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            enqueue(side)
        clear.fill_(7.0)
        wit.zero_()
        grad.zero_()
        graph.replay()
        side.synchronize()
    assert torch.equal(clear, want[0]) and torch.equal(wit, want[1]) and torch.equal(grad, want[2])
    assert float((clear.cpu().double() - ref.clear).abs().max()) <= ref.tol


# ---- the facades on ground truth ------------------------------------------------------------------------------------------------
def _fitted(gt, seed=gc.FACADE_SEED, cls=None):
    from diffco_amd import ForwardKinematicsDiffCo
    rob = gc.facade_parts()[0]
    torch.manual_seed(seed)
    fk = (cls or ForwardKinematicsDiffCo)(robot=rob, gamma=10, gt_check_func=gt)
    res = fk.fit(num_samples=1500, verify_ratio=0.2)
    return fk, res


def test_fit_without_labels_equals_the_fit_on_the_referees_labels():
    rob, checker, ref_check = gc.facade_case()
    fk_a, res_a = _fitted(checker)
    fk_b, res_b = _fitted(ref_check)
    assert ref_check.closest > ref_check.tol           # no configuration in the tolerance band: the labels must be equal
    assert torch.equal(fk_a.perceptron.support_points.cpu(), fk_b.perceptron.support_points.cpu())
    assert torch.equal(fk_a.perceptron.gains.cpu(), fk_b.perceptron.gains.cpu())
    assert [float(v) for v in res_a] == [float(v) for v in res_b]
    print("fit on ground truth: supports", len(fk_a.perceptron.support_points), "verify", [round(float(v), 4) for v in res_a])
    # verify() asks the ground truth itself
    torch.manual_seed(1)
    va = fk_a.verify(num_samples=300)
    torch.manual_seed(1)
    vb = fk_b.verify(num_samples=300)
    assert ref_check.closest > ref_check.tol and [float(v) for v in va] == [float(v) for v in vb]


def test_hybrid_check_motions_equals_the_referee_backed_call():
    from diffco_amd import HybridForwardKinematicsDiffCo
    rob, checker, ref_check = gc.facade_case()
    fk_a, _ = _fitted(checker, cls=HybridForwardKinematicsDiffCo)
    fk_b, _ = _fitted(ref_check, cls=HybridForwardKinematicsDiffCo)
    qa, qb = gc.facade_edges(24, 9)
    before = ref_check.samples
    hit_a, first_a = fk_a.check_motions(qa, qb, max_step=0.1, return_first=True)
    hit_b, first_b = fk_b.check_motions(qa, qb, max_step=0.1, return_first=True)
    assert ref_check.closest > ref_check.tol
    assert torch.equal(hit_a, hit_b) and torch.equal(first_a, first_b)
    assert fk_a.last_gt_checks == fk_b.last_gt_checks == ref_check.samples - before and fk_a.last_gt_checks > 0
    assert 0 < int(hit_a.sum()) < len(hit_a)


@pytest.mark.parametrize("rule", [dict(max_step=0.15), dict(res=9), dict(max_step=0.15, wrap=True)])
def test_checker_check_motions_equals_the_referee_on_the_materialised_samples(rule):
    from diffco_amd import _perceptron
    rob, checker, ref_check = gc.facade_case()
    qa, qb = gc.facade_edges(12, 5)
    if rule.get("wrap"):     # the Panda fixture has no continuous joint: a planar arm's angles all wrap
        rob, checker, ref_check, qa, qb = gc.planar_motion_case()
    hit, first = checker.check_motions(qa, qb, return_first=True, **rule)
    mask = _ops.wrap_mask(rule.get("wrap"), rob.dof, rob.fkine)
    pts, plan = _perceptron._motion_samples(qa, qb, rule.get("res"), rule.get("max_step"), None, mask)
    col = ref_check(pts)
    assert ref_check.closest > ref_check.tol
    want = torch.full((len(qa),), -1, dtype=torch.int64)
    for e in range(len(qa)):
        ks = plan.k[(plan.edge == e) & col]
        if len(ks):
            want[e] = int(ks.min())
    assert torch.equal(first.long(), want) and torch.equal(hit, want >= 0)
    assert torch.equal(checker.check_motions(qa, qb, **rule), hit)
    assert 0 < int(hit.sum()) < len(hit), hit


def test_group_ids_and_gradient_requests_are_checked_in_python():
    spheres, world, q, ref = gc.case("se3_m5_o37_g3")
    q32 = torch.from_numpy(q).cuda()
    rows, rad = world.device_rows(q32.device), spheres.radii_on(q32.device)[0]
    with pytest.raises(ValueError, match="outside \\[0, n_groups = 2\\)"):
        _ops.geom_clearance(spheres.descs[0], rad, rows, q32, n_groups=2)
    with pytest.raises(ValueError, match="the call has 1 groups"):
        geometry.SphereWorldChecker(spheres, world)._run(q32, 1, want_witness=False, want_grad=False)
    # unchecked, the kernel ignores the rows of the groups it was not given: group 0's column is the three-group call's
    c2, _, _ = _ops.geom_clearance(spheres.descs[0], rad, rows, q32, n_groups=2, check_groups=False)
    c3, _, _ = _ops.geom_clearance(spheres.descs[0], rad, rows, q32, n_groups=3)
    assert torch.equal(c2[:, 0], c3[:, 0]) and bool(torch.isinf(c2[:, 1]).all())
    checker = geometry.SphereWorldChecker(spheres, world)
    qg = q32.clone().requires_grad_(True)
    for kw in (dict(return_witness=True), dict(per_group=True)):
        with pytest.raises(ValueError, match="not differentiable"):
            checker.clearance(qg, **kw)
    assert checker.clearance(qg.detach(), return_witness=True)[1].shape == (len(q), 2)
    # the merged rows live in a buffer of their own, refreshed with the world
    merged = world.device_rows(q32.device, merged=True)
    assert merged.data_ptr() != rows.data_ptr() and merged.data_ptr() == world.device_rows(q32.device, merged=True).data_ptr()
    assert torch.equal(merged[:, 1:], rows[:, 1:]) and bool(((merged.view(torch.int32)[:, 0] >> 8) == 0).all())


def test_check_motions_and_call_share_one_comparison_under_a_margin():
    from diffco_amd import _perceptron
    rob, checker, _ = gc.facade_case(margin=0.0371)
    qa, qb = gc.facade_edges(12, 5)
    hit, first = checker.check_motions(qa, qb, max_step=0.15, return_first=True)
    pts, plan = _perceptron._motion_samples(qa, qb, None, 0.15, None, 0)
    col = checker(pts)
    want = torch.full((len(qa),), -1, dtype=torch.int64)
    for e in range(len(qa)):
        ks = plan.k[(plan.edge == e) & col]
        if len(ks):
            want[e] = int(ks.min())
    assert torch.equal(first.long(), want) and torch.equal(hit, want >= 0)
