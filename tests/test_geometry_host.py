"""CPU tests of diffco_amd.geometry: the referee's closed forms against hand-computed answers, the world's packing, the sphere
descriptions through the oracle's fp64 fkine, and the cap on what the GPU comparisons may skip."""
import math

import numpy as np
import pytest
import torch

import geometry_cases as gc
import helpers
from diffco_amd import _fkdesc, geometry
from diffco_amd.geometry import World, host_clearance_points
from oracle import oracle

INF = float("inf")


def _clear(world, points, radii=None, G=None):
    X = torch.tensor(points, dtype=torch.float64).reshape(1, -1, 3)
    r = torch.zeros(X.shape[1], dtype=torch.float64) if radii is None else torch.tensor(radii, dtype=torch.float64)
    return host_clearance_points(X, r, world, world.n_groups if G is None else G)


def _one(world, p, r=0.0):
    c, w = _clear(world, [p], [r])
    return float(c[0, 0])


def _shift(x, y, z, R=None):
    T = np.eye(4)
    T[:3, 3] = (x, y, z)
    if R is not None:
        T[:3, :3] = R
    return T


# ---- closed forms ---------------------------------------------------------------------------------------------------------------
def test_box_face_edge_corner_and_inside():
    w = World().add_box("b", [2, 4, 6], _shift(10, 0, 0))   # half extents (1, 2, 3) about (10, 0, 0)
    assert abs(_one(w, (12.5, 0.3, -1)) - 1.5) < 1e-12                       # face x
    assert abs(_one(w, (10.2, 2.7, 0)) - 0.7) < 1e-12                        # face y
    assert abs(_one(w, (14, 6, 1)) - 5.0) < 1e-12                            # edge: (3, 4, 0)
    assert abs(_one(w, (12, 4, 5)) - 3.0) < 1e-12                            # corner: (1, 2, 2)
    assert abs(_one(w, (10.25, 0.5, 1)) - (-0.75)) < 1e-12                   # inside: nearest face x, 0.75 deep
    assert abs(_one(w, (10, 0, 0)) - (-1.0)) < 1e-12                         # the centre
    assert abs(_one(w, (12.5, 0.3, -1), r=0.25) - 1.25) < 1e-12              # minus the sphere's radius


def test_rotated_box():
    c, s = math.cos(math.pi / 4), math.sin(math.pi / 4)
    Rz = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    w = World().add_box("b", [2, 2, 2], _shift(0, 0, 0, Rz))
    # the box's corner (1, 1, z) now points along +x at distance sqrt(2)
    assert abs(_one(w, (3, 0, 0)) - (3 - math.sqrt(2))) < 1e-12
    # along the rotated face normal (c, s, 0) the face is at distance 1
    assert abs(_one(w, (3 * c, 3 * s, 0.5)) - 2.0) < 1e-12


def test_zero_thickness_box():
    w = World().add_box("plate", [2, 2, 0])
    assert abs(_one(w, (0.5, 0.5, 0.3)) - 0.3) < 1e-12
    assert abs(_one(w, (0.5, 0.5, -0.3)) - 0.3) < 1e-12
    assert abs(_one(w, (0, 0, 0))) < 1e-12


def test_capsule_cap_and_barrel():
    w = World().add_capsule("c", 0.5, 2.0)    # axis segment z in [-1, 1]
    assert abs(_one(w, (2, 0, 0.3)) - 1.5) < 1e-12                           # barrel
    assert abs(_one(w, (0, 0, 3)) - 1.5) < 1e-12                             # cap, on the axis
    assert abs(_one(w, (3, 0, 5)) - 4.5) < 1e-12                             # cap: (3, 0, 4) from the end point
    assert abs(_one(w, (0.1, 0, 0)) - (-0.4)) < 1e-12                        # inside


def test_cylinder_rim_side_cap_and_inside():
    w = World().add_cylinder("y", 1.0, 4.0)   # radius 1, z in [-2, 2]
    assert abs(_one(w, (3, 0, 1)) - 2.0) < 1e-12                             # side
    assert abs(_one(w, (0.5, 0, 3.5)) - 1.5) < 1e-12                         # cap
    assert abs(_one(w, (4, 0, 6)) - 5.0) < 1e-12                             # rim: (3, 4)
    assert abs(_one(w, (0.5, 0, 0)) - (-0.5)) < 1e-12                        # inside, nearer the side
    assert abs(_one(w, (0, 0, 1.75)) - (-0.25)) < 1e-12                      # inside, nearer the cap


def test_sphere_and_radius():
    w = World().add_sphere("s", 2.0, _shift(1, 2, 3))
    assert abs(_one(w, (1, 2, 8)) - 3.0) < 1e-12
    assert abs(_one(w, (1, 2, 3)) - (-2.0)) < 1e-12
    assert abs(_one(w, (4, 6, 3), r=0.5) - 2.5) < 1e-12


def test_empty_group_and_empty_world():
    w = World().add_sphere("a", 1.0, group=0).add_sphere("b", 1.0, _shift(5, 0, 0), group=2)
    assert w.n_groups == 3
    c, wit = _clear(w, [(2, 0, 0)])
    assert c.tolist() == [[1.0, INF, 2.0]]
    assert wit.tolist() == [[[0, 0], [-1, -1], [1, 0]]]
    c, wit = _clear(World(), [(2, 0, 0)], G=2)
    assert c.tolist() == [[INF, INF]] and wit.tolist() == [[[-1, -1], [-1, -1]]]


def test_tie_order_is_obstacle_then_sphere():
    # two equal spheres of the world, two equal spheres of the robot: all four pairs tie
    w = World().add_sphere("a", 1.0, _shift(-3, 0, 0)).add_sphere("b", 1.0, _shift(3, 0, 0))
    c, wit = _clear(w, [(0, 0, 0), (0, 0, 0)])
    assert c.tolist() == [[2.0]] and wit.tolist() == [[[0, 0]]]
    # the second sphere is nearer to the second obstacle only: (1, 1) wins; nearer to both: (0, 1)
    c, wit = _clear(w, [(0, 0, 0), (1, 0, 0)])
    assert wit.tolist() == [[[1, 1]]]
    c, wit, second = host_clearance_points(torch.zeros(1, 2, 3, dtype=torch.float64), torch.tensor([0.0, 0.5], dtype=torch.float64),
                                           w, 1, return_runner_up=True)
    assert c.tolist() == [[1.5]] and wit.tolist() == [[[0, 1]]] and second.tolist() == [[1.5]]


def test_normals_of_the_referee():
    w = World().add_box("b", [2, 2, 2]).add_cylinder("y", 1.0, 2.0, _shift(10, 0, 0)).add_sphere("s", 1.0, _shift(0, 10, 0)) \
        .add_capsule("c", 0.5, 2.0, _shift(0, 0, 10))
    X = torch.tensor([[(3, 0, 0)], [(0.5, 0.2, 0)], [(10, 0, 4)], [(13, 0, 0)], [(0, 10, 0)], [(0, 0, 10.5)], [(4, 5, 0)]],
                     dtype=torch.float64)
    wit = torch.tensor([[0, 0], [0, 0], [1, 0], [1, 0], [2, 0], [3, 0], [0, 0]])
    n, m = geometry.host_witness_normals(X, w, wit)
    want = [(1, 0, 0), (1, 0, 0), (0, 0, 1), (1, 0, 0), (0, 0, 0), (0, 0, 0), (0.6, 0.8, 0)]
    assert torch.allclose(n, torch.tensor(want, dtype=torch.float64), atol=1e-12)
    assert m[4] == 0 and m[5] == 0 and m[0] > 0.5 and abs(float(m[1]) - 0.3) < 1e-12


# ---- World packing --------------------------------------------------------------------------------------------------------------
def _shapes():
    R = gc.random_rotation(np.random.default_rng(0))
    return {
        "box1": {"type": "Box", "params": {"extents": [1, 2, 3]}, "transform": _shift(0.1, 0.2, 0.3, R)},
        "sphere1": {"type": "Sphere", "params": {"radius": 0.5}, "transform": np.eye(4)},
        "cylinder1": {"type": "Cylinder", "params": {"radius": 0.25, "height": 1.5}, "transform": _shift(1, 0, 0)},
        "capsule1": {"type": "Capsule", "params": {"radius": 0.125, "height": 0.75}},
    }


def test_from_shape_dict_round_trip():
    shapes = _shapes()
    w = World.from_shape_dict(shapes, groups={"sphere1": 2})
    assert w.names == list(shapes) and w.groups == [0, 2, 0, 0] and w.n_groups == 3
    back = w.to_shape_dict()
    for name, s in shapes.items():
        assert back[name]["type"] == s["type"]
        assert back[name]["params"] == {k: (list(map(float, v)) if isinstance(v, list) else float(v)) for k, v in s["params"].items()}
        assert np.array_equal(back[name]["transform"], s.get("transform", np.eye(4)))
    rows = w.rows()
    assert rows.shape == (4, 16) and rows.dtype == np.float32
    assert rows[:, 0].view(np.int32).tolist() == [1, 0 | (2 << 8), 3, 2]
    T = shapes["box1"]["transform"]
    assert np.array_equal(rows[0, 1:10], T[:3, :3].T.reshape(-1).astype(np.float32))      # the rows of R^T, rounded once
    assert np.array_equal(rows[0, 10:13], T[:3, 3].astype(np.float32))
    assert rows[0, 13:].tolist() == [0.5, 1.0, 1.5] and rows[2, 13:].tolist() == [0.25, 0.75, 0.0]
    assert rows[3, 13:].tolist() == [0.125, 0.375, 0.0]


def test_merged_rows_clear_the_groups_and_nothing_else():
    w = World.from_shape_dict(_shapes(), groups={"sphere1": 2, "capsule1": 5})
    a, b = w.rows(), w.rows(merged=True)
    assert np.array_equal(a[:, 1:].view(np.int32), b[:, 1:].view(np.int32))
    assert b[:, 0].view(np.int32).tolist() == [1, 0, 3, 2] and a[:, 0].view(np.int32).tolist() == [1, 2 << 8, 3, 2 | (5 << 8)]
    assert np.array_equal(w.merged().rows().view(np.int32), b.view(np.int32))


def test_update_transform_changes_only_that_row_and_remove_drops_it():
    w = World.from_shape_dict(_shapes())
    before = w.rows()
    w.update_transform("cylinder1", _shift(4, 5, 6))
    after = w.rows()
    assert np.array_equal(before[[0, 1, 3]].view(np.int32), after[[0, 1, 3]].view(np.int32))
    assert after[2, 10:13].tolist() == [4, 5, 6] and np.array_equal(before[2, 13:], after[2, 13:])
    w.remove("sphere1")
    assert w.names == ["box1", "cylinder1", "capsule1"] and np.array_equal(w.rows().view(np.int32), after[[0, 2, 3]].view(np.int32))
    with pytest.raises(ValueError):
        w.remove("sphere1")


def test_mesh_and_bad_groups_raise():
    with pytest.raises(NotImplementedError, match="mesh"):
        World.from_shape_dict({"m": {"type": "Mesh", "params": {"file_obj": "x.obj"}}})
    with pytest.raises(ValueError, match="DCX_MAX_C"):
        World().add_sphere("s", 1.0, group=_fkdesc.MAX_C)
    with pytest.raises(ValueError, match="DCX_MAX_C"):
        World().add_sphere("s", 1.0, group=-1)
    with pytest.raises(ValueError, match="exists"):
        World().add_sphere("s", 1.0).add_box("s", [1, 1, 1])
    with pytest.raises(ValueError, match="unknown shape type"):
        World.from_shape_dict({"m": {"type": "Cone", "params": {}}})


# ---- RobotSpheres descriptions through the oracle's fp64 fkine ------------------------------------------------------------------
def _link_frames(model, q):
    """{link: (R [B, 3, 3], t [B, 3])} composed by hand in numpy from the joint table (fp32 constants, fp64 arithmetic)"""
    q = np.asarray(q, dtype=np.float64)
    B = len(q)
    f32 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)   # noqa: E731
    child = {j["child"]: j for j in model["joints"]}
    dof_of, n = {}, 0
    for ln in model["links"]:
        j = child.get(ln)
        if j is not None and j["type"] != "fixed" and j["mimic_joint"] is None:
            dof_of[j["name"]] = n
            n += 1

    def rot(axis, ang):
        ang = np.broadcast_to(np.asarray(ang, dtype=np.float64), (B,))
        c, s, R = np.cos(ang), np.sin(ang), np.zeros((B, 3, 3))
        i, j, k = axis, (axis + 1) % 3, (axis + 2) % 3
        R[:, i, i] = 1
        R[:, j, j], R[:, j, k], R[:, k, j], R[:, k, k] = c, -s, s, c
        return R

    out = {}

    def frame(ln):
        if ln not in out:
            j = child.get(ln)
            if j is None:
                out[ln] = (np.tile(np.eye(3), (B, 1, 1)), np.zeros((B, 3)))
            else:
                Rp, tp = frame(j["parent"])
                r, p, y = f32(j["rpy"])
                R = Rp @ rot(2, y) @ rot(1, p) @ rot(0, r)
                t = tp + Rp @ f32(j["xyz"])
                if j["type"] != "fixed":
                    v = q[:, dof_of[j["mimic_joint"] or j["name"]]]
                    if j["mimic_joint"] is not None:
                        v = v * j["mimic_multiplier"] + j["mimic_offset"]
                    ax = f32(j["axis"])
                    if j["type"] == "prismatic":
                        t = t + (R @ ax) * v[:, None]
                    else:
                        idx = 0 if abs(ax[0]) == 1 else 1 if abs(ax[1]) == 1 else 2
                        R = R @ rot(idx, np.sign(ax[idx]) * v)
                out[ln] = (R, t)
        return out[ln]

    for ln in model["links"]:
        frame(ln)
    return out


@pytest.mark.parametrize("seed", [5, 8, 32])
def test_urdf_spheres_sit_in_their_links_frames(seed):
    from diffco_amd.urdf import URDFRobotFK
    model = helpers.random_urdf_model(seed)
    rob = URDFRobotFK(helpers.urdf_xml(model))
    behind_fixed = [j["child"] for j in model["joints"] if j["type"] == "fixed"]
    zero_origin = [j["child"] for j in model["joints"] if not any(j["xyz"])]
    assert behind_fixed, "the seed has a link behind a fixed joint"
    rng = np.random.default_rng(seed)
    q = gc.sample_q(rob, 16, rng)
    frames = _link_frames(model, q)
    # offset (0, 0, 0): every link, the root and the links behind fixed joints and with zero joint origins included
    sp = geometry.RobotSpheres(rob, [(ln, (0, 0, 0), 0.1) for ln in model["links"]])
    X = gc.centres64(sp, q)
    for k, ln in enumerate(model["links"]):
        assert np.abs(X[:, k] - frames[ln][1]).max() < 1e-6, ln
    # ... which for the feature links are the robot's own link-origin features
    own = oracle.fkine(rob.fk_desc(), q.astype(np.float64), np.float64)    # [B, 3, L]
    for k, ln in enumerate(rob.unique_position_link_names):
        assert np.abs(own[:, :, k] - X[:, model["links"].index(ln)]).max() < 1e-6, ln
    # nonzero offsets: the same frames composed by hand
    links = behind_fixed + zero_origin + [model["links"][0], model["links"][-1]]
    offs = rng.standard_normal((len(links), 3)) * 0.2
    sp = geometry.RobotSpheres(rob, [(ln, tuple(o), 0.05) for ln, o in zip(links, offs)])
    X = gc.centres64(sp, q)
    for k, (ln, o) in enumerate(zip(links, offs)):
        R, t = frames[ln]
        want = t + R @ np.asarray(o, dtype=np.float32).astype(np.float64)
        # (the planner folds the offset through float64 constants and rounds once: 1e-6 covers the fp32 storage)
        assert np.abs(X[:, k] - want).max() < 1e-6, ln
    with pytest.raises(ValueError, match="no link"):
        geometry.RobotSpheres(rob, [("nope", (0, 0, 0), 0.1)])


def test_planar_arm_lowered_to_dh_reproduces_planar_desc():
    rob = helpers.make_robot("planar3")
    sp = geometry.spheres_on_control_points(rob, 0.1)
    assert sp.descs[0].kind == _fkdesc.DCX_FK_DH and sp.descs[0].point_dim == 3
    q = gc.sample_q(rob, 32, np.random.default_rng(1))
    X = gc.centres64(sp, q)
    own = oracle.fkine(rob.fk_desc(), q.astype(np.float64), np.float64)     # [B, 3, 2]
    assert np.abs(X[:, :, :2] - own).max() < 1e-12 and np.abs(X[:, :, 2]).max() == 0


def test_spheres_along_links_of_a_dh_arm_lie_on_the_segments():
    rob = helpers.make_robot("baxter_left")
    sp = geometry.spheres_along_links(rob, 0.05, 0.1)
    q = gc.sample_q(rob, 8, np.random.default_rng(2))
    X = gc.centres64(sp, q)
    origins = gc.centres64(geometry.RobotSpheres(rob, [((0, j), (0, 0, 0), 0.0) for j in range(7)]), q)
    base = np.zeros_like(origins[:, :1])   # frame -1: the chain's base, the identity here
    prev = np.concatenate([base, origins[:, :-1]], axis=1)
    per_frame = {}
    for k, (f, off, r) in enumerate(sp.spheres):
        assert r == 0.05
        j = f[1]
        a, b = origins[:, j], prev[:, j]
        L = np.linalg.norm(b - a, axis=-1)
        t = np.einsum("bi,bi->b", X[:, k] - a, b - a) / np.where(L > 0, L * L, 1)
        assert np.all((t > -1e-9) & (t < 1)) and np.abs(X[:, k] - (a + t[:, None] * (b - a))).max() < 1e-9, (k, f)
        per_frame.setdefault(j, []).append(float(np.median(t)))
    assert sorted(per_frame) == list(range(7))
    for j, ts in per_frame.items():     # from the frame's origin on, at most `spacing` apart
        L = float(np.linalg.norm(prev[0, j] - origins[0, j]))
        assert ts[0] == 0 and len(ts) == max(1, math.ceil(L / 0.1 - 1e-9)), (j, ts, L)


def test_more_than_32_spheres_split_into_chunks():
    rob = helpers.make_robot("baxter_left")
    rng = np.random.default_rng(3)
    sp = gc.random_spheres(rob, 70, rng, 1.0)
    assert sp.chunks == [(0, 32), (32, 64), (64, 70)] and [d.n_points for d in sp.descs] == [32, 32, 6]
    got = []
    for d, (a, b) in zip(sp.descs, sp.chunks):
        got += [((d.pt_chain[k], d.pt_frame[k]), tuple(d.pt_off[k][j] for j in range(3))) for k in range(b - a)]
    want = [(f, tuple(float(np.float32(v)) for v in off)) for f, off, _ in sp.spheres]
    assert got == want and len(sp) == 70 and sp.radii.shape == (70,)
    rob = gc.tree_robot()
    sp = gc.random_spheres(rob, 40, rng, 1.0)
    assert [d.n_points for d in sp.descs] == [32, 8] and all(not d.t_coord_major for d in sp.descs)
    X = gc.centres64(sp, gc.sample_q(rob, 4, rng))
    assert X.shape == (4, 40, 3)


# ---- the cap on what the GPU comparisons skip -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.CASE_NAMES)
def test_gpu_comparisons_skip_at_most_one_percent(name):
    spheres, world, q, ref = gc.case(name)
    assert ref.skipped_share() <= 0.01, (name, ref.skipped_share())
    if len(world):   # configuration 0 was placed inside the first obstacle
        assert float(ref.all[0]) < -ref.tol


def test_facade_configurations_keep_out_of_the_tolerance_band():
    rob, checker, ref_check = gc.facade_case()
    torch.manual_seed(gc.FACADE_SEED)
    q = rob.rand_configs(1500)
    ref_check(q)
    assert ref_check.closest > ref_check.tol, ref_check.closest
    assert 0.05 < float(ref_check(q).double().mean()) < 0.95


def test_motion_samples_of_the_gpu_tests_keep_out_of_the_tolerance_band():
    from diffco_amd import _ops, _perceptron
    rob, _, ref_check = gc.facade_case()
    for (E, seed), rule in (((24, 9), dict(max_step=0.1)), ((12, 5), dict(max_step=0.15)), ((12, 5), dict(res=9))):
        qa, qb = gc.facade_edges(E, seed)
        pts, plan = _perceptron._motion_samples(qa, qb, rule.get("res"), rule.get("max_step"), None, 0)
        col = ref_check(pts)
        assert ref_check.closest > ref_check.tol, (E, seed, rule, ref_check.closest)
        hit = torch.zeros(E, dtype=torch.bool).index_put_((plan.edge[col],), torch.tensor(True))
        assert 0 < int(hit.sum()) < E, (E, seed, rule)
    arm, _, ref_check, qa, qb = gc.planar_motion_case()
    pts, plan = _perceptron._motion_samples(qa, qb, None, 0.15, None, _ops.wrap_mask(True, 3, arm.fkine))
    col = ref_check(pts)
    assert ref_check.closest > ref_check.tol, ref_check.closest
    hit = torch.zeros(12, dtype=torch.bool).index_put_((plan.edge[col],), torch.tensor(True))
    assert 0 < int(hit.sum()) < 12
