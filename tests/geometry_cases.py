"""The cases the geometry tests share: robots with spheres, worlds of primitives, configurations - and the fp64 referee of each
(the oracle's fkine on the sphere descriptions, then diffco_amd.geometry.host_clearance_points), computed once per case.

The GPU tests (test_gpu_geometry.py) compare against `Referee`; the CPU test of the exclusion cap (test_geometry_host.py)
computes from the same referee how many entries those comparisons skip."""
import functools

import numpy as np
import torch

import helpers
from diffco_amd import geometry
from oracle import oracle

# (name, robot, M spheres, O obstacles, G groups, B configurations, seed)
CASES = [
    ("baxter_m5_o4", "baxter_left", 5, 4, 1, 65, 11),
    ("baxter_m40_o37_g3", "baxter_left", 40, 37, 3, 200, 12),
    ("planar3_m32_o4_g3", "planar3", 32, 4, 3, 64, 13),
    ("se2_m1_o1", "se2", 1, 1, 1, 1, 14),
    ("se3_m5_o37_g3", "se3", 5, 37, 3, 200, 15),
    ("tree_m32_o4", "tree", 32, 4, 1, 65, 36),
    ("tree_m40_o37_g3", "tree", 40, 37, 3, 64, 17),
    ("baxter_m5_o0_g3", "baxter_left", 5, 0, 3, 65, 18),
    ("baxter_m1_o1_b200", "baxter_left", 1, 1, 1, 200, 19),
]
CASE_NAMES = [c[0] for c in CASES]
TREE_SEED = 5


def tree_robot():
    from diffco_amd.urdf import URDFRobotFK
    return URDFRobotFK(helpers.urdf_xml(helpers.random_urdf_model(TREE_SEED)))


def make_robot(name):
    return tree_robot() if name == "tree" else helpers.make_robot(name)


def robot_frames(rob):
    from diffco_amd import model, urdf
    if isinstance(rob, urdf.URDFRobotFK):
        return list(rob.tree.links)
    if isinstance(rob, (model.RigidPlanarBody, model.RigidBody)):
        return [None]
    return [(0, j) for j in range(rob.dof)]


def random_spheres(rob, M, rng, size):
    from diffco_amd import model
    frames = robot_frames(rob)
    flat = isinstance(rob, model.RigidPlanarBody)
    out = []
    for k in range(M):
        f = frames[int(rng.integers(len(frames)))]
        off = rng.standard_normal(3) * 0.1 * size
        if flat:
            off[2] = 0.0
        if k == 0:
            off[:] = 0.0   # one sphere on a frame origin
        out.append((f, tuple(off), float(rng.uniform(0.02, 0.1) * size)))
    return geometry.RobotSpheres(rob, out)


def random_rotation(rng):
    Q, R = np.linalg.qr(rng.standard_normal((3, 3)))
    Q = Q * np.sign(np.diag(R))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return Q


def random_world(O, G, rng, reach, inside_point=None):
    """O primitives, the four types in turn, rotated, in the robot's workspace; G = 3 leaves group 1 empty; the first obstacle
    is put around `inside_point`; worlds of more than 4 obstacles hold a zero-thickness box"""
    w = geometry.World()
    for o in range(O):
        T = np.eye(4)
        T[:3, :3] = random_rotation(rng)
        T[:3, 3] = rng.uniform(-0.8, 0.8, 3) * reach
        s = rng.uniform(0.04, 0.2, 3) * reach
        if o == 0 and inside_point is not None:
            T[:3, 3] = inside_point + 0.2 * s[0] * rng.standard_normal(3) / np.sqrt(3)
        g = 0 if G == 1 else int(rng.choice([0, 2]))
        typ = o % 4
        if typ == 0:
            w.add_sphere(f"s{o}", s[0], T, g)
        elif typ == 1:
            ext = 2 * s
            if o == 5:
                ext[2] = 0.0
            w.add_box(f"b{o}", ext, T, g)
        elif typ == 2:
            w.add_capsule(f"c{o}", s[0], 2 * s[1], T, g)
        else:
            w.add_cylinder(f"y{o}", s[0], 2 * s[1], T, g)
    return w


def sample_q(rob, B, rng):
    lim = np.asarray(rob.limits, dtype=np.float64)
    return (rng.uniform(size=(B, rob.dof)) * (lim[:, 1] - lim[:, 0]) + lim[:, 0]).astype(np.float32)


def centres64(spheres, q):
    """[B, M, 3] float64 sphere centres: the oracle's fkine on each chunk's description"""
    parts = []
    for d in spheres.descs:
        X = oracle.fkine(d, np.asarray(q, dtype=np.float64), np.float64).reshape(len(q), d.n_points, d.point_dim)
        if d.point_dim == 2:
            X = np.concatenate([X, np.zeros_like(X[..., :1])], axis=-1)
        parts.append(X)
    return np.concatenate(parts, axis=1)


class Referee:
    """the fp64 answers of one case and what the comparisons may skip"""

    def __init__(self, spheres, world, q, G, margin=0.0):
        self.spheres, self.world, self.q, self.G, self.margin = spheres, world, q, G, margin
        X = torch.from_numpy(centres64(spheres, q))
        self.X = X
        r64 = spheres.radii.double()
        self.clear, self.wit, self.second = geometry.host_clearance_points(X, r64, world, G, return_runner_up=True)
        one = world.merged()
        self.all, self.wit_all, self.second_all = (t[:, 0] for t in geometry.host_clearance_points(X, r64, one, 1, True))
        self.normal, self.n_margin = geometry.host_witness_normals(X, one, self.wit_all)
        data = [X.abs().max().item() if X.numel() else 0.0]
        if len(world):
            data.append(float(np.abs(world.rows64()[:, 9:]).max()))
        self.s = max(1.0, *data)
        self.tol = 1e-5 * self.s
        # what the comparisons skip
        self.label_ok = (self.clear - margin).abs() > self.tol
        self.wit_ok = (self.second - self.clear > self.tol) | torch.isinf(self.clear)
        self.grad_ok = ((self.second_all - self.all > self.tol) & (self.n_margin >= 1e-3 * self.s)) | torch.isinf(self.all)

    def grad(self):
        """[B, dof] float64: the normal at the witness sphere through the oracle's fkine_vjp"""
        B, M = self.X.shape[:2]
        seed = torch.zeros((B, M, 3), dtype=torch.float64)
        has = self.wit_all[:, 0] >= 0
        k = self.wit_all[:, 1].clamp_min(0)
        seed[torch.arange(B), k] = torch.where(has[:, None], self.normal, torch.zeros_like(self.normal))
        out = np.zeros((B, self.spheres.dof))
        for d, (a, b) in zip(self.spheres.descs, self.spheres.chunks):
            g = seed[:, a:b, :d.point_dim].numpy()
            out += oracle.fkine_vjp(d, np.asarray(self.q, dtype=np.float64), np.ascontiguousarray(g), np.float64)
        return out

    def skipped_share(self):
        """the largest share of entries a comparison skips: labels and witnesses per (configuration, group), gradients per
        configuration"""
        share = lambda ok: int((~ok).sum()) / ok.numel() if ok.numel() else 0.0   # noqa: E731
        return max(share(self.label_ok), share(self.wit_ok), share(self.grad_ok))


@functools.lru_cache(maxsize=None)
def case(name):
    """(spheres, world, q float32 [B, dof], Referee) of a case, built once per process"""
    _, robot, M, O, G, B, seed = CASES[CASE_NAMES.index(name)]
    rng = np.random.default_rng(seed)
    rob = make_robot(robot)
    q = sample_q(rob, B, rng)
    probe = geometry.spheres_on_control_points(rob, 0.0)
    reach = float(np.abs(centres64(probe, q)).max())
    size = min(1.0, reach)
    spheres = random_spheres(rob, M, rng, size)
    # configuration 0 is inside the first obstacle by construction: around its sphere that moves the most over the batch
    X = centres64(spheres, q)
    world = random_world(O, G, rng, reach, inside_point=X[0, int(np.argmax(X.var(axis=0).sum(axis=-1)))])
    return spheres, world, q, Referee(spheres, world, q, G)


# ---- the facade tests' robot, world and referee-backed ground truth ----------------------------------------------------------------
FACADE_SEED = 4


class RefereeCheck:
    """`gt_check_func` backed by the fp64 referee; remembers how close any configuration came to the margin"""

    def __init__(self, spheres, world, margin=0.0):
        self.spheres, self.world, self.margin = spheres, world.merged(), margin
        self.closest, self.tol, self.calls, self.samples = float("inf"), 0.0, 0, 0

    def clearance(self, q):
        X = torch.from_numpy(centres64(self.spheres, q.detach().cpu().reshape(-1, self.spheres.dof).double().numpy()))
        c, _ = geometry.host_clearance_points(X, self.spheres.radii.double(), self.world, 1)
        s = max(1.0, float(X.abs().max()), float(np.abs(self.world.rows64()[:, 9:]).max()))
        self.tol = max(self.tol, 1e-5 * s)
        if len(c):
            self.closest = min(self.closest, float((c[:, 0] - self.margin).abs().min()))
        return c[:, 0]

    def __call__(self, q):
        self.calls += 1
        self.samples += len(q.reshape(-1, self.spheres.dof))
        return (self.clearance(q) < self.margin).to(q.device)


@functools.lru_cache(maxsize=None)
def facade_parts():
    rob = helpers.urdf_robot("urdf_panda")
    spheres = geometry.spheres_along_links(rob, 0.06, 0.08)
    world = geometry.World()
    world.add_box("table", [0.6, 0.8, 0.05], _pose(0.55, 0.0, 0.25))
    world.add_sphere("ball", 0.15, _pose(0.3, 0.4, 0.7))
    world.add_cylinder("post", 0.06, 0.9, _pose(0.35, -0.45, 0.45))
    world.add_capsule("bar", 0.05, 0.6, _pose(-0.2, 0.3, 0.8, random_rotation(np.random.default_rng(7))))
    return rob, spheres, world


def _pose(x, y, z, R=None):
    T = np.eye(4)
    T[:3, 3] = (x, y, z)
    if R is not None:
        T[:3, :3] = R
    return T


def facade_case(margin=0.0):
    rob, spheres, world = facade_parts()
    return rob, geometry.SphereWorldChecker(spheres, world, margin), RefereeCheck(spheres, world, margin)


def facade_edges(E, seed):
    rob = facade_parts()[0]
    torch.manual_seed(seed)
    a = rob.rand_configs(E)
    return a, a + 0.5 * torch.randn(E, rob.dof)


def planar_motion_case():
    """a planar arm (every angle wraps), spheres along its links, two obstacles, 12 edges across the +-pi seam"""
    arm = helpers.make_robot("planar3")
    spheres = geometry.spheres_along_links(arm, 0.1, 0.25)
    reach = float(arm.link_length.sum())
    world = geometry.World().add_box("b", [0.3 * reach, 0.3 * reach, 1.0], _pose(0.45 * reach, 0.3 * reach, 0))
    world.add_sphere("s", 0.15 * reach, _pose(-0.5 * reach, 0.1 * reach, 0))
    torch.manual_seed(6)
    qa, qb = (torch.rand(12, 3) * 2 - 1) * 3.0, (torch.rand(12, 3) * 2 - 1) * 3.0
    assert arm.wrap_mask == 0b111
    return arm, geometry.SphereWorldChecker(spheres, world), RefereeCheck(spheres, world), qa, qb
