"""A geometric ground truth on the device: a sphere model of the robot against a world of primitives.

What the reference takes from FCL / trimesh (`ShapeEnv`, collision_interfaces/env_interface.py:35-122) or from cuRobo's sphere
robot (collision_interfaces/curobo_interface.py) is here one fused launch, `dcx_geom_clearance`: forward kinematics of the
robot's spheres and their signed distances to spheres, oriented boxes, capsules and cylinders.  Meshes stay out of scope.

    world = World.from_shape_dict(shapes)                       # ShapeEnv's dict format
    spheres = spheres_along_links(robot, radius=0.06, spacing=0.08)
    checker = SphereWorldChecker(spheres, world)
    checker(q)                                                  # bool [N]: the `gt_check_func` contract of the facades
    ForwardKinematicsDiffCo(robot=robot, gt_check_func=checker).fit(num_samples=1500)

`host_clearance_points` states the same contract in torch ops on sphere centres (fp64 allowed): the referee of the tests and the
baseline of tools/geom_clearance_bench.py.  The product has no CPU forward kinematics, so it takes points, not configurations.
"""
import math

import numpy as np
import torch

from . import _fkdesc as fd
from . import _lib, _ops, model, urdf
from ._lib import GEOM_BOX, GEOM_CAPSULE, GEOM_CYLINDER, GEOM_SPHERE

_TYPE_NAMES = {"Sphere": GEOM_SPHERE, "Box": GEOM_BOX, "Capsule": GEOM_CAPSULE, "Cylinder": GEOM_CYLINDER}
_NAME_OF_TYPE = {v: k for k, v in _TYPE_NAMES.items()}


# ----------------------------------------------------------------------------- the world
class World:
    """Named primitives with a rigid transform and an obstacle group each (one clearance column per group: the per-obstacle
    labels a MultiDiffCo trains on).  Rows are packed on the host in fp64 and rounded once; the device copy is refreshed lazily
    after a change with one small copy into a buffer that is kept (moving an obstacle does not reallocate)."""

    def __init__(self):
        self.names = []
        self._type, self._group, self._T, self._p = [], [], [], []
        self._version = 0
        self._dev = {}   # (device, merged) -> [buffer [cap, 16] float32, version it holds]

    # -- editing
    def _add(self, name, typ, params, transform, group):
        if name in self.names:
            raise ValueError(f"World: an obstacle named {name!r} exists")
        group = int(group)
        if not 0 <= group < fd.MAX_C:
            raise ValueError(f"World: group {group} outside [0, DCX_MAX_C = {fd.MAX_C})")
        p = np.zeros(3, dtype=np.float64)
        p[:len(params)] = [float(v) for v in params]
        if not np.all(np.isfinite(p)) or np.any(p < 0):
            raise ValueError(f"World: {name!r} needs finite, non-negative sizes, got {params}")
        self.names.append(name)
        self._type.append(typ)
        self._group.append(group)
        self._T.append(self._transform(transform))
        self._p.append(p)
        self._version += 1
        return self

    @staticmethod
    def _transform(T):
        T = np.eye(4) if T is None else np.array(torch.as_tensor(T, dtype=torch.float64).cpu().numpy(), dtype=np.float64)
        if T.shape != (4, 4) or not np.all(np.isfinite(T)):
            raise ValueError("World: a transform is a finite 4x4 matrix")
        return T

    def add_sphere(self, name, radius, transform=None, group=0):
        return self._add(name, GEOM_SPHERE, (radius,), transform, group)

    def add_box(self, name, extents, transform=None, group=0):
        ext = [float(v) for v in extents]
        if len(ext) != 3:
            raise ValueError("World.add_box: extents are the three full side lengths")
        return self._add(name, GEOM_BOX, [0.5 * v for v in ext], transform, group)

    def add_capsule(self, name, radius, height, transform=None, group=0):
        """`height`: the length of the axis segment along local z (trimesh's Capsule), without the caps"""
        return self._add(name, GEOM_CAPSULE, (radius, 0.5 * float(height)), transform, group)

    def add_cylinder(self, name, radius, height, transform=None, group=0):
        return self._add(name, GEOM_CYLINDER, (radius, 0.5 * float(height)), transform, group)

    def remove(self, name):
        i = self.names.index(name)
        for lst in (self.names, self._type, self._group, self._T, self._p):
            del lst[i]
        self._version += 1

    def update_transform(self, name, T):
        self._T[self.names.index(name)] = self._transform(T)
        self._version += 1

    @classmethod
    def from_shape_dict(cls, shapes, groups=None):
        """`shapes`: ShapeEnv's dict (env_interface.py:40-47), name -> dict(type, params, transform); `groups`: name -> group."""
        w = cls()
        for name, s in shapes.items():
            typ, prm, T = s["type"], s.get("params", {}), s.get("transform")
            g = 0 if groups is None else groups.get(name, 0)
            if typ == "Mesh":
                raise NotImplementedError(f"World: {name!r} is a mesh; only Sphere, Box, Capsule and Cylinder are supported")
            if typ == "Sphere":
                w.add_sphere(name, prm["radius"], T, g)
            elif typ == "Box":
                w.add_box(name, prm["extents"], T, g)
            elif typ == "Capsule":
                w.add_capsule(name, prm["radius"], prm["height"], T, g)
            elif typ == "Cylinder":
                w.add_cylinder(name, prm["radius"], prm["height"], T, g)
            else:
                raise ValueError(f"World: unknown shape type {typ!r} for {name!r}")
        return w

    def to_shape_dict(self):
        out = {}
        for name, typ, T, p in zip(self.names, self._type, self._T, self._p):
            prm = {GEOM_SPHERE: lambda: dict(radius=p[0]), GEOM_BOX: lambda: dict(extents=[2 * v for v in p]),
                   GEOM_CAPSULE: lambda: dict(radius=p[0], height=2 * p[1]),
                   GEOM_CYLINDER: lambda: dict(radius=p[0], height=2 * p[1])}[typ]()
            out[name] = dict(type=_NAME_OF_TYPE[typ], params=prm, transform=T.copy())
        return out

    # -- packed forms
    def __len__(self):
        return len(self.names)

    def merged(self):
        """a copy with every obstacle in group 0: the world of the overall minimum"""
        w = World()
        w.names, w._type, w._T, w._p = list(self.names), list(self._type), [T.copy() for T in self._T], [p.copy() for p in self._p]
        w._group = [0] * len(self)
        return w

    @property
    def n_groups(self):
        return max(self._group, default=0) + 1

    @property
    def groups(self):
        return list(self._group)

    @property
    def types(self):
        return list(self._type)

    def rows64(self):
        """[O, 15] float64: the rows of R^T (9), the centre (3), the parameters (3) - what the rows are rounded from"""
        out = np.zeros((len(self), 15), dtype=np.float64)
        for i, (T, p) in enumerate(zip(self._T, self._p)):
            out[i, :9] = T[:3, :3].T.reshape(-1)
            out[i, 9:12] = T[:3, 3]
            out[i, 12:] = p
        return out

    def rows(self, merged=False):
        """[O, 16] float32: dcx_geom_obstacle rows (dword 0 holds the integer type | group << 8; merged: every group 0)"""
        out = np.zeros((len(self), 16), dtype=np.float32)
        out[:, 1:] = self.rows64().astype(np.float32)
        tg = np.array([t | ((0 if merged else g) << 8) for t, g in zip(self._type, self._group)], dtype=np.int32)
        out[:, 0] = tg.view(np.float32)
        return out

    def device_rows(self, dev, merged=False):
        """the rows on `dev`, a view [O, 16] of a buffer this world keeps (merged: the copy with every obstacle in group 0, the
        world of the overall minimum, kept beside it); refreshed with one small copy after a change"""
        dev = torch.device(dev)
        key = (dev, bool(merged))
        ent = self._dev.get(key)
        O = len(self)
        if ent is None or ent[0].shape[0] < O:
            cap = max(16, 2 * O if ent is not None else O)
            ent = self._dev[key] = [torch.zeros((cap, 16), device=dev, dtype=torch.float32), -1]
        if ent[1] != self._version:
            if O:
                ent[0][:O].copy_(torch.from_numpy(self.rows(merged)))
            ent[1] = self._version
        return ent[0][:O]


# ----------------------------------------------------------------------------- the referee
def _sgn(x):
    """+1 for x >= 0 (and +0), -1 below: the kernel's copysign(1, x) away from -0"""
    return torch.where(x < 0, -torch.ones_like(x), torch.ones_like(x))


def _local_points(X, rows):
    """l [N, M, O, 3] = R^T (p - c) for points X [N, M, 3] and rows [O, 15]"""
    Rt = rows[:, :9].reshape(-1, 3, 3)
    d = X[:, :, None, :] - rows[None, None, :, 9:12]
    return torch.einsum("oij,nmoj->nmoi", Rt, d)


def _signed_distances(l, types, p):
    """d [N, M, O] of local points l [N, M, O, 3] to solids of `types` [O] with parameters p [O, 3]"""
    lx, ly, lz = l[..., 0], l[..., 1], l[..., 2]
    zero = torch.zeros_like(lx)
    # sphere
    d_s = l.norm(dim=-1) - p[:, 0]
    # box
    u = l.abs() - p
    d_b = u.clamp_min(0).norm(dim=-1) + torch.minimum(u.max(dim=-1).values, zero)
    # capsule
    vz = lz - torch.maximum(torch.minimum(lz, p[:, 1].expand_as(lz)), (-p[:, 1]).expand_as(lz))
    d_c = torch.sqrt(lx * lx + ly * ly + vz * vz) - p[:, 0]
    # cylinder
    a = torch.sqrt(lx * lx + ly * ly) - p[:, 0]
    b = lz.abs() - p[:, 1]
    d_y = torch.minimum(torch.maximum(a, b), zero) + torch.sqrt(a.clamp_min(0) ** 2 + b.clamp_min(0) ** 2)
    t = types.expand_as(lx)
    return torch.where(t == GEOM_SPHERE, d_s, torch.where(t == GEOM_BOX, d_b, torch.where(t == GEOM_CAPSULE, d_c, d_y)))


def _world_arrays(world, dtype, device):
    rows = torch.from_numpy(world.rows64()).to(device=device, dtype=dtype)
    types = torch.tensor(world.types, dtype=torch.int64, device=device)
    groups = torch.tensor(world.groups, dtype=torch.int64, device=device)
    return rows, types, groups


def host_clearance_points(X, radii, world, n_groups, return_runner_up=False):
    """dcx_geom_clearance's contract in torch ops on sphere centres X [N, M, 3] (any float dtype, any device), radii [M]:
    -> (clearance [N, G], witness [N, G, 2] int64) with witness = (obstacle, sphere) of the first pair in (obstacle, sphere)
    order that attains the minimum; a group without obstacles gives +inf and (-1, -1).  `return_runner_up`: also the
    smallest value among the group's OTHER pairs [N, G] (+inf when there is none)."""
    X = torch.as_tensor(X)
    N, M = X.shape[0], X.shape[1]
    G, O = int(n_groups), len(world)
    radii = torch.as_tensor(radii, dtype=X.dtype, device=X.device)
    inf = float("inf")
    clear = torch.full((N, G), inf, dtype=X.dtype, device=X.device)
    wit = torch.full((N, G, 2), -1, dtype=torch.int64, device=X.device)
    second = torch.full((N, G), inf, dtype=X.dtype, device=X.device)
    if O == 0 or N == 0 or M == 0:
        return (clear, wit, second) if return_runner_up else (clear, wit)
    rows, types, groups = _world_arrays(world, X.dtype, X.device)
    d = _signed_distances(_local_points(X, rows), types, rows[:, 12:]) - radii[None, :, None]   # [N, M, O]
    flat = d.permute(0, 2, 1).reshape(N, O * M)   # pair index = o * M + k: argmin's first minimum is the contract's tie order
    for g in range(G):
        sel = (groups == g).repeat_interleave(M)
        if not bool(sel.any()):
            continue
        dg = torch.where(sel, flat, torch.full_like(flat, inf))
        # the first index of the minimum (torch.argmin does not promise which of several equal entries it returns)
        mn = dg.min(dim=1).values
        idx = torch.arange(O * M, device=X.device).expand(N, -1)
        first = torch.where(dg == mn[:, None], idx, torch.full_like(idx, O * M)).min(dim=1).values
        found = first < O * M    # false for rows of NaN
        first = first.clamp_max(O * M - 1)
        clear[:, g] = torch.where(found, mn, torch.full_like(mn, inf))
        wit[:, g, 0] = torch.where(found, first // M, torch.full_like(first, -1))
        wit[:, g, 1] = torch.where(found, first % M, torch.full_like(first, -1))
        if return_runner_up:
            rest = dg.scatter(1, first[:, None], inf)
            second[:, g] = rest.min(dim=1).values
    return (clear, wit, second) if return_runner_up else (clear, wit)


def host_witness_normals(X, world, witness):
    """the contract's normals for pairs `witness` [N, 2] = (obstacle, sphere) of centres X [N, M, 3]: (n [N, 3] in world
    coordinates, margin [N]) - the unit gradient of the solid's signed distance at the sphere's centre with the kernel's fixed
    choices where it is undefined (zero at a sphere's centre, on a capsule's axis segment and for the radial part on a
    cylinder's axis; the first of x, y, z that attains the maximum inside a box), and `margin`: how far the centre is from the
    nearest place where the normal changes discontinuously (+inf for pairs of -1)."""
    X = torch.as_tensor(X)
    N = X.shape[0]
    rows, types, _ = _world_arrays(world, X.dtype, X.device)
    n_out = torch.zeros((N, 3), dtype=X.dtype, device=X.device)
    margin = torch.full((N,), float("inf"), dtype=X.dtype, device=X.device)
    ok = witness[:, 0] >= 0
    if not bool(ok.any()) or len(world) == 0:
        return n_out, margin
    o = witness[:, 0].clamp_min(0)
    k = witness[:, 1].clamp_min(0)
    P = X[torch.arange(N, device=X.device), k]
    r = rows[o]
    Rt = r[:, :9].reshape(N, 3, 3)
    l = torch.einsum("nij,nj->ni", Rt, P - r[:, 9:12])
    p, t = r[:, 12:], types[o]
    lx, ly, lz = l[:, 0], l[:, 1], l[:, 2]
    zero, one = torch.zeros_like(lx), torch.ones_like(lx)

    def unit(v):
        nv = v.norm(dim=-1, keepdim=True)
        return torch.where(nv > 0, v / torch.where(nv > 0, nv, torch.ones_like(nv)), torch.zeros_like(v)), nv[:, 0]

    n_s, m_s = unit(l)
    # box
    u = l.abs() - p
    m = u.clamp_min(0)
    out = m.norm(dim=-1)
    sg = torch.stack([_sgn(lx), _sgn(ly), _sgn(lz)], -1)
    ax = torch.zeros(N, dtype=torch.int64, device=X.device)
    best = u[:, 0]
    for a_ in (1, 2):
        better = u[:, a_] > best
        ax = torch.where(better, torch.full_like(ax, a_), ax)
        best = torch.where(better, u[:, a_], best)
    inside = torch.nn.functional.one_hot(ax, 3).to(X.dtype) * sg
    n_b = torch.where((out > 0)[:, None], m * sg / torch.where(out > 0, out, one)[:, None], inside)
    us = u.sort(dim=-1, descending=True).values
    big = torch.full_like(u, float("inf"))
    # outside, n = m / |m| moves by (error of l) / |m| - unless a single axis carries it, which stays so while the other axes'
    # u keep away from 0; inside, the axis of the largest u changes where the two largest meet, its sign where l_axis = 0
    single = (u > 0).sum(dim=-1) == 1
    m_b_out = torch.where(single, torch.maximum(out, torch.where(u > 0, big, -u).min(dim=-1).values), out)
    m_b_in = torch.minimum(us[:, 0] - us[:, 1], l.abs().gather(1, ax[:, None])[:, 0])
    m_b = torch.where(out > 0, m_b_out, m_b_in)
    # capsule
    vz = lz - torch.maximum(torch.minimum(lz, p[:, 1]), -p[:, 1])
    n_c, m_c = unit(torch.stack([lx, ly, vz], -1))
    # cylinder
    h = torch.sqrt(lx * lx + ly * ly)
    rad = torch.stack([lx, ly], -1) / torch.where(h > 0, h, one)[:, None]
    rad = torch.where((h > 0)[:, None], rad, torch.zeros_like(rad))
    a, b = h - p[:, 0], lz.abs() - p[:, 1]
    ma, mb = a.clamp_min(0), b.clamp_min(0)
    oc = torch.sqrt(ma * ma + mb * mb)
    sz = _sgn(lz)
    n_out_c = torch.stack([ma * rad[:, 0], ma * rad[:, 1], mb * sz], -1) / torch.where(oc > 0, oc, one)[:, None]
    n_in_a = torch.stack([rad[:, 0], rad[:, 1], zero], -1)
    n_in_b = torch.stack([zero, zero, sz], -1)
    n_y = torch.where((oc > 0)[:, None], n_out_c, torch.where((a >= b)[:, None], n_in_a, n_in_b))
    m_y_out = torch.where((a > 0) & (b > 0), oc, torch.where(a > 0, torch.maximum(oc, -b), torch.maximum(oc, -a)))
    m_y_in = torch.minimum((a - b).abs(), torch.where(a >= b, h, lz.abs()))
    m_y = torch.where(oc > 0, m_y_out, m_y_in)
    t3 = t[:, None]
    nl = torch.where(t3 == GEOM_SPHERE, n_s, torch.where(t3 == GEOM_BOX, n_b, torch.where(t3 == GEOM_CAPSULE, n_c, n_y)))
    mg = torch.where(t == GEOM_SPHERE, m_s, torch.where(t == GEOM_BOX, m_b, torch.where(t == GEOM_CAPSULE, m_c, m_y)))
    nw = torch.einsum("nij,ni->nj", Rt, nl)   # R nl
    n_out = torch.where(ok[:, None], nw, n_out)
    margin = torch.where(ok, mg, margin)
    return n_out, margin


# ----------------------------------------------------------------------------- the robot's spheres
def plan_sphere_tree(tree, spheres, base_transform=None):
    """-> (chains, points, dof): `_fkdesc.tree_desc`'s arguments for spheres [(link name, (ox, oy, oz), radius)] on ANY links of
    a URDF tree.  As `urdf.plan_tree`, fixed joints are folded into the next movable joint's constant transform (float64
    products, rounded once when stored) and a link behind fixed joints becomes an offset in the frame of the last movable joint
    before it; unlike it, every link can carry points, with an offset of its own, and only the root-to-link paths that the
    spheres need become chains."""
    f32 = np.float32
    roots = [ln for ln in tree.links if ln not in tree.joint_of_child]
    if len(roots) != 1:
        raise ValueError(f"URDF: expected exactly one root link, found {roots}")
    dof_of_joint, n_dof = {}, 0
    for ln in tree.links:   # degrees of freedom in link order, mimic joints follow their driver (urdf.plan_tree)
        jt = tree.joint_of_child.get(ln)
        if jt is None or jt.type == "fixed" or jt.mimic_joint is not None:
            continue
        dof_of_joint[jt.name] = n_dof
        n_dof += 1
    for jt in tree.joints:
        if jt.mimic_joint is not None and jt.type != "fixed":
            dof_of_joint[jt.name] = dof_of_joint[jt.mimic_joint]

    def path_to(link):
        if link not in tree.links:
            raise ValueError(f"RobotSpheres: the robot has no link {link!r}")
        path = [link]
        while path[0] in tree.joint_of_child:
            path.insert(0, tree.joint_of_child[path[0]].parent)
        return path

    wanted = []
    for ln, _, _ in spheres:
        if ln not in wanted:
            wanted.append(ln)
    paths = [path_to(ln) for ln in wanted]
    paths = [p for i, p in enumerate(paths)
             if not any(len(o) > len(p) and o[:len(p)] == p for o in paths) and p not in paths[:i]]
    # a link in front of every movable joint needs a frame to sit in: a leading fixed identity joint, in every chain alike so
    # that the chains' common prefixes still merge
    def static(link):
        return all(tree.joint_of_child[ln].type == "fixed" for ln in path_to(link)[1:])

    lead = any(static(ln) for ln in wanted)
    chains, frame_of = [], {}
    base = np.eye(4) if base_transform is None else np.asarray(base_transform, dtype=np.float64).reshape(4, 4)
    for path in paths:
        c = len(chains)
        joints, pending = ([dict(type=fd.DCX_J_FIXED, fixed=fd.IDENTITY_BASE)] if lead else []), np.eye(4)
        frame_of.setdefault(path[0], (c, 0, np.eye(4)))
        for ln in path[1:]:
            jt = tree.joint_of_child[ln]
            origin = urdf._origin_matrix(jt.xyz.astype(f32).astype(np.float64), jt.rpy.astype(f32).astype(np.float64))
            if jt.type == "fixed":
                pending = pending @ origin
            else:
                if jt.type not in ("revolute", "continuous", "prismatic"):
                    raise ValueError(f"URDF: joint {jt.name} has unsupported type {jt.type!r}")
                mult, off = (jt.mimic_multiplier, jt.mimic_offset) if jt.mimic_joint is not None else (1.0, 0.0)
                entry = dict(q=dof_of_joint[jt.name], fixed=urdf._flat34(pending @ origin))
                ax = jt.axis.astype(f32)
                if jt.type == "prismatic":
                    if not np.any(ax != 0):
                        raise ValueError(f"URDF: prismatic joint {jt.name} has a zero axis")
                    entry.update(type=fd.DCX_J_PRISMATIC, axis=tuple(float(v) for v in ax), scale=mult, offset=off)
                else:
                    if abs(ax[0]) == 1:
                        kind, sgn = fd.DCX_J_REV_X, float(np.sign(ax[0]))
                    elif abs(ax[1]) == 1:
                        kind, sgn = fd.DCX_J_REV_Y, float(np.sign(ax[1]))
                    else:
                        kind, sgn = fd.DCX_J_REV_Z, float(np.sign(ax[2]))
                    entry.update(type=kind, scale=sgn * mult, offset=sgn * off)
                joints.append(entry)
                pending = np.eye(4)
            frame_of.setdefault(ln, (c, len(joints) - 1, pending.copy()))
        chains.append(dict(base=urdf._flat34(base), joints=joints))
    points = []
    for ln, off, _ in spheres:
        c, f, T = frame_of[ln]
        points.append((c, f, tuple((T @ np.array([off[0], off[1], off[2], 1.0], dtype=np.float64))[:3])))
    return chains, points, n_dof


def _planar_chain(robot):
    """a planar arm as one DH chain (a = link length, alpha = d = 0): frame j's origin is the arm's j-th link end, z = 0"""
    ll = [float(v) for v in robot.link_length.tolist()]
    n = len(ll)
    return dict(a=ll, d=[0.0] * n, alpha=[0.0] * n, theta0=[0.0] * n, joint_q=list(range(n)))


class RobotSpheres:
    """Spheres rigidly attached to a robot's frames: `spheres` is a list of (frame, (ox, oy, oz), radius).

    frame: a link name for a `URDFRobotFK` (any link; fixed joints are folded into the offset), (chain, joint index) for the
    DH robots of model.py and for a planar arm (lowered to a DH chain), anything (ignored: the body frame) for the SE(2) /
    SE(3) bodies, whose offsets are keypoints.  One `FkDesc` per chunk of at most DCX_MAX_POINTS spheres."""

    def __init__(self, robot, spheres):
        self.robot = robot
        self.dof = robot.dof
        self.spheres = [(f, tuple(float(v) for v in off), float(r)) for f, off, r in spheres]
        if not self.spheres:
            raise ValueError("RobotSpheres: no spheres")
        if any(not (r >= 0 and math.isfinite(r)) for _, _, r in self.spheres):
            raise ValueError("RobotSpheres: radii are finite and non-negative")
        self.radii = torch.tensor([r for _, _, r in self.spheres], dtype=torch.float32)
        n = len(self.spheres)
        self.chunks = [(i, min(n, i + fd.MAX_POINTS)) for i in range(0, n, fd.MAX_POINTS)]
        self.descs = [self._desc(self.spheres[a:b]) for a, b in self.chunks]
        self._radii_dev = {}

    def __len__(self):
        return len(self.spheres)

    def _desc(self, part):
        rob = self.robot
        if isinstance(rob, urdf.URDFRobotFK):
            if isinstance(rob, urdf.MultiURDFRobotFK):
                raise NotImplementedError("RobotSpheres: give each robot of a MultiURDFRobotFK its own spheres")
            chains, points, dof = plan_sphere_tree(rob.tree, part, rob.base_transform)
            return fd.tree_desc(dof, chains, points, coord_major=False)
        if isinstance(rob, model.RigidPlanarBody):
            return fd.keypoint_desc([off[:2] for _, off, _ in part], 2)
        if isinstance(rob, model.RigidBody):
            return fd.keypoint_desc([off for _, off, _ in part], 3)
        if isinstance(rob, model.RevolutePlanarRobot):
            pts = [(0, int(f[1]) if isinstance(f, (tuple, list)) else int(f), off) for f, off, _ in part]
            if any(not 0 <= j < rob.dof for _, j, _ in pts):
                raise ValueError("RobotSpheres: a planar arm's frames are (0, joint index)")
            return fd.dh_desc(rob.dof, [_planar_chain(rob)], pts)
        base = rob.fk_desc()
        if base is None or base.kind != fd.DCX_FK_DH:
            raise TypeError(f"RobotSpheres: no sphere description for {type(rob).__name__}")
        # a DH robot's chains as they stand in its own description (the table's sin / cos of alpha bit for bit), other points
        d = fd.FkDesc.from_buffer_copy(bytes(base))
        if len(part) > fd.MAX_POINTS:
            raise ValueError("RobotSpheres: chunk too large")
        d.n_points = len(part)
        for k in range(fd.MAX_POINTS):
            c, f, off = (int(part[k][0][0]), int(part[k][0][1]), part[k][1]) if k < len(part) else (0, 0, (0.0, 0.0, 0.0))
            if k < len(part) and not (0 <= c < d.n_chains and 0 <= f < d.chain_len[c]):
                raise ValueError(f"RobotSpheres: the robot has no frame (chain {c}, joint {f})")
            d.pt_chain[k], d.pt_frame[k] = c, f
            for j in range(3):
                d.pt_off[k][j] = float(off[j])
        return d

    def radii_on(self, dev):
        dev = torch.device(dev)
        if dev not in self._radii_dev:
            self._radii_dev[dev] = [self.radii[a:b].to(dev).contiguous() for a, b in self.chunks]
        return self._radii_dev[dev]

    def centres(self, q):
        """[B, M, 3] sphere centres through dcx_fkine (z = 0 for planar bodies): the torch composition's first half"""
        q = torch.reshape(q, (-1, self.dof))
        parts = []
        for d in self.descs:
            X = _ops.fkine(d, q)
            if d.point_dim == 2:
                X = torch.cat([X, torch.zeros_like(X[..., :1])], dim=-1)
            parts.append(X)
        return torch.cat(parts, dim=1)


def _dh_frames(robot):
    """[(chain, joint, a, sin_alpha, cos_alpha, d)] of a DH robot or a planar arm"""
    if isinstance(robot, model.RevolutePlanarRobot):
        return [(0, j, float(a), 0.0, 1.0, 0.0) for j, a in enumerate(robot.link_length.tolist())]
    d = robot.fk_desc()
    if d is None or d.kind != fd.DCX_FK_DH:
        raise TypeError(f"no DH frames for {type(robot).__name__}")
    return [(c, j, d.a[c][j], d.sin_alpha[c][j], d.cos_alpha[c][j], d.d[c][j])
            for c in range(d.n_chains) for j in range(d.chain_len[c])]


def spheres_on_control_points(robot, radius):
    """one sphere of `radius` on each control point of the robot's own description"""
    d = robot.fk_desc()
    if isinstance(robot, urdf.URDFRobotFK):
        if isinstance(robot, urdf.MultiURDFRobotFK):
            raise NotImplementedError("spheres_on_control_points: give each robot of a MultiURDFRobotFK its own spheres")
        return RobotSpheres(robot, [(ln, (0.0, 0.0, 0.0), radius) for ln in robot.unique_position_link_names])
    if isinstance(robot, model.RevolutePlanarRobot):
        return RobotSpheres(robot, [((0, j), (0.0, 0.0, 0.0), radius) for j in range(robot.dof)])
    if isinstance(robot, (model.RigidPlanarBody, model.RigidBody)):
        dim = d.point_dim
        return RobotSpheres(robot, [(None, tuple(d.keypoints[k][j] if j < dim else 0.0 for j in range(3)), radius)
                                    for k in range(d.n_points)])
    if d is None or d.kind != fd.DCX_FK_DH:
        raise TypeError(f"spheres_on_control_points: no sphere description for {type(robot).__name__}")
    return RobotSpheres(robot, [((d.pt_chain[k], d.pt_frame[k]), tuple(d.pt_off[k][j] for j in range(3)), radius)
                                for k in range(d.n_points)])


def _segment(frame, end, radius, spacing):
    """spheres from the frame's origin towards `end` (exclusive), at most `spacing` apart"""
    L = float(np.linalg.norm(end))
    n = max(1, int(math.ceil(L / spacing))) if L > 0 else 1
    return [(frame, tuple(float(v) * i / n for v in end), radius) for i in range(n)]


def spheres_along_links(robot, radius, spacing):
    """spheres of `radius` at most `spacing` apart along the robot's links.  URDF: from each link's origin to each child joint's
    origin (a leaf link: its origin alone).  DH (and planar arms): from frame j's origin to the previous frame's, which lies at
    the fixed offset -Rx(-alpha)(a, 0, d) in frame j."""
    if not spacing > 0:
        raise ValueError("spheres_along_links: spacing must be > 0")
    out = []
    if isinstance(robot, urdf.URDFRobotFK):
        if isinstance(robot, urdf.MultiURDFRobotFK):
            raise NotImplementedError("spheres_along_links: give each robot of a MultiURDFRobotFK its own spheres")
        tree = robot.tree
        for ln in tree.links:
            kids = tree.children.get(ln, [])
            if not kids:
                out.append((ln, (0.0, 0.0, 0.0), radius))
            for kid in kids:
                out += _segment(ln, tree.joint_of_child[kid].xyz.astype(np.float32).astype(np.float64), radius, spacing)
        # a link with several children starts a segment at its origin for each: one sphere there is enough
        seen, uniq = set(), []
        for s in out:
            if (s[0], s[1]) not in seen:
                seen.add((s[0], s[1]))
                uniq.append(s)
        return RobotSpheres(robot, uniq)
    for c, j, a, sa, ca, d in _dh_frames(robot):
        out += _segment((c, j), (-a, -sa * d, -ca * d), radius, spacing)
    return RobotSpheres(robot, out)


# ----------------------------------------------------------------------------- the checker
class _ClearanceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, checker):
        q32 = _ops._f32(q.reshape(-1, checker.spheres.dof), _ops._device(q.device))
        clear, _, grad = checker._run(q32, 1, want_witness=False, want_grad=True, groups=None)
        ctx.save_for_backward(grad)
        ctx.meta = (q.dtype, q.device, q.shape)
        return clear[:, 0].to(device=q.device, dtype=q.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        dtype, device, shape = ctx.meta
        out = grad * g.reshape(-1, 1).to(device=grad.device, dtype=grad.dtype)
        return out.to(device=device, dtype=dtype).reshape(shape), None


class SphereWorldChecker:
    """Ground truth of a `RobotSpheres` model in a `World`: `checker(q)` -> bool [N] (true = in collision, clearance <
    margin), on q's device - the `gt_check_func` of the facades and of HybridForwardKinematicsDiffCo."""

    def __init__(self, spheres, world, margin=0.0):
        self.spheres, self.world, self.margin = spheres, world, float(margin)

    # one call per chunk of <= DCX_MAX_POINTS spheres on the current stream; `groups` None: every obstacle in one group
    def _run(self, q32, n_groups, want_witness, want_grad, groups="world"):
        dev = q32.device
        rows = self.world.device_rows(dev, merged=groups is None)
        if groups is not None and self.world.n_groups > n_groups:
            raise ValueError(f"SphereWorldChecker: the world has obstacles in group {self.world.n_groups - 1}, the call has {n_groups} groups")
        out = (None, None, None)
        for ci, (desc, rad, (a, _)) in enumerate(zip(self.spheres.descs, self.spheres.radii_on(dev), self.spheres.chunks)):
            out = _ops.geom_clearance(desc, rad, rows, q32, n_groups=n_groups, sphere_base=a, accumulate=ci > 0,
                                      clearance=out[0], witness=out[1], grad=out[2], want_witness=want_witness,
                                      want_grad=want_grad, check_groups=False)   # (checked above, on the host)
        return out

    def _q32(self, q):
        q = torch.as_tensor(q)
        if q.shape[-1] != self.spheres.dof:
            raise ValueError(f"SphereWorldChecker: configurations have {self.spheres.dof} coordinates, got {tuple(q.shape)}")
        return q, _ops._f32(q.reshape(-1, self.spheres.dof), _ops._device(q.device))

    def clearance(self, q, per_group=False, return_witness=False):
        """the smallest signed distance between the robot's spheres and the world: [...] for q [..., dof] (differentiable
        through the kernel's gradient), or [..., G] with per_group=True.  return_witness: also the (obstacle, sphere) pair,
        int32 [..., 2] / [..., G, 2].  Only the plain call is differentiable: per_group or return_witness with a q that
        requires a gradient raises."""
        q = torch.as_tensor(q)
        lead = q.shape[:-1]
        if q.requires_grad and torch.is_grad_enabled():
            if per_group or return_witness:
                raise ValueError("SphereWorldChecker.clearance: per_group / return_witness results are not differentiable; "
                                 "detach q, or call clearance(q) for the differentiable overall minimum")
            return _ClearanceFn.apply(q, self).reshape(lead)
        q, q32 = self._q32(q)
        G = self.world.n_groups if per_group else 1
        clear, wit, _ = self._run(q32, G, want_witness=return_witness, want_grad=False, groups="world" if per_group else None)
        clear = clear.to(device=q.device, dtype=q.dtype if q.dtype.is_floating_point else torch.float32)
        clear = clear.reshape(*lead, G) if per_group else clear.reshape(lead)
        if not return_witness:
            return clear
        wit = wit.to(q.device)
        return clear, (wit.reshape(*lead, G, 2) if per_group else wit.reshape(*lead, 2))

    def __call__(self, q):
        return self.clearance(torch.as_tensor(q).detach()) < self.margin

    def labels(self, q):
        """[N, G] in {-1, +1}: +1 where the robot collides with an obstacle of group g"""
        c = self.clearance(torch.as_tensor(q).detach(), per_group=True)
        return torch.where(c < self.margin, torch.ones_like(c), -torch.ones_like(c))

    def check_motions(self, starts, targets, max_step=None, res=None, wrap=None, return_first=False, max_samples=None):
        """the motions starts[e] -> targets[e] on ground truth: the samples the proxy's check_motions takes, one clearance call
        over all of them, the first hit per edge.  -> collides [E] bool (and first_hit [E] int32, -1 = free)."""
        from . import _perceptron
        if (max_step is None) == (res is None):
            raise ValueError("check_motions: give max_step or res")
        qa, qb = torch.as_tensor(starts), torch.as_tensor(targets)
        qa, qb = qa.reshape(-1, self.spheres.dof), qb.reshape(-1, self.spheres.dof)
        mask = _ops.wrap_mask(wrap, self.spheres.dof, getattr(self.spheres.robot, "fkine", None))
        # a sample hits where __call__ says so: the one comparison, clearance < margin, as a +-1 score against margin 0
        hits = lambda p: torch.where(self(p), 1.0, -1.0)   # noqa: E731
        first, _ = _perceptron.host_motions(hits, qa, qb, res, max_step, 0.0, max_samples, mask)
        return _perceptron.motion_answer(first, return_first)
