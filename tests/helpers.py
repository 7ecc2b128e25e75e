"""Shared by the CPU (oracle) and GPU (parity) tests: golden loading, robot factory, error metric."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

KIND = {"rq": 0, "poly": 1, "mq": 2}

# which robot each score fixture was generated with (tools/make_golden.py)
CASE_ROBOT = {
    "cfg1_planar2_rq": "planar2", "cfg2_baxter_poly1": "baxter_left", "cfg2_baxter_rq": "baxter_left",
    "cfg2_panda_poly1": "panda", "cfg2_panda_rq": "panda", "headline_baxter_poly1_s2000": "baxter_left",
    "cfg3_baxter_rq_c5": "baxter_left", "cfg3_baxter_poly1_c5": "baxter_left", "cfg4_se3_nofk_rq": None,
    "cfg4_se3_keypts_rq": "se3", "misc_dualbaxter_poly1": "baxter_dual", "misc_dualpanda_rq": "dual_panda",
    "misc_panda5_mq": "panda5", "misc_se2_poly3": "se2", "misc_planar3_poly2": "planar3",
    "misc_planar7_rq_p3": "planar7", "misc_baxterR_mq_c2": "baxter_right", "edge_r0_baxter_poly1": "baxter_left",
    "edge_r0_planar3_poly2": "planar3",
}
FK_NAMES = ["planar2", "planar3", "planar7", "se2", "se3", "baxter_left", "baxter_right", "baxter_dual", "panda",
            "panda5", "dual_panda"]


URDF_NAMES = ["urdf_panda", "urdf_panda_nogripper", "urdf_fetch_arm", "urdf_iiwa7", "urdf_allegro", "urdf_trifinger",
              "urdf_jaco", "urdf_2link", "urdf_fetch", "urdf_iiwa7_allegro"]


def urdf_model(name):
    """the URDF-derived joint table stored with fk_<name>.npz (tools/make_golden_urdf.py)"""
    import json
    return json.loads(bytes(load("fk_" + name)["model"]).decode())


def urdf_xml(model):
    """URDF text of a stored joint table (kinematic content only) — exercises diffco_amd.urdf.parse_urdf"""
    out = ['<?xml version="1.0"?>', '<robot name="golden">']
    out += [f'  <link name="{ln}"/>' for ln in model["links"]]
    fmt = lambda v: " ".join(repr(float(x)) for x in v)  # noqa: E731
    for j in model["joints"]:
        out.append(f'  <joint name="{j["name"]}" type="{j["type"]}">')
        out.append(f'    <parent link="{j["parent"]}"/><child link="{j["child"]}"/>')
        out.append(f'    <origin xyz="{fmt(j["xyz"])}" rpy="{fmt(j["rpy"])}"/>')
        out.append(f'    <axis xyz="{fmt(j["axis"])}"/>')
        if j["lower"] is not None:
            out.append(f'    <limit lower="{j["lower"]!r}" upper="{j["upper"]!r}" effort="1" velocity="1"/>')
        if j["mimic_joint"] is not None:
            out.append(f'    <mimic joint="{j["mimic_joint"]}" multiplier="{j["mimic_multiplier"]!r}" '
                       f'offset="{j["mimic_offset"]!r}"/>')
        out.append("  </joint>")
    out.append("</robot>")
    return "\n".join(out)


def urdf_robot(name, **kw):
    from diffco_amd.urdf import URDFRobotFK
    return URDFRobotFK(urdf_xml(urdf_model(name)), **kw)


def dual_panda_robot(**kw):
    """the two-Panda MultiURDFRobotFK of fk_urdf_dual_panda.npz (bases from examples/tests/test_urdf_robot.py:59-74)"""
    from diffco_amd.urdf import MultiURDFRobotFK, URDFRobotFK
    xml, bases = urdf_xml(urdf_model("urdf_panda")), load("fk_urdf_dual_panda")["bases"]
    return MultiURDFRobotFK([URDFRobotFK(xml, name=f"panda{i + 1}", base_transform=b) for i, b in enumerate(bases)], **kw)


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def make_robot(name):
    """the diffco_amd.model robot matching a golden fixture's robot (parameters from fk_<name>.npz)"""
    from diffco_amd import model
    if name is None:
        return None
    if name.startswith("planar"):
        ll = load("fk_" + name)["link_length"]
        return model.RevolutePlanarRobot(ll.tolist(), 0.1)
    if name == "se2":
        kp = load("fk_se2")["keypoints"]  # [2, M]
        return model.RigidPlanarBody([("box", tuple(kp[:, i].tolist()), (1, 1)) for i in range(kp.shape[1])])
    if name == "se3":
        return model.RigidBody(keypoints=load("fk_se3")["keypoints"])
    return {"baxter_left": model.BaxterLeftArmFK, "baxter_right": model.BaxterRightArmFK,
            "baxter_dual": model.BaxterDualArmFK, "panda": model.PandaFK,
            "panda5": lambda: model.PandaFK(fingers=False), "dual_panda": model.DualPandaFK}[name]()


def desc_for(name, dof=None):
    from diffco_amd import _fkdesc
    rob = make_robot(name)
    return _fkdesc.none_desc(dof) if rob is None else rob.fk_desc()


def relerr(a, ref):
    """max|a - ref| / max|ref|  — the parity metric"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    den = np.abs(ref).max()
    return float(np.abs(a - ref).max() / (den if den > 0 else 1.0))


def case_kernel(d):
    kind = str(d["kind"])
    kp = d["kparams"]
    return KIND[kind], float(kp[0]), float(kp[1]) if len(kp) > 1 else 0.0


# ---------------------------------------------------------------------------------------------
# test-local torch stand-ins (host-logic tests run without a GPU; the product has no CPU path)
class TorchKernel:
    """direct-difference torch kernels with the reference call signature — a *foreign* callable as far
    as diffco_amd is concerned (no dcx_spec), used to drive the host-side trainer on CPU"""

    def __init__(self, kind, p0, p1=0.0):
        self.kind, self.p0, self.p1 = kind, p0, p1

    def __call__(self, xs, x_primes):
        import torch
        if xs.ndim < x_primes.ndim:
            xs = xs[None]
        a, b = xs.reshape(len(xs), -1), x_primes.reshape(len(x_primes), -1)
        d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
        if self.kind == "rq":
            k = (1 + self.p0 / self.p1 * d2) ** (-self.p1)
            return k.squeeze(0) if k.shape[0] == 1 else k
        if self.kind == "poly1":
            r = torch.where(d2 > 0, d2.clamp_min(1e-30).sqrt(), torch.zeros_like(d2))
            return r / self.p1
        raise ValueError(self.kind)


class TorchDHRobot:
    """differentiable torch FK of a single DH chain built from a diffco_amd robot's description"""

    def __init__(self, rob):
        import torch
        d = rob.fk_desc()
        n = d.chain_len[0]
        self.dof, self.limits = rob.dof, rob.limits
        g = lambda arr: torch.tensor([arr[0][i] for i in range(n)], dtype=torch.float64)
        self.a, self.d, self.sa, self.ca, self.t0 = g(d.a), g(d.d), g(d.sin_alpha), g(d.cos_alpha), g(d.theta0)
        self.frames = [d.pt_frame[k] for k in range(d.n_points)]
        self.offs = [[d.pt_off[k][j] for j in range(3)] for k in range(d.n_points)]

    def fkine(self, q, reuse=False):
        import torch
        q = q.reshape(-1, self.dof)
        T = torch.eye(4, dtype=q.dtype).expand(len(q), 4, 4)
        cum = []
        for i in range(self.dof):
            th = q[:, i] + self.t0[i].to(q.dtype)
            c, s = th.cos(), th.sin()
            z, o = torch.zeros_like(c), torch.ones_like(c)
            sa, ca, a, d = (t[i].to(q.dtype) for t in (self.sa, self.ca, self.a, self.d))
            A = torch.stack([torch.stack([c, -s * ca, s * sa, a * c], -1), torch.stack([s, c * ca, -c * sa, a * s], -1),
                             torch.stack([z, sa * o, ca * o, d * o], -1), torch.stack([z, z, z, o], -1)], 1)
            T = T @ A
            cum.append(T)
        pts = []
        for f, off in zip(self.frames, self.offs):
            v = torch.tensor(off + [1.0], dtype=q.dtype)
            pts.append((cum[f] @ v)[:, :3])
        return torch.stack(pts, 1)


# ---------------------------------------------------------------------------------------------
# random URDF trees (tests of the DCX_FK_TREE path beyond the reference's robot files)
def random_urdf_model(seed, n_links=9, max_children=2):
    """joint table of a random kinematic tree: revolute / continuous / prismatic / fixed joints, axes +-x/y/z (and
    off-axis vectors for prismatic joints), random origins, an occasional mimic joint"""
    rng = np.random.default_rng(seed)
    links = ["base"] + [f"l{i}" for i in range(1, n_links)]
    joints, n_children, movable = [], {ln: 0 for ln in links}, []
    for i in range(1, n_links):
        cands = [ln for ln in links[:i] if n_children[ln] < max_children]
        parent = cands[int(rng.integers(len(cands)))] if rng.random() < 0.4 else cands[-1]
        n_children[parent] += 1
        jtype = str(rng.choice(["revolute", "revolute", "continuous", "prismatic", "fixed"]))
        axis = [0.0, 0.0, 0.0]
        if jtype == "prismatic" and rng.random() < 0.5:
            axis = rng.standard_normal(3).round(3).tolist()
        else:
            axis[int(rng.integers(3))] = float(rng.choice([-1.0, 1.0]))
        xyz = (rng.standard_normal(3) * 0.3).round(4).tolist() if rng.random() < 0.85 else [0.0, 0.0, 0.0]
        rpy = (rng.uniform(-np.pi, np.pi, 3)).round(4).tolist() if rng.random() < 0.7 else [0.0, 0.0, 0.0]
        j = dict(name=f"j{i}", type=jtype, parent=parent, child=links[i], xyz=xyz, rpy=rpy, axis=axis, lower=None,
                 upper=None, mimic_joint=None, mimic_multiplier=1.0, mimic_offset=0.0)
        if jtype in ("revolute", "prismatic") and rng.random() < 0.8:
            j["lower"], j["upper"] = -1.5, 2.0
        if jtype != "fixed" and movable and rng.random() < 0.15:
            j["mimic_joint"] = movable[int(rng.integers(len(movable)))]
            j["mimic_multiplier"], j["mimic_offset"] = float(rng.choice([-1.0, 0.5, 2.0])), float(rng.uniform(-0.2, 0.2))
        elif jtype != "fixed":
            movable.append(j["name"])
        joints.append(j)
    return dict(links=links, joints=joints)


def reference_tree_fk(model, q):
    """independent float64 FK of a joint table, written from the URDF semantics the reference implements
    (rigid_body.py:82-140): link frame = parent frame * origin * motion; returns {link: [B, 3] origin positions}"""
    q = np.asarray(q, dtype=np.float64)
    B = len(q)

    def rot(axis_idx, ang):
        c, s, R = np.cos(ang), np.sin(ang), np.zeros((B, 3, 3))
        i, j, k = axis_idx, (axis_idx + 1) % 3, (axis_idx + 2) % 3
        R[:, i, i] = 1
        R[:, j, j], R[:, j, k], R[:, k, j], R[:, k, k] = c, -s, s, c
        return R

    f32 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)  # noqa: E731  (the reference stores fp32)
    child_joint = {j["child"]: j for j in model["joints"]}
    dof, dof_of = 0, {}
    for ln in model["links"]:  # dof order = link order
        j = child_joint.get(ln)
        if j is not None and j["type"] != "fixed" and j["mimic_joint"] is None:
            dof_of[j["name"]] = dof
            dof += 1
    frames = {}

    def frame(ln):
        if ln in frames:
            return frames[ln]
        j = child_joint.get(ln)
        if j is None:
            R, t = np.tile(np.eye(3), (B, 1, 1)), np.zeros((B, 3))
        else:
            Rp, tp = frame(j["parent"])
            r, p, y = f32(j["rpy"])
            one = lambda a, idx: rot(idx, np.full(B, a))  # noqa: E731
            Ro = one(y, 2) @ one(p, 1) @ one(r, 0)
            R, t = Rp @ Ro, tp + np.einsum("bij,j->bi", Rp, f32(j["xyz"]))
            if j["type"] != "fixed":
                src = j["mimic_joint"] or j["name"]
                v = q[:, dof_of[src]]
                if j["mimic_joint"] is not None:
                    v = v * j["mimic_multiplier"] + j["mimic_offset"]
                ax = f32(j["axis"])
                if j["type"] == "prismatic":
                    t = t + np.einsum("bij,j->bi", R, ax)[:, :] * v[:, None]
                else:
                    idx = 0 if abs(ax[0]) == 1 else 1 if abs(ax[1]) == 1 else 2
                    R = R @ rot(idx, np.sign(ax[idx]) * v)
        frames[ln] = (R, t)
        return frames[ln]

    return {ln: frame(ln)[1] for ln in model["links"]}, dof


# ---------------------------------------------------------------------------------------------
# motion checks and costs (dcx_check_motions, dcx_motion_cost): the samples of their rules and the fp64 referees
def motion_samples(qa, qb, res=None, max_step=None, open_end=False, dtype=np.float32, counts=None):
    """per edge (x [n, dof], t [n], u [dof] or None, target flags [n]): the samples of check_motions' rules (res: the points of
    line_predict; max_step: the points of utils.dense_path, open_end dropping the target), t_k the interpolation parameter
    (x_k = qa + t_k (qb - qa); float64) and u the unit direction under max_step (dx_k / dqb = t_k (I - u u^T) there).
    float32: formed operation by operation as the kernels form them.  float64: the same map in float64 - the differentiable
    restatement the chain rule is checked against; `counts` (samples per edge, target included) holds the counts fixed."""
    F = np.float32
    out = []
    for e, (a, b) in enumerate(zip(np.asarray(qa, dtype), np.asarray(qb, dtype))):
        if dtype == np.float64:
            d = b - a
            if res is not None:
                t = np.arange(res, dtype=np.float64) / res
                out.append((a[None] + t[:, None] * d[None], t, None, np.zeros(res, bool)))
                continue
            L = float(np.sqrt((d * d).sum()))
            steps = int(np.ceil(L / max_step)) if counts is None else int(counts[e]) - (0 if open_end else 1)
            steps = steps if L > 0 else 0
            t = np.arange(steps, dtype=np.float64) * max_step / L if L > 0 else np.zeros(0)
            u = d / L if L > 0 else np.zeros(len(d))
            p = a[None] + t[:, None] * d[None]
            tgt = np.zeros(steps, bool)
            if not open_end:
                p, t, tgt = np.concatenate([p, b[None]]), np.concatenate([t, [1.0]]), np.concatenate([tgt, [True]])
            out.append((p.reshape(-1, len(a)), t, u, tgt))
            continue
        d = (b - a).astype(F)
        if res is not None:
            k = np.arange(res, dtype=F)
            p = (a[None] + d[None] * (k / F(res))[:, None]).astype(F)
            out.append((p, k.astype(np.float64) / res, None, np.zeros(res, bool)))
            continue
        l2 = F(0)
        for v in d:
            l2 = F(l2 + F(v * v))
        L = F(np.sqrt(l2))
        steps = int(np.ceil(F(L * F(F(1) / F(max_step)))))
        frac = F(F(F(1) / L) * F(max_step)) if L > 0 else F(0)   # (L = 0: no interior sample)
        k = np.arange(steps, dtype=F)
        p = (a[None] + k[:, None] * (d * frac)[None]).astype(F)
        t = k.astype(np.float64) * max_step / float(L) if L > 0 else np.zeros(0)
        u = d.astype(np.float64) / float(L) if L > 0 else np.zeros(len(d))
        tgt = np.zeros(steps, bool)
        if not open_end:
            p = np.concatenate([p, b[None]]).astype(F)
            t = np.concatenate([t, [1.0]])
            tgt = np.concatenate([tgt, [True]])
        out.append((p.reshape(-1, len(a)), t, u, tgt))
    return out


def motion_points(qa, qb, res=None, max_step=None, open_end=False):
    """every edge's fp32 samples (motion_samples' points alone)"""
    return [p for p, *_ in motion_samples(qa, qb, res, max_step, open_end)]


def motion_chain(samples, s, g, weight):
    """fp64 cost and endpoint gradients from per-sample hinge values s [N] and gradients g [N, dof] (already d(w h)/dx)"""
    cost, ga, gb, i = [], [], [], 0
    for p, t, u, tgt in samples:
        n = len(p)
        se, ge = s[i:i + n], g[i:i + n]
        i += n
        cost.append(weight * se.sum())
        if u is None:   # res rule
            gb.append((t[:, None] * ge).sum(0))
            ga.append(((1 - t)[:, None] * ge).sum(0))
            continue
        P = np.eye(len(u)) - np.outer(u, u)
        inner = ~tgt
        T = P @ (t[inner][:, None] * ge[inner]).sum(0)
        gb.append(T + ge[tgt].sum(0))
        ga.append(ge[inner].sum(0) - T)
    return np.array(cost), np.array(ga), np.array(gb)


def motion_scores(desc, kern, sup, W, samples):
    """fp64 oracle scores [N, C] of every edge's samples, concatenated"""
    from oracle import oracle
    flat = np.concatenate([p for p, *_ in samples]) if samples else np.zeros((0, desc.dof), np.float32)
    return oracle.score_grad(desc, kern[0], kern[1], kern[2], sup, W, flat, dtype=np.float64)[0]


def motion_oracle(desc, kern, sup, W, samples, margin, weight=1.0, scores=None, grad=True):
    """the fp64 referee of both motion calls on the given samples, a dict: per edge 'first' (first index with some
    score_c - margin_c > 0, -1 if none), 'tie' (some sample within 1e-4 max|s| of a margin), 'cost', 'ga', 'gb' (the chain
    on the host; grad=True) and the scales 'abs_s' (sum over samples and classes of |s_c|) and 'g_inf' (sum over samples of
    ||d(w h)/dx_k||_inf); per sample 's' [N, C] and 'g' [N, dof]"""
    from oracle import oracle
    flat = np.concatenate([p for p, *_ in samples]) if samples else np.zeros((0, desc.dof), np.float32)
    C = np.asarray(W).reshape(len(sup), -1).shape[1]
    mg = np.broadcast_to(np.asarray(margin, np.float64).reshape(-1), (C,))
    s = motion_scores(desc, kern, sup, W, samples) if scores is None else scores
    band = 1e-4 * np.abs(s).max(initial=0)
    out = dict(s=s)
    first, tie, abs_s, i = [], [], [], 0
    for p, *_ in samples:
        se = s[i:i + len(p)] - mg
        i += len(p)
        hit = (se > 0).any(axis=1)
        first.append(int(np.argmax(hit)) if hit.any() else -1)
        tie.append(bool((np.abs(se) <= band).any()))
        abs_s.append(float(np.abs(se + mg).sum()))
    out.update(first=np.array(first, int), tie=np.array(tie, bool), abs_s=np.array(abs_s))
    if grad:
        up = (s - mg > 0).astype(np.float64) * weight
        _, g, _ = oracle.score_grad(desc, kern[0], kern[1], kern[2], sup, W, flat, upstream=up, dtype=np.float64)
        h = np.clip(s - mg, 0, None).sum(1)
        out["cost"], out["ga"], out["gb"] = motion_chain(samples, h, g, weight)
        out["g"] = g
        ends = np.cumsum([0] + [len(p) for p, *_ in samples])
        gi = np.abs(g).max(axis=1, initial=0) if len(g) else np.zeros(0)
        out["g_inf"] = np.array([gi[ends[k]:ends[k + 1]].sum() for k in range(len(samples))])
    return out


def motion_oracle_first(desc, kern, sup, W, pts, margin):
    """(first colliding index per edge by the fp64 oracle, edges inside the tie band) of the fp32 points pts (one array per edge)"""
    r = motion_oracle(desc, kern, sup, W, [(p, None, None, None) for p in pts], margin, grad=False)
    return r["first"], r["tie"]


def motion_oracle_cost(desc, kern, sup, W, samples, margin, weight):
    """(cost, grad_a, grad_b, tie flags) in fp64: scores and per-class hinge gradients by the oracle, the chain on the host"""
    r = motion_oracle(desc, kern, sup, W, samples, margin, weight)
    return r["cost"], r["ga"], r["gb"], r["tie"]


# ---------------------------------------------------------------------------------------------
# the shape fuzz (tests/test_gpu_fuzz.py): kernels, transforms and the motion calls' case table - plain data, importable
# without a GPU (tests/test_motion_referee.py checks what the table covers)
KERNELS = [(0, 10.0, 2.0), (1, 1.0, 1.0), (0, 3.0, 3.0), (1, 3.0, 2.0), (1, 2.0, 1.0), (2, 0.7, 0.0)]

# robots of the fuzz by name: their feature width is fixed, the case table names it as D
FUZZ_ROBOTS = {"baxter": lambda: make_robot("baxter_left"), "baxter_dual": lambda: make_robot("baxter_dual"),
               "panda": lambda: make_robot("panda"), "panda5": lambda: make_robot("panda5"),
               "dual_panda": lambda: make_robot("dual_panda"), "urdf_dual_panda": lambda: dual_panda_robot()}
FUZZ_ROBOTS.update({n: (lambda n=n: urdf_robot(n)) for n in URDF_NAMES})


def kernel_family(kind, p0, p1):
    """the sweep's kernel function family for a kernel (the model's rule: 0 KF_RQ2, 1 KF_POLY1, 2 KF_GEN)"""
    return 0 if (kind == 0 and p1 == 2.0) else 1 if (kind == 1 and p0 == 1.0) else 2


def fuzz_desc(kind, D, rng):
    """(FK description, dof, configuration limits [dof, 2]) of a fuzz case: the identity transform (D = dof), a planar arm
    (D = 2 dof), SE(2) / SE(3) bodies with D / 2, D / 3 random keypoints, or one of FUZZ_ROBOTS (D = its feature width)"""
    from diffco_amd import _fkdesc as fd
    box = lambda dof: np.tile([-1.5, 1.5], (dof, 1))  # noqa: E731
    if kind == "none":
        return fd.none_desc(D), D, box(D)
    if kind == "planar":  # D = 2 * dof
        return fd.planar_desc((0.2 + rng.random(D // 2)).tolist()), D // 2, box(D // 2)
    if kind == "se3":
        kp = rng.uniform(-0.5, 0.5, (D // 3, 3))  # SE(3) body with D / 3 keypoints
        return fd.keypoint_desc(kp, 3), 6, box(6)
    if kind == "se2":
        kp = rng.uniform(-0.5, 0.5, (D // 2, 2))
        return fd.keypoint_desc(kp, 2), 3, box(3)
    rob = FUZZ_ROBOTS[kind]()
    lim = np.asarray(rob.limits, np.float64)
    return rob.fk_desc(), rob.dof, lim


# (kind, D, C, kernel index into KERNELS, rule, runs of empty edges) for dcx_check_motions and dcx_motion_cost.  rule: "res"
# (res in 7 .. 13), "closed" (max_step) or "open" (max_step with open_end: motion costs; the checks take the closed rule).
# Padded widths: D below its compiled width (dcx_internal.h kTemplateD).  Empty runs: > 64 consecutive edges without samples
# inside one tile (over max_samples; zero length under open_end), between normal edges.
MOTION_CASES = [
    ("none", 2, 3, 1, "res", False), ("none", 3, 6, 2, "closed", False), ("none", 5, 1, 0, "open", False),
    ("none", 7, 8, 5, "res", False), ("none", 7, 1, 1, "open", True), ("none", 13, 2, 3, "closed", False),
    ("none", 17, 4, 4, "open", False), ("none", 19, 7, 0, "res", False), ("none", 29, 5, 1, "closed", False),
    ("none", 31, 1, 2, "open", False), ("none", 32, 6, 0, "res", False),
    ("planar", 4, 2, 0, "closed", False), ("planar", 36, 3, 5, "open", False), ("planar", 48, 1, 1, "res", False),
    ("planar", 60, 5, 2, "closed", False), ("planar", 64, 1, 0, "open", False),
    ("se2", 6, 4, 0, "res", False), ("se2", 8, 1, 4, "closed", False), ("se2", 30, 8, 1, "open", False),
    ("se3", 24, 2, 5, "res", False), ("se3", 27, 1, 1, "closed", False), ("se3", 33, 4, 0, "open", False),
    ("se3", 45, 6, 3, "res", False), ("se3", 51, 1, 4, "closed", False), ("se3", 69, 3, 1, "open", False),
    ("se3", 72, 7, 5, "res", False), ("se3", 78, 2, 0, "closed", False), ("se3", 90, 1, 2, "open", False),
    ("se3", 96, 4, 1, "res", False),
    ("baxter", 12, 1, 1, "open", True), ("baxter", 12, 5, 0, "closed", False), ("panda", 21, 3, 0, "res", False),
    ("panda5", 15, 1, 2, "open", False), ("baxter_dual", 24, 8, 1, "closed", False), ("dual_panda", 42, 1, 0, "res", False),
    ("urdf_panda", 27, 2, 1, "open", False), ("urdf_panda_nogripper", 18, 6, 5, "res", False),
    ("urdf_iiwa7", 24, 1, 0, "closed", False), ("urdf_trifinger", 39, 5, 1, "open", False),
    ("urdf_jaco", 42, 7, 3, "res", False), ("urdf_2link", 9, 4, 1, "closed", False),
    ("urdf_allegro", 60, 1, 1, "open", True), ("urdf_fetch", 63, 8, 0, "res", False),
    ("urdf_dual_panda", 54, 1, 5, "closed", False), ("urdf_iiwa7_allegro", 84, 5, 0, "open", False),
]


def template_widths():
    """the compiled feature widths, parsed from dcx_internal.h kTemplateD"""
    import re
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "diffco_amd", "csrc", "dcx_internal.h")).read()
    m = re.search(r"kTemplateD\[\]\s*=\s*\{([^}]*)\}", src)
    assert m, "kTemplateD not found in dcx_internal.h"
    return [int(x) for x in m.group(1).split(",")]


def template_d_for(D, widths=None):
    """the compiled width a feature width D runs at (dcx_internal.h template_d_for)"""
    return next(w for w in (widths or template_widths()) if D <= w)


def motion_cases(entry):
    """the cases the shape fuzz runs for one entry point: "check" (dcx_check_motions) or "cost" (dcx_motion_cost)"""
    assert entry in ("check", "cost")
    return list(MOTION_CASES)
