"""Helpers of the dense-check trajectory tests (test_gpu_traj_dense.py): small fixtures - a robot, a few dozen
supports, paths that cross them - and the float64 restatement of one iteration of the dense-check Adam loop (include/dcx.h,
dcx_traj_dense_run), everything on the CPU: the collision term and its endpoint gradients from helpers.motion_samples /
motion_oracle on the fp64 oracle, the rest in torch float64 on the oracle's FK."""
import numpy as np
import torch

from helpers import make_robot, motion_oracle, motion_samples, random_urdf_model, urdf_xml

F = np.float32
KERNELS = {"poly": (1, 1.0, 1.0), "rq": (0, 10.0, 2.0)}


def robot(name):
    if name == "baxter":
        return make_robot("baxter_left")
    if name == "planar3":
        return make_robot("planar3")
    from diffco_amd.urdf import URDFRobotFK
    rob = URDFRobotFK(urdf_xml(random_urdf_model(1003, n_links=8)))
    assert rob.dof >= 3 and rob.fk_desc().kind == 5 and rob.fk_desc().t_coord_major
    return rob


MAX_STEP = 0.11


class Fixture:
    """robot `name`, S supports with C weight columns under kernel `kern`, R paths of W waypoints that pass the supports, and a
    margin per class below part of the scores along them.  The paths are random walks whose segment lengths are (k + 1/2) *
    MAX_STEP, k = 1 .. 4: sampled at MAX_STEP no length is near a multiple of the stride, and a few Adam steps of a small lr
    (each moves a segment's length by at most 2 sqrt(dof) lr) keep it so.  quirks: path 1 repeats a waypoint (an open edge with
    no samples), path 2 is shifted until a waypoint lies outside the joint limits."""

    def __init__(self, name, kern, C, R, W, S=60, seed=0, quirks=True):
        from oracle import oracle
        self.rob = robot(name)
        self.desc, self.kern, self.C, self.R, self.W = self.rob.fk_desc(), KERNELS[kern], C, R, W
        dof = self.dof = self.rob.dof
        g = np.random.default_rng(seed)
        lim = self.rob.limits.numpy().astype(np.float64)
        lo, hi = np.maximum(lim[:, 0], -2.0), np.minimum(lim[:, 1], 2.0)
        dirn = g.normal(size=(R, W - 1, dof))
        dirn /= np.linalg.norm(dirn, axis=2, keepdims=True)
        length = (g.integers(1, 5, (R, W - 1, 1)) + 0.5) * MAX_STEP
        if quirks and W >= 5 and R > 1:
            length[1, 1] = 0.0                                   # path 1: waypoint 2 repeats waypoint 1
        paths = np.concatenate([g.uniform(lo, hi, (R, 1, dof)), dirn * length], axis=1).cumsum(axis=1)
        if quirks and W >= 5 and R > 2:
            paths[2, :, 0] += lim[0, 1] + 0.1 - paths[2, 3, 0]   # path 2: waypoint 3 outside the joint limits
        self.paths = paths.astype(F)
        # supports on and around the paths, so that samples of every path are above their margin
        pick = self.paths.reshape(-1, dof)[g.integers(0, R * W, S)]
        self.sup_q = (pick + 0.25 * g.normal(size=(S, dof))).astype(F)
        self.sup = oracle.fkine(self.desc, self.sup_q, F)
        self.weights = (g.normal(size=(S, C)) * (0.05 if kern == "poly" else 1.0)).astype(F)
        s = oracle.score_grad(self.desc, *self.kern, self.sup, self.weights, self.paths.reshape(-1, dof), dtype=np.float64)[0]
        # per class: half-way between two neighbouring waypoint scores, at most the 60th percentile of any path's own
        s = np.sort(s.reshape(R, W, C), axis=1)
        k = min(W - 2, int(0.6 * W))
        self.margin = (0.5 * (s[:, k] + s[:, k + 1])).min(axis=0).astype(F)
        self.limits = self.rob.limits.float()

    def model(self, ops):
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")
        return ops.ScoreModel(self.desc, *self.kern, t(self.sup), t(self.weights))


class _OracleFK(torch.autograd.Function):
    """the fp64 oracle's FK with its vjp: [W, dof] -> [W, D] in the transform's own feature layout"""

    @staticmethod
    def forward(ctx, desc, q):
        from oracle import oracle
        ctx.desc = desc
        ctx.save_for_backward(q)
        return torch.from_numpy(oracle.fkine(desc, q.detach().numpy(), np.float64))

    @staticmethod
    def backward(ctx, gX):
        from oracle import oracle
        (q,) = ctx.saved_tensors
        return None, torch.from_numpy(oracle.fkine_vjp(ctx.desc, q.detach().numpy(), gX.contiguous().numpy(), np.float64))


def control_points(desc, q):
    """[W, n_points, point_dim] float64, differentiable"""
    X = _OracleFK.apply(desc, q)
    if desc.kind == 5 and desc.t_coord_major:
        return X.reshape(len(q), desc.point_dim, desc.n_points).transpose(1, 2)
    return X.reshape(len(q), desc.n_points, desc.point_dim)


def dense_collision(fx, p, max_step, margin, normalize):
    """the collision term of path p [W, dof] (float64 values, sampled as fp32 like the device samples them): (collision,
    gradient [W, dof] of it, per-slot sample counts [W] in the layout e = w, and the smallest |score_c - margin_c| of any sample
    relative to max |score|: above the fp32 sweep's rounding, fp32 and fp64 agree on which hinges are active)"""
    W = len(p)
    p32 = np.asarray(p, F)
    smp = motion_samples(p32[:-1], p32[1:], max_step=max_step, open_end=True) + \
        motion_samples(p32[-1:], p32[-1:], max_step=max_step, open_end=False)
    r = motion_oracle(fx.desc, fx.kern, fx.sup, fx.weights, smp, margin, 1.0)
    counts = np.array([len(x) for x, *_ in smp])
    n_r = int(counts.sum())
    f = W / (n_r * fx.C) if normalize else 1.0
    g = np.zeros((W, fx.dof))
    g[:W - 1] += r["ga"][:W - 1]
    g[1:] += r["gb"][:W - 1]
    g[W - 1] += r["gb"][W - 1]
    gap = float(np.abs(r["s"] - np.asarray(margin, np.float64).reshape(1, -1)).min() / np.abs(r["s"]).max())
    return float(r["cost"].sum()) * f, g * f, counts, gap


def dense_step(fx, p, m, v, t, lr, max_step, max_speed, margin, normalize, weights=(1.0, 10.0, 10.0, 10.0), move=None,
               betas=(0.9, 0.999), eps=1e-8):
    """one iteration in float64: new p, m, v, the seven loss terms of stats[r, :7], the gradient, the per-slot sample counts, the hinge gap"""
    w_diff, w_col, w_mm, w_jl = weights
    col, g_col, counts, gap = dense_collision(fx, p.numpy(), max_step, margin, normalize)
    q = p.clone().requires_grad_(True)
    cp = control_points(fx.desc, q)
    seg = (cp[1:] - cp[:-1]).square().sum(dim=2)
    mm = torch.clamp(seg - max_speed ** 2, min=0).sum()
    lim = fx.limits.double()
    jl = (torch.clamp(lim[:, 0] - q, min=0) + torch.clamp(q - lim[:, 1], min=0)).sum()
    diff = seg.sum()
    rest = w_diff * diff + w_mm * mm + w_jl * jl
    (g,) = torch.autograd.grad(rest, q)
    g = g + w_col * torch.from_numpy(g_col)
    if move is None:
        g[[0, -1]] = 0.0
    else:
        g[~torch.as_tensor(move, dtype=torch.bool)] = 0.0
    m = betas[0] * m + (1 - betas[0]) * g
    v = betas[1] * v + (1 - betas[1]) * g * g
    denom = v.sqrt() / np.sqrt(1 - betas[1] ** t) + eps
    pn = p - lr / (1 - betas[0] ** t) * m / denom
    constraint = w_col * col + w_mm * mm + w_jl * jl
    terms = torch.stack([w_diff * diff + constraint, w_diff * diff, constraint, g.norm(), torch.tensor(col, dtype=torch.float64), mm, jl]).detach()
    return pn.detach(), m, v, terms, g, counts, gap


def off_multiples(p, max_step, rel=1e-3):
    """no segment's length within `rel` relative of a positive multiple of max_step: the fp32 and fp64 sample counts cannot
    differ"""
    L = np.linalg.norm(np.diff(np.asarray(p, np.float64), axis=0), axis=1)
    x = L[L > 0] / max_step
    near = np.round(x)   # (below half a stride the count is 1 whatever the rounding: the multiple 0 is no threshold)
    return bool(((near == 0) | (np.abs(x - near) > rel * x)).all())


def dense_state(model, limits, paths):
    """device buffers + ctypes state of R paths for the dense calls (col_score / col_grad NULL: not read)"""
    import ctypes as C
    from diffco_amd import _lib
    R, W, dof = paths.shape
    dev = model.dev
    f32 = dict(device=dev, dtype=torch.float32)
    path = torch.as_tensor(paths).to(**f32).contiguous().clone()
    b = dict(path=path, adam_m=torch.zeros_like(path), adam_v=torch.zeros_like(path), limits=limits.to(**f32).contiguous(),
             stats=torch.zeros((R, 8), **f32), lowest_loss=torch.full((R,), float("inf"), **f32),
             lowest_obj=torch.full((R,), float("inf"), **f32), lowest_path=path.clone(),
             best_valid_obj=torch.full((R,), float("inf"), **f32), best_valid_path=path.clone(),
             done=torch.zeros(R, device=dev, dtype=torch.int32), steps=torch.zeros(R, device=dev, dtype=torch.int32),
             n_checks=torch.zeros(R, device=dev, dtype=torch.int64), edge_cost=torch.zeros(R * W, **f32),
             grad_a=torch.zeros((R * W, dof), **f32), grad_b=torch.zeros((R * W, dof), **f32),
             n_samples=torch.zeros(R * W, device=dev, dtype=torch.int32))
    p = lambda k: C.c_void_p(b[k].data_ptr()) if b[k].numel() else None
    st = _lib.TrajState(R, W, p("path"), p("adam_m"), p("adam_v"), p("limits"), None, None, p("stats"), p("lowest_loss"),
                        p("lowest_obj"), p("lowest_path"), p("best_valid_obj"), p("best_valid_path"), p("done"), p("steps"))
    return st, b


def dense_io(b, move=None, history=None, edges=True):
    import ctypes as C
    from diffco_amd import _lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    e = [p(b[k]) if edges else None for k in ("edge_cost", "grad_a", "grad_b", "n_samples")]
    return _lib.TrajDenseIO(p(move), p(history), p(b["n_checks"]), *e)


def dense_run(lib, model, st, opt, dopt, io, margin_dev, first_step, n_iters, work=None):
    """dcx_traj_dense_run on torch's current stream with a workspace of the size the library asks for"""
    import ctypes as C
    from diffco_amd import _lib
    need = int(lib.dcx_traj_dense_work_bytes(model._h, st.n_paths, st.n_waypoints, dopt.max_samples))
    if work is None:
        work = torch.empty(max(need, 1), device=model.dev, dtype=torch.uint8)
    _lib.check(lib.dcx_traj_dense_run(model._h, C.byref(st), C.byref(opt), C.byref(dopt), C.byref(io),
                                      C.c_void_p(margin_dev.data_ptr()) if margin_dev is not None else None, first_step, n_iters,
                                      C.c_void_p(work.data_ptr()), need, model._st()))
    return work
