"""The case table, inputs and float64 referee of the trajectory fuzz (tests/test_gpu_traj_fuzz.py; tests/test_traj_referee.py
checks the referee and what the table covers).  Plain data and numpy on the CPU oracle, importable without a GPU.

A case is one (transform, feature width, class count, kernel, waypoints, paths) point of dcx_traj_adam_run / dcx_traj_adam_run_mc.
Its hinges are tie-free BY CONSTRUCTION: the per-class margins and max_speed^2 sit in the middle of the widest gap between the
30 % and 70 % quantiles of the referee's scores / squared segment lengths, and that half-gap is at least 32 x the largest
difference between the oracle run in fp32 and in fp64 on the same inputs - so an fp32 kernel whose error is of the order of the fp32
oracle's cannot see another set of active hinges than the referee.  Nothing is dropped from any case.  Joint limits need no band:
paths and limits are fp32 values in both arithmetics."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from helpers import KERNELS, fuzz_desc, kernel_family, template_d_for

F = np.float32
S_SUPPORTS = 150
BAND_FACTOR = 32.0
LDS_BYTES = 160 * 1024   # a CU's LDS (gfx950)

# bitwise: the persistent kernel and the launch loop take the same support slices under pinned knobs, so (e) holds them to equal
# bits; False carries the reason in one line (the fp64 legs apply either way)
TrajCase = namedtuple("TrajCase", "kind D C ki W R bitwise reason", defaults=(True, ""))

_NO_MC = "no persistent instantiation for several classes at this width / kernel function: both settings run the launch loop"
_LONG = "W > 64: no persistent form, both settings run the launch loop"
_NO_FIT = "the persistent carve (traj_fused_plan) exceeds 150 KB at every nw for this tree: both settings run the launch loop"

TRAJ_CASES = [
    TrajCase("none", 2, 3, 1, 3, 3), TrajCase("planar", 4, 2, 0, 2, 1), TrajCase("se2", 6, 4, 0, 64, 3),
    TrajCase("se2", 8, 1, 4, 20, 3), TrajCase("baxter", 12, 1, 0, 63, 3), TrajCase("baxter", 12, 5, 1, 33, 3),
    TrajCase("panda5", 15, 1, 2, 30, 3), TrajCase("urdf_panda_nogripper", 18, 6, 5, 20, 3, False, _NO_MC),
    TrajCase("panda", 21, 3, 0, 40, 3), TrajCase("baxter_dual", 24, 8, 1, 30, 3),
    TrajCase("none", 13, 2, 3, 65, 3, False, _LONG), TrajCase("none", 7, 7, 0, 130, 3, False, _LONG),
    TrajCase("urdf_panda", 27, 2, 1, 50, 3, False, _NO_MC), TrajCase("se2", 30, 8, 1, 25, 1, False, _NO_MC),
    TrajCase("none", 31, 1, 2, 45, 3), TrajCase("planar", 36, 3, 5, 18, 3, False, _NO_MC),
    TrajCase("dual_panda", 42, 1, 0, 22, 3), TrajCase("planar", 48, 1, 1, 24, 3),
    TrajCase("se3", 51, 1, 4, 40, 3), TrajCase("urdf_dual_panda", 54, 1, 5, 16, 3),
    TrajCase("planar", 60, 5, 2, 30, 3, False, _NO_MC), TrajCase("urdf_fetch", 63, 8, 0, 12, 3, False, _NO_MC),
    TrajCase("planar", 64, 1, 0, 64, 3), TrajCase("se3", 72, 1, 1, 65, 3, False, _LONG),
    TrajCase("urdf_iiwa7_allegro", 84, 5, 0, 10, 3, False, _NO_MC), TrajCase("se3", 90, 1, 2, 12, 1),
    # one class on the 84-wide tree: the instantiation exists, the carve does not fit (traj_run's fallback to the launch loop)
    TrajCase("urdf_iiwa7_allegro", 84, 1, 1, 12, 3, False, _NO_FIT),
    # a two-chain arm with >= 120 active supports: traj_run's rule gives 8 waves, the several-wave J^T route with both chains
    TrajCase("baxter_dual", 24, 1, 3, 20, 3),
    TrajCase("se3", 96, 4, 1, 20, 3, False, _NO_MC),
]


def case_id(c):
    return f"{c.kind}-D{c.D}-C{c.C}-k{c.ki}-W{c.W}-R{c.R}"


def case_rng(case, what="traj"):
    return np.random.default_rng(zlib.crc32(repr((what,) + tuple(case[:6])).encode()))   # deterministic across processes


def step_carve_bytes(dof, D, frame_floats, W, prog_floats=2048):
    """traj_kernels.hip traj_lds_bytes with nw = ceil(W / 64) slabs; prog_floats: an upper bound of the staged FK program"""
    nw = (W + 63) // 64
    return 4 * (prog_floats + 2 * nw * 64 * dof + 2 * nw * 64 * D + nw * 64 * frame_floats + 128)


def points_of(desc, X):
    """features [N, D] in the transform's own layout -> control points [N, n_points, point_dim] (URDF trees are coord-major)"""
    X = np.asarray(X).reshape(len(X), -1)
    if int(desc.kind) == 5 and desc.t_coord_major:
        return X.reshape(len(X), desc.point_dim, desc.n_points).transpose(0, 2, 1)
    return X.reshape(len(X), desc.n_points, desc.point_dim)


def features_of(desc, P):
    """the inverse of points_of: [N, n_points, point_dim] -> [N, D]"""
    if int(desc.kind) == 5 and desc.t_coord_major:
        return np.ascontiguousarray(P.transpose(0, 2, 1)).reshape(len(P), -1)
    return np.ascontiguousarray(P).reshape(len(P), -1)


def traj_paths(case, rng, lim=None, dof=None):
    """fp32 paths [R, W, dof]: a straight line between two random configurations with the second pulled to 30 % of the way, plus
    0.01 span noise; about 30 % of the waypoints displaced by 0.25 span N(0, 1) (segment lengths spread out).  W >= 5: waypoint 2
    above every upper limit by 0.2, waypoint 3 below the even joints' lower limits by 0.1, and path 0 repeats its first waypoint (a
    zero-length segment).  Shorter paths: the last waypoint of path 0 above the upper limits, its first below the even lower ones."""
    if lim is None:
        _, dof, lim = fuzz_desc(case.kind, case.D, case_rng(case, "desc"))
        lim = usable_limits(lim)
    R, W = case.R, case.W
    lo, hi = lim[:, 0], lim[:, 1]
    span = hi - lo
    a, far = rng.uniform(lo, hi, (R, 1, dof)), rng.uniform(lo, hi, (R, 1, dof))
    b = a + 0.3 * (far - a)
    t = np.linspace(0.0, 1.0, W)[None, :, None]
    p = a * (1 - t) + b * t + 0.01 * span * rng.standard_normal((R, W, dof))
    moved = rng.random((R, W)) < 0.3
    p = p + moved[:, :, None] * 0.25 * span * rng.standard_normal((R, W, dof))
    if W >= 5:
        p[:, 2] = hi + 0.2
        p[:, 3, 0::2] = lo[0::2] - 0.1
        p[0, 1] = p[0, 0]
    else:
        p[0, W - 1] = hi + 0.2
        p[0, 0, 0::2] = lo[0::2] - 0.1
    return p.astype(F)


def usable_limits(lim):
    """the case's joint limits [dof, 2] as the fp32 values the kernel is handed (continuous joints: a finite box)"""
    return np.clip(np.asarray(lim, np.float64), -2.5, 2.5).astype(F).astype(np.float64)


def default_opts(margin=0.0, max_speed=0.3, **kw):
    """dcx_traj_opts as a dict, every entry the fp32 value the kernel sees (reference weights 1, 10, 10, 10)"""
    o = dict(lr=0.02, beta1=0.9, beta2=0.999, eps=1e-8, w_diff=1.0, w_collision=10.0, w_max_move=10.0, w_joint_limit=10.0,
             safety_margin=margin, max_speed=max_speed, valid_tol=1e-2, grad_tol=1e-4)
    o.update(kw)
    return {k: float(F(v)) for k, v in o.items()}


OPT_FIELDS = ("lr", "beta1", "beta2", "eps", "w_diff", "w_collision", "w_max_move", "w_joint_limit", "safety_margin", "max_speed",
              "valid_tol", "grad_tol")


def adam_update(q, g, m0, v0, t, o):
    """the scalar Adam update of traj_adam_step_kernel in float64: (m, v, new q)"""
    m = o["beta1"] * m0 + (1.0 - o["beta1"]) * g
    v = o["beta2"] * v0 + (1.0 - o["beta2"]) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - o["beta2"] ** t) + o["eps"]
    return m, v, q - o["lr"] / (1.0 - o["beta1"] ** t) * m / denom


def traj_terms(desc, kern, sup, weights, limits32, path, margin, opts, want_grad=True):
    """float64 loss terms (include/dcx.h, dcx_traj_state) of ONE path [W, dof] and the gradient of the loss with both endpoints
    zeroed, from oracle.score_grad(want_jac=True), oracle.fkine and oracle.fkine_vjp alone.  A dict: stats [7] (loss, objective,
    constraint, |grad|, collision, max_move, joint_limit), g [W, dof], s [W, C] (scores), seg [W - 1, n_points] (squared segment
    lengths per control point)"""
    from oracle import oracle
    q = np.asarray(path, np.float64)
    Wp, dof = q.shape
    C = np.asarray(weights).reshape(len(sup), -1).shape[1]
    mg = np.broadcast_to(np.asarray(margin, np.float64).reshape(-1), (C,))
    s, _, jac = oracle.score_grad(desc, kern[0], kern[1], kern[2], sup, weights, q, want_jac=True, dtype=np.float64)
    act = (s - mg) > 0
    col = np.where(act, s - mg, 0.0).sum()
    P = points_of(desc, oracle.fkine(desc, q, dtype=np.float64))
    d = P[1:] - P[:-1]
    seg = (d * d).sum(axis=2)
    ms2 = opts["max_speed"] ** 2   # (the kernel squares the same fp32 value in fp32: traj_setup takes that ulp off the half-gap)
    over = (seg - ms2) > 0
    diff, mm = seg.sum(), np.where(over, seg - ms2, 0.0).sum()
    lo, hi = np.asarray(limits32, np.float64)[:, 0], np.asarray(limits32, np.float64)[:, 1]
    below, above = q < lo, q > hi
    jl = np.where(below, lo - q, 0.0).sum() + np.where(above, q - hi, 0.0).sum()
    objective = opts["w_diff"] * diff
    constraint = opts["w_collision"] * col + opts["w_max_move"] * mm + opts["w_joint_limit"] * jl
    out = dict(s=s, seg=seg, active=act)
    g = np.zeros_like(q)
    if want_grad:
        coef = 2.0 * (opts["w_diff"] + opts["w_max_move"] * over)[:, :, None] * d      # d loss / d (P[w + 1] - P[w])
        gP = np.zeros_like(P)
        gP[1:] += coef
        gP[:-1] -= coef
        g = oracle.fkine_vjp(desc, q, features_of(desc, gP), dtype=np.float64)
        g = g + opts["w_collision"] * (act[:, :, None] * jac).sum(axis=1)
        g = g + opts["w_joint_limit"] * (above.astype(np.float64) - below.astype(np.float64))
        g[0] = 0.0
        g[-1] = 0.0
    out["g"] = g
    out["stats"] = np.array([objective + constraint, objective, constraint, np.sqrt((g * g).sum()), col, mm, jl])
    return out


def traj_referee(desc, kern, sup, W, limits32, path, margin, opts, m0, v0, t):
    """one Adam step of one path in float64 (see traj_terms), from the moments m0, v0 at 1-based step t: traj_terms' dict plus m, v
    and q_new"""
    out = traj_terms(desc, kern, sup, W, limits32, path, margin, opts)
    out["m"], out["v"], out["q_new"] = adam_update(np.asarray(path, np.float64), out["g"], np.asarray(m0, np.float64),
                                                   np.asarray(v0, np.float64), t, opts)
    return out


def widest_gap(values):
    """(midpoint, half-gap) of the widest gap between neighbouring values from the 30 % to the 70 % quantile of `values`"""
    v = np.sort(np.asarray(values, np.float64).reshape(-1))
    n = len(v)
    if n == 1:
        return 0.5 * v[0], 0.5 * abs(v[0])
    i0, i1 = int(np.floor(0.3 * (n - 1))), int(np.ceil(0.7 * (n - 1)))
    if i1 == i0:
        i0, i1 = max(i0 - 1, 0), min(i0 + 1, n - 1)
    gaps = np.diff(v[i0:i1 + 1])
    k = int(np.argmax(gaps))
    return 0.5 * (v[i0 + k] + v[i0 + k + 1]), 0.5 * gaps[k]


def _nearest_f32_inside(mid, half):
    """the fp32 value nearest to `mid` and how far the neighbouring values then are: (value, remaining half-gap)"""
    x = float(F(mid))
    return x, half - abs(x - mid)


@functools.lru_cache(maxsize=None)
def traj_setup(case):
    """everything one case is run and judged with, computed once: desc, dof, kern, sup [S, D] fp32, weights [S, C] fp32, limits32
    [dof, 2], paths [R, W, dof] fp32, margin [C] and max_speed (fp32 values), the half-gaps around them (`gap_s` [C], `gap_seg`) and
    the largest fp32-versus-fp64 difference of the oracle on the same inputs (`err_s`, `err_seg`), opts (default_opts with this
    case's margin[0] and max_speed)"""
    from oracle import oracle
    rng = case_rng(case)
    desc, dof, lim = fuzz_desc(case.kind, case.D, case_rng(case, "desc"))
    lim = usable_limits(lim)
    kern = KERNELS[case.ki]
    sup_q = rng.uniform(lim[:, 0], lim[:, 1], (S_SUPPORTS, dof)).astype(F)
    sup = oracle.fkine(desc, sup_q, dtype=F).reshape(S_SUPPORTS, -1)
    assert sup.shape[1] == case.D, (case, sup.shape)
    weights = (0.05 * rng.standard_normal((S_SUPPORTS, case.C))).astype(F)
    weights[rng.random((S_SUPPORTS, case.C)) < 0.2] = 0.0
    paths = traj_paths(case, rng, lim, dof)
    flat = paths.reshape(-1, dof)
    s64 = oracle.score_grad(desc, *kern, sup, weights, flat, dtype=np.float64)[0]
    s32 = oracle.score_grad(desc, *kern, sup, weights, flat, dtype=F)[0]
    err_s = float(np.abs(s32.astype(np.float64) - s64).max())
    P64 = points_of(desc, oracle.fkine(desc, flat, dtype=np.float64)).reshape(case.R, case.W, desc.n_points, desc.point_dim)
    P32 = points_of(desc, oracle.fkine(desc, flat, dtype=F)).reshape(P64.shape)
    d64, d32 = P64[:, 1:] - P64[:, :-1], (P32[:, 1:] - P32[:, :-1]).astype(F)
    seg64 = (d64 * d64).sum(axis=3)
    seg32 = np.zeros(d32.shape[:3], F)
    for c in range(d32.shape[3]):
        seg32 = (seg32 + (d32[..., c] * d32[..., c]).astype(F)).astype(F)
    err_seg = float(np.abs(seg32.astype(np.float64) - seg64).max())
    margin, gap_s = np.zeros(case.C, F), np.zeros(case.C)
    for c in range(case.C):
        mid, half = widest_gap(s64[:, c])
        x, gap_s[c] = _nearest_f32_inside(mid, half)
        margin[c] = x
    mid, half = widest_gap(seg64[seg64 > 0])
    # max_speed is the fp32 value the kernel is handed; it squares it in fp32, the referee in float64: the half-gap is what is
    # left around BOTH squares
    max_speed = float(F(np.sqrt(mid)))
    gap_seg = half - max(abs(max_speed ** 2 - mid), abs(float(F(max_speed) * F(max_speed)) - mid))
    opts = default_opts(float(margin[0]), max_speed)
    return dict(desc=desc, dof=dof, kern=kern, sup=sup, weights=weights, limits32=lim.astype(F), paths=paths, margin=margin,
                gap_s=gap_s, gap_seg=gap_seg, err_s=err_s, err_seg=err_seg, opts=opts, s64=s64.reshape(case.R, case.W, case.C),
                seg64=seg64)


@functools.lru_cache(maxsize=None)
def traj_reference(case, warm):
    """the referee's step of every path of a case, computed once and shared: warm = False from zero moments at step 1, warm = True
    from caller-supplied moments at first_step = 5 (m0 = 0.3 g_scale N(0, 1), v0 uniform in [1, 4] g_scale^2, g_scale the largest
    gradient entry of the case: the update stays smooth in g; zero at the endpoints).  (list of traj_referee dicts, m0 [R, W, dof] fp32, v0, t)"""
    x = traj_setup(case)
    R, W, dof = x["paths"].shape
    args = (x["desc"], x["kern"], x["sup"], x["weights"], x["limits32"])
    zero = np.zeros((W, dof))
    cold = [traj_referee(*args, x["paths"][r], x["margin"], x["opts"], zero, zero, 1) for r in range(R)]
    if not warm:
        m0, v0, t = np.zeros((R, W, dof), F), np.zeros((R, W, dof), F), 1
    else:
        rng = case_rng(case, "warm")
        gs = max(max(float(np.abs(c["g"]).max()) for c in cold), 1e-3)
        m0 = (0.3 * gs * rng.standard_normal((R, W, dof))).astype(F)
        v0 = (rng.uniform(1.0, 4.0, (R, W, dof)) * gs * gs).astype(F)
        m0[:, [0, -1]] = 0.0   # the endpoints' gradient is always zero, so are their moments in any state the loop can reach
        v0[:, [0, -1]] = 0.0
        t = 5
    if not warm:
        return cold, m0, v0, t
    return [traj_referee(*args, x["paths"][r], x["margin"], x["opts"], m0[r], v0[r], t) for r in range(R)], m0, v0, t


# ---- what traj_run (dcx_api.hip) decides per case, restated from its rules: which rows (e) can hold to equal bits -----------
def compiled_classes(C):
    """the class count a model is compiled at (dcx_api.hip: Cc)"""
    return C if C <= 1 else 4 if C <= 4 else 5 if C == 5 else 8


def has_persistent_form(case):
    """traj_fused_kernel is INSTANTIATED for this row (score_inst.hip): W <= 64, and for several classes D <= 24 with
    RQKernel(p = 2) / Polyharmonic(1).  Whether traj_run then launches it also depends on the carve fitting 150 KB (lds_of),
    which needs the transform's frame plan: the GPU test reads the route taken off col_score, which only the launch loop writes"""
    if case.W > 64:
        return False
    if case.C > 1:
        return template_d_for(case.D) <= 24 and kernel_family(*KERNELS[case.ki]) in (0, 1)
    return True
