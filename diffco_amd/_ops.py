"""torch-facing wrappers of the C ABI (include/dcx.h): device buffers in, device buffers out.

PyTorch is plumbing here (allocation, streams, autograd bookkeeping); all arithmetic of the
score/grad path happens in libdcx.so.  CPU tensors are moved to the GPU, computed there and
moved back to the caller's device and dtype, so reference scripts written for CPU tensors run
unchanged on a GPU box.  Without a GPU every function raises (no CPU fallback).
"""
import ctypes as C
import math
import numbers

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._fkdesc import DCX_K_MQ, DCX_K_POLY, DCX_K_RQ, FkDesc, none_desc  # noqa: F401


def _device(dev=None):
    _lib.require_gpu()
    if dev is not None and torch.device(dev).type == "cuda":
        d = torch.device(dev)
        return torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())
    return torch.device("cuda", torch.cuda.current_device())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream(dev):
    """torch's current stream on `dev` as the C ABI's `void* stream` (the raw handle straight from torch's C layer: building
    a torch.cuda.Stream object to read its handle cost 5 us per call, tools/api_profile.py)"""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(dev.index))
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _on_device:
    """`with _on_device(dev):` = torch.cuda.device(dev) when another device is current, nothing at all otherwise (the library
    selects the model's device itself; the guard only keeps the CALLER's current device what it was)"""
    __slots__ = ("guard",)

    def __init__(self, dev):
        cur = _raw_device() if _raw_device is not None else torch.cuda.current_device()
        self.guard = None if cur == dev.index else torch.cuda.device(dev)

    def __enter__(self):
        if self.guard is not None:
            self.guard.__enter__()

    def __exit__(self, *exc):
        if self.guard is not None:
            self.guard.__exit__(*exc)
        return False


def _f32(t, dev):
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else C.c_void_p(0)


def _kparams(p0, p1=0.0):
    return (C.c_float * 2)(float(p0), float(p1))


# ----------------------------------------------------------------------------- FK
class _FkineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, desc):
        lib = _lib.require_gpu()
        dev = _device(q.device)
        q32 = _f32(q.reshape(-1, desc.dof), dev)
        B = q32.shape[0]
        X = torch.empty((B, desc.feature_dim), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(lib.dcx_fkine(dev.index, C.byref(desc), _ptr(q32), B, _ptr(X), _stream(dev)))
        ctx.desc, ctx.dev, ctx.in_dtype, ctx.in_device, ctx.in_shape = desc, dev, q.dtype, q.device, q.shape
        ctx.save_for_backward(q32)
        return X.reshape(B, *desc.feature_shape).to(device=q.device, dtype=q.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gX):
        lib = _lib.require_gpu()
        (q32,) = ctx.saved_tensors
        desc, dev = ctx.desc, ctx.dev
        B = q32.shape[0]
        g32 = _f32(gX.reshape(B, -1), dev)
        gq = torch.empty((B, desc.dof), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(lib.dcx_fkine_vjp(dev.index, C.byref(desc), _ptr(q32), _ptr(g32), B, _ptr(gq), _stream(dev)))
        return gq.to(device=ctx.in_device, dtype=ctx.in_dtype).reshape(ctx.in_shape), None


def fkine(desc: FkDesc, q: torch.Tensor) -> torch.Tensor:
    """control points [B, m, d] of configurations q [B, dof] (differentiable; HIP forward and vjp)."""
    return _FkineFn.apply(q, desc)


# ----------------------------------------------------------------------------- kernel matrix
def kernel_matrix(kind, p0, p1, x: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """K[b, j] = K(x_b, s_j) for x [B, D], s [S, D]; result on x's device/dtype (not differentiable)."""
    lib = _lib.require_gpu()
    if x.requires_grad or s.requires_grad:
        raise _lib.DcxError("kernel callables are not differentiable on their own; differentiate through "
                            "DiffCo.score / poly_score / rbf_score (fused HIP gradient) instead")
    dev = _device(x.device if x.device.type == "cuda" else s.device)
    x32, s32 = _f32(x, dev), _f32(s, dev)
    B, D = x32.shape
    S = s32.shape[0]
    if s32.shape[1] != D:
        raise ValueError(f"kernel: feature widths differ ({D} vs {s32.shape[1]})")
    K = torch.empty((B, S), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(lib.dcx_kernel_matrix(dev.index, kind, _kparams(p0, p1), _ptr(x32), B, _ptr(s32), S, D, _ptr(K),
                                         _stream(dev)))
    return K.to(device=x.device, dtype=x.dtype)


SOLVE_MAX_N = 3072   # dcx_solve takes up to DCX_SOLVE_MAX_N = 4096; beyond ~3000 unknowns the library LU is the faster one
SOLVE_MAX_RHS = 64


def _solve_device(a32: torch.Tensor, b32: torch.Tensor) -> torch.Tensor:
    """dcx_solve on device fp32 tensors a32 [n, n], b32 [n, r]: x [n, r] (device fp32).  Raises torch's LinAlgError on an
    exactly singular matrix, as torch.linalg.solve does."""
    lib = _lib.require_gpu()
    dev = a32.device
    n, r = b32.shape
    nbytes = int(lib.dcx_solve_work_bytes(n, r))
    work = torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.float64)
    x = torch.empty((n, r), device=dev, dtype=torch.float32)
    info = torch.zeros(2, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        for flags in (0, 1):
            _lib.check(lib.dcx_solve(dev.index, _ptr(a32), _ptr(b32), n, r, _ptr(x), _ptr(work), nbytes, _ptr(info), flags,
                                     _stream(dev)))
            code = int(info[0].item())
            if code >= 0:
                break
            # a grid barrier gave up (another kernel held the CUs): the inputs are untouched, run again as one workgroup
    if code < 0:
        raise _lib.DcxError("dcx_solve: the solve did not complete")
    if code > 0:
        raise torch.linalg.LinAlgError(f"dcx_solve: the matrix is singular (pivot {code} is exactly zero)")
    return x


def solve(kmat: torch.Tensor, rhs: torch.Tensor) -> torch.Tensor:
    """x with kmat @ x = rhs, solved on the GPU: the S x S system of fit_poly (reference kernel_perceptrons.py:283,
    deprecated/MultiDiffCo.py:149).  float32 systems of up to 3072 unknowns: dcx_solve, one launch (LU with partial pivoting,
    fp64 inside, fp32 in and out: csrc/solve_kernels.hip); beyond, for more than 64 right-hand sides, and for FLOAT64 systems
    (dcx_solve reads fp32: a float64 `kmat + reg * eye` with a small `reg` would lose it on the way in - ADVICE r4) torch's
    hipSOLVER binding, a plain library factorisation in the caller's precision.  Result on kmat's device and dtype.  An exactly
    zero (or NaN) pivot raises torch.linalg.LinAlgError from dcx_solve, as LAPACK's info does; the library route returns what
    hipSOLVER returns.  Like every other op here it needs the GPU."""
    _lib.require_gpu()
    dev = _device(kmat.device)
    n = kmat.shape[-1]
    if kmat.dtype != torch.float64 and kmat.dim() == 2 and rhs.dim() in (1, 2) and 1 <= n <= SOLVE_MAX_N and rhs.shape[0] == n \
            and 1 <= rhs.numel() // n <= SOLVE_MAX_RHS:
        x = _solve_device(_f32(kmat, dev), _f32(rhs.reshape(n, -1), dev))
        return x.reshape(rhs.shape).to(device=kmat.device, dtype=kmat.dtype)
    x = torch.linalg.solve(kmat.detach().to(dev), rhs.detach().to(device=dev, dtype=kmat.dtype))
    return x.to(device=kmat.device)


def fit_nodes(kind, p0, p1, feats: torch.Tensor, targets: torch.Tensor, reg: float = 0.0) -> torch.Tensor:
    """fit_poly in one piece: nodes with (K(feats, feats) + reg I) nodes = targets, the kernel matrix built and solved on
    the device without leaving it (dcx_kernel_matrix + dcx_solve).  feats [S, ...], targets [S] or [S, C]; result on
    targets' device and dtype."""
    lib = _lib.require_gpu()
    dev = _device(feats.device)
    f = _f32(feats.reshape(len(feats), -1), dev)
    S, D = f.shape
    if S > SOLVE_MAX_N or targets.numel() // max(S, 1) > SOLVE_MAX_RHS:
        K = kernel_matrix(kind, p0, p1, f, f)
        if reg:
            K = K + reg * torch.eye(S, device=dev, dtype=K.dtype)
        return solve(K, _f32(targets, dev)).to(device=targets.device, dtype=targets.dtype)
    K = torch.empty((S, S), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(lib.dcx_kernel_matrix(dev.index, kind, _kparams(p0, p1), _ptr(f), S, _ptr(f), S, D, _ptr(K), _stream(dev)))
    if reg:
        K.diagonal().add_(reg)
    x = _solve_device(K, _f32(targets.reshape(S, -1), dev))
    return x.reshape(targets.shape).to(device=targets.device, dtype=targets.dtype)


# ----------------------------------------------------------------------------- perceptron trainer
def train_perceptron_device(kind, p0, p1, beta, feats, y, gains, hypo, K, max_iteration):
    """The whole perceptron loop in one persistent launch (dcx_train_perceptron).  feats [N, D], y / gains / hypo
    [N] or [N, C], K [N, N] or None (cold start: allocated as zeros on the device).  Returns device tensors
    (gains, hypo, K) in fp32 with y's shape, and (iterations, converged)."""
    lib = _lib.require_gpu()
    dev = _device(feats.device)
    f = _f32(feats.reshape(len(feats), -1), dev)
    N, D = f.shape
    shape = tuple(y.shape)
    yy = _f32(y.reshape(N, -1), dev)
    Cn = yy.shape[1]
    def run(flags):
        g = _f32(gains.reshape(N, -1), dev).clone()
        h = _f32(hypo.reshape(N, -1), dev).clone()
        Kd = torch.zeros((N, N), device=dev, dtype=torch.float32) if K is None else _f32(K, dev).clone()
        info = torch.zeros(2, device=dev, dtype=torch.int32)
        with torch.cuda.device(dev):
            _lib.check(lib.dcx_train_perceptron_ex(dev.index, kind, _kparams(p0, p1), float(beta), _ptr(f), N, D, _ptr(yy), Cn,
                                                   _ptr(g), _ptr(h), _ptr(Kd), int(max_iteration), _ptr(info), flags, _stream(dev)))
        it, conv = (int(v) for v in info.tolist())
        return g, h, Kd, it, conv

    g, h, Kd, it, conv = run(0)
    if conv < 0:
        # a grid-wide barrier of the multi-workgroup trainer gave up (another kernel holding CUs for seconds): the run's
        # buffers are copies, so the whole training simply runs again on the one-workgroup kernels - asked for per call
        # (DCX_TRAIN_ONE_WORKGROUP), not through the process-wide knob other threads and the tests may have set
        g, h, Kd, it, conv = run(1)
        if conv < 0:
            raise _lib.DcxError("dcx_train_perceptron: the trainer did not complete")
    return g.reshape(shape), h.reshape(shape), Kd, it, bool(conv)


# ----------------------------------------------------------------------------- fused score model
MOTION_MAX_SAMPLES = 10000   # the default limit on one edge's samples (max_step rule): longer edges answer -2


def wrap_mask(wrap, dof, transform=None):
    """the motion calls' `wrap` argument as dcx_check_motions_ex's bitmask (bit j: coordinate j is an angle on the circle, the
    edge runs along its shortest arc).  None / False: 0, the straight edge.  An int: the mask itself.  A sequence of dof
    bools: one per coordinate.  True: the `wrap_mask` of the robot whose bound `fkine` is `transform` (model.py, urdf.py)."""
    if wrap is None or wrap is False:
        return 0
    if wrap is True:
        mask = getattr(getattr(transform, "__self__", None), "wrap_mask", None)
        if mask is None:
            raise ValueError("wrap=True needs a transform that is the fkine of a robot with a wrap_mask (diffco_amd.model / urdf): "
                             "pass the mask itself, or one bool per coordinate")
        wrap = mask
    if isinstance(wrap, numbers.Integral):
        mask = int(wrap)
    else:
        flags = torch.as_tensor(wrap).reshape(-1).tolist()
        if len(flags) != dof or any(f not in (0, 1, False, True) for f in flags):
            raise ValueError(f"wrap: expected one bool per coordinate ({dof}), got {len(flags)} values")
        mask = sum(1 << j for j, f in enumerate(flags) if f)
    if mask < 0 or mask >> dof:
        raise ValueError(f"wrap mask {mask:#x} has a bit at or above dof = {dof}")
    return mask


def wrapped_delta(qa, qb, mask):
    """qb - qa [E, dof] with the masked coordinates along the shortest arc (utils.wrap2pi of the difference; differentiable)"""
    d = qb - qa
    if mask:
        from .utils import wrap2pi
        on = torch.tensor([bool((mask >> j) & 1) for j in range(d.shape[-1])], device=d.device)
        d = torch.where(on, wrap2pi(d), d)
    return d


def motion_bound(qa32, qb32, max_step, limit=MOTION_MAX_SAMPLES, wrap=None):
    """max_samples for a max_step call: the longest edge's sample count (+ 1 against a rounding of its length that differs
    from the kernel's), at most `limit`.  One small reduction read back: dcx_check_motions sizes its grid from E * max_samples,
    and a loose bound launches a block per tile it could have had (measured: profiles/r07_motion_checks.txt).  `wrap`
    (wrap_mask's values but True): the lengths are those of the wrapped edges."""
    if len(qa32) == 0:
        return 1
    L = float(wrapped_delta(qa32, qb32, wrap_mask(wrap, qa32.shape[-1])).norm(dim=1).max())
    if not L == L or L == float("inf"):
        return limit
    return int(min(limit, math.ceil(L * (1.0 / float(max_step))) + 2))


def knn(queries, points, k, wrap=None, max_dist=None, exclude_self=False, self_offset=None, transform=None):
    """the k nearest of points [N, dof] for each of queries [Q, dof] under the motion calls' metric (dcx_knn): (idx int32 [Q, k],
    dist2 float32 [Q, k]) on the points' device, ordered by (dist2, index) ascending; unfilled slots hold -1 / +inf.  dist2 is,
    bit for bit, the squared edge length check_motions(queries[i], points[idx], wrap=wrap) walks.
    `wrap` as wrap_mask (True: the mask of the robot whose fkine is `transform`).  `max_dist`: a radius (squared in float32).
    `exclude_self`: queries are the points themselves (the same tensor or equal shapes), none its own neighbour;
    `self_offset`: queries are points[self_offset : self_offset + Q]."""
    lib = _lib.require_gpu()
    points = torch.as_tensor(points)
    queries = torch.as_tensor(queries)
    dev = _device(points.device if points.device.type == "cuda" else queries.device)
    if points.dim() != 2 or queries.dim() != 2 or queries.shape[1] != points.shape[1]:
        raise ValueError(f"knn: queries {tuple(queries.shape)} and points {tuple(points.shape)} must be [Q, dof] and [N, dof]")
    if exclude_self:
        if self_offset not in (None, 0):
            raise ValueError("knn: exclude_self means self_offset = 0")
        if queries is not points and queries.shape != points.shape:
            raise ValueError("knn: exclude_self needs the queries to be the points")
        self_offset = 0
    dof = points.shape[1]
    p32 = _f32(points, dev)
    q32 = p32 if queries is points else _f32(queries, dev)
    Q, N = len(q32), len(p32)
    d2 = float("inf") if max_dist is None else float(torch.tensor(float(max_dist), dtype=torch.float32).square())
    opt = _lib.KnnOpts(int(k), 0, wrap_mask(wrap, dof, transform), d2, 0, -1 if self_offset is None else int(self_offset), (C.c_int64 * 2)(0, 0))
    idx = torch.empty((Q, int(k)), device=dev, dtype=torch.int32)
    dist2 = torch.empty((Q, int(k)), device=dev, dtype=torch.float32)
    nbytes = int(lib.dcx_knn_work_bytes(Q, N, dof, int(k)))
    # as the motion calls: torch's caching allocator is the per-device cache (a freed block is reused on its stream, no hipMalloc)
    work = torch.empty(max(nbytes, 1), device=dev, dtype=torch.uint8)
    with _on_device(dev):
        _lib.check(lib.dcx_knn(dev.index, _ptr(q32), Q, _ptr(p32), N, dof, C.byref(opt), _ptr(idx), _ptr(dist2), _ptr(work),
                               work.numel(), _stream(dev)))
    return idx, dist2


def geom_clearance(desc: FkDesc, radii, obstacles, q, n_groups=1, sphere_base=0, accumulate=False, clearance=None, witness=None,
                   grad=None, want_witness=True, want_grad=False, check_groups=True):
    """dcx_geom_clearance: the spheres of `desc` (its control points, radii [M] float32 on the device) against `obstacles`
    ([O, 16] float32 rows of dcx_geom_obstacle on the device) for q [B, dof] float32 on the device ->
    (clearance [B, G] float32, witness [B, G, 2] int32 or None, grad [B, dof] float32 or None).  `accumulate`: the three
    tensors are an earlier chunk's results and are updated in place (entries only where this chunk is strictly smaller).
    `check_groups`: the rows' group ids are read back (one small reduction) and one at or above n_groups raises - the kernel
    would ignore such rows; pass False where the groups are known (geometry.SphereWorldChecker checks its World on the host)
    or where the call must not synchronise."""
    lib = _lib.require_gpu()
    dev = q.device
    B, G, O = len(q), int(n_groups), len(obstacles)
    _check_tensor("geom_clearance: q", q, torch.float32, (B, desc.dof), dev)
    _check_tensor("geom_clearance: radii", radii, torch.float32, (desc.n_points,), dev)
    _check_tensor("geom_clearance: obstacles", obstacles, torch.float32, (O, 16), dev)
    if accumulate and clearance is None:
        raise ValueError("geom_clearance: accumulate needs the earlier call's tensors")
    if clearance is None:
        clearance = torch.empty((B, G), device=dev, dtype=torch.float32)
        witness = torch.empty((B, G, 2), device=dev, dtype=torch.int32) if want_witness else None
        grad = torch.empty((B, desc.dof), device=dev, dtype=torch.float32) if want_grad else None
    _check_tensor("geom_clearance: clearance", clearance, torch.float32, (B, G), dev)
    if witness is not None:
        _check_tensor("geom_clearance: witness", witness, torch.int32, (B, G, 2), dev)
    if grad is not None:
        _check_tensor("geom_clearance: grad", grad, torch.float32, (B, desc.dof), dev)
    if check_groups and O:
        top = int((obstacles.view(torch.int32)[:, 0] >> 8).max())
        low = int((obstacles.view(torch.int32)[:, 0] >> 8).min())
        if top >= G or low < 0:
            raise ValueError(f"geom_clearance: an obstacle row has group {top if top >= G else low}, outside [0, n_groups = {G})")
    opt = _lib.GeomOpts(G, int(sphere_base), int(bool(accumulate)), 0)
    with _on_device(dev):
        _lib.check(lib.dcx_geom_clearance(dev.index, C.byref(desc), _ptr(radii), _ptr(obstacles), O, _ptr(q), B, C.byref(opt),
                                          _ptr(clearance), _ptr(witness), _ptr(grad), _stream(dev)))
    return clearance, witness, grad


def _check_tensor(label, t, dtype, shape, dev, kind=None):
    """raises ValueError unless t is a contiguous `dtype` tensor of `shape` on `dev`.  `label`: how the message names it;
    `kind`: how it names the expected tensor where that is not "<dtype> tensor <shape>"."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != dev or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{label} must be a contiguous {kind or f'{dtype} tensor {tuple(shape)}'} on {dev}")
    return t


def rrt_extract_paths(state, W, out=None):
    """the solved paths of an RRT state (dcx_rrt_extract_paths; `state` maps nodes [R, 2, cap, dof] float32, parent [R, 2, cap],
    status [R], link [R, 2] (int32) to contiguous tensors on one GPU): (path [R, W, dof] float32, count [R] int32) there.
    count[r] = n where problem r's n waypoints fit and were written, -n where n > W (the row is left as it is: zeros), 0 for a
    problem without a path.  W = 0 asks for the sizes alone.  `out`: the [R, W, dof] tensor to write into.  One launch on torch's current stream, nothing read back."""
    lib = _lib.require_gpu()
    nodes = state["nodes"]
    if nodes.dim() != 4 or nodes.device.type != "cuda":
        raise ValueError("rrt_extract_paths: state['nodes'] must be a [R, 2, cap, dof] tensor on a GPU")
    dev = nodes.device
    R, _, cap, dof = (int(v) for v in nodes.shape)
    kinds = dict(nodes=torch.float32, parent=torch.int32, status=torch.int32, link=torch.int32)
    shapes = dict(nodes=(R, 2, cap, dof), parent=(R, 2, cap), status=(R,), link=(R, 2))
    for name, dt in kinds.items():
        _check_tensor(f"rrt_extract_paths: state[{name!r}]", state[name], dt, shapes[name], dev)
    W = int(W)
    if W < 0:
        raise ValueError("rrt_extract_paths: W must be >= 0")
    if out is None:
        path = torch.zeros((R, W, dof), device=dev, dtype=torch.float32)
    else:
        path = _check_tensor("rrt_extract_paths: out", out, torch.float32, (R, W, dof), dev, kind=f"float32 tensor {(R, W, dof)}")
    count = torch.zeros(R, device=dev, dtype=torch.int32)
    st = _lib.RrtState(state["nodes"].data_ptr(), state["parent"].data_ptr(), 0, state["status"].data_ptr(), state["link"].data_ptr(), 0)
    with _on_device(dev):
        _lib.check(lib.dcx_rrt_extract_paths(dev.index, C.byref(st), R, cap, dof, _ptr(path), _ptr(count), W, _stream(dev)))
    return path, count


_RRTSTAR_KINDS = dict(nodes=torch.float32, parent=torch.int32, elen=torch.float32, cost=torch.float32, count=torch.int32,
                      status=torch.int32, goal_node=torch.int32, first_round=torch.int32)


def _rrtstar_state(label, state, dev):
    """(dcx_rrtstar_state, R, cap, dof) of `state`: the eight tensors, contiguous on `dev`"""
    nodes = state["nodes"]
    if not isinstance(nodes, torch.Tensor) or nodes.dim() != 3 or nodes.device.type != "cuda":
        raise ValueError(f"{label}: state['nodes'] must be a [R, cap, dof] tensor on a GPU")
    dev = nodes.device if dev is None else dev
    R, cap, dof = (int(v) for v in nodes.shape)
    shapes = dict(nodes=(R, cap, dof), parent=(R, cap), elen=(R, cap), cost=(R, cap), count=(R,), status=(R,), goal_node=(R,),
                  first_round=(R,))
    for name, dt in _RRTSTAR_KINDS.items():
        _check_tensor(f"{label}: state[{name!r}]", state[name], dt, shapes[name], dev)
    return _lib.RrtStarState(*(state[n].data_ptr() for n in _lib.RRTSTAR_STATE)), R, cap, dof


def rrtstar_extract_paths(state, W, out=None):
    """the paths to the goal nodes of an RRT* state (dcx_rrtstar_extract_paths; `state` maps dcx_rrtstar_state's fields to
    contiguous tensors on one GPU): (path [R, W, dof] float32, count [R] int32) there.  count[r] = n where problem r's n
    waypoints fit and were written (root first), -n where n > W (the row is left as it is: zeros), 0 for a problem without a goal
    node.  W = 0 asks for the sizes alone.  `out`: the [R, W, dof] tensor to write into.  One launch on torch's current stream,
    nothing read back."""
    lib = _lib.require_gpu()
    st, R, cap, dof = _rrtstar_state("rrtstar_extract_paths", state, None)
    dev = state["nodes"].device
    W = int(W)
    if W < 0:
        raise ValueError("rrtstar_extract_paths: W must be >= 0")
    if out is None:
        path = torch.zeros((R, W, dof), device=dev, dtype=torch.float32)
    else:
        path = _check_tensor("rrtstar_extract_paths: out", out, torch.float32, (R, W, dof), dev, kind=f"float32 tensor {(R, W, dof)}")
    count = torch.zeros(R, device=dev, dtype=torch.int32)
    with _on_device(dev):
        _lib.check(lib.dcx_rrtstar_extract_paths(dev.index, C.byref(st), R, cap, dof, _ptr(path), W, _ptr(count), _stream(dev)))
    return path, count


def _rrtstar_sample_opts(label, limits, dof, dev, seed, P, cap, mode, goal_bias, uniform_mix, tries, mask):
    """dcx_rrtstar_sample_opts over `limits` ([dof, 2] float32, contiguous on `dev`)"""
    _check_tensor(f"{label}: limits", limits, torch.float32, (dof, 2), dev)
    if mode not in _lib.RRTSTAR_SAMPLE_MODES:
        raise ValueError(f"{label}: mode must be one of {sorted(_lib.RRTSTAR_SAMPLE_MODES)}, got {mode!r}")
    return _lib.RrtStarSampleOpts(limits.data_ptr(), int(seed) & 0xFFFFFFFFFFFFFFFF, float(goal_bias), float(uniform_mix),
                                  _lib.RRTSTAR_SAMPLE_MODES[mode], int(tries), int(P), int(cap), int(dof), 0, mask, (C.c_int64 * 2)(0, 0))


def rrtstar_sample(state, goals, limits, seed, g, P, mode="informed", goal_bias=0.1, uniform_mix=0., tries=8, wrap=None):
    """round g's samples of an RRT* state drawn on the device (dcx_rrtstar_sample; `state` maps dcx_rrtstar_state's fields to
    contiguous tensors on one GPU, goals [R, dof] and limits [dof, 2] float32 there): (samples [R, P, dof] float32, info [R, P]
    int32) there.  info: -1 the problem is not running (its start row), 0 uniform in the limits, 1 the goal row, 2 + t informed
    and accepted at try t, 2 + tries informed and fallen back to the uniform point.  `mode`: "uniform" or "informed".  One
    launch on torch's current stream, nothing read back."""
    lib = _lib.require_gpu()
    st, R, cap, dof = _rrtstar_state("rrtstar_sample", state, None)
    dev = state["nodes"].device
    _check_tensor("rrtstar_sample: goals", goals, torch.float32, (R, dof), dev)
    opt = _rrtstar_sample_opts("rrtstar_sample", limits, dof, dev, seed, P, cap, mode, goal_bias, uniform_mix, tries, wrap_mask(wrap, dof))
    samples = torch.empty((R, int(P), dof), device=dev, dtype=torch.float32)
    info = torch.empty((R, int(P)), device=dev, dtype=torch.int32)
    with _on_device(dev):
        _lib.check(lib.dcx_rrtstar_sample(dev.index, C.byref(st), R, _ptr(goals), C.byref(opt), int(g), _ptr(samples), _ptr(info),
                                          _stream(dev)))
    return samples, info


def path_resample(path, count, T, mask=0, out=None):
    """R paths resampled to T waypoints each, equally spaced in arc length (dcx_path_resample; path [R, W, dof] float32 and count
    [R] int32, contiguous on one GPU; mask: the wrap bitmask): (out [R, T, dof] float32, out_count [R] int32, length [R] float32)
    there.  out_count[r] is T, or 0 for a row without a path (count < 2, or a length that is NaN or infinite): that row of `out`
    is left as it is, zeros.  `out`: the [R, T, dof] tensor to write into.  One launch on torch's current stream, nothing read
    back."""
    lib = _lib.require_gpu()
    if not isinstance(path, torch.Tensor) or path.dim() != 3 or path.device.type != "cuda":
        raise ValueError("path_resample: path must be a [R, W, dof] tensor on a GPU")
    dev = path.device
    R, W, dof = (int(v) for v in path.shape)
    _check_tensor("path_resample: path", path, torch.float32, (R, W, dof), dev)
    _check_tensor("path_resample: count", count, torch.int32, (R,), dev)
    T, mask = int(T), int(mask)
    if mask < 0 or mask >> dof:
        raise ValueError(f"wrap mask {mask:#x} has a bit at or above dof = {dof}")
    if out is None:
        out = torch.zeros((R, max(T, 0), dof), device=dev, dtype=torch.float32)
    else:
        _check_tensor("path_resample: out", out, torch.float32, (R, T, dof), dev)
    out_count = torch.zeros(R, device=dev, dtype=torch.int32)
    length = torch.full((R,), float("nan"), device=dev, dtype=torch.float32)
    nbytes = int(lib.dcx_path_resample_work_bytes(R, W))
    # as the motion calls: torch's caching allocator is the per-device cache (a freed block is reused on its stream, no hipMalloc)
    work = torch.empty(max(nbytes, 1), device=dev, dtype=torch.uint8)
    with _on_device(dev):
        _lib.check(lib.dcx_path_resample(dev.index, _ptr(path), _ptr(count), R, W, dof, mask, T, _ptr(out), _ptr(out_count),
                                         _ptr(length), _ptr(work), work.numel(), _stream(dev)))
    return out, out_count, length


def _sssp_graph(fn, rowptr, col, weight):
    """dcx_graph of a CSR on one GPU: (the struct, N, device).  Shapes, kinds and placement are checked; the CSR's contents
    (sorted rows, symmetry, weights >= 0) are the caller's, as include/dcx.h says."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.device.type != "cuda" or rowptr.dim() != 1 or len(rowptr) < 1:
        raise ValueError(f"{fn}: rowptr must be an int32 tensor [N + 1] on a GPU")
    dev = rowptr.device
    N = len(rowptr) - 1
    _check_tensor(f"{fn}: rowptr", rowptr, torch.int32, (N + 1,), dev)
    if not isinstance(col, torch.Tensor) or col.dim() != 1:
        raise ValueError(f"{fn}: col must be an int32 tensor [nnz]")
    nnz = len(col)
    _check_tensor(f"{fn}: col", col, torch.int32, (nnz,), dev)
    _check_tensor(f"{fn}: weight", weight, torch.float32, (nnz,), dev)
    return _lib.Graph(rowptr.data_ptr(), col.data_ptr() if nnz else 0, weight.data_ptr() if nnz else 0, N, nnz, (C.c_int64 * 2)(0, 0)), N, dev


def sssp_run(rowptr, col, weight, link_idx, link_len, dist, pred, round0, n_rounds, changed=None):
    """rounds round0 .. round0 + n_rounds - 1 of the min-plus relaxation over the CSR (rowptr, col, weight) for Q queries
    (dcx_sssp_run; include/dcx.h, "roadmap queries"): the state dist [2, N, Q] float32 and pred [N, Q] int32 is advanced in
    place, round 0 sets it from the start links link_idx / link_len [Q, k] (int32, -1 = no link / float32).  Returns changed
    int32 [n_rounds] on the device: 1 where the round changed anything.  Everything is a contiguous tensor on one GPU; the
    launches go to torch's current stream, nothing is allocated (with `changed` given) or read back."""
    fn = "sssp_run"
    lib = _lib.require_gpu()
    g, N, dev = _sssp_graph(fn, rowptr, col, weight)
    if not isinstance(dist, torch.Tensor) or dist.dim() != 3:
        raise ValueError(f"{fn}: dist must be a float32 tensor [2, N, Q]")
    Q = int(dist.shape[2])
    _check_tensor(f"{fn}: dist", dist, torch.float32, (2, N, Q), dev)
    _check_tensor(f"{fn}: pred", pred, torch.int32, (N, Q), dev)
    if not isinstance(link_idx, torch.Tensor) or link_idx.dim() != 2:
        raise ValueError(f"{fn}: link_idx must be an int32 tensor [Q, k]")
    k = int(link_idx.shape[1])
    _check_tensor(f"{fn}: link_idx", link_idx, torch.int32, (Q, k), dev)
    _check_tensor(f"{fn}: link_len", link_len, torch.float32, (Q, k), dev)
    round0, n_rounds = int(round0), int(n_rounds)
    if round0 < 0 or n_rounds < 0:
        raise ValueError(f"{fn}: round0 and n_rounds must be >= 0")
    if changed is None:
        changed = torch.zeros(n_rounds, device=dev, dtype=torch.int32)
    _check_tensor(f"{fn}: changed", changed, torch.int32, (n_rounds,), dev)
    st = _lib.SsspState(dist.data_ptr(), pred.data_ptr(), (C.c_int64 * 2)(0, 0))
    links = _lib.SsspLinks(link_idx.data_ptr(), link_len.data_ptr(), (C.c_int64 * 2)(0, 0))
    with _on_device(dev):
        _lib.check(lib.dcx_sssp_run(dev.index, C.byref(g), Q, C.byref(links), k, C.byref(st), round0, n_rounds, _ptr(changed),
                                    _stream(dev)))
    return changed


def sssp_extract_paths(rowptr, col, weight, nodes, dist, pred, rounds_done, mode, starts, goals, goal_idx, goal_len, direct_len, W,
                       out=None):
    """the routes of Q queries after rounds_done rounds of sssp_run (dcx_sssp_extract_paths): (path [Q, W, dof] float32, count
    [Q] int32, length [Q] float32) on the state's GPU.  mode [Q] int32: 0 no path, 1 the two-point path (start, goal) of length
    direct_len, 2 the shortest route through the goal links goal_idx / goal_len [Q, k].  count[q] = n where the n waypoints
    fit and were written, -n where n > W (the row is left as it is: zeros), 0 without a route; W = 0 asks for the sizes
    alone.  `out`: the [Q, W, dof] tensor to write into.  One launch on torch's current stream, nothing read back."""
    fn = "sssp_extract_paths"
    lib = _lib.require_gpu()
    g, N, dev = _sssp_graph(fn, rowptr, col, weight)
    if not isinstance(dist, torch.Tensor) or dist.dim() != 3:
        raise ValueError(f"{fn}: dist must be a float32 tensor [2, N, Q]")
    Q = int(dist.shape[2])
    _check_tensor(f"{fn}: dist", dist, torch.float32, (2, N, Q), dev)
    _check_tensor(f"{fn}: pred", pred, torch.int32, (N, Q), dev)
    if not isinstance(nodes, torch.Tensor) or nodes.dim() != 2:
        raise ValueError(f"{fn}: nodes must be a float32 tensor [N, dof]")
    dof = int(nodes.shape[1])
    _check_tensor(f"{fn}: nodes", nodes, torch.float32, (N, dof), dev)
    if not isinstance(goal_idx, torch.Tensor) or goal_idx.dim() != 2:
        raise ValueError(f"{fn}: goal_idx must be an int32 tensor [Q, k]")
    k = int(goal_idx.shape[1])
    _check_tensor(f"{fn}: goal_idx", goal_idx, torch.int32, (Q, k), dev)
    _check_tensor(f"{fn}: goal_len", goal_len, torch.float32, (Q, k), dev)
    _check_tensor(f"{fn}: mode", mode, torch.int32, (Q,), dev)
    _check_tensor(f"{fn}: starts", starts, torch.float32, (Q, dof), dev)
    _check_tensor(f"{fn}: goals", goals, torch.float32, (Q, dof), dev)
    _check_tensor(f"{fn}: direct_len", direct_len, torch.float32, (Q,), dev)
    W, rounds_done = int(W), int(rounds_done)
    if W < 0 or rounds_done < 1:
        raise ValueError(f"{fn}: W must be >= 0 and rounds_done >= 1")
    path = torch.zeros((Q, W, dof), device=dev, dtype=torch.float32) if out is None else out
    _check_tensor(f"{fn}: out", path, torch.float32, (Q, W, dof), dev)
    count = torch.zeros(Q, device=dev, dtype=torch.int32)
    length = torch.full((Q,), float("inf"), device=dev, dtype=torch.float32)
    st = _lib.SsspState(dist.data_ptr(), pred.data_ptr(), (C.c_int64 * 2)(0, 0))
    links = _lib.SsspLinks(goal_idx.data_ptr(), goal_len.data_ptr(), (C.c_int64 * 2)(0, 0))
    with _on_device(dev):
        _lib.check(lib.dcx_sssp_extract_paths(dev.index, C.byref(g), _ptr(nodes), dof, C.byref(st), rounds_done, Q, k, _ptr(mode),
                                              _ptr(starts), _ptr(goals), C.byref(links), _ptr(direct_len), _ptr(path), _ptr(count),
                                              _ptr(length), W, _stream(dev)))
    return path, count, length


def _lazy_graph(fn, lazy, nnz, dev):
    """dcx_lazy_graph of lazy = (eid [nnz], ent [M, 2], ends [M, 2] int32, state [M] uint8) on the graph's GPU: (the struct, M)"""
    eid, ent, ends, state = lazy
    if not isinstance(state, torch.Tensor) or state.dim() != 1:
        raise ValueError(f"{fn}: the edges' state must be a uint8 tensor [M]")
    M = len(state)
    _check_tensor(f"{fn}: eid", eid, torch.int32, (nnz,), dev)
    _check_tensor(f"{fn}: ent", ent, torch.int32, (M, 2), dev)
    _check_tensor(f"{fn}: ends", ends, torch.int32, (M, 2), dev)
    _check_tensor(f"{fn}: the edges' state", state, torch.uint8, (M,), dev)
    return _lib.LazyGraph(eid.data_ptr() if nnz else 0, ent.data_ptr() if M else 0, ends.data_ptr() if M else 0,
                          state.data_ptr() if M else 0, M, (C.c_int64 * 2)(0, 0)), M


def sssp_mark_routes(rowptr, col, weight, lazy, nodes, dist, pred, rounds_done, mode, goal_idx, goal_len, capacity, out=None,
                     work=None):
    """the still unchecked edges of the routes Q queries have after rounds_done rounds of sssp_run (dcx_sssp_mark_routes;
    include/dcx.h, "lazy roadmap queries"), lazy = (eid [nnz], ent [M, 2], ends [M, 2] int32, state [M] uint8).  Returns
    (pending [Q] int32, list [capacity] int32, qa, qb [capacity, dof] float32, n_out [2] int32) on the GPU: n_out = (total,
    n = min(total, capacity)), list[:n] the marked edge ids in ascending order, qa[:n] / qb[:n] their ends' rows of nodes; the
    entries from n on are left as they are (zeros in fresh tensors).  `out`: the five tensors to write into; `work`: a uint8
    tensor of at least dcx_sssp_mark_routes_work_bytes(M) bytes.  Four launches on torch's current stream, nothing allocated
    (with `out` and `work` given) or read back.  With Q = 0 or M = 0 nothing is launched and fresh tensors are zeros."""
    fn = "sssp_mark_routes"
    lib = _lib.require_gpu()
    g, N, dev = _sssp_graph(fn, rowptr, col, weight)
    lz, M = _lazy_graph(fn, lazy, len(col), dev)
    if not isinstance(dist, torch.Tensor) or dist.dim() != 3:
        raise ValueError(f"{fn}: dist must be a float32 tensor [2, N, Q]")
    Q = int(dist.shape[2])
    _check_tensor(f"{fn}: dist", dist, torch.float32, (2, N, Q), dev)
    _check_tensor(f"{fn}: pred", pred, torch.int32, (N, Q), dev)
    if not isinstance(nodes, torch.Tensor) or nodes.dim() != 2:
        raise ValueError(f"{fn}: nodes must be a float32 tensor [N, dof]")
    dof = int(nodes.shape[1])
    _check_tensor(f"{fn}: nodes", nodes, torch.float32, (N, dof), dev)
    if not isinstance(goal_idx, torch.Tensor) or goal_idx.dim() != 2:
        raise ValueError(f"{fn}: goal_idx must be an int32 tensor [Q, k]")
    k = int(goal_idx.shape[1])
    _check_tensor(f"{fn}: goal_idx", goal_idx, torch.int32, (Q, k), dev)
    _check_tensor(f"{fn}: goal_len", goal_len, torch.float32, (Q, k), dev)
    _check_tensor(f"{fn}: mode", mode, torch.int32, (Q,), dev)
    capacity, rounds_done = int(capacity), int(rounds_done)
    if capacity < 0 or rounds_done < 1:
        raise ValueError(f"{fn}: capacity must be >= 0 and rounds_done >= 1")
    if out is None:
        out = (torch.zeros(Q, device=dev, dtype=torch.int32), torch.zeros(capacity, device=dev, dtype=torch.int32),
               torch.zeros((capacity, dof), device=dev, dtype=torch.float32), torch.zeros((capacity, dof), device=dev, dtype=torch.float32),
               torch.zeros(2, device=dev, dtype=torch.int32))
    pending, lst, qa, qb, n_out = out
    _check_tensor(f"{fn}: pending", pending, torch.int32, (Q,), dev)
    _check_tensor(f"{fn}: list", lst, torch.int32, (capacity,), dev)
    _check_tensor(f"{fn}: qa", qa, torch.float32, (capacity, dof), dev)
    _check_tensor(f"{fn}: qb", qb, torch.float32, (capacity, dof), dev)
    _check_tensor(f"{fn}: n_out", n_out, torch.int32, (2,), dev)
    nbytes = int(lib.dcx_sssp_mark_routes_work_bytes(M))
    if work is None:
        work = torch.empty(max(nbytes, 1), device=dev, dtype=torch.uint8)
    if not isinstance(work, torch.Tensor) or work.dtype != torch.uint8 or work.device != dev or not work.is_contiguous() or work.numel() < nbytes:
        raise ValueError(f"{fn}: work must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}")
    st = _lib.SsspState(dist.data_ptr(), pred.data_ptr(), (C.c_int64 * 2)(0, 0))
    links = _lib.SsspLinks(goal_idx.data_ptr(), goal_len.data_ptr(), (C.c_int64 * 2)(0, 0))
    with _on_device(dev):
        _lib.check(lib.dcx_sssp_mark_routes(dev.index, C.byref(g), C.byref(lz), _ptr(nodes), dof, C.byref(st), rounds_done, Q, k,
                                            _ptr(mode), C.byref(links), _ptr(pending), _ptr(lst), _ptr(qa), _ptr(qb), capacity,
                                            _ptr(n_out), _ptr(work), work.numel(), _stream(dev)))
    return pending, lst, qa, qb, n_out


def graph_apply_checks(rowptr, col, weight, lazy, lst, n_out, hit, any_blocked=None):
    """the verdicts of the edges sssp_mark_routes listed, written into the graph (dcx_graph_apply_checks): for i < n_out[1] (read
    on the device) the state of edge lst[i] becomes 2 where hit[i] else 1, and both CSR entries of an edge that hit get the
    weight +inf.  `weight` and the edges' state (lazy[3]) ARE WRITTEN.  hit: uint8 or bool, as long as lst (the capacity).
    Returns any_blocked int32 [1] on the GPU.  Two launches on torch's current stream, nothing read back."""
    fn = "graph_apply_checks"
    lib = _lib.require_gpu()
    g, N, dev = _sssp_graph(fn, rowptr, col, weight)
    lz, M = _lazy_graph(fn, lazy, len(col), dev)
    if not isinstance(lst, torch.Tensor) or lst.dim() != 1:
        raise ValueError(f"{fn}: list must be an int32 tensor [capacity]")
    cap = len(lst)
    _check_tensor(f"{fn}: list", lst, torch.int32, (cap,), dev)
    _check_tensor(f"{fn}: n_out", n_out, torch.int32, (2,), dev)
    if isinstance(hit, torch.Tensor) and hit.dtype == torch.bool:
        hit = hit.view(torch.uint8)
    _check_tensor(f"{fn}: hit", hit, torch.uint8, (cap,), dev)
    if any_blocked is None:
        any_blocked = torch.zeros(1, device=dev, dtype=torch.int32)
    _check_tensor(f"{fn}: any_blocked", any_blocked, torch.int32, (1,), dev)
    if cap == 0:
        return any_blocked
    with _on_device(dev):
        _lib.check(lib.dcx_graph_apply_checks(dev.index, C.byref(g), C.byref(lz), _ptr(lst), _ptr(n_out), _ptr(hit), _ptr(any_blocked),
                                              _stream(dev)))
    return any_blocked


def compose_path_cost(edge_cost, paths, dof):
    """[T] costs of paths [T, W, dof] from an edge-cost callable edge_cost(qa, qb, open_end) under the max_step rule: the
    open-ended edges p[i] -> p[i + 1] plus the zero-length edge p[-1] -> p[-1] (its one sample is p[-1]) cover the points of
    utils.dense_path(p, max_step) once each"""
    paths = torch.as_tensor(paths)
    T, W = paths.shape[0], paths.shape[1]
    if T == 0 or W == 0:
        return paths.new_zeros(T)
    p = paths.reshape(T, W, dof)
    cost = edge_cost(p[:, -1], p[:, -1], False).reshape(T)
    if W > 1:
        seg = edge_cost(p[:, :-1].reshape(-1, dof), p[:, 1:].reshape(-1, dof), True)
        cost = seg.reshape(T, W - 1).sum(dim=1) + cost
    return cost


def compose_path_worst(edge_worst, paths, dof):
    """(worst [T], segment [T], sample [T]) of paths [T, W, dof] from an edge callable edge_worst(qa, qb) -> (worst, idx, cls)
    [T * (W - 1)] under the closed max_step rule: the maximum over the path's segments, the first one in (segment, sample)
    order.  worst is a gather of the edge values, so it is differentiable wherever they are.  W == 1: the zero-length edge
    p[0] -> p[0] (its one sample is p[0])."""
    paths = torch.as_tensor(paths)
    T, W = paths.shape[0], paths.shape[1]
    p = paths.reshape(T, W, dof)
    if W == 1:
        a, b = p[:, 0], p[:, 0]
    else:
        a, b = p[:, :-1].reshape(-1, dof), p[:, 1:].reshape(-1, dof)
    worst, idx, _ = edge_worst(a, b)
    S = max(W - 1, 1)
    worst, idx = worst.reshape(T, S), idx.reshape(T, S)
    if T == 0:
        return worst.new_zeros(0), idx.new_zeros(0, dtype=torch.int64), idx.new_zeros(0, dtype=torch.int64)
    # the first maximum: torch.max's index on ties is unspecified, so take the smallest segment that attains the value
    top = worst.detach().max(dim=1, keepdim=True).values
    at = (worst.detach() == top) | (torch.isnan(worst.detach()) & torch.isnan(top))
    seg = at.int().argmax(dim=1)
    return worst.gather(1, seg[:, None])[:, 0], seg, idx.gather(1, seg[:, None])[:, 0].long()


class ScoreModel:
    """Owns one ``dcx_model`` (device copy of support rows + FK parameters).  `update()` refills it in place with new
    supports / weights (same transform, kernel and class count): no reallocation while they fit `capacity`."""

    @staticmethod
    def _rows(support_feat, weights, dev):
        sf = support_feat.detach().reshape(len(support_feat), -1).to(dtype=torch.float32).contiguous()
        w = weights.detach().to(dtype=torch.float32)
        w = (w.reshape(-1, 1) if w.ndim == 1 else w).contiguous()
        if len(sf) != len(w):
            raise ValueError(f"{len(sf)} supports but {len(w)} weight rows")
        # tensors already on the model's GPU are packed there by one kernel (dcx_model_create_ex); CPU tensors take the
        # library's host path; another GPU's tensors come over first
        if sf.is_cuda and sf.device != dev:
            sf = sf.to(dev)
        if w.is_cuda and w.device != dev:
            w = w.to(dev)
        if sf.is_cuda != w.is_cuda:
            sf, w = sf.to(dev), w.to(dev)
        return sf, w

    def __init__(self, desc, kind, p0, p1, support_feat, weights, device=None, capacity=0):
        lib = _lib.require_gpu()
        self.dev = _device(device)
        self.desc = desc if desc is not None else none_desc(int(support_feat.reshape(len(support_feat), -1).shape[1]))
        sf, w = self._rows(support_feat, weights, self.dev)
        self.S, self.C, self.dof, self.D = len(sf), int(w.shape[1]), self.desc.dof, self.desc.feature_dim
        if len(sf) and sf.shape[1] != self.D:
            raise ValueError(f"supports have {sf.shape[1]} features, the transform produces {self.D}")
        self.kernel = (int(kind), float(p0), float(p1))
        self.capacity = max(int(capacity), self.S)
        handle = C.c_void_p()
        with torch.cuda.device(self.dev):
            _lib.check(lib.dcx_model_create_ex(C.byref(handle), self.dev.index, C.byref(self.desc), kind,
                                               _kparams(p0, p1), _ptr(sf), _ptr(w), self.S, self.D, self.C,
                                               self.capacity, _stream(self.dev)))
        self._h = handle
        self._lib = lib
        self.leases = 0          # holders that need the rows to stay as they are (acquire / release)
        self.revision = 0        # bumped by update(): a backward pass that re-sweeps checks it still sees its forward's rows
        self._streams = set()    # raw handles of the streams that have launched this model since the last update()

    def acquire(self):
        """take a lease: while any is held, a FusedScorer builds a NEW model for changed state instead of refilling this one"""
        self.leases += 1
        return self

    def release(self):
        self.leases = max(0, self.leases - 1)

    def update(self, support_feat, weights):
        """new supports / weights into the same model (dcx_model_update): what train / fit_poly / update do to a checker's
        state every round of an active-learning loop.  The refill is enqueued on torch's CURRENT stream; launches of this
        model that went to other streams since the last update are waited for first (device-side, one event each), so a
        sweep still running elsewhere never reads half-packed rows."""
        sf, w = self._rows(support_feat, weights, self.dev)
        if int(w.shape[1]) != self.C or (len(sf) and sf.shape[1] != self.D):
            raise ValueError("update() keeps the model's feature width and class count")
        cur = torch.cuda.current_stream(self.dev)
        for h in self._streams:
            if h != cur.cuda_stream:
                cur.wait_stream(torch.cuda.ExternalStream(h, device=self.dev))
        self._streams.clear()
        with torch.cuda.device(self.dev):
            _lib.check(self._lib.dcx_model_update(self._h, _ptr(sf), _ptr(w), len(sf), _stream(self.dev)))
        self.S = len(sf)
        self.capacity = max(self.capacity, self.S)
        self.revision += 1
        return self

    def _st(self):
        """torch's current stream as the C ABI wants it, remembered for update()'s cross-stream wait"""
        st = _stream(self.dev)
        self._streams.add(st.value or 0)
        return st

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._lib.dcx_model_destroy(h)
            except Exception:
                pass

    # raw entry points on fp32 device tensors -------------------------------------------
    def score_raw(self, q32):
        B = q32.shape[0]
        out = torch.empty((B, self.C), device=self.dev, dtype=torch.float32)
        with _on_device(self.dev):
            _lib.check(self._lib.dcx_score(self._h, _ptr(q32), B, _ptr(out), self._st()))
        return out

    def score_grad_raw(self, q32, upstream32=None, want_score=True):
        B = q32.shape[0]
        out = torch.empty((B, self.C), device=self.dev, dtype=torch.float32) if want_score else None
        grad = torch.empty((B, self.dof), device=self.dev, dtype=torch.float32)
        with _on_device(self.dev):
            _lib.check(self._lib.dcx_score_grad(self._h, _ptr(q32), B, _ptr(upstream32), _ptr(out), _ptr(grad),
                                                self._st()))
        return out, grad

    def score_jac_raw(self, q32):
        B = q32.shape[0]
        out = torch.empty((B, self.C), device=self.dev, dtype=torch.float32)
        jac = torch.empty((B, self.C, self.dof), device=self.dev, dtype=torch.float32)
        with _on_device(self.dev):
            _lib.check(self._lib.dcx_score_jac(self._h, _ptr(q32), B, _ptr(out), _ptr(jac), self._st()))
        return out, jac

    def score_hess_raw(self, q32, upstream32=None):
        """(gradient [B, dof], Hessian [B, dof, dof]) of sum_c upstream * score w.r.t. q — analytic second derivatives
        (dcx_score_hess; the reference double-backwards through dist_est, optim.py:380-391)"""
        B = q32.shape[0]
        grad = torch.empty((B, self.dof), device=self.dev, dtype=torch.float32)
        hess = torch.empty((B, self.dof, self.dof), device=self.dev, dtype=torch.float32)
        with _on_device(self.dev):
            _lib.check(self._lib.dcx_score_hess(self._h, _ptr(q32), B, _ptr(upstream32), _ptr(grad), _ptr(hess),
                                                self._st()))
        return grad, hess

    def margins(self, margin):
        """a safety margin as the C ABI wants it: C host floats (a scalar serves every class, like the reference's broadcast in
        `dist_est(p) - safety_margin`, optim.py:88-89)"""
        if torch.is_tensor(margin):
            margin = margin.detach().reshape(-1).tolist()
        elif not isinstance(margin, (list, tuple)):
            try:
                margin = [float(v) for v in margin.reshape(-1)]      # numpy
            except AttributeError:
                margin = [float(margin)]
        if len(margin) == 1:
            margin = list(margin) * self.C
        if len(margin) != self.C:
            raise ValueError(f"{len(margin)} safety margins for a score with {self.C} outputs")
        return (C.c_float * self.C)(*(float(v) for v in margin))

    def score_hinge_grad_raw(self, q32, margin, weight):
        """(score [B, C], d/dq of weight * sum_c clamp(score_c - margin_c, 0) [B, dof]) - the optimisers' collision term
        (optim.py:88-89); `margin`: a number or one per class.  One launch for one class, two (class scores, then the sweep
        whose upstream is the hinge's indicator) for several."""
        B = q32.shape[0]
        out = torch.empty((B, self.C), device=self.dev, dtype=torch.float32)
        grad = torch.empty((B, self.dof), device=self.dev, dtype=torch.float32)
        with _on_device(self.dev):
            _lib.check(self._lib.dcx_score_hinge_grad_mc(self._h, _ptr(q32), B, self.margins(margin), float(weight), _ptr(out),
                                                         _ptr(grad), self._st()))
        return out, grad

    def check_motions(self, qa, qb, res=None, max_step=None, margin=0., max_samples=None, wrap=None):
        """batched motion checks (dcx_check_motions): for E straight joint-space motions qa[e] -> qb[e] ([E, dof] each),
        (first_hit, n_samples), int32 device tensors [E]: the first sample index with score_c - margin_c > 0 for some class
        (-1: free; -2: the edge needs more than `max_samples` samples and was not checked) and the edge's sample count.
        Exactly one rule: `res` (the points of Perceptron.line_predict) or `max_step` (the points of utils.dense_path).
        `margin`: a number or one per class (a device tensor stays on the device).  Three launches on torch's current
        stream.  The launch grid is sized from E * max_samples, so the bound should be tight: max_samples=None under the
        max_step rule derives it from the longest edge (one read-back of a reduction; edges beyond MOTION_MAX_SAMPLES
        still answer -2).  A given max_samples reads nothing back (capturable).
        `wrap` (wrap_mask: an int bitmask or one bool per coordinate): those coordinates are angles on the circle and the
        edge runs along their shortest arc (dcx_check_motions_ex; the res rule's points are utils.anglin's)."""
        qa32, qb32, E, res, max_step, max_samples, mask = self._motion_args("check_motions", qa, qb, res, max_step, max_samples, wrap)
        opt = _lib.MotionOpts(res, max_step, max_samples, 0)
        mg = self._motion_margin(margin)
        first = torch.empty(E, device=self.dev, dtype=torch.int32)
        n = torch.empty(E, device=self.dev, dtype=torch.int32)
        nbytes = self._lib.dcx_motion_work_bytes(self._h, E)
        work = self._work(nbytes)
        with _on_device(self.dev):
            _lib.check(self._lib.dcx_check_motions_ex(self._h, _ptr(qa32), _ptr(qb32), E, C.byref(opt), _ptr(mg), _ptr(first),
                                                      _ptr(n), _ptr(work), nbytes, mask, self._st()))
        return first, n

    def rrt_connect_run(self, state, samples, round0, range, max_step, max_samples, cap, margin=0., wrap=None):
        """T rounds of batched RRT-Connect (dcx_rrt_connect_run) on the caller's state, in place: `state` maps nodes
        [R, 2, cap, dof] float32, parent [R, 2, cap], count [R, 2], status [R], link [R, 2], solved_round [R] (int32) to
        contiguous tensors on the model's device; samples [T, R, P, dof] float32 there.  Rounds round0 .. round0 + T - 1 are
        enqueued on torch's current stream; nothing is read back (capturable).  `margin` as check_motions."""
        T, R, P = (int(v) for v in samples.shape[:3])
        kinds = dict(nodes=torch.float32, parent=torch.int32, count=torch.int32, status=torch.int32, link=torch.int32,
                     solved_round=torch.int32)
        shapes = dict(nodes=(R, 2, cap, self.dof), parent=(R, 2, cap), count=(R, 2), status=(R,), link=(R, 2), solved_round=(R,))
        for name, dt in kinds.items():
            _check_tensor(f"rrt_connect_run: state[{name!r}]", state[name], dt, shapes[name], self.dev)
        _check_tensor("rrt_connect_run: samples", samples, torch.float32, (T, R, P, self.dof), self.dev,
                      kind=f"float32 tensor [T, R, P, {self.dof}]")
        st = _lib.RrtState(*(state[n].data_ptr() for n in kinds))
        opt = _lib.RrtOpts(float(range), float(max_step), int(max_samples), P, int(cap), 0, wrap_mask(wrap, self.dof),
                           (C.c_int64 * 2)(0, 0))
        mg = self._motion_margin(margin)
        nbytes = self._lib.dcx_rrt_work_bytes(self._h, R, P)
        work = self._work(nbytes)
        with _on_device(self.dev):
            _lib.check(self._lib.dcx_rrt_connect_run(self._h, C.byref(st), R, _ptr(samples), T, int(round0), C.byref(opt), _ptr(mg),
                                                     _ptr(work), nbytes, self._st()))

    def rrtstar_run(self, state, goals, samples, round0, range, max_step, radius, near, max_samples, margin=0., wrap=None, _cost=None):
        """T rounds of batched RRT* (dcx_rrtstar_run) on the caller's state, in place: `state` maps dcx_rrtstar_state's fields
        (nodes [R, cap, dof], elen and cost [R, cap] float32; parent [R, cap], count, status, goal_node, first_round [R] int32)
        to contiguous tensors on the model's device; goals [R, dof] and samples [T, R, P, dof] float32 there.  `near`: K, the
        near set's size (0: plain RRT with costs); `radius`: its radius.  Rounds round0 .. round0 + T - 1 are enqueued on
        torch's current stream; nothing is read back (capturable).  `margin` as check_motions."""
        if samples.dim() != 4:
            raise ValueError("rrtstar_run: samples must be [T, R, P, dof]")
        T, R, P = (int(v) for v in samples.shape[:3])
        st, R0, cap, _ = _rrtstar_state("rrtstar_run", state, self.dev)
        if R0 != R or int(state["nodes"].shape[2]) != self.dof:
            raise ValueError(f"rrtstar_run: state['nodes'] must be [{R}, cap, {self.dof}]")
        _check_tensor("rrtstar_run: samples", samples, torch.float32, (T, R, P, self.dof), self.dev,
                      kind=f"float32 tensor [T, R, P, {self.dof}]")
        _check_tensor("rrtstar_run: goals", goals, torch.float32, (R, self.dof), self.dev)
        opt = _lib.RrtStarOpts(float(range), float(max_step), float(radius), int(max_samples), P, int(near), cap, 0,
                               wrap_mask(wrap, self.dof), (C.c_int64 * 2)(0, 0))
        mg = self._motion_margin(margin)
        if _cost is not None:   # (rrtstar_run_cost)
            nbytes = self._lib.dcx_rrtstar_cost_work_bytes(self._h, R, P, int(near))
            work = self._work(nbytes)
            with _on_device(self.dev):
                _lib.check(self._lib.dcx_rrtstar_run_cost(self._h, C.byref(st), R, _ptr(goals), _ptr(samples), T, int(round0),
                                                          C.byref(opt), C.byref(_cost), _ptr(mg), _ptr(work), nbytes, self._st()))
            return
        nbytes = self._lib.dcx_rrtstar_work_bytes(self._h, R, P, int(near))
        work = self._work(nbytes)
        with _on_device(self.dev):
            _lib.check(self._lib.dcx_rrtstar_run(self._h, C.byref(st), R, _ptr(goals), _ptr(samples), T, int(round0), C.byref(opt),
                                                 _ptr(mg), _ptr(work), nbytes, self._st()))

    @staticmethod
    def _rrtstar_cost_opts(gain, band):
        return _lib.RrtStarCostOpts(_lib.RRTSTAR_COST_PEAK, float(gain), float(band), 0, (C.c_int64 * 2)(0, 0))

    def rrtstar_run_cost(self, state, goals, samples, round0, range, max_step, radius, near, max_samples, gain, band, margin=0.,
                         wrap=None):
        """rrtstar_run under clearance-weighted edge costs (dcx_rrtstar_run_cost): an edge with peak w = max over its samples of
        score - margin is free where w <= 0 and costs C = L * (1 + gain * max(w + band, 0)), every operation fp32 and rounded
        alone; state['elen'] holds C.  gain, band >= 0; gain = 0 is rrtstar_run bit for bit.  Everything else as rrtstar_run."""
        self.rrtstar_run(state, goals, samples, round0, range, max_step, radius, near, max_samples, margin=margin, wrap=wrap,
                         _cost=self._rrtstar_cost_opts(gain, band))

    def rrtstar_run_sampled_cost(self, state, goals, limits, seed, T, slots, round0, range, max_step, radius, near, max_samples, gain,
                                 band, **kw):
        """rrtstar_run_sampled under rrtstar_run_cost's objective (dcx_rrtstar_run_sampled_cost); `kw`: rrtstar_run_sampled's
        mode, goal_bias, uniform_mix, tries, margin, wrap, samples_out and info_out.  The informed draw reads the goal node's
        cost, which is never below its path's length: the ellipsoid stays admissible."""
        self.rrtstar_run_sampled(state, goals, limits, seed, T, slots, round0, range, max_step, radius, near, max_samples,
                                 _cost=self._rrtstar_cost_opts(gain, band), **kw)

    def rrtstar_run_sampled(self, state, goals, limits, seed, T, slots, round0, range, max_step, radius, near, max_samples,
                            mode="informed", goal_bias=0.1, uniform_mix=0., tries=8, margin=0., wrap=None, samples_out=None,
                            info_out=None, _cost=None):
        """T rounds of batched RRT* whose samples are drawn on the device at the start of each round (dcx_rrtstar_run_sampled:
        per round rrtstar_sample's launch on the state as it stands, then rrtstar_run's round), in place on `state`; `state`,
        goals, range .. max_samples, margin and wrap as rrtstar_run; limits [dof, 2] float32 on the model's device; seed, mode,
        goal_bias, uniform_mix and tries as _ops.rrtstar_sample.  samples_out [T, R, slots, dof] float32 / info_out
        [T, R, slots] int32: where the rounds' samples and info words are kept (None: nowhere).  Rounds round0 .. round0 + T - 1
        are enqueued on torch's current stream; nothing is read back (capturable)."""
        T, P = int(T), int(slots)
        st, R, cap, _ = _rrtstar_state("rrtstar_run_sampled", state, self.dev)
        if int(state["nodes"].shape[2]) != self.dof:
            raise ValueError(f"rrtstar_run_sampled: state['nodes'] must be [R, cap, {self.dof}]")
        _check_tensor("rrtstar_run_sampled: goals", goals, torch.float32, (R, self.dof), self.dev)
        mask = wrap_mask(wrap, self.dof)
        sopt = _rrtstar_sample_opts("rrtstar_run_sampled", limits, self.dof, self.dev, seed, P, cap, mode, goal_bias, uniform_mix, tries,
                                    mask)
        if samples_out is not None:
            _check_tensor("rrtstar_run_sampled: samples_out", samples_out, torch.float32, (T, R, P, self.dof), self.dev)
        if info_out is not None:
            _check_tensor("rrtstar_run_sampled: info_out", info_out, torch.int32, (T, R, P), self.dev)
        opt = _lib.RrtStarOpts(float(range), float(max_step), float(radius), int(max_samples), P, int(near), cap, 0, mask,
                               (C.c_int64 * 2)(0, 0))
        mg = self._motion_margin(margin)
        if _cost is not None:   # (rrtstar_run_sampled_cost)
            nbytes = self._lib.dcx_rrtstar_sampled_cost_work_bytes(self._h, R, P, int(near))
            work = self._work(nbytes)
            with _on_device(self.dev):
                _lib.check(self._lib.dcx_rrtstar_run_sampled_cost(self._h, C.byref(st), R, _ptr(goals), C.byref(sopt), T, int(round0),
                                                                  C.byref(opt), C.byref(_cost), _ptr(mg), _ptr(work), nbytes,
                                                                  _ptr(samples_out), _ptr(info_out), self._st()))
            return
        nbytes = self._lib.dcx_rrtstar_sampled_work_bytes(self._h, R, P, int(near))
        work = self._work(nbytes)
        with _on_device(self.dev):
            _lib.check(self._lib.dcx_rrtstar_run_sampled(self._h, C.byref(st), R, _ptr(goals), C.byref(sopt), T, int(round0),
                                                         C.byref(opt), _ptr(mg), _ptr(work), nbytes, _ptr(samples_out),
                                                         _ptr(info_out), self._st()))

    def shortcut_run(self, state, draws, max_step, max_samples, margin=0., wrap=None, partial=False, cost=None, seg=None):
        """T rounds of batched path shortcutting (dcx_path_shortcut_run; partial=True: dcx_path_shortcut_partial_run, chords
        between points inside segments, W also the capacity a path may grow into) on the caller's state, in place: `state` maps
        path [R, W, dof] float32, count [R] and accepted [R] (int32) to contiguous tensors on the model's device; draws
        [T, R, P, 2] float32 there.  The rounds are enqueued on torch's current stream; nothing is read back (capturable).
        `margin` as check_motions.
        cost=(gain, band): the rounds under the clearance objective (dcx_path_shortcut_run_cost / _partial_run_cost: a chord is
        kept only if it is free and costs less than what it removes, C = L * (1 + gain * max(w + band, 0)) per edge); `seg`
        [R, W] float32 on the model's device then holds the segments' costs, in place as the rest of the state."""
        if draws.dim() != 4:
            raise ValueError("shortcut_run: draws must be [T, R, P, 2]")
        if (cost is None) != (seg is None):
            raise ValueError("shortcut_run: cost=(gain, band) and seg [R, W] go together")
        T, R, P = (int(v) for v in draws.shape[:3])
        path = state["path"]
        if path.dim() != 3:
            raise ValueError("shortcut_run: state['path'] must be [R, W, dof]")
        W = int(path.shape[1])
        kinds = dict(path=torch.float32, count=torch.int32, accepted=torch.int32)
        shapes = dict(path=(R, W, self.dof), count=(R,), accepted=(R,))
        for name, dt in kinds.items():
            _check_tensor(f"shortcut_run: state[{name!r}]", state[name], dt, shapes[name], self.dev)
        _check_tensor("shortcut_run: draws", draws, torch.float32, (T, R, P, 2), self.dev, kind="float32 tensor [T, R, P, 2]")
        st = _lib.ShortcutState(*(state[n].data_ptr() for n in kinds))
        opt = _lib.ShortcutOpts(float(max_step), int(max_samples), P, W, wrap_mask(wrap, self.dof), (C.c_int64 * 2)(0, 0))
        mg = self._motion_margin(margin)
        if cost is not None:
            _check_tensor("shortcut_run: seg", seg, torch.float32, (R, W), self.dev)
            co = self._rrtstar_cost_opts(*cost)
            if partial:
                nbytes = self._lib.dcx_path_shortcut_partial_cost_work_bytes(self._h, R, P, W)
                run = self._lib.dcx_path_shortcut_partial_run_cost
            else:
                nbytes, run = self._lib.dcx_path_shortcut_cost_work_bytes(self._h, R, P), self._lib.dcx_path_shortcut_run_cost
            work = self._work(nbytes)
            with _on_device(self.dev):
                _lib.check(run(self._h, C.byref(st), _ptr(seg), R, _ptr(draws), T, C.byref(opt), C.byref(co), _ptr(mg), _ptr(work),
                               nbytes, self._st()))
            return
        if partial:
            nbytes, run = self._lib.dcx_path_shortcut_partial_work_bytes(self._h, R, P, W), self._lib.dcx_path_shortcut_partial_run
        else:
            nbytes, run = self._lib.dcx_path_shortcut_work_bytes(self._h, R, P), self._lib.dcx_path_shortcut_run
        work = self._work(nbytes)
        with _on_device(self.dev):
            _lib.check(run(self._h, C.byref(st), R, _ptr(draws), T, C.byref(opt), _ptr(mg), _ptr(work), nbytes, self._st()))

    def _motion_args(self, name, qa, qb, res, max_step, max_samples, wrap):
        """what every motion call starts with: (qa32, qb32 [E, dof] fp32 on the device, E, res, max_step, max_samples, mask) with
        the rule as the options struct holds it (0 / 0.0 for the one not given).  max_samples=None is `res`, or under max_step
        motion_bound's (one read-back)."""
        if (res is None) == (max_step is None):
            raise ValueError(f"{name} takes exactly one of res and max_step")
        mask = wrap_mask(wrap, self.dof)
        # (as_tensor costs 0.3 us even on a tensor: skipping it there pays for this method's own call)
        qa32 = _f32((qa if isinstance(qa, torch.Tensor) else torch.as_tensor(qa)).reshape(-1, self.dof), self.dev)
        qb32 = _f32((qb if isinstance(qb, torch.Tensor) else torch.as_tensor(qb)).reshape(-1, self.dof), self.dev)
        if qa32.shape != qb32.shape:
            raise ValueError(f"{len(qa32)} start and {len(qb32)} target configurations")
        if max_samples is None:
            max_samples = int(res) if res is not None else motion_bound(qa32, qb32, max_step, wrap=mask)
        return (qa32, qb32, len(qa32), int(res) if res is not None else 0, float(max_step) if max_step is not None else 0.0,
                int(max_samples), mask)

    def _work(self, nbytes):
        """a call's workspace of nbytes (what its dcx_*_work_bytes answers): torch's caching allocator is the per-device cache
        (a freed block is reused on its stream, no hipMalloc)"""
        return torch.empty(max(nbytes, 1), device=self.dev, dtype=torch.uint8)

    def _motion_margin(self, margin):
        """the motion calls' margin argument: None (all zero), or [C] device floats (a device tensor stays on the device)"""
        if torch.is_tensor(margin) and margin.device == self.dev:
            # (no copy through the host: the call can be captured in a graph)
            return margin.detach().to(torch.float32).reshape(-1).expand(self.C).contiguous()
        if torch.is_tensor(margin) or not (isinstance(margin, (int, float)) and float(margin) == 0.0):
            return torch.tensor(list(self.margins(margin)), dtype=torch.float32).to(self.dev)
        return None

    def motion_cost_raw(self, qa, qb, res=None, max_step=None, margin=0., weight=1., open_end=False, max_samples=None,
                        wrap=None):
        """differentiable motion costs (dcx_motion_cost): for E straight joint-space motions qa[e] -> qb[e] ([E, dof] each),
        (cost [E], grad_a [E, dof], grad_b [E, dof], n_samples [E] int32), fp32 device tensors:
        cost[e] = weight * sum over the edge's samples of sum_c max(0, score_c - margin_c), and its gradients with respect to
        qa[e] and qb[e] through the interpolation.  Exactly one rule, as check_motions: `res` or `max_step`; `open_end` drops
        the target sample under max_step (the edges of a path plus its last waypoint then cover utils.dense_path once).
        Edges over `max_samples` answer NaN.  max_samples=None under max_step derives the bound from the longest edge (one
        read-back); a given bound reads nothing back (capturable).  Four launches (C > 1: five) on torch's current stream.
        `wrap`: as check_motions (dcx_motion_cost_ex); the gradients' unit direction is that of the wrapped edge."""
        qa32, qb32, E, res, max_step, max_samples, mask = self._motion_args("motion_cost", qa, qb, res, max_step, max_samples, wrap)
        opt = _lib.MotionCostOpts(res, max_step, max_samples, 1 if open_end else 0)
        mg = self._motion_margin(margin)
        cost = torch.empty(E, device=self.dev, dtype=torch.float32)
        ga = torch.empty((E, self.dof), device=self.dev, dtype=torch.float32)
        gb = torch.empty((E, self.dof), device=self.dev, dtype=torch.float32)
        n = torch.empty(E, device=self.dev, dtype=torch.int32)
        nbytes = self._lib.dcx_motion_cost_work_bytes(self._h, E, max_samples)
        work = self._work(nbytes)
        with _on_device(self.dev):
            _lib.check(self._lib.dcx_motion_cost_ex(self._h, _ptr(qa32), _ptr(qb32), E, C.byref(opt), _ptr(mg), float(weight),
                                                    _ptr(cost), _ptr(ga), _ptr(gb), _ptr(n), _ptr(work), nbytes, mask,
                                                    self._st()))
        return cost, ga, gb, n

    def motion_cost(self, qa, qb, res=None, max_step=None, margin=0., weight=1., open_end=False, max_samples=None, wrap=None):
        """[E] motion costs (motion_cost_raw), differentiable with respect to qa and qb (backward: upstream[e] * grad_*[e]; no
        second derivatives).  Returned on qa's device and dtype."""
        qa, qb = torch.as_tensor(qa), torch.as_tensor(qb)
        kw = dict(res=res, max_step=max_step, margin=margin, weight=weight, open_end=open_end, max_samples=max_samples, wrap=wrap)
        if not ((qa.requires_grad or qb.requires_grad) and torch.is_grad_enabled()):
            cost = self.motion_cost_raw(qa, qb, **kw)[0]
            return cost.to(device=qa.device, dtype=qa.dtype)
        return _MotionCostFn.apply(qa, qb, self, kw)

    def path_cost(self, paths, max_step, margin=0., weight=1., max_samples=None, wrap=None):
        """[T] collision costs of T piecewise-straight paths [T, W, dof]: weight * sum over utils.dense_path(p, max_step)'s
        points of sum_c max(0, score_c - margin_c), differentiable with respect to every waypoint (compose_path_cost).
        `wrap`: every segment runs along the shortest arc of the masked coordinates (motion_cost's)."""
        kw = dict(max_step=max_step, margin=margin, weight=weight, max_samples=max_samples, wrap=wrap)
        return compose_path_cost(lambda a, b, open_end: self.motion_cost(a, b, open_end=open_end, **kw), paths, self.dof)

    def motion_worst_raw(self, qa, qb, res=None, max_step=None, margin=0., max_samples=None, wrap=None, grad=False):
        """worst-sample motion queries (dcx_motion_worst): for E straight joint-space motions qa[e] -> qb[e] ([E, dof] each) on
        check_motions' sample set, (worst [E] fp32, idx [E] int32, cls [E] int32, n_samples [E] int32[, grad_a, grad_b
        [E, dof] fp32]) device tensors: worst[e] = max over the edge's samples of max_c (score_c - margin_c), the smallest
        sample index that attains it, the smallest class that attains it there, and with grad=True the gradient of worst[e]
        with respect to qa[e] and qb[e] through that sample.  Edges over `max_samples`: NaN / -2 / -1, NaN gradient rows.
        `res`, `max_step`, `margin`, `max_samples` (None: the bound of motion_bound; a given bound reads nothing back and
        the call can be captured) and `wrap` as check_motions."""
        qa32, qb32, E, res, max_step, max_samples, mask = self._motion_args("motion_worst", qa, qb, res, max_step, max_samples, wrap)
        opt = _lib.MotionOpts(res, max_step, max_samples, 0)
        mg = self._motion_margin(margin)
        worst = torch.empty(E, device=self.dev, dtype=torch.float32)
        idx = torch.empty(E, device=self.dev, dtype=torch.int32)
        cls = torch.empty(E, device=self.dev, dtype=torch.int32)
        n = torch.empty(E, device=self.dev, dtype=torch.int32)
        ga = torch.empty((E, self.dof), device=self.dev, dtype=torch.float32) if grad else None
        gb = torch.empty((E, self.dof), device=self.dev, dtype=torch.float32) if grad else None
        nbytes = self._lib.dcx_motion_worst_work_bytes(self._h, E)
        work = self._work(nbytes)
        with _on_device(self.dev):
            _lib.check(self._lib.dcx_motion_worst(self._h, _ptr(qa32), _ptr(qb32), E, C.byref(opt), _ptr(mg), _ptr(worst), _ptr(idx),
                                                  _ptr(cls), _ptr(n), _ptr(ga), _ptr(gb), _ptr(work), nbytes, mask, self._st()))
        return (worst, idx, cls, n, ga, gb) if grad else (worst, idx, cls, n)

    def motion_worst(self, qa, qb, res=None, max_step=None, margin=0., max_samples=None, wrap=None):
        """(worst [E], idx [E], cls [E]) of motion_worst_raw; worst is differentiable with respect to qa and qb (backward:
        upstream[e] * grad_*[e], the sub-gradient through the worst sample; no second derivatives) and is returned on qa's
        device and dtype."""
        qa, qb = torch.as_tensor(qa), torch.as_tensor(qb)
        kw = dict(res=res, max_step=max_step, margin=margin, max_samples=max_samples, wrap=wrap)
        if not ((qa.requires_grad or qb.requires_grad) and torch.is_grad_enabled()):
            worst, idx, cls, _ = self.motion_worst_raw(qa, qb, **kw)
            return worst.to(device=qa.device, dtype=qa.dtype), idx, cls
        return _MotionWorstFn.apply(qa, qb, self, kw)

    def path_worst(self, paths, max_step, margin=0., max_samples=None, wrap=None):
        """(worst [T], segment [T], sample [T]) of T piecewise-straight paths [T, W, dof]: the peak of max_c (score_c -
        margin_c) over every segment's closed max_step sample set, the first maximum in (segment, sample) order; worst is
        differentiable with respect to every waypoint (compose_path_worst over motion_worst)."""
        kw = dict(max_step=max_step, margin=margin, max_samples=max_samples, wrap=wrap)
        return compose_path_worst(lambda a, b: self.motion_worst(a, b, **kw), paths, self.dof)

    def motion_band_raw(self, qa, qb, lo, hi, res=None, max_step=None, max_samples=None, wrap=None, unc_cap=0, want_q=True):
        """one dcx_motion_band call with a list capacity of `unc_cap` entries; nothing is read back (capturable when
        max_samples is given and lo / hi are numbers or device tensors).  A dict of device tensors: verdict, first_hit,
        n_samples, n_uncertain [E] int32, unc_total [1] int64, unc_edge, unc_sample [unc_cap] int32, unc_q [unc_cap, dof]
        fp32 (None without want_q).  Only the first min(unc_total, unc_cap) list entries are written."""
        qa32, qb32, E, res, max_step, max_samples, mask = self._motion_args("motion_band", qa, qb, res, max_step, max_samples, wrap)
        on_dev = lambda t: torch.is_tensor(t) and t.device == self.dev
        if not (on_dev(lo) or on_dev(hi)):   # (device thresholds are not read back: there hit wins, as in the C call)
            bad = [c for c, (l, h) in enumerate(zip(self.margins(lo), self.margins(hi))) if l > h]
            if bad:
                raise ValueError(f"motion_band: lo > hi for class {bad[0]}")
        cap = int(unc_cap)
        if cap < 0:
            raise ValueError("motion_band: a negative list capacity")
        opt = _lib.MotionOpts(res, max_step, max_samples, 0)
        lo_t, hi_t = self._motion_margin(lo), self._motion_margin(hi)
        i32 = lambda *shape: torch.empty(shape, device=self.dev, dtype=torch.int32)
        r = dict(verdict=i32(E), first_hit=i32(E), n_samples=i32(E), n_uncertain=i32(E),
                 unc_total=torch.zeros(1, device=self.dev, dtype=torch.int64), unc_edge=i32(cap), unc_sample=i32(cap),
                 unc_q=torch.empty((cap, self.dof), device=self.dev, dtype=torch.float32) if want_q else None)
        out = _lib.MotionBandOut(*(_ptr(r[k]) for k in ("verdict", "first_hit", "n_samples", "n_uncertain", "unc_total",
                                                        "unc_edge", "unc_sample", "unc_q")), cap)
        nbytes = self._lib.dcx_motion_band_work_bytes(self._h, E, max_samples)
        work = self._work(nbytes)
        with _on_device(self.dev):
            _lib.check(self._lib.dcx_motion_band(self._h, _ptr(qa32), _ptr(qb32), E, C.byref(opt), _ptr(lo_t), _ptr(hi_t),
                                                 C.byref(out), _ptr(work), nbytes, mask, self._st()))
        return r

    def motion_band(self, qa, qb, lo, hi, res=None, max_step=None, max_samples=None, wrap=None, max_uncertain=None, want_q=True):
        """hybrid motion checks (dcx_motion_band): for E straight joint-space motions qa[e] -> qb[e] ([E, dof] each) on
        check_motions' sample set and two thresholds lo <= hi (a number or one per class, as `margin`), a sample is a sure hit
        where score_c - hi_c > 0 for some class, surely clear where score_c - lo_c <= 0 for every class, and uncertain
        otherwise (a NaN score included).  Returns (verdict, first_hit, n_uncertain, unc_edge, unc_sample, unc_q), device tensors:
          verdict [E] int32      1 a sure hit, else 2 an uncertain sample, else 0; -2: over `max_samples`, not checked
          first_hit [E] int32    the first sure hit: check_motions(margin=hi)'s answer, bit for bit
          n_uncertain [E] int32  the uncertain samples of a verdict-2 edge, 0 for every other edge
          unc_edge, unc_sample [U] int32, unc_q [U, dof] fp32 (None without want_q): the uncertain samples of the verdict-2
                                 edges in (edge, sample) order with their configurations - what a ground-truth checker still
                                 has to look at
        max_uncertain=None: U is the full count.  The call picks a capacity, reads the count back - this SYNCHRONISES - and
        repeats once with the exact capacity if the list was cut.  max_uncertain given: the list arrays have that many rows,
        of which the first min(unc_total, max_uncertain) are written; nothing is read back (with max_samples given the call
        can be captured) and unc_total ([1] int64, device) is returned as a seventh value.
        Raises ValueError where lo > hi for some class.  `res`, `max_step`, `max_samples` and `wrap` as check_motions."""
        kw = dict(res=res, max_step=max_step, max_samples=max_samples, wrap=wrap, want_q=want_q)
        keys = ("verdict", "first_hit", "n_uncertain", "unc_edge", "unc_sample", "unc_q")
        if max_uncertain is not None:
            r = self.motion_band_raw(qa, qb, lo, hi, unc_cap=max_uncertain, **kw)
            return tuple(r[k] for k in keys) + (r["unc_total"],)
        E = torch.as_tensor(qa).reshape(-1, self.dof).shape[0]
        r = self.motion_band_raw(qa, qb, lo, hi, unc_cap=max(4096, 2 * E), **kw)
        total = int(r["unc_total"])
        if total > len(r["unc_edge"]):
            r = self.motion_band_raw(qa, qb, lo, hi, unc_cap=total, **kw)
        cut = lambda t: None if t is None else t[:total]
        return r["verdict"], r["first_hit"], r["n_uncertain"], cut(r["unc_edge"]), cut(r["unc_sample"]), cut(r["unc_q"])

    def score_band(self, q, lo, hi):
        """(label [B] int32, unc_idx [U] int64) for configurations q [B, dof]: label 1 where score_c - hi_c > 0 for some class,
        0 where score_c - lo_c <= 0 for every class, 2 otherwise, and the ascending indices of the label-2 configurations.
        It is motion_band(q, q, res=1): one sample per "edge" (synchronises, as motion_band without max_uncertain)."""
        verdict, _, _, unc_edge, _, _ = self.motion_band(q, q, lo, hi, res=1, want_q=False)
        return verdict, unc_edge.to(torch.int64)

    # autograd-aware ------------------------------------------------------------------------
    def score(self, q: torch.Tensor) -> torch.Tensor:
        """[B, C] scores for q [B, dof]; differentiable w.r.t. q (gradient from the fused HIP pass)."""
        if not (q.requires_grad and torch.is_grad_enabled()):
            # nothing to differentiate: the score-only sweep, no autograd.Function around it (its apply() alone cost 10 us of
            # a 17 us call: profiles/r05_api_latency.txt)
            s = self.score_raw(_f32(q.reshape(-1, self.dof), self.dev))
            return s if (s.device == q.device and s.dtype == q.dtype) else s.to(device=q.device, dtype=q.dtype)
        return _ScoreFn.apply(q, self)

    def score_and_grad(self, q: torch.Tensor, upstream: torch.Tensor = None):
        """(score [B, C], d(sum_c upstream*score)/dq [B, dof]) in ONE launch, no autograd graph."""
        q32 = _f32(q.reshape(-1, self.dof), self.dev)
        up = None if upstream is None else _f32(upstream.reshape(-1, self.C), self.dev)
        s, g = self.score_grad_raw(q32, up)
        return s.to(device=q.device, dtype=q.dtype), g.to(device=q.device, dtype=q.dtype)


def _is_batched(t):
    """True inside torch.vmap (e.g. torch.autograd.functional.jacobian(vectorize=True) batching the backward)"""
    ft = getattr(torch._C, "_functorch", None)
    for name in ("is_batchedtensor", "is_legacy_batchedtensor"):  # torch.vmap / the legacy vmap autograd still uses
        f = getattr(ft, name, None)
        if f is not None and f(t):
            return True
    return False


class _ScoreFn(torch.autograd.Function):
    """score = model(q), differentiable w.r.t. q.

    C == 1: when q needs a gradient the forward launch is the fused score+gradient pass and backward is one
    elementwise multiply.  C > 1: forward is the score-only sweep; backward runs ONE sweep with the actual upstream
    (`dcx_score_grad`) — unless it is being vmapped (`torch.autograd.functional.jacobian(vectorize=True)`, the
    reference's optim.py:211-216, batches the backward over one-hot upstreams): then the full Jacobian is formed once
    (`dcx_score_jac`, one sweep per class) and contracted with torch ops, which vmap can batch."""

    @staticmethod
    def forward(ctx, q, model):
        q32 = _f32(q.reshape(-1, model.dof), model.dev)
        ctx.model, ctx.in_shape, ctx.in_dtype, ctx.in_device = model, q.shape, q.dtype, q.device
        if ctx.needs_input_grad[0] and model.C == 1:
            s, jac = model.score_jac_raw(q32)
            ctx.save_for_backward(jac.reshape(-1, model.dof).to(device=q.device, dtype=q.dtype))   # d score / d q  [B, dof]
        else:
            s = model.score_raw(q32)
            ctx.save_for_backward(q32)
            ctx.revision = model.revision   # (C > 1: backward sweeps again - against the rows this forward saw, or not at all)
        return s.to(device=q.device, dtype=q.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gs):
        (saved,) = ctx.saved_tensors
        model = ctx.model
        if model.C == 1:  # saved = d score / d q  [B, dof]; gs [B, 1]: ONE elementwise launch
            return (gs * saved).reshape(ctx.in_shape), None
        q32 = saved
        if model.revision != ctx.revision:
            # train / fit_poly / update refilled the model's rows in place between this forward and its backward:
            # the gradient would be the NEW model's
            raise RuntimeError("the checker's supports / weights changed between the forward pass of a multi-class score and its "
                               "backward pass: run backward before retraining (or score again)")
        if _is_batched(gs):
            _, jac = model.score_jac_raw(q32)  # [B, C, dof]
            jac = jac.to(device=ctx.in_device, dtype=ctx.in_dtype)
            return (gs.unsqueeze(-1) * jac).sum(dim=-2).reshape(ctx.in_shape), None
        _, g = model.score_grad_raw(q32, _f32(gs.reshape(-1, model.C), model.dev), want_score=False)
        return g.to(device=ctx.in_device, dtype=ctx.in_dtype).reshape(ctx.in_shape), None


class _EndpointGradFn(torch.autograd.Function):
    """f(qa, qb, model, kw) whose forward saves d f[e] / d qa[e] and d f[e] / d qb[e] in the inputs' shapes: backward scales them
    by the upstream of the first output (no second derivatives)"""

    @staticmethod
    @once_differentiable
    def backward(ctx, up, *_):
        ga, gb = ctx.saved_tensors
        up = up.reshape((-1,) + (1,) * (ga.dim() - 1))
        return (up * ga if ctx.needs_input_grad[0] else None), (up * gb if ctx.needs_input_grad[1] else None), None, None


class _MotionCostFn(_EndpointGradFn):
    """cost = motion_cost(qa, qb) [E]: ONE dcx_motion_cost call forms the cost and both endpoint gradients"""

    @staticmethod
    def forward(ctx, qa, qb, model, kw):
        cost, ga, gb, _ = model.motion_cost_raw(qa, qb, **kw)
        ctx.save_for_backward(ga.to(device=qa.device, dtype=qa.dtype).reshape(qa.shape),
                              gb.to(device=qb.device, dtype=qb.dtype).reshape(qb.shape))
        return cost.to(device=qa.device, dtype=qa.dtype)


class _MotionWorstFn(_EndpointGradFn):
    """(worst, idx, cls) = motion_worst(qa, qb): ONE dcx_motion_worst call forms the peak and both endpoint gradients"""

    @staticmethod
    def forward(ctx, qa, qb, model, kw):
        worst, idx, cls, _, ga, gb = model.motion_worst_raw(qa, qb, grad=True, **kw)
        ctx.save_for_backward(ga.to(device=qa.device, dtype=qa.dtype).reshape(qa.shape),
                              gb.to(device=qb.device, dtype=qb.dtype).reshape(qb.shape))
        ctx.mark_non_differentiable(idx, cls)
        return worst.to(device=qa.device, dtype=qa.dtype), idx, cls
