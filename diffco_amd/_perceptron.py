"""Logic shared by the checkers: the kernel-perceptron trainer and the glue that turns a checker's
state (transform, kernel, supports, weights) into a fused HIP score model.

The trainer is inherently sequential (one argmin per iteration).  For diffco_amd kernels the whole loop runs
in ONE persistent launch on the GPU (`dcx_train_perceptron`, csrc/train_kernels.hip — SURVEY.md §8f-1); for a
foreign kernel callable the same algorithm runs as a host loop below, filling kernel rows by calling it like
the reference does.  Behaviour restated from the reference: DiffCo.train_perceptron
kernel_perceptrons.py:98-137 and MultiDiffCo.train_perceptron deprecated/MultiDiffCo.py:50-83.
"""
from typing import NamedTuple

import torch

from . import _ops
from .kernel import FKKernel, KernelFunc


# ----------------------------------------------------------------------------- row fill
class RowFiller:
    """`fill(i)` -> K(x_i, X) as a 1-D tensor on `out_device`.

    For a diffco_amd kernel the features are uploaded once and every row is one
    `dcx_kernel_matrix` launch (B = 1); a foreign callable is simply called like the reference does."""

    def __init__(self, kernel_func, feats, out_device):
        self.kernel_func, self.out_device = kernel_func, out_device
        self.spec = kernel_func.dcx_spec() if isinstance(kernel_func, KernelFunc) and not isinstance(
            kernel_func, FKKernel) else None
        if self.spec is not None:
            self.dev = _ops._device(feats.device)
            self.flat = feats.reshape(len(feats), -1).to(device=self.dev, dtype=torch.float32).contiguous()
            self.dtype = feats.dtype
        else:
            self.feats = feats

    def __call__(self, i):
        if self.spec is not None:
            kind, p0, p1 = self.spec
            row = _ops.kernel_matrix(kind, p0, p1, self.flat[i:i + 1], self.flat)
            return row.reshape(-1).to(device=self.out_device, dtype=self.dtype)
        row = self.kernel_func(self.feats[i], self.feats)
        return row.reshape(-1).to(self.out_device)


# ----------------------------------------------------------------------------- trainer
def _one_class_step(y, hypo, gains, K, fill, beta):
    """One perceptron step for one label column.  Returns True when this column has converged.
    y / hypo / gains are 1-D views that are updated in place."""
    margin = y * hypo
    worst = int(torch.argmin(margin))
    if K[worst, worst] == 0:  # row not computed yet (k(x, x) != 0 marks a filled row)
        row = fill(worst)
        K[worst] = row
        K[:, worst] = row
    if margin[worst] <= 0:
        target = beta ** ((1 + y[worst]) / 2) * y[worst]  # beta scales the positive target
        step = (target - hypo[worst]) / K[worst, worst]
        gains[worst] += step
        hypo += step * K[worst]
        return False
    # every sample is on the right side: try to retire a support that is classified correctly without itself
    active = gains != 0
    slack = y * (hypo - gains * torch.diagonal(K)) * active
    cand = int(torch.argmax(slack))
    if slack[cand] > 0 and int(active.sum()) > 1:
        hypo -= gains[cand] * K[cand]
        gains[cand] = 0
        return False
    return True


def train_perceptron(y, hypo, gains, K, fill, beta, max_iteration, progress=None):
    """Run the (multi-)label kernel perceptron in place.  1-D y: one column; 2-D y [N, C]: the
    columns take one step each per outer iteration and share K.  Returns iterations used."""
    if y.ndim == 1:
        it = 0
        for it in range(max_iteration):
            if progress is not None:
                progress.update(1)
            if _one_class_step(y, hypo, gains, K, fill, beta):
                break
        return it
    C = y.shape[1]
    done = torch.zeros(C, dtype=torch.bool)
    it = 0
    for it in range(max_iteration):
        if progress is not None:
            progress.update(1)
        for c in range(C):
            if _one_class_step(y[:, c], hypo[:, c], gains[:, c], K, fill, beta):
                done[c] = True
        if bool(done.all()):
            break
    return it


def device_trainer_spec(kernel_func):
    """(kind, p0, p1) when the training kernel can run inside the persistent device trainer, else None.
    DCX_HOST_TRAINER=1 forces the host loop (A/B and debugging)."""
    import os
    if os.environ.get("DCX_HOST_TRAINER") == "1":
        return None
    if isinstance(kernel_func, KernelFunc) and not isinstance(kernel_func, FKKernel):
        return kernel_func.dcx_spec()
    return None


def run_trainer(kernel_func, feats, y, gains, hypo, K, beta, max_iteration, progress=None, cold=False):
    """Train in place semantics, wherever it is fastest: the persistent device kernel for diffco_amd kernels
    (one launch for the whole loop), the host loop otherwise.  K may be None for a cold start (the N x N matrix is
    then created where the trainer runs).  Returns (gains, hypo, K, iterations)."""
    spec = device_trainer_spec(kernel_func)
    if K is None and (spec is None or not cold):
        K = torch.zeros((len(y), len(y)), dtype=gains.dtype, device=gains.device)  # lazily filled
    if spec is None:
        fill = RowFiller(kernel_func, feats, K.device)
        it = train_perceptron(y, hypo, gains, K, fill, beta, max_iteration, progress)
        return gains, hypo, K, it
    out_dev, out_dtype = gains.device, gains.dtype
    g, h, Kd, it, _ = _ops.train_perceptron_device(spec[0], spec[1], spec[2], beta, feats, y, gains, hypo,
                                                   None if cold else K, max_iteration)
    if progress is not None:
        progress.update(it)
    # gains / hypothesis go back to where the caller keeps them; the N x N kernel matrix stays on the GPU (callers
    # only ever take the support sub-block of it: see sub_block)
    return g.to(device=out_dev, dtype=out_dtype), h.to(device=out_dev, dtype=out_dtype), Kd, it


def solve_system(kernel_func, kmat, rhs):
    """fit_poly's S x S solve: on the GPU for diffco_amd kernels (`_ops.solve`); a foreign kernel callable is user
    code evaluated where its tensors live, like the host trainer above, and its system is solved there too."""
    if isinstance(kernel_func, KernelFunc) and kernel_func.dcx_spec() is not None or isinstance(kernel_func, FKKernel):
        return _ops.solve(kmat, rhs)
    return torch.linalg.solve(kmat, rhs.to(kmat.dtype))


def fit_system(kernel_func, feats, targets, reg=0.0):
    """fit_poly's nodes: (K(feats, feats) + reg I) nodes = targets.  For a diffco_amd kernel on plain feature rows the
    matrix is built and solved on the device in one go (`_ops.fit_nodes`: dcx_kernel_matrix + dcx_solve, nothing but the
    nodes comes back); anything else builds the matrix through the callable and goes through solve_system."""
    spec = kernel_func.dcx_spec() if isinstance(kernel_func, KernelFunc) else None
    if spec is not None and len(feats) >= 1:
        return _ops.fit_nodes(spec[0], spec[1], spec[2], feats, targets, reg)
    kmat = kernel_func(feats, feats)
    if reg:
        kmat = kmat + reg * torch.eye(len(kmat), dtype=kmat.dtype, device=kmat.device)
    return solve_system(kernel_func, kmat, targets.to(kmat.dtype))


def sub_block(K, idx, device, dtype):
    """K[idx][:, idx] gathered where K lives, then moved to (device, dtype)"""
    i = idx.to(K.device)
    return K[i[:, None], i[None, :]].to(device=device, dtype=dtype)


# ----------------------------------------------------------------------------- fused-model glue
def transform_desc(transform):
    """FK description when `transform` is the bound `fkine` of a diffco_amd.model robot, else None."""
    owner = getattr(transform, "__self__", None)
    if owner is not None and getattr(transform, "__name__", "") == "fkine":
        fk = getattr(owner, "fk_desc", None)
        if callable(fk):
            return fk()
    return None


def kernel_spec(kernel_func):
    spec = kernel_func.dcx_spec() if isinstance(kernel_func, KernelFunc) else None
    if spec is None:
        raise TypeError(
            f"{type(kernel_func).__name__} is not a diffco_amd kernel: the score path is HIP-only and supports "
            "kernel.RQKernel / Polyharmonic / MultiQuadratic (optionally wrapped in kernel.FKKernel)")
    return spec


def _foreign(m, transform):
    """True where `transform` is a foreign callable: the model `m` has no FK of its own, the transform runs in torch and only
    what follows it fuses.  The motion calls then take the host route."""
    return m.desc.kind == 0 and transform is not None


class FusedScorer:
    """Caches the ScoreModel built from (transform, kernel, supports, weights) and rebuilds it when any of them
    changes.  The cache holds strong references to the two tensors it was built from and compares by identity plus
    in-place version, so a freed-and-reallocated tensor at the same address can never alias the cached model; edits
    that bypass the version counter (`t.data[...] = ...`, `set_`) must be followed by `invalidate()` — the checkers
    call it from train / fit_poly / to / filter_support_points_.

    Ownership (round 5: an explicit count instead of `sys.getrefcount`).  When the checker's state changes but the model's
    structure (transform, kernel, class count, feature width, device) does not, the cached model is REFILLED in place
    (`ScoreModel.update`: same storage, FK tables, per-stream scratch) - unless somebody holds a lease on it
    (`ScoreModel.acquire()` / `release()`: a ShardedAdamRun while it iterates, an optimiser's constraint terms), in which
    case the holder keeps the rows it started with and the cache builds a new model.  `model()` hands out the cache's own
    model: a caller that keeps it across a later train / fit_poly and needs it unchanged takes a lease.  (A multi-class score's
    backward pass re-sweeps the model: it checks `ScoreModel.revision` and raises if the rows were refilled after its forward.)

    The per-call check compares the transform by IDENTITY (a robot's bound `fkine`): a robot whose FK parameters (link lengths,
    DH table, URDF tree) are edited in place after the checker has scored keeps the same bound method, so such an edit must
    be followed by `invalidate()` - like the `.data` edits above.  The robots of diffco_amd.model / urdf do not change after
    construction."""

    def __init__(self):
        self._key, self._model, self._sup, self._w = None, None, None, None
        self._struct, self._retired = None, None
        self._fast = None   # (transform, kernel_func, device string, spec) of the cached model: the per-call check

    def model(self, transform, kernel_func, support_feat, weights, device=None):
        spec = kernel_spec(kernel_func)
        # the per-call path (an optimiser asks thousands of times between two state changes): same objects, same in-place
        # versions, same kernel parameters -> the cached model, without rebuilding the description key (bytes of a 5 KB struct)
        if (self._model is not None and self._sup is support_feat and self._w is weights and self._fast is not None
                and self._fast[0] is transform and self._fast[1] is kernel_func and self._fast[3] == spec
                and self._fast[2] == (device if device is None else str(device))
                and self._key[2] == support_feat._version and self._key[3] == weights._version
                and self._key[4] == tuple(support_feat.shape) and self._key[5] == tuple(weights.shape)):
            return self._model
        desc = transform_desc(transform)
        key = (None if desc is None else desc.key(), spec, support_feat._version, weights._version,
               tuple(support_feat.shape), tuple(weights.shape), str(device))
        if self._model is None or self._sup is not support_feat or self._w is not weights or key != self._key:
            old = self._model if self._model is not None else self._retired
            width = int(support_feat.reshape(len(support_feat), -1).shape[1]) if len(support_feat) else -1
            struct = (key[0], spec, int(weights.reshape(len(weights), -1).shape[1]), width, str(device))
            # refilled in place only while nobody holds a lease on the model (see the class docstring), and only for the same
            # structure INCLUDING the feature width (a refit on different-width features must rebuild, not raise)
            same_shape = (old is not None and self._struct == struct and width == old.D
                          and len(support_feat) <= 4 * max(old.capacity, 1) and old.leases == 0)
            if same_shape:
                # the same transform / kernel / class count with new supports or weights (train, fit_poly, update): the
                # model is refilled in place (dcx_model_update) - its storage, FK tables and per-stream scratch stay
                self._model = old.update(support_feat, weights)
            else:
                # (room to grow: an active-learning loop adds supports round by round)
                self._model = _ops.ScoreModel(desc, spec[0], spec[1], spec[2], support_feat, weights, device=device,
                                              capacity=len(support_feat) + len(support_feat) // 4)
            self._struct = (key[0], spec, self._model.C, self._model.D, str(device))
            self._retired = None
            self._key, self._sup, self._w = key, support_feat, weights
        self._fast = (transform, kernel_func, device if device is None else str(device), spec)
        return self._model

    def score(self, transform, kernel_func, support_feat, weights, point):
        """[B, C] = K(T(point), supports) @ weights, differentiable w.r.t. `point`."""
        dev = point.device if point.device.type == "cuda" else (
            support_feat.device if support_feat.device.type == "cuda" else None)
        m = self.model(transform, kernel_func, support_feat, weights, dev)
        if _foreign(m, transform):
            # foreign transform: run it in torch (its own autograd), fuse everything after it
            feats = transform(point)
            return m.score(feats.reshape(len(feats), -1))
        return m.score(point.reshape(-1, m.dof))

    def invalidate(self):
        # the state changed behind the version counters: the next call refills the model (kept aside) instead of rebuilding it
        if self._model is not None:
            self._retired = self._model
        self._key, self._model, self._sup, self._w, self._fast = None, None, None, None, None


# ---- the motion calls' source ------------------------------------------------------------------------------------------------
class MotionSource(NamedTuple):
    """what a checker's motion calls run on: the checker itself (`owner.last_route` says which route the last call took:
    "fused" or "host"), its FusedScorer and the state the scorer's model is built from.  A checker builds one per call."""
    owner: object
    fused: object
    transform: object
    kernel_func: object
    support_feat: object
    weights: object

    def wrap_mask(self, wrap, dof):
        """_ops.wrap_mask; True: the mask of the robot that owns `transform`"""
        return _ops.wrap_mask(wrap, dof, self.transform)

    def model(self, device=None):
        """the ScoreModel, on `device` where that is a GPU, else where the supports live"""
        sf = self.support_feat
        dev = device if device is not None and device.type == "cuda" else (sf.device if sf.device.type == "cuda" else None)
        return self.fused.model(self.transform, self.kernel_func, sf, self.weights, dev)

    def score(self, p):
        """the host route's score callable (keeps autograd)"""
        return self.fused.score(self.transform, self.kernel_func, self.support_feat, self.weights, p)

    def score_detached(self, p):
        return self.score(p).detach()

    def route(self, name, qa, qb, res, max_step, wrap):
        """what every motion call starts with: (qa, qb, mask, model, host).  host is None on the fused route (no transform, or a
        diffco_amd robot's fkine: one call into the library) and the endpoints as float32 on the model's device on the host
        route (a foreign callable: the host composition over `score`).  The ValueErrors come before anything touches the
        device."""
        if (res is None) == (max_step is None):
            raise ValueError(f"{name} takes exactly one of res and max_step")
        qa, qb = torch.as_tensor(qa), torch.as_tensor(qb)
        mask = self.wrap_mask(wrap, qa.shape[-1])
        m = self.model(qa.device)
        if _foreign(m, self.transform):
            self.owner.last_route = "host"
            return qa, qb, mask, m, (qa.to(device=m.dev, dtype=torch.float32), qb.to(device=m.dev, dtype=torch.float32))
        self.owner.last_route = "fused"
        return qa, qb, mask, m, None


def _raise_over(name, over, hint="pass a larger max_samples or max_step"):
    """raises ValueError for the edges flagged in `over` [E] bool: those over max_samples (a read-back)"""
    if bool(over.any()):
        bad = over.nonzero().reshape(-1)[:8].tolist()
        raise ValueError(f"{name}: edges {bad} need more than max_samples samples ({hint})")


# ---- the host compositions' samples ------------------------------------------------------------------------------------------
def _wrap_points(pts, mask):
    """the masked coordinates of the points brought back to [-pi, pi) (utils.wrap2pi; slope 1 under autograd)"""
    from .utils import wrap2pi
    if not mask:
        return pts
    on = torch.tensor([bool((mask >> j) & 1) for j in range(pts.shape[-1])], device=pts.device)
    return torch.where(on, wrap2pi(pts), pts)


def _edge_counts(qa, qb, res, max_step, wrap, open_end=False):
    """(d [E, dof], L [E], n [E]) of the edges qa[e] -> qb[e]: the delta (`wrap`, a bitmask: along the shortest arc of the
    masked coordinates), its length (None under the res rule) and the sample count of the rule (open_end: without the target)"""
    d = _ops.wrapped_delta(qa, qb, wrap)
    if res is not None:
        return d, None, torch.full((len(qa),), int(res), dtype=torch.int64, device=qa.device)
    L = d.norm(dim=-1)
    steps = torch.ceil(L / max_step).to(torch.int64)
    return d, L, steps if open_end else steps + 1


class _SamplePlan(NamedTuple):
    """which samples a host composition materialises: the edges' (d, L, n) of _edge_counts, ok [E] the edges within the limit,
    n_ok [E] their counts (0 for the others), and per sample its edge [N] and index k [N]; edge e's samples start at offs[e]"""
    d: object
    L: object
    n: object
    ok: object
    n_ok: object
    edge: object
    offs: object
    k: object


def _sample_plan(qa, qb, res, max_step, max_samples, wrap, open_end=False):
    """the one index plan of the host compositions: the rule's counts, the limit (max_samples; None: `res`, or
    MOTION_MAX_SAMPLES under max_step), and the flat (edge, k) list of the edges within it"""
    d, L, n = _edge_counts(qa, qb, res, max_step, wrap, open_end)
    limit = int(res) if (max_samples is None and res is not None) else (
        _ops.MOTION_MAX_SAMPLES if max_samples is None else int(max_samples))
    ok = n <= limit
    n_ok = torch.where(ok, n, torch.zeros_like(n))
    edge = torch.repeat_interleave(torch.arange(len(qa), device=qa.device), n_ok)
    offs = torch.cumsum(n_ok, 0) - n_ok
    k = torch.arange(len(edge), device=qa.device) - offs[edge]
    return _SamplePlan(d, L, n, ok, n_ok, edge, offs, k)


def _res_points(qa, d, edge, k, res, wrap):
    """the res rule's points (Perceptron.line_predict's; utils.anglin's on the masked coordinates)"""
    return _wrap_points(qa[edge] + d[edge] * (k.to(qa.dtype) / int(res))[:, None], wrap)


def _check_points(qa, qb, d, L, n, edge, k, res, max_step, wrap):
    """sample k[i] of the edge edge[i] in the check form: line_predict's / dense_path's arithmetic, what dcx_check_motions
    walks - the step vector d * (max_step / L) scaled by k, and qb itself at the last sample.  (d, L, n): _edge_counts."""
    if res is not None:
        return _res_points(qa, d, edge, k, res, wrap)
    frac = max_step / L
    pts = _wrap_points(qa[edge] + k.to(qa.dtype)[:, None] * (d[edge] * frac[edge][:, None]), wrap)
    last = k == n[edge] - 1
    return torch.where(last[:, None], qb[edge], pts)


def _grad_points(qa, qb, d, L, n, edge, k, res, max_step, wrap, open_end):
    """sample k[i] of the edge edge[i] in the differentiable form, what dcx_motion_cost / dcx_motion_worst walk: the unit
    direction u = d / L scaled by k * max_step (it rounds differently from the check form), and qb at the last sample of a
    closed edge.  Differentiable with respect to qa and qb."""
    if res is not None:
        return _res_points(qa, d, edge, k, res, wrap)
    # u = d / L differentiably (the sample counts are constants); L = 0 edges have only the target sample
    Ld = L[:, None]
    u = d / torch.where(Ld > 0, Ld, torch.ones_like(Ld))
    pts = _wrap_points(qa[edge] + (k.to(qa.dtype) * max_step)[:, None] * u[edge], wrap)
    if not open_end:
        last = k == n[edge] - 1
        pts = torch.where(last[:, None], qb[edge], pts)
    return pts


def _motion_samples(qa, qb, res, max_step, max_samples, wrap):
    """every checked edge's points, materialised in the check form: (pts [N, dof], the plan)"""
    p = _sample_plan(qa, qb, res, max_step, max_samples, wrap)
    return _check_points(qa, qb, p.d, p.L, p.n, p.edge, p.k, res, max_step, wrap), p


# ---- batched motion checks ---------------------------------------------------------------------------------------------------
def host_motions(score_fn, qa, qb, res=None, max_step=None, margin=0., max_samples=None, wrap=0):
    """the composition a caller would write without dcx_check_motions: every edge's points (line_predict's / dense_path's
    arithmetic; `wrap`, a bitmask: utils.anglin's on the masked coordinates) materialised, ONE score launch over all of them,
    the first hit per edge.  Same answers, (first_hit, n_samples)."""
    qa, qb = qa.reshape(len(qa), -1), qb.reshape(len(qb), -1)
    E, dev = len(qa), qa.device
    pts, p = _motion_samples(qa, qb, res, max_step, max_samples, wrap)
    n, ok, edge, k = p.n, p.ok, p.edge, p.k
    first = torch.full((E,), -1, dtype=torch.int64, device=dev)
    if len(pts):
        s = score_fn(pts).reshape(len(pts), -1)
        mg = torch.as_tensor(margin, dtype=s.dtype, device=s.device).reshape(-1)
        hit = (s - mg > 0).any(dim=-1)
        big = torch.iinfo(torch.int64).max
        cand = torch.where(hit, k, torch.full_like(k, big))
        first = torch.full((E,), big, dtype=torch.int64, device=dev).scatter_reduce(0, edge, cand, reduce="amin")
        first = torch.where(first == big, torch.full_like(first, -1), first)
    first = torch.where(ok, first, torch.full_like(first, -2))
    return first.to(torch.int32), n.clamp(max=2 ** 31 - 1).to(torch.int32)


def check_motions(src, qa, qb, res=None, max_step=None, margin=0., max_samples=None, wrap=None):
    """(first_hit, n_samples) of the motions qa[e] -> qb[e] on the source's model: one dcx_check_motions call on the fused
    route, the host composition on the host route (MotionSource.route; the points scored in one launch).  `wrap`
    (_ops.wrap_mask; True: the mask of the robot that owns the transform): those coordinates run along their shortest arc."""
    qa, qb, mask, m, host = src.route("check_motions", qa, qb, res, max_step, wrap)
    if host is not None:
        return host_motions(src.score_detached, *host, res, max_step, margin, max_samples, mask)
    return m.check_motions(qa, qb, res=res, max_step=max_step, margin=margin, max_samples=max_samples, wrap=mask)


def _motion_model(src, device=None, margin=0.):
    """(ScoreModel, margin) where check_motions above takes the fused route on this source, else None (a foreign transform:
    the host composition).  What a planner needs to enqueue the fused motion checks itself (rrt.rrt_connect)."""
    m = src.model(device)
    return None if _foreign(m, src.transform) else (m, margin)


def motion_answer(first, return_first):
    """the facades' answer: collides [E] bool (+ first_hit); raises for edges over max_samples (a read-back)"""
    _raise_over("check_motions", first == -2)
    hit = first >= 0
    return (hit, first) if return_first else hit


# ---- hybrid motion checks ----------------------------------------------------------------------------------------------------
def host_motion_band(score_fn, qa, qb, lo, hi, res=None, max_step=None, max_samples=None, wrap=0, want_q=True):
    """the composition a caller would write without dcx_motion_band: host_motions' samples materialised, ONE score launch over
    all of them, the two thresholds, a segment reduction per edge and a `nonzero` for the list.  ScoreModel.motion_band's
    outputs in its order: (verdict, first_hit, n_uncertain, unc_edge, unc_sample, unc_q)."""
    qa, qb = qa.reshape(len(qa), -1), qb.reshape(len(qb), -1)
    E, dev = len(qa), qa.device
    pts, p = _motion_samples(qa, qb, res, max_step, max_samples, wrap)
    ok, edge, k = p.ok, p.edge, p.k
    big = torch.iinfo(torch.int64).max
    first = torch.full((E,), -1, dtype=torch.int64, device=dev)
    n_unc = torch.zeros(E, dtype=torch.int64, device=dev)
    listed = torch.zeros(len(pts), dtype=torch.bool, device=dev)
    if len(pts):
        s = score_fn(pts).reshape(len(pts), -1)
        lo_t = torch.as_tensor(lo, dtype=s.dtype, device=s.device).reshape(-1)
        hi_t = torch.as_tensor(hi, dtype=s.dtype, device=s.device).reshape(-1)
        hit = (s - hi_t > 0).any(dim=-1)
        clear = (s - lo_t <= 0).all(dim=-1)           # (a NaN score is neither: the sample is uncertain)
        unc = ~hit & ~clear
        cand = torch.where(hit, k, torch.full_like(k, big))
        first = torch.full((E,), big, dtype=torch.int64, device=dev).scatter_reduce(0, edge, cand, reduce="amin")
        first = torch.where(first == big, torch.full_like(first, -1), first)
        n_unc = n_unc.index_add(0, edge, unc.to(torch.int64))
        n_unc = torch.where(first >= 0, torch.zeros_like(n_unc), n_unc)   # an edge with a sure hit is decided
        listed = unc & (first[edge] < 0)
    verdict = torch.where(first >= 0, torch.ones_like(first), torch.where(n_unc > 0, torch.full_like(first, 2), torch.zeros_like(first)))
    verdict = torch.where(ok, verdict, torch.full_like(verdict, -2))
    first = torch.where(ok, first, torch.full_like(first, -2))
    at = listed.nonzero().reshape(-1)                  # ascending flat index: (edge, sample) order
    i32 = torch.int32
    return (verdict.to(i32), first.to(i32), n_unc.to(i32), edge[at].to(i32), k[at].to(i32), pts[at] if want_q else None)


def motion_band(src, qa, qb, lo, hi, res=None, max_step=None, max_samples=None, wrap=None, want_q=True):
    """(verdict, first_hit, n_uncertain, unc_edge, unc_sample, unc_q) of the motions qa[e] -> qb[e] on the source's model:
    dcx_motion_band on the fused route, the host composition on the host route (MotionSource.route).  Both read the list's
    length back.  Raises ValueError where lo > hi.  `wrap`: as check_motions."""
    qa, qb, mask, m, host = src.route("motion_band", qa, qb, res, max_step, wrap)
    kw = dict(res=res, max_step=max_step, max_samples=max_samples, wrap=mask, want_q=want_q)
    if host is not None:
        lo_c, hi_c = list(m.margins(lo)), list(m.margins(hi))
        if any(l > h for l, h in zip(lo_c, hi_c)):
            raise ValueError("motion_band: lo > hi")
        return host_motion_band(src.score_detached, *host, lo_c, hi_c, **kw)
    return m.motion_band(qa, qb, lo, hi, **kw)


def score_band(src, q, lo, hi):
    """(label [B] int32, unc_idx [U] int64) of the configurations q: motion_band(q, q, res=1), one sample per "edge", on
    either route"""
    verdict, _, _, unc_edge, _, _ = motion_band(src, q, q, lo, hi, res=1, want_q=False)
    return verdict, unc_edge.to(torch.int64)


# ---- differentiable motion costs ---------------------------------------------------------------------------------------------
def host_motion_cost(score_fn, qa, qb, res=None, max_step=None, margin=0., weight=1., open_end=False, max_samples=None, wrap=0):
    """the composition a caller would write without dcx_motion_cost: every edge's points materialised differentiably
    (check_motions' arithmetic; `wrap`, a bitmask: the wrapped delta and wrapped points, both of slope 1), scored through
    autograd, the hinge reduced per edge with index_add.  [E] costs, differentiable with respect to qa and qb; NaN for an
    edge over max_samples."""
    qa, qb = qa.reshape(len(qa), -1), qb.reshape(len(qb), -1)
    E, dev = len(qa), qa.device
    p = _sample_plan(qa, qb, res, max_step, max_samples, wrap, open_end)
    ok, edge = p.ok, p.edge
    pts = _grad_points(qa, qb, p.d, p.L, p.n, edge, p.k, res, max_step, wrap, open_end)
    cost = torch.zeros(E, dtype=qa.dtype, device=dev)
    if len(pts):
        s = score_fn(pts).reshape(len(pts), -1)
        mg = torch.as_tensor(margin, dtype=s.dtype, device=s.device).reshape(-1)
        h = (s - mg).clamp(min=0).sum(dim=-1)
        cost = cost.index_add(0, edge, h.to(cost.dtype))
    cost = weight * cost
    return torch.where(ok, cost, torch.full_like(cost, float("nan")))


def motion_cost(src, qa, qb, res=None, max_step=None, margin=0., weight=1., open_end=False, max_samples=None, wrap=None):
    """[E] differentiable motion costs on the source's model: one dcx_motion_cost call on the fused route, the host
    composition on the host route (MotionSource.route).  Raises ValueError for edges over max_samples (a read-back).
    `wrap`: as check_motions."""
    qa, qb, mask, m, host = src.route("motion_cost", qa, qb, res, max_step, wrap)
    kw = dict(res=res, max_step=max_step, margin=margin, weight=weight, open_end=open_end, max_samples=max_samples, wrap=mask)
    if host is not None:
        cost = host_motion_cost(src.score, *host, **kw).to(device=qa.device, dtype=qa.dtype)
    else:
        cost = m.motion_cost(qa, qb, **kw)
    _raise_over("motion_cost", torch.isnan(cost), "or hold non-finite values")
    return cost


def path_cost(src, paths, max_step, margin=0., weight=1., max_samples=None, wrap=None):
    """[T] differentiable collision costs of paths [T, W, dof] (ScoreModel.path_cost's composition over either route)"""
    paths = torch.as_tensor(paths)
    dof = paths.shape[-1]
    kw = dict(max_step=max_step, margin=margin, weight=weight, max_samples=max_samples, wrap=src.wrap_mask(wrap, dof))
    return _ops.compose_path_cost(lambda a, b, open_end: motion_cost(src, a, b, open_end=open_end, **kw), paths, dof)


# ---- worst-sample motion queries ---------------------------------------------------------------------------------------------
def _first_where(at, dim):
    """the smallest index along `dim` where `at` holds (argmax of a tie is unspecified in torch: a min over masked indices)"""
    n = at.shape[dim]
    shape = [1] * at.dim()
    shape[dim] = n
    ar = torch.arange(n, device=at.device).reshape(shape)
    return torch.where(at, ar, torch.full_like(ar, n)).amin(dim=dim)


def host_motion_worst(score_fn, qa, qb, res=None, max_step=None, margin=0., max_samples=None, wrap=0):
    """the composition a caller would write without dcx_motion_worst: every edge's points materialised differentiably
    (check_motions' closed sample set; `wrap`, a bitmask: the wrapped delta and wrapped points), scored through autograd, and a
    segment arg-max: (worst [E], idx [E] int32, cls [E] int32, n_samples [E] int32).  worst[e] = max over the edge's samples
    of max_c (score_c - margin_c) (a NaN score counts as -inf), the smallest sample that attains it, the smallest class that
    attains it there; differentiable with respect to qa and qb through that sample.  An edge over max_samples: NaN / -2 / -1."""
    qa, qb = qa.reshape(len(qa), -1), qb.reshape(len(qb), -1)
    E, dev = len(qa), qa.device
    p = _sample_plan(qa, qb, res, max_step, max_samples, wrap)
    n, ok, n_ok, edge, offs, k = p.n, p.ok, p.n_ok, p.edge, p.offs, p.k
    pts = _grad_points(qa, qb, p.d, p.L, n, edge, k, res, max_step, wrap, False)
    nan = float("nan")
    worst = torch.full((E,), nan, dtype=qa.dtype, device=dev)
    idx = torch.full((E,), -2, dtype=torch.int64, device=dev)
    cls = torch.full((E,), -1, dtype=torch.int64, device=dev)
    if len(pts):
        s = score_fn(pts).reshape(len(pts), -1)
        mg = torch.as_tensor(margin, dtype=s.dtype, device=s.device).reshape(-1)
        v = s - mg
        vd = torch.nan_to_num(v.detach(), nan=-float("inf"), posinf=float("inf"), neginf=-float("inf"))
        vk, _ = vd.max(dim=-1)
        ck = _first_where(vd == vk[:, None], 1)
        top = torch.full((E,), -float("inf"), dtype=vk.dtype, device=dev).scatter_reduce(0, edge, vk, reduce="amax", include_self=True)
        big = torch.iinfo(torch.int64).max
        first = torch.full((E,), big, dtype=torch.int64, device=dev).scatter_reduce(
            0, edge, torch.where(vk == top[edge], k, torch.full_like(k, big)), reduce="amin", include_self=True)
        has = ok & (n_ok > 0)
        flat = (offs + torch.where(has, first, torch.zeros_like(first))).clamp(max=len(pts) - 1)
        cbest = ck[flat]
        picked = v[flat, cbest]                      # differentiable: the worst sample's winning class score
        picked = torch.where(torch.isnan(picked.detach()), torch.full_like(picked, -float("inf")), picked)
        worst = torch.where(has, picked.to(qa.dtype), worst)
        idx = torch.where(has, first, idx)
        cls = torch.where(has, cbest, cls)
    return worst, idx.to(torch.int32), cls.to(torch.int32), n.clamp(max=2 ** 31 - 1).to(torch.int32)


def motion_worst(src, qa, qb, res=None, max_step=None, margin=0., max_samples=None, wrap=None):
    """(worst [E], idx [E], cls [E]) of the motions qa[e] -> qb[e] on the source's model: one dcx_motion_worst call on the
    fused route, the host composition on the host route (MotionSource.route).  worst is differentiable with respect to qa
    and qb.  Raises ValueError for edges over max_samples (a read-back).  `wrap`: as check_motions."""
    qa, qb, mask, m, host = src.route("motion_worst", qa, qb, res, max_step, wrap)
    kw = dict(res=res, max_step=max_step, margin=margin, max_samples=max_samples, wrap=mask)
    if host is not None:
        worst, idx, cls, _ = host_motion_worst(src.score, *host, **kw)
        worst = worst.to(device=qa.device, dtype=qa.dtype)
    else:
        worst, idx, cls = m.motion_worst(qa, qb, **kw)
    _raise_over("motion_worst", idx == -2)
    return worst, idx, cls


def path_worst(src, paths, max_step, margin=0., max_samples=None, wrap=None):
    """(worst [T], segment [T], sample [T]) of paths [T, W, dof] (ScoreModel.path_worst's composition over either route)"""
    paths = torch.as_tensor(paths)
    dof = paths.shape[-1]
    kw = dict(max_step=max_step, margin=margin, max_samples=max_samples, wrap=src.wrap_mask(wrap, dof))
    return _ops.compose_path_worst(lambda a, b: motion_worst(src, a, b, **kw), paths, dof)

