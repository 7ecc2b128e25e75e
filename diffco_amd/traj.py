"""Fused, batched-restart Adam trajectory optimiser (BASELINE config #5).

Same inputs, option keys and result record as `optim.adam_traj_optimize` (reference diffco/optim.py:13-163), but
all NUM_RE_TRIALS restarts advance together on the GPU inside native code (`dcx_traj_adam_run_mc`): one persistent
launch per <= 192 iterations when a path is one tile of the sweep, else per iteration the fused score + hinge-gradient
sweep over every waypoint of every restart and the fused Adam step (FK-coupled path terms, J^T, Adam update,
best-so-far bookkeeping).  No host synchronisation inside the loop (the reference syncs every iteration,
optim.py:107-118).  `dist_est` may have several outputs (a MultiDiffCo's rbf_score) with options['safety_margin'] one
number or one per class - the reference's `clamp(dist_est(p) - safety_margin, min=0).sum()` (optim.py:88-89 as
scripts/2d_trajopt.py:94-102 and scripts/active.py:28-121 call it).

The restarts are initialised exactly like the reference's sequential trials (trial 0: init_solution or the
straight line, later trials: torch.rand in joint limits, same seed, same order), and the returned record follows
the reference's policy — the first trial, in order, that produced a valid path wins; otherwise the lowest loss
seen anywhere — so a reference run and this one answer the same question.  Arithmetic is fp32 on the device (the
reference optimises in fp64 on the host).
"""
import ctypes as C
import time

import torch

from . import _lib, _ops
from .optim import (COLLISION_WEIGHT, DIF_WEIGHT, JOINT_LIMIT_WEIGHT, MAX_MOVE_WEIGHT, STATIONARY_GRAD_NORM,
                    VALID_CONSTRAINT_LOSS, _np, _PathProblem)


def _resolve_model(dist_est, device=None):
    """ScoreModel behind `dist_est`: a ScoreModel, or a bound score method of a diffco_amd checker.  A checker whose transform is
    not a diffco_amd robot's `fkine` cannot be fused (its model scores FEATURES; only `FusedScorer.score` runs the foreign
    transform in front of it): TypeError, and the callers keep their host route (the escape loop used to score the
    raw configurations of such a checker)."""
    if isinstance(dist_est, _ops.ScoreModel):
        return dist_est
    owner, name = getattr(dist_est, "__self__", None), getattr(dist_est, "__name__", "")
    if owner is None:
        raise TypeError("fused_adam_traj_optimize needs a ScoreModel or a bound poly_score / rbf_score / score method "
                        "of a diffco_amd checker (an arbitrary callable cannot be fused)")
    from .deprecated import DiffCo as OldDiffCo
    from .kernel_perceptrons import DiffCo as NewDiffCo
    tf, model = None, None
    if isinstance(owner, NewDiffCo):
        tf = owner.transform
        if name == "poly_score":
            model = owner._poly_fused.model(tf, owner.rbf_kernel, owner.support_transformed, owner.rbf_nodes, device)
        elif name in ("score", "score_original"):
            model = owner._score_fused.model(tf, owner.kernel_func, owner.support_transformed, owner.gains, device)
    elif isinstance(owner, OldDiffCo):
        if name in ("rbf_score", "poly_score"):
            tf = owner.fkine
            feats = owner.support_fkine if tf is not None else owner.support_points
            model = owner._rbf_fused.model(tf, owner.rbf_kernel, feats, owner.rbf_nodes, device)
        elif name in ("score", "score_original"):
            tf, pk, feats = owner._score_state()
            model = owner._score_fused.model(tf, pk, feats, owner.gains, device)
    if model is None:
        raise TypeError(f"cannot fuse {dist_est!r}")
    if tf is not None and model.desc.kind == 0:
        raise TypeError(f"cannot fuse {dist_est!r}: its transform is not the fkine of a diffco_amd robot")
    return model


def select_trial(best_valid_obj, lowest_loss, lowest_obj, steps, n_waypoints):
    """The reference's selection policy over per-trial summaries (1-D tensors over trials, in trial order):
    the first trial that found a valid path wins (optim.py:129-131, sequential trials stop there), otherwise the
    lowest loss seen in any trial (optim.py:134-141).  Returns (trial, found, cost, cnt_check) with cnt_check =
    what the sequential reference would have evaluated."""
    valid = torch.isfinite(best_valid_obj)
    if bool(valid.any()):
        t = int(torch.nonzero(valid)[0])
        return t, True, float(best_valid_obj[t]), int(steps[:t + 1].sum().item()) * n_waypoints
    t = int(torch.argmin(lowest_loss))
    return t, False, float(lowest_obj[t]), int(steps.sum().item()) * n_waypoints


class ShardedAdamRun:
    """R_total restarts of one trajectory problem advanced together by the fused Adam step, sharded over the ranks of
    a torch.distributed group (one process per GPU; `group=None` and no initialised process group = one rank).

    Rank r owns the contiguous restarts `shard_bounds(R_total, r, world)` and runs them with `dcx_traj_adam_run`
    (one persistent launch per <= 192 iterations when a path fits one tile); nothing is exchanged while iterating —
    restarts are independent — and `finish()` gathers only the per-restart summaries (4 floats each) plus the candidate
    paths.  `fused_adam_traj_optimize` and bench.py's config #5 are both built on this class."""

    def __init__(self, model, limits, init_paths, lr, safety_margin, max_speed, valid_tol=None, grad_tol=None,
                 group=None, sharded=None):
        import torch.distributed as dist
        from .sharded import shard_bounds
        self.lib = _lib.require_gpu()
        self.model, self.group = model.acquire(), group   # a lease: the checker's cache must not refill these rows under the run
        self.n_total = len(init_paths)
        self.sharded = (group is not None or bool(sharded)) and dist.is_initialized()
        self.rank, self.world = (dist.get_rank(group), dist.get_world_size(group)) if self.sharded else (0, 1)
        lo, hi = shard_bounds(self.n_total, self.rank, self.world)
        self.lo, self.hi, self.R = lo, hi, hi - lo
        dev = model.dev
        f32 = dict(device=dev, dtype=torch.float32)
        W, dof = init_paths.shape[1], init_paths.shape[2]
        self.W, self.dof = W, dof
        path = init_paths[lo:hi].to(**f32).contiguous().clone() if self.R else torch.empty((0, W, dof), **f32)
        R, inf = self.R, float('inf')
        self.margin = model.margins(safety_margin)    # one per class (a number serves all of them)
        self.t = dict(path=path, adam_m=torch.zeros_like(path), adam_v=torch.zeros_like(path),
                      limits=limits.to(**f32).contiguous(), col_score=torch.empty((R * W * model.C,), **f32),
                      col_grad=torch.empty((R * W, dof), **f32), stats=torch.zeros((R, 8), **f32),
                      lowest_loss=torch.full((R,), inf, **f32), lowest_obj=torch.full((R,), inf, **f32),
                      lowest_path=path.clone(), best_valid_obj=torch.full((R,), inf, **f32),
                      best_valid_path=path.clone(), done=torch.zeros((R,), device=dev, dtype=torch.int32),
                      steps=torch.zeros((R,), device=dev, dtype=torch.int32))
        self.st = _lib.TrajState(R, W, *(C.c_void_p(v.data_ptr() if v.numel() else 0) for v in self.t.values()))
        self.opt = _lib.TrajOpts(lr, 0.9, 0.999, 1e-8, DIF_WEIGHT, COLLISION_WEIGHT, MAX_MOVE_WEIGHT, JOINT_LIMIT_WEIGHT,
                                 float(self.margin[0]), float(max_speed),
                                 VALID_CONSTRAINT_LOSS if valid_tol is None else float(valid_tol),
                                 STATIONARY_GRAD_NORM if grad_tol is None else float(grad_tol))
        self.it = 0

    def close(self):
        """give the model's lease back (idempotent; also done when the run is garbage-collected)"""
        m, self._released = self.model, getattr(self, "_released", False) or not hasattr(self, "model")
        if not self._released:
            self._released = True
            m.release()

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001
            pass

    def run(self, n_iters):
        """enqueue n_iters more iterations on torch's current stream (no host synchronisation)"""
        if self.R and n_iters > 0:
            dev = self.model.dev
            with torch.cuda.device(dev):
                stream = self.model._st()
                _lib.check(self.lib.dcx_traj_adam_run_mc(self.model._h, C.byref(self.st), C.byref(self.opt), self.margin,
                                                         self.it + 1, int(n_iters), stream))
        self.it += n_iters

    def all_done(self):
        return self.R == 0 or bool(self.t['done'].all())

    def finish(self):
        """(summaries [R_total, 4] on the host: best_valid_obj, lowest_loss, lowest_obj, steps; best_valid_path,
        lowest_path [R_total, W, dof] on the device) — identical on every rank"""
        from .sharded import all_gather_rows
        t = self.t
        if self.R and bool((t['stats'][:, 7] < 0).any()):
            # the cluster form of the persistent kernel (csrc/traj_fused.h) waited ~1 s for a peer workgroup's rows
            raise _lib.DcxError("dcx_traj_adam_run: a workgroup exchange gave up (stats[:, 7] == -1); the paths were left "
                                "as the last launch found them.  DCX_TRAJ_YS=1 runs one workgroup per path")
        summ = torch.stack([t['best_valid_obj'], t['lowest_loss'], t['lowest_obj'], t['steps'].float()], dim=1)
        bvp, lop = t['best_valid_path'], t['lowest_path']
        if self.sharded and self.world > 1:
            summ = all_gather_rows(summ, self.n_total, self.group)
            bvp = all_gather_rows(bvp, self.n_total, self.group)
            lop = all_gather_rows(lop, self.n_total, self.group)
        return summ.cpu(), bvp, lop


class DenseAdamRun:
    """R restarts of one trajectory problem advanced together by the dense-check Adam loop (`dcx_traj_dense_run`): the
    collision hinge is charged on the points of utils.dense_path(p, max_step) - along the segments, not at the waypoints only -
    so a path cannot pass through an obstacle thinner than a stride between two waypoints.  ShardedAdamRun's shape (buffers,
    lease, run(n), all_done(), finish()) on one device; per iteration the library's motion-cost launches and one step launch,
    nothing read back.

    normalize: the collision term is the MEAN hinge times W (Weighted's) instead of the sum (path_cost's).  move: [W] bools, a
    waypoint with False keeps its place (None: the endpoints are fixed).  wrap: the SAMPLING mask (the motion calls' `wrap`);
    rewrap: the coordinates wrapped to [-pi, pi) after every step.  stop_tol > 0: a restart whose constraint value is <= stop_tol
    takes that step and stops.  history=True: run(n) keeps the paths after each of its steps in self.history ([n, R, W, dof]
    per call).  max_samples: the most samples one segment may need; a restart with a longer segment is frozen where it stands
    (`over_bound()`); None: twice the longest initial segment's count plus 8."""

    def __init__(self, model, limits, init_paths, lr, safety_margin, max_step, max_speed=None, max_samples=None, wrap=None,
                 rewrap=None, normalize=False, stop_tol=0., move=None, history=False, weights=None, betas=(0.9, 0.999), eps=1e-8,
                 valid_tol=None, grad_tol=None):
        self.lib = _lib.require_gpu()
        self.model = model.acquire()   # a lease: the checker's cache must not refill these rows under the run
        dev = model.dev
        f32 = dict(device=dev, dtype=torch.float32)
        R, W, dof = init_paths.shape
        self.R, self.W, self.dof = R, W, dof
        path = init_paths.to(**f32).contiguous().clone()
        inf = float('inf')
        mask, remask = _ops.wrap_mask(wrap, dof), _ops.wrap_mask(rewrap, dof)
        if max_samples is None:
            bound = _ops.motion_bound(path[:, :-1].reshape(-1, dof), path[:, 1:].reshape(-1, dof), max_step, wrap=mask) if R else 1
            max_samples = min(_ops.MOTION_MAX_SAMPLES, 2 * bound + 8)
        self.max_samples = int(max_samples)
        self.margin = torch.tensor(list(model.margins(safety_margin)), dtype=torch.float32).to(dev)   # [C] device floats
        self.t = dict(path=path, adam_m=torch.zeros_like(path), adam_v=torch.zeros_like(path),
                      limits=limits.to(**f32).contiguous(), stats=torch.zeros((R, 8), **f32),
                      lowest_loss=torch.full((R,), inf, **f32), lowest_obj=torch.full((R,), inf, **f32),
                      lowest_path=path.clone(), best_valid_obj=torch.full((R,), inf, **f32),
                      best_valid_path=path.clone(), done=torch.zeros((R,), device=dev, dtype=torch.int32),
                      steps=torch.zeros((R,), device=dev, dtype=torch.int32))
        self.n_checks = torch.zeros((R,), device=dev, dtype=torch.int64)
        self.move = None if move is None else torch.as_tensor(move).reshape(-1).to(device=dev, dtype=torch.bool).to(torch.uint8).contiguous()
        if self.move is not None and len(self.move) != W:
            raise ValueError(f"move: expected one flag per waypoint ({W}), got {len(self.move)}")
        ptr = lambda v: C.c_void_p(v.data_ptr() if v is not None and v.numel() else 0)
        t = self.t
        self.st = _lib.TrajState(R, W, ptr(t['path']), ptr(t['adam_m']), ptr(t['adam_v']), ptr(t['limits']), None, None,
                                 ptr(t['stats']), ptr(t['lowest_loss']), ptr(t['lowest_obj']), ptr(t['lowest_path']),
                                 ptr(t['best_valid_obj']), ptr(t['best_valid_path']), ptr(t['done']), ptr(t['steps']))
        w = (DIF_WEIGHT, COLLISION_WEIGHT, MAX_MOVE_WEIGHT, JOINT_LIMIT_WEIGHT) if weights is None else tuple(float(v) for v in weights)
        self.opt = _lib.TrajOpts(float(lr), float(betas[0]), float(betas[1]), float(eps), *w, float(self.margin[0]) if R else 0.,
                                 float(max_step if max_speed is None else max_speed),
                                 VALID_CONSTRAINT_LOSS if valid_tol is None else float(valid_tol),
                                 STATIONARY_GRAD_NORM if grad_tol is None else float(grad_tol))
        self.dopt = _lib.TrajDenseOpts(float(max_step), self.max_samples, mask, remask, 1 if normalize else 0, float(stop_tol))
        nbytes = int(self.lib.dcx_traj_dense_work_bytes(model._h, R, W, self.max_samples))
        self.work = torch.empty(max(nbytes, 1), device=dev, dtype=torch.uint8)
        self.work_bytes = nbytes
        self.keep_history, self.history = bool(history), []
        self.it = 0

    close = ShardedAdamRun.close
    __del__ = ShardedAdamRun.__del__

    def run(self, n_iters):
        """enqueue n_iters more iterations on torch's current stream (no host synchronisation)"""
        if self.R and n_iters > 0:
            dev = self.model.dev
            hist = torch.empty((n_iters, self.R, self.W, self.dof), device=dev, dtype=torch.float32) if self.keep_history else None
            io = _lib.TrajDenseIO(C.c_void_p(self.move.data_ptr()) if self.move is not None else None,
                                  C.c_void_p(hist.data_ptr()) if hist is not None else None, C.c_void_p(self.n_checks.data_ptr()),
                                  None, None, None, None)
            with torch.cuda.device(dev):
                _lib.check(self.lib.dcx_traj_dense_run(self.model._h, C.byref(self.st), C.byref(self.opt), C.byref(self.dopt),
                                                       C.byref(io), C.c_void_p(self.margin.data_ptr()), self.it + 1, int(n_iters),
                                                       C.c_void_p(self.work.data_ptr()), self.work_bytes, self.model._st()))
            if hist is not None:
                self.history.append(hist)
        self.it += n_iters

    def all_done(self):
        return self.R == 0 or bool(self.t['done'].all())

    def over_bound(self):
        """bool [R] on the host: the restarts frozen because a segment needed more than max_samples samples"""
        return (self.t['stats'][:, 7] == -2).cpu()

    def finish(self):
        """(summaries [R, 5] on the host: best_valid_obj, lowest_loss, lowest_obj, steps, n_checks; best_valid_path,
        lowest_path [R, W, dof] on the device)"""
        t = self.t
        summ = torch.stack([t['best_valid_obj'].double(), t['lowest_loss'].double(), t['lowest_obj'].double(), t['steps'].double(),
                            self.n_checks.double()], dim=1)
        return summ.cpu(), t['best_valid_path'], t['lowest_path']


def _dense_adam_traj_optimize(robot, model, prob, inits, options, lr, wrap, t0, start_cfg, target_cfg):
    """fused_adam_traj_optimize under options['dense_check']: the same restarts, selection policy and record, on DenseAdamRun"""
    max_iter, seed = options['MAXITER'], options['seed']
    W = inits[0].shape[0]
    run = DenseAdamRun(model, robot.limits, torch.stack(inits), lr, prob.safety_margin, prob.max_speed,
                       max_samples=options.get('dense_max_samples'), wrap=wrap, grad_tol=options.get('stationary_grad_norm'))
    chunk = int(options.get('fused_chunk', 50))
    while run.it < max_iter:
        run.run(min(chunk, max_iter - run.it))
        if run.it < max_iter and run.all_done():
            break
    summ, best_valid_path, lowest_path = run.finish()
    over = run.over_bound()
    run.close()
    bvo, lol, loo, nst, nck = (summ[:, i] for i in range(5))
    t_win, found, cost, _ = select_trial(bvo.float(), lol.float(), loo.float(), nst, W)
    cnt = int(nck[:t_win + 1].sum().item()) if found else int(nck.sum().item())
    solution = (best_valid_path if found else lowest_path)[t_win]
    return {'start_cfg': _np(start_cfg).tolist(), 'target_cfg': _np(target_cfg).tolist(), 'cnt_check': cnt,
            'cost': cost, 'time': time.time() - t0, 'success': found, 'seed': seed,
            'solution': solution.double().cpu().numpy().tolist(),
            'trial': t_win, 'cnt_check_batched': int(nck.sum().item()), 'iterations_enqueued': run.it,
            'dense_check': True, 'dense_max_samples': run.max_samples,
            'dense_frozen_on_bound': [int(i) for i in torch.nonzero(over).reshape(-1)]}


def optimize_paths(robot, dist_est, paths, counts=None, *, n_waypoints, options, wrap=None):
    """R different planning problems optimised at once from their planned paths: `paths` / `counts` (what rrt_connect's
    path_tensor(), Roadmap.query_batch and shortcut_paths return, or a list of [W_r, dof] tensors or None) are resampled to
    n_waypoints waypoints each (resample.resample_paths: the endpoints keep their bits) and the R rows run as ONE DenseAdamRun -
    its rows are independent problems: fixed endpoints, `done`, `steps` and the best paths are all per row.  No walk over the
    paths on the host between the stages; the summaries are read back once at the end.

    options: 'MAXITER', 'max_speed', 'safety_margin', 'extra_optimizer_options'['lr'], 'dense_max_samples',
    'stationary_grad_norm' and 'fused_chunk', as fused_adam_traj_optimize reads them under 'dense_check' (the restart keys
    'NUM_RE_TRIALS', 'N_WAYPOINTS', 'init_solution' and 'seed' are not read: nothing is drawn).  `wrap` as on the motion calls.
    A row without a path after resampling (count 0) enters the run frozen - no step is taken on it - and answers None.
    Returns a list with one entry per input path, in order: None, or a dict with 'success', 'cost' (select_trial's policy on
    that row alone: the best valid path and its objective, else the lowest-loss path), 'solution' (the [n_waypoints, dof] device
    tensor), 'steps', 'cnt_check' (the samples scored for it) and 'frozen_on_bound' (a segment outgrew dense_max_samples)."""
    from .resample import resample_paths
    model = _resolve_model(dist_est)
    if robot.fk_desc().key() != model.desc.key():
        raise ValueError("the checker's transform is not this robot's fkine: the fused step shares one FK")
    res = resample_paths(paths, counts, n_waypoints=n_waypoints, wrap=wrap, transform=robot.fkine)
    R, T, dof = res.path.shape
    if R == 0:
        return []
    mask = _ops.wrap_mask(wrap, dof, robot.fkine)
    max_iter = int(options['MAXITER'])
    lr = options.get('extra_optimizer_options', {}).get('lr', 5e-1)
    run = DenseAdamRun(model, robot.limits, res.path.to(model.dev), lr, options.get('safety_margin', 0.0), options['max_speed'],
                       max_samples=options.get('dense_max_samples'), wrap=mask, grad_tol=options.get('stationary_grad_norm'))
    t = run.t
    dead = res.count.to(model.dev) == 0
    t['done'].copy_(dead.to(torch.int32))   # frozen from the start: the step kernel leaves a done row as it is
    chunk = int(options.get('fused_chunk', 50))
    while run.it < max_iter:
        run.run(min(chunk, max_iter - run.it))
        if run.it < max_iter and run.all_done():
            break
    # the one read-back of results: per row best_valid_obj, lowest_loss, lowest_obj, steps, n_checks, frozen on the bound, no path
    summ = torch.stack([t['best_valid_obj'].double(), t['lowest_loss'].double(), t['lowest_obj'].double(), t['steps'].double(),
                        run.n_checks.double(), (t['stats'][:, 7] == -2).double(), dead.double()], dim=1).cpu()
    best_valid_path, lowest_path = t['best_valid_path'], t['lowest_path']
    run.close()
    records = []
    for r in range(R):
        if summ[r, 6]:
            records.append(None)
            continue
        _, found, cost, _ = select_trial(summ[r:r + 1, 0].float(), summ[r:r + 1, 1].float(), summ[r:r + 1, 2].float(),
                                         summ[r:r + 1, 3], T)
        records.append({'success': found, 'cost': cost, 'solution': (best_valid_path if found else lowest_path)[r],
                        'steps': int(summ[r, 3]), 'cnt_check': int(summ[r, 4]), 'frozen_on_bound': bool(summ[r, 5])})
    return records


def fused_adam_traj_optimize(robot, dist_est, start_cfg, target_cfg, options, group=None, wrap=None):
    """Drop-in for `optim.adam_traj_optimize` with all restarts batched on the GPU.  With an initialised
    torch.distributed `group` (or the default group when options['distributed'] is true) the restarts are sharded
    across ranks (`ShardedAdamRun`); every rank returns the same record.

    options['dense_check'] true: the collision hinge is charged along the segments (`DenseAdamRun`, one device; the points of
    utils.dense_path(p, max_speed)); options['dense_max_samples'] bounds one segment's samples (default: from the longest
    initial segment, with headroom) and the record's 'dense_frozen_on_bound' lists the restarts that froze on it.  `wrap`, as on
    the motion calls, samples along the shortest arc of the masked coordinates.  'cnt_check' then counts the samples scored."""
    if wrap is not None and not options.get('dense_check'):
        raise ValueError("fused_adam_traj_optimize(wrap=...) needs options['dense_check']: the waypoint-only loop samples no segment")
    n_trials, max_iter = options['NUM_RE_TRIALS'], options['MAXITER']
    lr = options.get('extra_optimizer_options', {}).get('lr', 5e-1)
    seed = options['seed']
    torch.manual_seed(seed)
    prob = _PathProblem(robot, start_cfg, target_cfg, options)
    t0 = time.time()
    model = _resolve_model(dist_est)   # any class count: a MultiDiffCo score under options['safety_margin'] = a number or [C]
    desc = robot.fk_desc()
    if desc.key() != model.desc.key():
        raise ValueError("the checker's transform is not this robot's fkine: the fused step shares one FK")

    # ---- initial paths, exactly as the reference's sequential trials would draw them ----------------------
    inits = [prob.make_init(t).clone() for t in range(n_trials)]
    W, dof = inits[0].shape
    if W == 2:  # nothing to optimise (reference: optim.py:61-72)
        return {'start_cfg': _np(start_cfg).tolist(), 'target_cfg': _np(target_cfg).tolist(), 'cnt_check': 0,
                'cost': 0.0, 'time': time.time() - t0, 'success': True, 'seed': seed,
                'solution': inits[0].numpy().tolist()}
    if any(p.shape != (W, dof) for p in inits):
        raise ValueError("all restarts must have the same number of waypoints (init_solution vs N_WAYPOINTS)")
    if options.get('dense_check'):
        return _dense_adam_traj_optimize(robot, model, prob, inits, options, lr, _ops.wrap_mask(wrap, dof, robot.fkine), t0,
                                         start_cfg, target_cfg)

    run = ShardedAdamRun(model, robot.limits, torch.stack(inits), lr, prob.safety_margin, prob.max_speed,
                         grad_tol=options.get('stationary_grad_norm'), group=group,
                         sharded=options.get('distributed', False))
    chunk = int(options.get('fused_chunk', 50))  # iterations enqueued between two "all done?" checks
    while run.it < max_iter:
        run.run(min(chunk, max_iter - run.it))
        if run.it < max_iter and run.all_done():  # this rank's restarts are all frozen (no collective inside the loop)
            break
    # ---- gather the per-restart summaries (and paths) and apply the reference's selection policy ----------
    summ, best_valid_path, lowest_path = run.finish()
    run.close()
    bvo, lol, loo, nst = summ[:, 0], summ[:, 1], summ[:, 2], summ[:, 3]
    t_win, found, cost, cnt = select_trial(bvo, lol, loo, nst, W)
    solution = (best_valid_path if found else lowest_path)[t_win]
    return {'start_cfg': _np(start_cfg).tolist(), 'target_cfg': _np(target_cfg).tolist(), 'cnt_check': cnt,
            'cost': cost, 'time': time.time() - t0, 'success': found, 'seed': seed,
            'solution': solution.double().cpu().numpy().tolist(),
            'trial': t_win, 'cnt_check_batched': int(nst.sum().item()) * W, 'iterations_enqueued': run.it}
