"""The reference's checker facades over the HIP score path: `RBFDiffCo` and `ForwardKinematicsDiffCo`
(reference diffco/collision_checkers.py:28-125 CollisionChecker, :127-316 RBFDiffCo, :318-509 ForwardKinematicsDiffCo).

Host logic only — dataset bookkeeping, the fit / update / verify flow, the safety bias — restated so that the
tutorial's

    fkdc = ForwardKinematicsDiffCo(robot=panda_urdf_robot, gamma=10, gt_check_func=my_checker)
    fkdc.fit(q, labels)                       # or fit(num_samples=...) with a gt_check_func
    fkdc.collision_score(q)                   # differentiable, one fused HIP launch

runs with `perceptron.train` on the device trainer, `fit_poly` on HIP kernel rows and `poly_score` on the fused
kernel with the URDF tree inside it.  The ground truth enters as labels or as a `gt_check_func(q) -> {0,1}[N]`: the
reference derives labels from FCL/trimesh collision geometry (`robot.collision(q, other=environment)`); here
`diffco_amd.geometry.SphereWorldChecker` - a sphere model of the robot against a world of primitives, one fused HIP
launch - is such a callable (meshes and `environment=` stay out of scope).
"""
import os
import time
import torch

from . import _ops, _perceptron, kernel
from .kernel_perceptrons import DiffCo
from .urdf import MultiURDFRobotFK, URDFRobotFK


class CollisionChecker:
    def __init__(self, robot=None, robot_base_transform=None, environment=None, robot_topic=None,
                 planning_scene_topic=None, gt_check_func=None, device='cpu'):
        if robot_topic is not None or planning_scene_topic is not None:
            raise NotImplementedError("ROS robot / planning-scene interfaces are outside diffco_amd's scope")
        if environment is not None:
            raise NotImplementedError("collision environments (ShapeEnv / PCDEnv, FCL ground truth) are outside "
                                      "diffco_amd's scope: pass labels to fit() or a gt_check_func")
        if isinstance(robot, str):
            if not os.path.isfile(robot):
                raise ValueError('Invalid robot URDF file path')
            robot = URDFRobotFK(robot, name=os.path.basename(robot).split('.')[0], base_transform=robot_base_transform)
        self.robot = robot
        self.environment = None
        self.device = device
        self.gt_check_func = gt_check_func

    def _ground_truth(self, q):
        if self.gt_check_func is None:
            raise ValueError("no ground truth available: pass labels or construct the checker with gt_check_func "
                             "(diffco_amd.geometry.SphereWorldChecker is one)")
        return self.gt_check_func(q)

    def collision(self, q):
        return self._ground_truth(q)

    def fkine(self, q, return_collision=False, **kwargs):
        if return_collision:
            raise NotImplementedError("collision-geometry poses need the URDF's meshes (outside diffco_amd's scope)")
        return self.robot.link_positions(q)

    def normalizer(self, unnormalized_q):
        raise NotImplementedError

    def unnormalizer(self, normalized_q):
        raise NotImplementedError

    def _generate_dataset(self, q, labels, dists, num_samples, fix_joints=None, fix_joint_values=None, verbose=False):
        """(q, labels in {0, 1}, dists) for fit(): missing configurations are drawn from the joint limits, missing
        labels come from the ground-truth callable, missing distances are zeros"""
        q = self.robot.rand_configs(num_samples) if q is None else q
        if fix_joints is not None:
            q[:, fix_joints] = torch.as_tensor(fix_joint_values, dtype=q.dtype, device=q.device)
        if labels is not None:
            labels = labels.gt(0).to(q.dtype)
        else:
            t0 = time.perf_counter()
            labels = self._ground_truth(q)
            if verbose:
                print(f'Labels generated in {time.perf_counter() - t0:.2f}s')
        return q, labels, (q.new_zeros(len(q)) if dists is None else dists)


class RBFDiffCo(CollisionChecker):
    """DiffCo without a forward-kinematics transform (configuration-space kernel)"""

    def __init__(self, robot=None, robot_base_transform=None, environment=None, robot_topic=None,
                 planning_scene_topic=None, gt_check_func=None, device='cpu', kernel_func=None,
                 perceptron_class=DiffCo, **perceptron_kwargs):
        super().__init__(robot=robot, robot_base_transform=robot_base_transform, environment=environment,
                         robot_topic=robot_topic, planning_scene_topic=planning_scene_topic,
                         gt_check_func=gt_check_func, device=device)
        self.kernel_func = kernel.RQKernel(perceptron_kwargs.pop('gamma', 10)) if kernel_func is None else kernel_func
        self.perceptron = perceptron_class(kernel_func=self.kernel_func, **perceptron_kwargs)
        self._init_state()

    def _init_state(self):
        self.q_verify = None
        self.labels_verify = None
        self.safety_bias = 0
        self.perceptron_trained = False

    def fit(self, q=None, labels=None, dists=None, update=False, exist_mask=None, num_samples=5000, verify_ratio=0.1,
            verbose=False, **get_dataset_kwargs):
        """train (or update) the perceptron, fit the polyharmonic inference model on the labels, set the safety
        bias; 0 < verify_ratio < 1 holds out that share of the data and returns (acc, tpr, tnr) on it"""
        get_dataset_kwargs['verbose'] = not self.perceptron_trained
        q, labels, dists = self._generate_dataset(q, labels, dists, num_samples, **get_dataset_kwargs)
        num_samples = len(q)
        labels = (2 * labels - 1).type(q.dtype)
        labels_verify = None
        if 0 < verify_ratio < 1:
            num_verify = int(verify_ratio * num_samples)
            verify_mask = torch.zeros(len(q), dtype=torch.bool)
            if exist_mask is None:
                verify_mask[torch.randperm(len(q))[:num_verify]] = True
            else:
                # update(verify=ratio): the reference passes the full-length exist_mask on with the held-out subset
                # (collision_checkers.py:183-200, 246-252) and fails on the shape; here the current supports always
                # stay in the training part and the mask is cut to it
                fresh = torch.nonzero(~exist_mask.cpu()).reshape(-1)
                verify_mask[fresh[torch.randperm(len(fresh))[:num_verify]]] = True
                exist_mask = exist_mask[~verify_mask.to(exist_mask.device)]
            # (index_select: see kernel_perceptrons.train_perceptron)
            i_train, i_verify = torch.where(~verify_mask)[0], torch.where(verify_mask)[0]
            pick = lambda t, i: t.index_select(0, i.to(t.device))  # noqa: E731
            q_train, q_verify = pick(q, i_train), pick(q, i_verify)
            labels_train, labels_verify = pick(labels, i_train), pick(labels, i_verify)
            dists_train = pick(dists, i_train)
        elif verify_ratio:
            raise ValueError(f'verify_ratio should be in (0, 1), got {verify_ratio}')
        else:
            q_train, labels_train, dists_train = q, labels, dists
            q_verify = self.robot.rand_configs(100)
        self.perceptron.train(q_train, labels_train, update=update, exist_mask=exist_mask,
                              max_iteration=len(q_train), distance=dists_train, verbose=verbose)
        self.perceptron.fit_poly(kernel_func=kernel.Polyharmonic(k=1, epsilon=1), target='label')
        self.safety_bias = self._calculate_safety_bias(q_verify)
        if verify_ratio:  # verification needs self.safety_bias
            result = self.verify(q_verify, labels_verify, verbose=verbose)
            self.q_verify = q_verify
        else:
            result = (None, None, None)
        self.perceptron_trained = True
        return result

    def update(self, q=None, labels=None, dists=None, exploit_std=0.3, num_samples=100, num_exploit_samples=None,
               num_explore_samples=None, verify=False, verbose=False):
        """active-learning step: Gaussian samples around the supports + uniform samples + the supports themselves,
        re-labelled and fitted with `update=True` (the supports keep their gains as a jump start)"""
        num_exploit_samples = num_samples if num_exploit_samples is None else num_exploit_samples
        num_explore_samples = num_samples if num_explore_samples is None else num_explore_samples
        exist_mask = None
        if q is None:
            supports = self.perceptron.support_points
            if num_exploit_samples > len(supports):
                mul = (num_exploit_samples // len(supports)) + (num_exploit_samples % len(supports) > 0)
                selected = torch.arange(len(supports))
            else:
                mul = 1
                selected = torch.randperm(len(supports))[:num_exploit_samples]
            sel = supports[selected]
            lim = self.robot.joint_limits.to(device=sel.device, dtype=sel.dtype)
            exploit = torch.randn(mul, len(sel), self.robot._n_dofs, dtype=sel.dtype, device=sel.device) * exploit_std + sel[None]
            exploit = torch.clamp(exploit, min=lim[:, 0], max=lim[:, 1]).reshape(-1, self.robot._n_dofs)
            explore = self.robot.rand_configs(num_explore_samples).to(device=sel.device, dtype=sel.dtype)
            q = torch.cat([exploit, explore, supports], dim=0)
            exist_mask = torch.zeros(len(q), dtype=torch.bool, device=sel.device)
            exist_mask[-len(supports):] = True
        return self.fit(q, labels, dists, update=True, exist_mask=exist_mask, verify_ratio=verify, verbose=verbose)

    def _verification_set(self, num_samples):
        """a fresh random set of `num_samples` configurations (remembered), else the one kept from the last fit"""
        if num_samples is None and self.q_verify is None:
            raise ValueError('self.q_verify or num_samples should be provided')
        if num_samples is not None:
            self.q_verify = self.robot.rand_configs(num_samples)
        return self.q_verify

    def verify(self, q_verify=None, labels_verify=None, num_samples=None, verbose=False):
        if q_verify is None:
            q_verify = self._verification_set(num_samples)
        scores = self.perceptron.poly_score(q_verify)
        if labels_verify is None:
            labels_verify = (2 * self._ground_truth(q_verify) - 1).type(q_verify.dtype)

        def rates(pred):
            pred = (2 * pred - 1).reshape_as(labels_verify)
            acc = torch.sum(pred == labels_verify, dtype=torch.float32) / len(pred)
            tpr = torch.sum(pred[labels_verify == 1] == 1, dtype=torch.float32) / (labels_verify == 1).sum()
            tnr = torch.sum(pred[labels_verify == -1] == -1, dtype=torch.float32) / (labels_verify == -1).sum()
            return acc, tpr, tnr

        acc, tpr, tnr = rates(scores > 0)
        if verbose:
            print(f'Test acc: {acc:.4f}, TPR {tpr:.4f}, TNR {tnr:.4f}')
        acc, tpr, tnr = rates(scores + self.safety_bias > 0)
        if verbose:
            print(f'Biased Test acc: {acc:.4f}, TPR {tpr:.4f}, TNR {tnr:.4f}')
        return acc, tpr, tnr  # the reference returns the biased rates

    def collision(self, q):
        return self.collision_score(q) > 0

    def collision_score(self, q, bias=None):
        """q [..., dof] -> scores [..., 1] (+ safety bias)"""
        bias = self.safety_bias if bias is None else bias
        shape_q = q.shape
        raw = self.perceptron.poly_score(q.reshape(-1, shape_q[-1]))
        return raw.reshape(shape_q[:-1] + raw.shape[1:]) + bias

    def check_motions(self, q_start, q_end, max_step=None, res=None, bias=None, return_first=False, max_samples=None, wrap=None):
        """is the straight motion q_start[e] -> q_end[e] in collision, by `collision_score` (poly score + bias > 0; bias
        defaults to safety_bias) at its samples?  Exactly one rule: `max_step` (utils.dense_path's points) or `res`
        (line_predict's).  bool [E]; with return_first also the first colliding sample index (-1 = free).
        `wrap` (None, True: the robot's own circular coordinates, an int bitmask or one bool per coordinate): those
        coordinates are angles and the edge runs along their shortest arc."""
        first, _ = _perceptron.check_motions(self._poly_source(), q_start, q_end, res=res, max_step=max_step, margin=self._margin(bias),
                                             max_samples=max_samples, wrap=wrap)
        return _perceptron.motion_answer(first, return_first)

    def _poly_source(self):
        """what the motion calls run on: the perceptron's poly_score state; this checker reports the route (last_route)"""
        p = self.perceptron
        return _perceptron.MotionSource(self, p._poly_fused, p.transform, p.rbf_kernel, p.support_transformed, p.rbf_nodes)

    def _margin(self, bias=None):
        """the motion calls' margin for a bias (None: safety_bias): score + bias > 0 is score - margin > 0"""
        bias = self.safety_bias if bias is None else bias
        return -bias if not torch.is_tensor(bias) else -bias.detach().reshape(-1)

    def _rrt_model(self, device=None):
        """(ScoreModel, margin) of check_motions' fused route - the safety bias becomes the margin - or None where it takes the
        host route (rrt.rrt_connect)"""
        return _perceptron._motion_model(self._poly_source(), device, self._margin())

    def motion_cost(self, q_start, q_end, max_step=None, res=None, bias=None, weight=1., open_end=False, max_samples=None,
                    wrap=None):
        """[E] collision costs of the motions q_start[e] -> q_end[e] by `collision_score`: weight * sum over the samples of
        max(0, poly score + bias) (bias defaults to safety_bias), differentiable with respect to both endpoints.  Exactly one
        rule, as check_motions (open_end drops the target sample under max_step; `wrap` as there)."""
        return _perceptron.motion_cost(self._poly_source(), q_start, q_end, res=res, max_step=max_step, margin=self._margin(bias),
                                       weight=weight, open_end=open_end, max_samples=max_samples, wrap=wrap)

    def path_cost(self, paths, max_step, bias=None, weight=1., max_samples=None, wrap=None):
        """[T] collision costs of paths [T, W, dof] by `collision_score` over utils.dense_path(p, max_step)'s points,
        differentiable with respect to every waypoint (`wrap` as check_motions: per segment)"""
        return _perceptron.path_cost(self._poly_source(), paths, max_step, margin=self._margin(bias), weight=weight,
                                     max_samples=max_samples, wrap=wrap)

    def motion_worst(self, q_start, q_end, max_step=None, res=None, bias=None, max_samples=None, wrap=None):
        """(worst [E], sample [E], class [E]) of the motions q_start[e] -> q_end[e]: the peak of `collision_score` (poly score
        + bias; bias defaults to safety_bias) over check_motions' samples and the first sample that attains it.  worst is
        differentiable with respect to both endpoints.  Exactly one rule and `wrap` as check_motions."""
        return _perceptron.motion_worst(self._poly_source(), q_start, q_end, res=res, max_step=max_step, margin=self._margin(bias),
                                        max_samples=max_samples, wrap=wrap)

    def path_worst(self, paths, max_step, bias=None, max_samples=None, wrap=None):
        """(worst [T], segment [T], sample [T]) of paths [T, W, dof] by `collision_score` (the closed max_step rule per segment,
        the first maximum in (segment, sample) order); worst is differentiable with respect to every waypoint"""
        return _perceptron.path_worst(self._poly_source(), paths, max_step, margin=self._margin(bias), max_samples=max_samples,
                                      wrap=wrap)

    def motion_bias_sweep(self, q_start, q_end, biases, max_step=None, res=None, max_samples=None, wrap=None):
        """bool [len(biases), E]: would the motion q_start[e] -> q_end[e] collide under each candidate bias?  ONE worst-sample
        call at bias 0 answers every bias: row b is worst_at_zero_bias + biases[b] > 0, what check_motions(bias=biases[b])
        returns (up to the rounding of the sum at a tie)."""
        worst, _, _ = self.motion_worst(q_start, q_end, max_step=max_step, res=res, bias=0.0, max_samples=max_samples, wrap=wrap)
        b = torch.as_tensor(biases, dtype=worst.dtype, device=worst.device).reshape(-1)
        return worst.detach()[None, :] + b[:, None] > 0

    def _calculate_safety_bias(self, q_verify):
        """a third of the smaller of |min score| and |max score| over q_verify (collision_checkers.py:497-503; the
        reference defines it on the FK subclass only and its RBFDiffCo.fit calls it regardless)"""
        scores = self.perceptron.poly_score(q_verify)[:, 0]
        return min(scores.min().abs(), scores.max().abs()) / 3

    def normalizer(self, unnormalized_q):
        lim = self.robot.joint_limits
        return (unnormalized_q - lim[:, 0]) / (lim[:, 1] - lim[:, 0])

    def unnormalizer(self, normalized_q):
        lim = self.robot.joint_limits
        return normalized_q * (lim[:, 1] - lim[:, 0]) + lim[:, 0]


class ForwardKinematicsDiffCo(RBFDiffCo):
    """DiffCo on the link-origin features of a URDF robot (recommended for manipulators): the kinematic tree is
    fused into the HIP score kernel (`robot.fkine` is the perceptron's transform)"""

    def __init__(self, robot=None, robot_base_transform=None, environment=None, robot_topic=None,
                 planning_scene_topic=None, gt_check_func=None, device='cpu', perceptron_class=DiffCo,
                 **perceptron_kwargs):
        CollisionChecker.__init__(self, robot=robot, robot_base_transform=robot_base_transform, environment=environment,
                                  robot_topic=robot_topic, planning_scene_topic=planning_scene_topic,
                                  gt_check_func=gt_check_func, device=device)
        if not isinstance(self.robot, (URDFRobotFK, MultiURDFRobotFK)):
            raise TypeError("ForwardKinematicsDiffCo needs a diffco_amd URDFRobotFK / MultiURDFRobotFK (or a URDF path)")
        self.unique_position_link_names = list(self.robot.unique_position_link_names)
        self.tensorized_fkine = self.robot.fkine
        self.kernel_func = kernel.RQKernel(perceptron_kwargs.pop('gamma', 10))
        self.kernel_transform = self.robot.fkine  # a bound diffco_amd fkine: fused, not called
        self.perceptron = perceptron_class(kernel_func=self.kernel_func, transform=self.kernel_transform,
                                           **perceptron_kwargs)
        self._init_state()

    def _uniform_sample_on_transformed_manifold(self, transform, num_samples):
        """rejection-sample configurations with density proportional to sqrt(det(J J^T + 1e-4 I)) of `transform`,
        i.e. uniformly on the image manifold (J through the HIP vjp, one row of the Jacobian per backward)"""
        def jac_det(q):
            q = q.clone().detach().requires_grad_(True)
            pos = transform(q).reshape(len(q), -1)
            D = pos.shape[-1]
            jac = torch.zeros(len(q), D, q.shape[-1], device=q.device, dtype=q.dtype)
            eye = torch.eye(D, device=q.device, dtype=q.dtype)
            for i in range(D):
                (g,) = torch.autograd.grad(pos, q, eye[i][None].expand_as(pos), retain_graph=True)
                jac[:, i] = g
            if jac.shape[-2] > jac.shape[-1]:
                jac = jac.transpose(-2, -1)
            gram = torch.matmul(jac, jac.transpose(-2, -1)) + 1e-4 * torch.eye(jac.shape[-2], device=q.device, dtype=q.dtype)
            return torch.linalg.det(gram).sqrt()

        rand_q = self.robot.rand_configs(num_samples)
        det = jac_det(rand_q)
        max_det = 1.1 * det.max()
        valid, count = [], 0
        while True:
            accepted = rand_q[det > torch.rand(len(rand_q), dtype=rand_q.dtype) * max_det]
            valid.append(accepted)
            count += len(accepted)
            if count >= num_samples:
                break
            rand_q = self.robot.rand_configs(num_samples)
            det = jac_det(rand_q)
        return torch.cat(valid, dim=0)[:num_samples]

    def _generate_dataset(self, q, labels, dists, num_samples, verbose=False, sample_transform=None, **kwargs):
        if sample_transform is not None:  # 'fkine' or any callable: sample uniformly on that map's image
            named = {'fkine': self.tensorized_fkine}
            transform = named.get(sample_transform) if isinstance(sample_transform, str) else sample_transform
            if not callable(transform):
                raise ValueError(f'Invalid sample_transform: {sample_transform}')
            q = self._uniform_sample_on_transformed_manifold(transform, num_samples)
        return super()._generate_dataset(q, labels, dists, len(q) if q is not None else num_samples, verbose=verbose, **kwargs)

    def collision_score(self, q=None, bias=None, q_link_pos=None):
        """q [..., dof], or q_link_pos [..., 3, L] link origins that bypass the forward kinematics"""
        bias = self.safety_bias if bias is None else bias
        if q is not None:
            shape_q = q.shape
            raw = self.perceptron.poly_score(point=q.reshape(-1, shape_q[-1]))
            raw = raw.reshape(shape_q[:-1] + raw.shape[1:])
        elif q_link_pos is not None:
            shape = q_link_pos.shape
            raw = self.perceptron.poly_score(transformed_point=q_link_pos.reshape(-1, *shape[-2:]))
            raw = raw.reshape(shape[:-2] + raw.shape[1:])
        else:
            raise ValueError("collision_score needs q or q_link_pos")
        return raw + bias


class HybridForwardKinematicsDiffCo(ForwardKinematicsDiffCo):
    """ForwardKinematicsDiffCo used safely in a planner: the proxy's verdict counts where the unbiased poly score is clearly
    above +band or at or below -band, and only the configurations inside the band go to `gt_check_func` (a callable
    q [U, dof] -> bool [U]).  `band` defaults to safety_bias.  With lazy_line_check only the worst configuration of a line is
    ground-truth checked.  `last_gt_checks` counts the configurations the last call handed to the ground truth.

    The reference's class (collision_checkers.py:511-548) reads `self.safe_bias` in its non-lazy branch, an attribute nothing
    defines, so that branch raises as written; the band it means is [-safety_bias, +safety_bias] on the unbiased score."""

    def __init__(self, robot=None, robot_base_transform=None, environment=None, robot_topic=None,
                 planning_scene_topic=None, gt_check_func=None, device='cpu', lazy_line_check=False, perceptron_class=DiffCo,
                 **perceptron_kwargs):
        super().__init__(robot=robot, robot_base_transform=robot_base_transform, environment=environment,
                         robot_topic=robot_topic, planning_scene_topic=planning_scene_topic, gt_check_func=gt_check_func,
                         device=device, perceptron_class=perceptron_class, **perceptron_kwargs)
        self.lazy_line_check = lazy_line_check
        self.last_gt_checks = 0

    def _band(self, band):
        band = self.safety_bias if band is None else band
        band = float(band)
        if not band >= 0:
            raise ValueError(f"the uncertainty band must be >= 0, got {band}")
        return band

    def _gt(self, q, device):
        self.last_gt_checks += len(q)
        return torch.as_tensor(self.gt_check_func(q)).reshape(-1).to(device=device, dtype=torch.bool)

    def collision(self, q, band=None):
        """bool labels q.shape[:-1] (the reference's lines 538-548 with the band it means).  Not lazy: a score above +band
        collides, one at or below -band is free, and the configurations between go through `gt_check_func` in ONE call, in
        order; their labels replace the proxy's.  Lazy (q: the points of one line): the labels are score + safety_bias > 0,
        and the one configuration with the largest score is ground-truth checked."""
        self.last_gt_checks = 0
        shape = q.shape[:-1]
        q2 = q.reshape(-1, q.shape[-1])
        if self.lazy_line_check:
            s = self.collision_score(q2, bias=0).reshape(len(q2), -1).amax(dim=-1)
            labels = s + self.safety_bias > 0
            if len(q2):
                i = s.argmax()
                labels[i] = self._gt(q2[i:i + 1], labels.device)[0]
            return labels.reshape(shape)
        band = self._band(band)
        label, unc_idx = _perceptron.score_band(self._poly_source(), q2, -band, band)
        labels = (label == 1).to(q2.device)
        if len(unc_idx):
            unc_idx = unc_idx.to(q2.device)
            labels[unc_idx] = self._gt(q2[unc_idx], q2.device)
        return labels.reshape(shape)

    def check_motions(self, q_start, q_end, max_step=None, res=None, band=None, return_first=False, max_samples=None, wrap=None):
        """is the straight motion q_start[e] -> q_end[e] in collision?  bool [E]; with return_first also the first sample that
        collided - sure, or confirmed by the ground truth - (-1 = free).  One dcx_motion_band call on the unbiased poly score
        with lo = -band, hi = +band (`band` defaults to safety_bias); exactly one rule and `wrap` as
        ForwardKinematicsDiffCo.check_motions.
        Not lazy: `gt_check_func` is called once on the uncertain samples of the edges without a sure hit; such an edge
        collides iff one of its listed samples does.  Lazy: one dcx_motion_worst call at bias 0; only the worst sample of each
        edge whose peak lies in the band is ground-truth checked, and the edge takes its label (the sample returned with
        return_first is then the edge's worst sample, not its first one above the band)."""
        band = self._band(band)
        self.last_gt_checks = 0
        q_start, q_end = torch.as_tensor(q_start), torch.as_tensor(q_end)
        kw = dict(res=res, max_step=max_step, max_samples=max_samples, wrap=wrap)
        if self.lazy_line_check:
            worst, idx, _ = _perceptron.motion_worst(self._poly_source(), q_start, q_end, margin=0., **kw)
            worst, first = worst.detach(), idx.to(torch.int64)
            hit = worst > band
            unc = ~hit & ~(worst <= -band)
            first = torch.where(hit | unc, first, torch.full_like(first, -1))
            e = unc.nonzero().reshape(-1)
            if len(e):
                q = self._motion_points(q_start, q_end, e, first[e], res, max_step, wrap)
                gt = self._gt(q, hit.device)
                hit[e] = gt
                first[e] = torch.where(gt, first[e], torch.full_like(first[e], -1))
            return (hit, first.to(torch.int32)) if return_first else hit
        verdict, first, _, unc_edge, unc_sample, unc_q = _perceptron.motion_band(self._poly_source(), q_start, q_end, -band, band, **kw)
        _perceptron._raise_over("check_motions", verdict == -2)
        hit = verdict == 1
        first = first.clone()
        if len(unc_edge):
            gt = self._gt(unc_q.to(device=q_start.device, dtype=q_start.dtype), hit.device)
            edges, samples = unc_edge.to(torch.int64)[gt], unc_sample[gt]
            hit[edges] = True
            big = torch.iinfo(torch.int32).max
            confirmed = torch.full_like(first, big).scatter_reduce(0, edges, samples, reduce="amin")
            first = torch.where(confirmed < big, confirmed, first)
        return (hit, first) if return_first else hit

    def _rrt_model(self, device=None):
        """None: an edge's verdict may need the ground truth, so a planner goes through check_motions (rrt.host_rrt_connect)"""
        return None

    def _motion_points(self, q_start, q_end, edges, samples, res, max_step, wrap):
        """sample samples[i] of the edge edges[i]: the points the host composition materialises (_perceptron._check_points)"""
        qa = q_start.reshape(-1, q_start.shape[-1])[edges.to(q_start.device)]
        qb = q_end.reshape(-1, q_end.shape[-1])[edges.to(q_end.device)]
        mask = _ops.wrap_mask(wrap, qa.shape[-1], self.perceptron.transform)
        d, L, n = _perceptron._edge_counts(qa, qb, res, max_step, mask)
        each = torch.arange(len(qa), device=qa.device)
        return _perceptron._check_points(qa, qb, d, L, n, each, samples.to(qa.device), res, max_step, mask)
