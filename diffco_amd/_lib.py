"""Loader for libdcx.so (the HIP implementation) via ctypes.

There is no CPU implementation of the hot path in this package: if the library is missing
or no GPU is visible, every op raises.  `import torch` happens first on purpose — torch
bundles its own libamdhip64; loading ours afterwards binds to the already-mapped runtime so
both share streams and allocations.
"""
import ctypes as C
import os

import torch  # noqa: F401  (must precede CDLL, see docstring)

from ._fkdesc import FkDesc

_HERE = os.path.dirname(os.path.abspath(__file__))
# DCX_LIB: developer override used by tools/sweep.py to A/B kernel variants; never a CPU path
LIB_PATH = os.environ.get("DCX_LIB") or os.path.join(_HERE, "libdcx.so")

# every symbol include/dcx.h declares: (restype, argtypes)
_c_fp = C.c_void_p  # device/host float pointers travel as raw addresses
SYMBOLS = {
    "dcx_version": (C.c_int, []),
    "dcx_last_error": (C.c_char_p, []),
    "dcx_device_count": (C.c_int, []),
    "dcx_debug_set": (C.c_int, [C.c_char_p, C.c_int64]),
    "dcx_debug_clock_probe": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_int32), C.c_void_p]),
    "dcx_model_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(FkDesc), C.c_int, C.POINTER(C.c_float),
                                   _c_fp, _c_fp, C.c_int64, C.c_int32, C.c_int32]),
    "dcx_model_create_ex": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(FkDesc), C.c_int, C.POINTER(C.c_float),
                                      _c_fp, _c_fp, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_void_p]),
    "dcx_model_update": (C.c_int, [C.c_void_p, _c_fp, _c_fp, C.c_int64, C.c_void_p]),
    "dcx_model_destroy": (None, [C.c_void_p]),
    "dcx_model_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "dcx_score": (C.c_int, [C.c_void_p, _c_fp, C.c_int64, _c_fp, C.c_void_p]),
    "dcx_score_grad": (C.c_int, [C.c_void_p, _c_fp, C.c_int64, _c_fp, _c_fp, _c_fp, C.c_void_p]),
    "dcx_score_jac": (C.c_int, [C.c_void_p, _c_fp, C.c_int64, _c_fp, _c_fp, C.c_void_p]),
    "dcx_score_hess": (C.c_int, [C.c_void_p, _c_fp, C.c_int64, _c_fp, _c_fp, _c_fp, C.c_void_p]),
    "dcx_score_hinge_grad": (C.c_int, [C.c_void_p, _c_fp, C.c_int64, C.c_float, C.c_float, _c_fp, _c_fp, C.c_void_p]),
    "dcx_score_hinge_grad_mc": (C.c_int, [C.c_void_p, _c_fp, C.c_int64, C.POINTER(C.c_float), C.c_float, _c_fp, _c_fp, C.c_void_p]),
    "dcx_traj_adam_run_mc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.c_int32, C.c_void_p]),
    "dcx_traj_adam_step_mc": (C.c_int, [C.c_int, C.POINTER(FkDesc), C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.c_int32,
                                        C.c_void_p]),
    "dcx_traj_adam_step": (C.c_int, [C.c_int, C.POINTER(FkDesc), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "dcx_traj_adam_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "dcx_escape_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int64]),
    "dcx_escape_adam": (C.c_int, [C.c_void_p, _c_fp, C.c_int64, _c_fp, C.c_void_p, C.c_void_p, C.c_size_t, _c_fp, C.c_void_p,
                                  C.c_void_p]),
    "dcx_train_perceptron": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_float), C.c_float, _c_fp, C.c_int64, C.c_int32, _c_fp,
                                       C.c_int32, _c_fp, _c_fp, _c_fp, C.c_int32, _c_fp, C.c_void_p]),
    "dcx_train_perceptron_ex": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_float), C.c_float, _c_fp, C.c_int64, C.c_int32, _c_fp,
                                          C.c_int32, _c_fp, _c_fp, _c_fp, C.c_int32, _c_fp, C.c_int32, C.c_void_p]),
    "dcx_fkine": (C.c_int, [C.c_int, C.POINTER(FkDesc), _c_fp, C.c_int64, _c_fp, C.c_void_p]),
    "dcx_fkine_vjp": (C.c_int, [C.c_int, C.POINTER(FkDesc), _c_fp, _c_fp, C.c_int64, _c_fp, C.c_void_p]),
    "dcx_dh_frames": (C.c_int, [C.c_int, _c_fp, C.c_int64, C.c_int32, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, C.c_void_p]),
    "dcx_dh_frames_vjp": (C.c_int, [C.c_int, _c_fp, C.c_int64, C.c_int32, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, C.c_void_p]),
    "dcx_euler_frames": (C.c_int, [C.c_int, _c_fp, C.c_int64, _c_fp, C.c_void_p]),
    "dcx_euler_frames_vjp": (C.c_int, [C.c_int, _c_fp, _c_fp, C.c_int64, _c_fp, C.c_void_p]),
    "dcx_kernel_matrix": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_float), _c_fp, C.c_int64, _c_fp, C.c_int64,
                                    C.c_int32, _c_fp, C.c_void_p]),
    "dcx_motion_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int64]),
    "dcx_check_motions": (C.c_int, [C.c_void_p, _c_fp, _c_fp, C.c_int64, C.c_void_p, _c_fp, _c_fp, _c_fp, C.c_void_p, C.c_size_t,
                                    C.c_void_p]),
    "dcx_motion_cost_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_int32]),
    "dcx_motion_cost": (C.c_int, [C.c_void_p, _c_fp, _c_fp, C.c_int64, C.c_void_p, _c_fp, C.c_float, _c_fp, _c_fp, _c_fp, _c_fp,
                                  C.c_void_p, C.c_size_t, C.c_void_p]),
    # the two motion calls with a per-coordinate wrap mask (uint64 before the stream)
    "dcx_check_motions_ex": (C.c_int, [C.c_void_p, _c_fp, _c_fp, C.c_int64, C.c_void_p, _c_fp, _c_fp, _c_fp, C.c_void_p, C.c_size_t,
                                       C.c_uint64, C.c_void_p]),
    "dcx_motion_cost_ex": (C.c_int, [C.c_void_p, _c_fp, _c_fp, C.c_int64, C.c_void_p, _c_fp, C.c_float, _c_fp, _c_fp, _c_fp, _c_fp,
                                     C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p]),
    # worst-sample motion queries: peak score per edge, where, against which class, and its endpoint gradients
    "dcx_motion_worst_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int64]),
    "dcx_motion_worst": (C.c_int, [C.c_void_p, _c_fp, _c_fp, C.c_int64, C.c_void_p, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp, _c_fp,
                                   C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p]),
    # hybrid motion checks: sure verdicts per edge and the ordered list of the samples that still need the ground truth
    "dcx_motion_band_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_int32]),
    "dcx_motion_band": (C.c_int, [C.c_void_p, _c_fp, _c_fp, C.c_int64, C.c_void_p, _c_fp, _c_fp, C.c_void_p, C.c_void_p, C.c_size_t,
                                  C.c_uint64, C.c_void_p]),
    # dense-check Adam trajectory loop: the collision hinge along the segments (dcx_motion_cost_ex per iteration)
    "dcx_traj_dense_step": (C.c_int, [C.c_int, C.POINTER(FkDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_void_p]),
    "dcx_traj_dense_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "dcx_traj_dense_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _c_fp, C.c_int32, C.c_int32,
                                     C.c_void_p, C.c_size_t, C.c_void_p]),
    # k nearest neighbours under the motion calls' metric (no model)
    "dcx_knn_work_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "dcx_knn": (C.c_int, [C.c_int, _c_fp, C.c_int64, _c_fp, C.c_int64, C.c_int32, C.c_void_p, _c_fp, _c_fp, C.c_void_p, C.c_size_t,
                          C.c_void_p]),
    # geometric ground truth: the robot's spheres against a world of primitives (no model)
    "dcx_geom_clearance": (C.c_int, [C.c_int, C.POINTER(FkDesc), _c_fp, C.c_void_p, C.c_int64, _c_fp, C.c_int64, C.c_void_p, _c_fp,
                                     C.c_void_p, _c_fp, C.c_void_p]),
    # batched RRT-Connect: R trees grown in lockstep over the kNN metric and the motion checks
    "dcx_rrt_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_int32]),
    "dcx_rrt_connect_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _c_fp, C.c_int32, C.c_int64, C.c_void_p, _c_fp, C.c_void_p,
                                      C.c_size_t, C.c_void_p]),
    # batched RRT*: one tree per problem, parent choice and rewiring over a near set, and the paths to the goal nodes as one tensor
    "dcx_rrtstar_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32]),
    "dcx_rrtstar_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _c_fp, _c_fp, C.c_int32, C.c_int64, C.c_void_p, _c_fp, C.c_void_p,
                                  C.c_size_t, C.c_void_p]),
    "dcx_rrtstar_extract_paths": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, _c_fp, C.c_int32, _c_fp, C.c_void_p]),
    # RRT*'s samples drawn on the device: one round's rows from the state as it stands, and the run that draws and plans
    "dcx_rrtstar_sample": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, _c_fp, C.c_void_p, C.c_int64, _c_fp, _c_fp, C.c_void_p]),
    "dcx_rrtstar_sampled_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32]),
    "dcx_rrtstar_run_sampled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _c_fp, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, _c_fp,
                                          C.c_void_p, C.c_size_t, _c_fp, _c_fp, C.c_void_p]),
    # RRT* under clearance-weighted edge costs: dcx_rrtstar_run / _run_sampled with dcx_rrtstar_cost_opts after the options
    "dcx_rrtstar_cost_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32]),
    "dcx_rrtstar_run_cost": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _c_fp, _c_fp, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, _c_fp,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    "dcx_rrtstar_sampled_cost_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32]),
    "dcx_rrtstar_run_sampled_cost": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _c_fp, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p,
                                               C.c_void_p, _c_fp, C.c_void_p, C.c_size_t, _c_fp, _c_fp, C.c_void_p]),
    # batched path shortcutting over the motion checks, and the solved paths of an RRT state as one tensor
    "dcx_path_shortcut_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_int32]),
    "dcx_path_shortcut_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _c_fp, C.c_int32, C.c_void_p, _c_fp, C.c_void_p,
                                        C.c_size_t, C.c_void_p]),
    "dcx_rrt_extract_paths": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, _c_fp, _c_fp, C.c_int32, C.c_void_p]),
    # partial shortcuts: chords between points inside segments, on the same state and options (W is also the capacity)
    "dcx_path_shortcut_partial_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32]),
    "dcx_path_shortcut_partial_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _c_fp, C.c_int32, C.c_void_p, _c_fp, C.c_void_p,
                                                C.c_size_t, C.c_void_p]),
    # shortcuts under the clearance objective: both modes with the caller's seg [R, W] after the state and dcx_rrtstar_cost_opts
    # after the options
    "dcx_path_shortcut_cost_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_int32]),
    "dcx_path_shortcut_run_cost": (C.c_int, [C.c_void_p, C.c_void_p, _c_fp, C.c_int64, _c_fp, C.c_int32, C.c_void_p, C.c_void_p, _c_fp,
                                             C.c_void_p, C.c_size_t, C.c_void_p]),
    "dcx_path_shortcut_partial_cost_work_bytes": (C.c_size_t, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32]),
    "dcx_path_shortcut_partial_run_cost": (C.c_int, [C.c_void_p, C.c_void_p, _c_fp, C.c_int64, _c_fp, C.c_int32, C.c_void_p, C.c_void_p,
                                                     _c_fp, C.c_void_p, C.c_size_t, C.c_void_p]),
    # roadmap queries: min-plus relaxation over the roadmap's CSR for Q start/goal pairs, and their routes as one tensor
    "dcx_sssp_run": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                               C.c_void_p]),
    "dcx_sssp_extract_paths": (C.c_int, [C.c_int, C.c_void_p, _c_fp, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p,
                                         _c_fp, _c_fp, C.c_void_p, _c_fp, _c_fp, C.c_void_p, _c_fp, C.c_int32, C.c_void_p]),
    # lazy roadmap queries: the unchecked edges of the current shortest routes as one ordered list, and the verdicts written back
    "dcx_sssp_mark_routes_work_bytes": (C.c_size_t, [C.c_int64]),
    "dcx_sssp_mark_routes": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, _c_fp, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _c_fp, _c_fp, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    "dcx_graph_apply_checks": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # batched path resampling: R paths of uneven length as rows of T waypoints, equally spaced in arc length (no model)
    "dcx_path_resample_work_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "dcx_path_resample": (C.c_int, [C.c_int, _c_fp, _c_fp, C.c_int64, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, _c_fp, _c_fp, _c_fp,
                                    C.c_void_p, C.c_size_t, C.c_void_p]),
    "dcx_solve_work_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "dcx_solve": (C.c_int, [C.c_int, _c_fp, _c_fp, C.c_int64, C.c_int64, _c_fp, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int32,
                            C.c_void_p]),
}



class TrajState(C.Structure):
    """ctypes mirror of dcx_traj_state (include/dcx.h)"""
    _fields_ = [("n_paths", C.c_int32), ("n_waypoints", C.c_int32)] + [
        (n, C.c_void_p) for n in ("path", "adam_m", "adam_v", "limits", "col_score", "col_grad", "stats", "lowest_loss",
                                  "lowest_obj", "lowest_path", "best_valid_obj", "best_valid_path", "done", "steps")]


class TrajOpts(C.Structure):
    """ctypes mirror of dcx_traj_opts (include/dcx.h)"""
    _fields_ = [(n, C.c_float) for n in ("lr", "beta1", "beta2", "eps", "w_diff", "w_collision", "w_max_move",
                                         "w_joint_limit", "safety_margin", "max_speed", "valid_tol", "grad_tol")]


class EscapeOpts(C.Structure):
    """ctypes mirror of dcx_escape_opts (include/dcx.h)"""
    _fields_ = [(n, C.c_float) for n in ("lr", "beta1", "beta2", "eps")] + [
        (n, C.c_int32) for n in ("n_steps", "record_freq", "joint", "compact_every")] + [("wrap_mask", C.c_uint64)]


class MotionOpts(C.Structure):
    """ctypes mirror of dcx_motion_opts (include/dcx.h)"""
    _fields_ = [("res", C.c_int32), ("max_step", C.c_float), ("max_samples", C.c_int32), ("reserved", C.c_int32)]


class MotionBandOut(C.Structure):
    """ctypes mirror of dcx_motion_band_out (include/dcx.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("verdict", "first_hit", "n_samples", "n_uncertain", "unc_total", "unc_edge",
                                          "unc_sample", "unc_q")] + [("unc_cap", C.c_int64), ("reserved", C.c_int64 * 2)]


KNN_MAX_K = 64   # DCX_KNN_MAX_K


class KnnOpts(C.Structure):
    """ctypes mirror of dcx_knn_opts (include/dcx.h)"""
    _fields_ = [("k", C.c_int32), ("reserved0", C.c_int32), ("wrap_mask", C.c_uint64), ("max_dist2", C.c_float),
                ("reserved1", C.c_int32), ("self_offset", C.c_int64), ("reserved", C.c_int64 * 2)]


GEOM_SPHERE, GEOM_BOX, GEOM_CAPSULE, GEOM_CYLINDER = range(4)   # DCX_GEOM_*


class GeomObstacle(C.Structure):
    """ctypes mirror of dcx_geom_obstacle (include/dcx.h): one 64-byte row"""
    _fields_ = [("type_group", C.c_int32), ("rt", C.c_float * 9), ("c", C.c_float * 3), ("p", C.c_float * 3)]


class GeomOpts(C.Structure):
    """ctypes mirror of dcx_geom_opts (include/dcx.h)"""
    _fields_ = [("n_groups", C.c_int32), ("sphere_base", C.c_int32), ("accumulate", C.c_int32), ("reserved", C.c_int32)]


RRT_MAX_SLOTS = 16        # DCX_RRT_MAX_SLOTS
RRT_MAX_CAP = 1 << 20     # DCX_RRT_MAX_CAP


class RrtState(C.Structure):
    """ctypes mirror of dcx_rrt_state (include/dcx.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("nodes", "parent", "count", "status", "link", "solved_round")]


class RrtOpts(C.Structure):
    """ctypes mirror of dcx_rrt_opts (include/dcx.h)"""
    _fields_ = [("range", C.c_float), ("max_step", C.c_float), ("max_samples", C.c_int32), ("slots", C.c_int32), ("cap", C.c_int32),
                ("reserved0", C.c_int32), ("wrap_mask", C.c_uint64), ("reserved", C.c_int64 * 2)]


RRTSTAR_MAX_NEAR = 16     # DCX_RRTSTAR_MAX_NEAR
RRTSTAR_MAX_CAP = 1 << 16  # DCX_RRTSTAR_MAX_CAP
RRTSTAR_STATE = ("nodes", "parent", "elen", "cost", "count", "status", "goal_node", "first_round")


class RrtStarState(C.Structure):
    """ctypes mirror of dcx_rrtstar_state (include/dcx.h)"""
    _fields_ = [(n, C.c_void_p) for n in RRTSTAR_STATE]


class RrtStarOpts(C.Structure):
    """ctypes mirror of dcx_rrtstar_opts (include/dcx.h)"""
    _fields_ = [("range", C.c_float), ("max_step", C.c_float), ("radius", C.c_float), ("max_samples", C.c_int32), ("slots", C.c_int32),
                ("near", C.c_int32), ("cap", C.c_int32), ("reserved0", C.c_int32), ("wrap_mask", C.c_uint64), ("reserved", C.c_int64 * 2)]


RRTSTAR_MAX_TRIES = 16                    # DCX_RRTSTAR_MAX_TRIES
RRTSTAR_SAMPLE_MODES = {"uniform": 0, "informed": 1}   # DCX_RRTSTAR_SAMPLE_UNIFORM, DCX_RRTSTAR_SAMPLE_INFORMED
RRTSTAR_SAMPLE_MAX_PROBLEMS = 1 << 28     # DCX_RRTSTAR_SAMPLE_MAX_PROBLEMS


RRTSTAR_COST_PEAK = 1   # dcx_rrtstar_cost_opts' mode


class RrtStarCostOpts(C.Structure):
    """ctypes mirror of dcx_rrtstar_cost_opts (include/dcx.h)"""
    _fields_ = [("mode", C.c_int32), ("gain", C.c_float), ("band", C.c_float), ("reserved0", C.c_int32), ("reserved", C.c_int64 * 2)]


class RrtStarSampleOpts(C.Structure):
    """ctypes mirror of dcx_rrtstar_sample_opts (include/dcx.h)"""
    _fields_ = [("limits", C.c_void_p), ("seed", C.c_uint64), ("goal_bias", C.c_float), ("uniform_mix", C.c_float), ("mode", C.c_int32),
                ("tries", C.c_int32), ("slots", C.c_int32), ("cap", C.c_int32), ("dof", C.c_int32), ("reserved0", C.c_int32),
                ("wrap_mask", C.c_uint64), ("reserved", C.c_int64 * 2)]


SHORTCUT_MAX_SLOTS = 16           # DCX_SHORTCUT_MAX_SLOTS
SHORTCUT_MAX_WAYPOINTS = 1 << 16  # DCX_SHORTCUT_MAX_WAYPOINTS


class ShortcutState(C.Structure):
    """ctypes mirror of dcx_shortcut_state (include/dcx.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("path", "count", "accepted")]


class ShortcutOpts(C.Structure):
    """ctypes mirror of dcx_shortcut_opts (include/dcx.h)"""
    _fields_ = [("max_step", C.c_float), ("max_samples", C.c_int32), ("slots", C.c_int32), ("W", C.c_int32),
                ("wrap_mask", C.c_uint64), ("reserved", C.c_int64 * 2)]


class Graph(C.Structure):
    """ctypes mirror of dcx_graph (include/dcx.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("rowptr", "col", "weight")] + [("N", C.c_int64), ("nnz", C.c_int64), ("reserved", C.c_int64 * 2)]


class SsspState(C.Structure):
    """ctypes mirror of dcx_sssp_state (include/dcx.h)"""
    _fields_ = [("dist", C.c_void_p), ("pred", C.c_void_p), ("reserved", C.c_int64 * 2)]


class SsspLinks(C.Structure):
    """ctypes mirror of dcx_sssp_links (include/dcx.h)"""
    _fields_ = [("idx", C.c_void_p), ("len", C.c_void_p), ("reserved", C.c_int64 * 2)]


class LazyGraph(C.Structure):
    """ctypes mirror of dcx_lazy_graph (include/dcx.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("eid", "ent", "ends", "state")] + [("M", C.c_int64), ("reserved", C.c_int64 * 2)]


class MotionCostOpts(C.Structure):
    """ctypes mirror of dcx_motion_cost_opts (include/dcx.h)"""
    _fields_ = [("res", C.c_int32), ("max_step", C.c_float), ("max_samples", C.c_int32), ("open_end", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class TrajDenseOpts(C.Structure):
    """ctypes mirror of dcx_traj_dense_opts (include/dcx.h)"""
    _fields_ = [("max_step", C.c_float), ("max_samples", C.c_int32), ("wrap_mask", C.c_uint64), ("rewrap_mask", C.c_uint64),
                ("normalize", C.c_int32), ("stop_tol", C.c_float), ("reserved", C.c_int32 * 4)]


class TrajDenseIO(C.Structure):
    """ctypes mirror of dcx_traj_dense_io (include/dcx.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("move", "history", "n_checks", "edge_cost", "grad_a", "grad_b", "n_samples")]


_lib = None


class DcxError(RuntimeError):
    pass


class DcxUnsupported(DcxError):
    """DCX_ERR_UNSUPPORTED: the shape / kind is outside what the library is compiled for"""


def load():
    """Load libdcx.so (once) and bind every declared symbol.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DcxError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C diffco_amd/csrc -j8`.  diffco_amd has no CPU fallback for the score/grad path.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().dcx_last_error()
        raise (DcxUnsupported if rc == 2 else DcxError)(f"libdcx error {rc}: {msg.decode() if msg else '?'}")


_gpu_ok = False


def require_gpu():
    """the loaded library, after checking ONCE per process that a GPU is there (every op calls this: the check itself -
    torch.cuda.is_available + hipGetDeviceCount - cost 2 us of a 10 us call)"""
    global _gpu_ok
    if _gpu_ok:
        return _lib
    lib = load()
    if not torch.cuda.is_available() or lib.dcx_device_count() < 1:
        raise DcxError("diffco_amd: no MI355X/HIP device visible — the score/grad path is HIP-only "
                       "(there is deliberately no CPU fallback)")
    _gpu_ok = True
    return lib
