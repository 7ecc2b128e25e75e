"""diffco_amd — MI355X-native implementation of DiffCo's score(+gradient) hot path.

Same public surface as the reference package for that path (`diffco.kernel`, `diffco.model`,
`diffco.optim`, `diffco.utils`, `DiffCo`, `MultiDiffCo`, `DiffCoBeta`); the arithmetic runs in
hand-written HIP kernels for gfx950 behind the C ABI of include/dcx.h (libdcx.so).
Importing the package needs neither the library nor a GPU; calling a score/FK/kernel op does,
and raises loudly otherwise — there is no CPU fallback.
"""
from . import kernel, model, utils  # noqa: F401
from .kernel_perceptrons import DiffCo  # noqa: F401
from .deprecated import MultiDiffCo, DiffCoBeta  # noqa: F401
from . import deprecated  # noqa: F401
from . import optim  # noqa: F401
from . import sharded  # noqa: F401
from . import traj  # noqa: F401
from . import escape  # noqa: F401
from . import urdf  # noqa: F401
from .urdf import URDFRobotFK, MultiURDFRobotFK  # noqa: F401
from . import collision_checkers  # noqa: F401
from .collision_checkers import RBFDiffCo, ForwardKinematicsDiffCo, HybridForwardKinematicsDiffCo  # noqa: F401
from .traj import fused_adam_traj_optimize, optimize_paths  # noqa: F401
from . import roadmap  # noqa: F401
from .roadmap import Roadmap, knn, knn_edges  # noqa: F401
from . import rrt  # noqa: F401
from .rrt import rrt_connect, host_rrt_connect, RRTResult  # noqa: F401
from . import rrtstar  # noqa: F401
from .rrtstar import rrt_star, host_rrt_star, clearance_cost_paths, RRTStarResult  # noqa: F401
from . import shortcut  # noqa: F401
from .shortcut import shortcut_paths, host_shortcut_paths, ShortcutResult  # noqa: F401
from . import resample  # noqa: F401
from .resample import resample_paths, host_resample_paths, ResampleResult  # noqa: F401
from . import geometry  # noqa: F401
from .geometry import (World, RobotSpheres, SphereWorldChecker, host_clearance_points, spheres_on_control_points,  # noqa: F401
                       spheres_along_links)

__all__ = ["geometry", "World", "RobotSpheres", "SphereWorldChecker", "host_clearance_points", "spheres_on_control_points", "spheres_along_links", "resample", "resample_paths", "host_resample_paths", "ResampleResult", "optimize_paths", "shortcut", "shortcut_paths", "host_shortcut_paths", "ShortcutResult", "rrt","rrt_connect", "host_rrt_connect", "RRTResult", "rrtstar", "rrt_star", "host_rrt_star", "clearance_cost_paths", "RRTStarResult", "kernel", "model", "utils", "optim", "sharded", "traj", "escape", "fused_adam_traj_optimize", "roadmap", "Roadmap", "knn", "knn_edges", "urdf", "URDFRobotFK", "MultiURDFRobotFK", "collision_checkers", "RBFDiffCo", "ForwardKinematicsDiffCo", "HybridForwardKinematicsDiffCo", "deprecated", "DiffCo", "MultiDiffCo", "DiffCoBeta"]
