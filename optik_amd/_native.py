"""ctypes view of the kernel-layer C ABI (``include/optik_hip.h``) in ``liboptik_amd.so``.

The shared library is built in-tree by ``optik_amd.build`` (hipcc, gfx950).  There is
no CPU fallback anywhere in this package: if the library is missing, or no GPU is
usable, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import math
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "liboptik_amd.so")
# diagnostics only (tools/: tuning variants and -DOPTIK_PROFILE builds of the same sources)
if os.environ.get("OPTIK_AMD_LIB"):
    LIB_PATH = os.path.abspath(os.environ["OPTIK_AMD_LIB"])

MAX_DOF = 8
IK_EARLY_EXIT = 1
IK_FIND_ANY = 2
IK_RESTART_MAJOR = 4
UINT64_MAX = 0xFFFFFFFFFFFFFFFF

RES_FAILURE, RES_ROUNDOFF, RES_FORCED_STOP, RES_ITER_CAP = -1, -4, -5, -100
RES_STOPVAL, RES_FTOL, RES_XTOL = 2, 3, 4
# rand 0.9.2 random_range(lb..=ub) reading (include/optik_hip.h: OPTIK_HIP_RANGE_*)
RANGE_SINGLE_INCLUSIVE, RANGE_NEW_INCLUSIVE = 0, 1


class OptikHipError(RuntimeError):
    pass


class SolverConfigC(C.Structure):
    """CSolverConfig (optik-cpp/src/lib.rs:10-20), 96 bytes."""
    _fields_ = [
        ("solution_mode", C.c_int32),
        ("_pad", C.c_int32),
        ("max_time", C.c_double),
        ("max_restarts", C.c_uint64),
        ("tol_f", C.c_double),
        ("tol_df", C.c_double),
        ("tol_dx", C.c_double),
        ("linear_weight", C.c_double * 3),
        ("angular_weight", C.c_double * 3),
    ]


class IkOutputs(C.Structure):
    _fields_ = [
        ("d_x", C.c_void_p), ("d_f", C.c_void_p), ("d_status", C.c_void_p), ("d_evals", C.c_void_p),
        ("d_win_x", C.c_void_p), ("d_win_f", C.c_void_p), ("d_win_idx", C.c_void_p),
        ("d_win_key", C.c_void_p),
    ]


class IkSolutionsOutputs(C.Structure):
    """optik_hip_ik_solutions_outputs (include/optik_hip.h)."""
    _fields_ = [("d_count", C.c_void_p), ("d_x", C.c_void_p), ("d_f", C.c_void_p), ("d_idx", C.c_void_p),
                ("d_key", C.c_void_p)]


MAX_SOLUTIONS = 256  # OPTIK_HIP_MAX_SOLUTIONS
MAX_SOLUTION_RESTARTS = 1 << 22  # OPTIK_ROBOT_MAX_SOLUTION_RESTARTS


def check_solutions_args(k, min_dist):
    """The argument rules of optik_hip_ik_solutions, checked on the host: (k, min_dist) as int, float."""
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MAX_SOLUTIONS:
        raise ValueError(f"k must be an integer in 1..{MAX_SOLUTIONS}, got {k!r}")
    min_dist = float(min_dist)
    if not (min_dist >= 0.0 and min_dist != float("inf")):
        raise ValueError(f"min_dist must be finite and >= 0, got {min_dist!r}")
    return int(k), min_dist


class IkRegionOutputs(C.Structure):
    """optik_hip_ik_region_outputs (include/optik_hip.h)."""
    _fields_ = [("d_x", C.c_void_p), ("d_violation", C.c_void_p), ("d_status", C.c_void_p),
                ("d_iterations", C.c_void_p), ("d_key", C.c_void_p), ("d_count", C.c_void_p), ("d_sol_x", C.c_void_p),
                ("d_sol_violation", C.c_void_p), ("d_sol_idx", C.c_void_p), ("d_sol_key", C.c_void_p)]


REGION_DOUBLES = 19  # OPTIK_HIP_REGION_DOUBLES: ref[7], lo[6], hi[6]
REGION_RESTARTS = 256  # the default restarts of ik_region (the table)


def check_region_restarts(restarts):
    """The restart count of Robot.ik_region*: an integer in 1 .. MAX_SOLUTION_RESTARTS."""
    if isinstance(restarts, bool) or int(restarts) != restarts or not 1 <= int(restarts) <= MAX_SOLUTION_RESTARTS:
        raise ValueError(f"restarts must be an integer in 1..{MAX_SOLUTION_RESTARTS}, got {restarts!r}")
    return int(restarts)


class IkPathOutputs(C.Structure):
    """optik_hip_ik_path_outputs (include/optik_hip.h)."""
    _fields_ = [("d_x", C.c_void_p), ("d_f", C.c_void_p), ("d_idx", C.c_void_p), ("d_key", C.c_void_p),
                ("d_step", C.c_void_p), ("d_last", C.c_void_p)]


PATH_MAX_RESTARTS = 4096  # OPTIK_HIP_PATH_MAX_RESTARTS


def check_max_step(max_step):
    """The max_step rule of optik_hip_ik_path, checked on the host: >= 0, +inf for no limit; as float."""
    max_step = float(max_step)
    if not max_step >= 0.0:
        raise ValueError(f"max_step must be >= 0 (+inf: no limit), got {max_step!r}")
    return max_step


class LaunchInfo(C.Structure):
    _fields_ = [("grid", C.c_int32), ("block", C.c_int32), ("lds_bytes", C.c_int32),
                ("tiles", C.c_int32), ("kernel_ms", C.c_float)]


_lib = None


def lib():
    """Load liboptik_amd.so; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OptikHipError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950).  optik_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.optik_hip_device_count.restype = C.c_int
    L.optik_hip_set_option.argtypes = [C.c_char_p, C.c_longlong]
    L.optik_hip_get_option.argtypes = [C.c_char_p]
    L.optik_hip_get_option.restype = C.c_longlong
    L.optik_hip_last_error.restype = C.c_char_p
    L.optik_hip_chain_create.argtypes = [dp, dp, ip, C.c_int32, dp, dp, C.c_int32, C.POINTER(vp)]
    L.optik_hip_chain_destroy.argtypes = [vp]
    L.optik_hip_chain_num_positions.argtypes = [vp]
    L.optik_hip_chain_set_range_rule.argtypes = [vp, C.c_int32]
    L.optik_hip_chain_range_rule.argtypes = [vp]
    L.optik_hip_eval_batch.argtypes = [vp, C.POINTER(SolverConfigC), dp, dp, vp, C.c_int64, vp, vp, vp]
    L.optik_hip_fk_batch.argtypes = [vp, dp, vp, C.c_int64, vp, vp, vp]
    L.optik_hip_seed_batch.argtypes = [vp, C.c_uint64, C.c_int64, vp, vp]
    L.optik_hip_manip_batch.argtypes = [vp, dp, vp, C.c_int64, vp, vp, vp]
    ip = C.POINTER(C.c_int32)
    L.optik_hip_chain_set_collision_model.argtypes = [vp, ip, dp, dp, C.c_int32, ip, C.c_int32, C.c_double]
    L.optik_hip_chain_set_world.argtypes = [vp, dp, C.c_int32, dp, C.c_int32]
    L.optik_hip_chain_set_world_grid.argtypes = [vp, dp, C.c_double, C.c_int32, C.c_int32, C.c_int32, vp]
    L.optik_hip_world_grid_bake.argtypes = [vp, dp, C.c_double, C.c_int32, C.c_int32, C.c_int32, vp, vp]
    L.optik_hip_world_grid_from_occupancy.argtypes = [vp, C.c_double, C.c_int32, C.c_int32, C.c_int32, vp, C.c_double,
                                                      vp, vp]
    L.optik_hip_occupancy_from_points.argtypes = [vp, dp, C.c_double, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int64,
                                                  vp, C.c_int32, vp, vp]
    L.optik_hip_depth_integrate.argtypes = [vp, dp, C.c_double, C.c_int32, C.c_int32, C.c_int32, vp, vp, C.c_int32,
                                            C.c_int32, C.c_int32, dp, dp, vp, C.c_int32, C.c_double, C.c_double,
                                            C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp]
    L.optik_hip_occupancy_from_map.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32, C.c_int32,
                                               vp, vp]
    L.optik_hip_world_grid_from_mesh.argtypes = [vp, dp, C.c_double, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32,
                                                 C.c_double, vp, vp]
    L.optik_hip_mesh_tile.restype = C.c_int32
    L.optik_hip_mesh_pairs_per_launch.argtypes = [C.c_int64]
    L.optik_hip_mesh_pairs_per_launch.restype = C.c_int64
    L.optik_hip_sphere_fit.argtypes = [vp, dp, C.c_double, C.c_int32, C.c_int32, C.c_int32, vp, vp, C.c_int64, C.c_double,
                                       C.c_double, C.c_int32, vp, vp, vp, vp, vp, vp, C.c_int64, vp]
    L.optik_hip_sphere_fit_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64]
    L.optik_hip_sphere_fit_workspace_bytes.restype = C.c_int64
    L.optik_hip_fit_tile.restype = C.c_int32
    L.optik_hip_fit_pairs_per_launch.argtypes = [C.c_int64]
    L.optik_hip_fit_pairs_per_launch.restype = C.c_int64
    L.optik_hip_link_frames_batch.argtypes = [vp, dp, vp, C.c_int64, vp, vp]
    L.optik_hip_collision_batch.argtypes = [vp, dp, vp, C.c_int64, vp, vp, vp]
    L.optik_hip_collision_motion_batch.argtypes = [vp, dp, vp, vp, C.c_int64, C.c_double, vp, vp, vp, vp, vp]
    L.optik_hip_chain_set_motion_resolution.argtypes = [vp, C.c_double]
    L.optik_hip_collision_motion_certify_batch.argtypes = [vp, dp, vp, vp, C.c_int64, C.c_double, C.c_double,
                                                           C.c_int32, vp, vp, vp, vp, vp]
    L.optik_hip_constraint_batch.argtypes = [vp, dp, dp, dp, dp, vp, C.c_int64, vp, vp, vp]
    L.optik_hip_constraint_project_batch.argtypes = [vp, dp, dp, dp, dp, vp, C.c_int64, C.c_double, C.c_int32,
                                                     C.c_double, C.c_double, vp, vp, vp, vp, vp]
    L.optik_hip_constraint_motion_batch.argtypes = [vp, dp, dp, dp, dp, vp, vp, C.c_int64, C.c_double, C.c_double, vp,
                                                    vp, vp, vp, vp]
    L.optik_hip_diff_ik_batch.argtypes = [vp, dp, vp, vp, C.c_int64, vp, C.c_int64, C.c_int64, vp, vp, vp, vp]
    L.optik_hip_collision_witness_batch.argtypes = [vp, dp, vp, C.c_int64, vp, vp, vp, vp]
    L.optik_hip_diff_ik_avoid_batch.argtypes = [vp, dp, vp, vp, C.c_int64, vp, C.c_int64, C.c_int64, C.c_double,
                                                C.c_double, C.c_double, vp, vp, vp, vp]
    L.optik_hip_path_optimize.argtypes = [vp, dp, vp, C.c_int32, C.c_int64, C.c_int32, C.c_double, C.c_double,
                                          C.c_double, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp]
    L.optik_hip_path_optimize_constrained.argtypes = [vp, dp, vp, C.c_int32, C.c_int64, C.c_int32, C.c_double,
                                                      C.c_double, C.c_double, C.c_double, C.c_double, dp, dp, dp,
                                                      C.c_double, C.c_int32, C.c_double, C.c_double, vp, vp, vp, vp, vp,
                                                      vp, vp, vp]
    L.optik_hip_collision_repair_batch.argtypes = [vp, dp, vp, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_int32,
                                                   C.c_double, dp, dp, dp, C.c_double, C.c_int32, C.c_double,
                                                   C.c_double, vp, vp]
    L.optik_hip_roadmap_knn.argtypes = [vp, vp, C.c_int64, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp]
    L.optik_hip_roadmap_edges.argtypes = [vp, dp, vp, C.c_int64, vp, C.c_int32, vp, C.c_int32, C.c_double, C.c_int32,
                                          vp, vp]
    L.optik_hip_roadmap_query.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int64, vp, vp, C.c_int32,
                                          vp, vp, C.c_int32, vp, C.c_int32, vp, vp, vp, vp, vp]
    L.optik_hip_roadmap_query_route.argtypes = L.optik_hip_roadmap_query.argtypes[:-1] + [vp, vp, vp]
    L.optik_hip_roadmap_query_goals.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int64,
                                                vp, vp, C.c_int32, vp, vp, C.c_int32, vp, C.c_int32, vp, vp, vp, vp, vp,
                                                vp, vp, vp]
    L.optik_hip_roadmap_lazy_reset.argtypes = [vp, dp, vp, C.c_int32, vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp]
    query_args = [vp, vp, C.c_int64, vp, vp, C.c_int32, vp, vp, C.c_int32, vp, C.c_int32, C.c_int32, vp, vp, vp, vp,
                  C.POINTER(C.c_int32), C.POINTER(C.c_int64), vp]
    L.optik_hip_roadmap_lazy_plan.argtypes = [vp, dp, vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_double] + query_args
    L.optik_hip_roadmap_lazy_plan_from_flags.argtypes = [vp, vp, C.c_int32, vp, vp, vp, vp, C.c_int32, vp,
                                                         vp] + query_args
    goals_query_args = [vp, vp, vp, C.c_int32, C.c_int64, vp, vp, C.c_int32, vp, vp, C.c_int32, vp, C.c_int32, C.c_int32,
                        C.c_int32, vp, vp, vp, vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int64), vp]
    L.optik_hip_roadmap_lazy_plan_goals.argtypes = [vp, dp, vp, C.c_int32, vp, vp, vp, C.c_int32,
                                                    C.c_double] + goals_query_args
    L.optik_hip_roadmap_lazy_plan_goals_from_flags.argtypes = [vp, vp, C.c_int32, vp, vp, vp, vp, C.c_int32, vp,
                                                               vp] + goals_query_args
    L.optik_hip_rrt_plan.argtypes = [vp, dp, vp, vp, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_uint64, C.c_int32,
                                     C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp]
    L.optik_hip_rrt_plan_goals.argtypes = [vp, dp, vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                           C.c_uint64, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.optik_hip_rrt_plan_constrained.argtypes = [vp, dp, dp, dp, dp, C.c_double, C.c_double, C.c_int32, C.c_double,
                                                 C.c_double, vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, C.c_double,
                                                 C.c_double, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp,
                                                 vp, vp, vp, vp, vp]
    L.optik_hip_rrt_chunk.argtypes = [vp, C.c_int32]
    L.optik_hip_rrt_chunk.restype = C.c_int64
    # test hook: nearest and steer on the caller's own tree (include/optik_hip.h)
    L.optik_hip_rrt_nearest_from_nodes.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, C.c_int64, C.c_double, vp, vp, vp,
                                                   vp]
    L.optik_hip_path_shortcut.argtypes = [vp, dp, vp, vp, C.c_int32, C.c_int64, C.c_int32, C.c_double, C.c_double,
                                          C.c_int32, vp, vp, vp, vp, vp, vp]
    L.optik_hip_path_resample.argtypes = [vp, vp, vp, C.c_int32, C.c_int64, C.c_int32, vp, vp, vp]
    L.optik_hip_path_shortcut_chunk.argtypes = [vp, C.c_int32]
    L.optik_hip_path_shortcut_constrained.argtypes = [vp, dp, vp, vp, C.c_int32, C.c_int64, C.c_int32, C.c_double,
                                                      C.c_double, C.c_int32, dp, dp, dp, C.c_double, C.c_double,
                                                      C.c_int32, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp, vp]
    L.optik_hip_path_resample_constrained.argtypes = [vp, dp, vp, vp, C.c_int32, C.c_int64, C.c_int32, dp, dp, dp,
                                                      C.c_double, C.c_int32, C.c_double, C.c_double, vp, vp, vp, vp]
    L.optik_hip_constraint_motion_mask.argtypes = [vp, dp, dp, dp, dp, vp, vp, C.c_int64, C.c_double, C.c_double, vp, vp]
    L.optik_hip_path_shortcut_constrained_chunk.argtypes = [vp, C.c_int32]
    L.optik_hip_path_shortcut_constrained_chunk.restype = C.c_int64
    L.optik_hip_path_time.argtypes = [vp, vp, vp, C.c_int32, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.optik_hip_trajectory_sample.argtypes = [vp, vp, vp, C.c_int32, C.c_int64, vp, vp, vp, C.c_double, C.c_int32, vp,
                                              vp, vp]
    L.optik_hip_path_time_tool.argtypes = [vp, vp, vp, C.c_int32, C.c_int64, vp, vp, dp, dp, vp, vp, vp, vp, vp, vp,
                                           vp, vp, vp, vp]
    L.optik_hip_path_time_spline.argtypes = [vp, vp, vp, C.c_int32, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                             vp, vp, vp]
    L.optik_hip_path_shortcut_chunk.restype = C.c_int64
    L.optik_hip_ik_batch.argtypes = [vp, C.POINTER(SolverConfigC), vp, vp, C.c_int32, dp,
                                     C.c_uint64, C.c_uint64, C.c_uint32, C.c_double,
                                     C.POINTER(IkOutputs), vp]
    L.optik_hip_ik_solutions.argtypes = [vp, C.POINTER(SolverConfigC), vp, vp, C.c_int32, dp, C.c_uint64,
                                         C.c_uint64, C.c_double, C.c_int32, C.c_double,
                                         C.POINTER(IkSolutionsOutputs), vp]
    L.optik_hip_ik_path.argtypes = [vp, C.POINTER(SolverConfigC), vp, vp, C.c_int32, C.c_int32, dp, C.c_uint64,
                                    C.c_uint64, C.c_uint32, C.c_double, C.c_double, C.POINTER(IkPathOutputs), vp]
    L.optik_hip_ik_region.argtypes = [vp, dp, vp, vp, C.c_int32, C.c_uint64, C.c_uint64, C.c_double, C.c_int32,
                                      C.c_double, C.c_double, C.c_int32, dp, dp, dp, C.c_double, C.c_int32, C.c_double,
                                      C.POINTER(IkRegionOutputs), vp]
    L.optik_hip_ik_region_repair.argtypes = [vp, dp, vp, vp, C.c_int32, C.c_uint64, C.c_uint64, C.c_double, C.c_int32,
                                             C.c_double, C.c_double, C.c_int32, dp, dp, dp, C.c_double, C.c_int32,
                                             C.c_double, vp, C.POINTER(IkRegionOutputs), vp]
    # test hooks: the selection stages on the caller's own keys (include/optik_hip.h)
    L.optik_hip_select_from_keys.argtypes = [vp, vp, vp, vp, C.c_int32, C.c_uint64, C.c_uint64, C.POINTER(IkOutputs), vp]
    L.optik_hip_solutions_from_keys.argtypes = [vp, vp, vp, vp, C.c_int32, C.c_uint64, C.c_uint64, C.c_int32,
                                                C.c_double, C.POINTER(IkSolutionsOutputs), vp]
    L.optik_hip_path_select_from_keys.argtypes = [vp, vp, vp, vp, vp, C.c_int32, C.c_uint64, C.c_uint64, C.c_double,
                                                  C.POINTER(IkPathOutputs), vp, vp]
    L.optik_hip_ik_host.argtypes = [vp, C.POINTER(SolverConfigC), dp, dp, C.c_int32, dp,
                                    C.c_uint64, C.c_uint64, C.c_uint32, C.c_double, dp, dp,
                                    C.POINTER(C.c_uint64), dp]
    L.optik_hip_probe.argtypes = [C.c_int32, dp, dp, C.c_int64, dp]
    L.optik_hip_probe_math.argtypes = [C.c_int32, dp, C.c_int64, dp]
    L.optik_hip_set_timing.argtypes = [vp, C.c_int32]
    L.optik_hip_last_launch.argtypes = [vp, C.POINTER(LaunchInfo)]
    L.optik_hip_timing_mean.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    _lib = L
    return L


MAX_MOTION_STEPS = 4096  # include/optik_hip.h: OPTIK_HIP_MAX_MOTION_STEPS


def check_resolution(h, allow_zero=False):
    """The resolution of a motion check as a float: finite and > 0 (allow_zero: 0 switches the ik_path pass off)."""
    h = float(h)
    if not (math.isfinite(h) and (h > 0.0 or (allow_zero and h == 0.0))):
        raise ValueError("motion resolution must be finite and " + (">= 0" if allow_zero else "> 0") + f", got {h}")
    return h


# include/optik_hip.h: OPTIK_HIP_CONSTRAINT_*; the statuses and defaults of optik_hip_constraint_project_batch
CONSTRAINT_PROJECTED, CONSTRAINT_BUDGET, CONSTRAINT_FAILED = 0, 1, 2
CONSTRAINT_MAX_ITERS = 4096
CONSTRAINT_ITERS, CONSTRAINT_DAMPING, CONSTRAINT_MAX_STEP = 256, 1e-6, 0.5  # (the table)
CONSTRAINT_TOL = 1e-6  # the default tol of the projection and the checks above it


def check_constraint_tol(tol):
    tol = float(tol)
    if not (math.isfinite(tol) and tol >= 0.0):
        raise ValueError(f"pose constraint: tol must be finite and >= 0, got {tol}")
    return tol


def check_project_args(tol, iters, damping, max_step):
    tol, iters, damping, max_step = check_constraint_tol(tol), int(iters), float(damping), float(max_step)
    if not 0 <= iters <= CONSTRAINT_MAX_ITERS:
        raise ValueError(f"pose constraint: iters must be 0 .. {CONSTRAINT_MAX_ITERS}, got {iters}")
    if not (math.isfinite(damping) and damping >= 0.0 and math.isfinite(max_step) and max_step > 0.0):
        raise ValueError("pose constraint: needs damping >= 0 and max_step > 0, both finite")
    return tol, iters, damping, max_step


# include/optik_hip.h: OPTIK_HIP_CERTIFY_*; the statuses of optik_hip_collision_motion_certify_batch
CERTIFY_FREE, CERTIFY_BLOCKED, CERTIFY_LIMIT, CERTIFY_NAN = 0, 1, 2, 3
CERTIFY_MAX_STEPS = 65536
CERTIFY_STEPS = 4096  # the default max_steps: tol = lam_max / 4000 on a segment that stays free
CERTIFY_GRID_LIPSCHITZ = math.sqrt(3.0)  # valid for every true distance field (csrc/advance_measure.hpp)


def check_certify_args(tol, grid_lipschitz=None, max_steps=CERTIFY_STEPS):
    """The argument rules of optik_hip_collision_motion_certify_batch, checked on the host: (tol, grid_lipschitz,
    max_steps) as float, float, int; grid_lipschitz None is sqrt(3)."""
    tol = float(tol)
    if not (math.isfinite(tol) and tol > 0.0):
        raise ValueError(f"tol must be finite and > 0, got {tol!r}")
    G = CERTIFY_GRID_LIPSCHITZ if grid_lipschitz is None else float(grid_lipschitz)
    if not (math.isfinite(G) and G > 0.0):
        raise ValueError(f"grid_lipschitz must be finite and > 0, got {grid_lipschitz!r}")
    if isinstance(max_steps, bool) or int(max_steps) != max_steps or not 2 <= int(max_steps) <= CERTIFY_MAX_STEPS:
        raise ValueError(f"max_steps must be an integer in 2 .. {CERTIFY_MAX_STEPS}, got {max_steps!r}")
    return tol, G, int(max_steps)


MAX_MESH_TRIANGLES = 1 << 20  # include/optik_hip.h: OPTIK_HIP_MAX_MESH_TRIANGLES


def mesh_tile():
    """MESH_TILE of csrc/mesh_measure.hpp: the triangles optik_hip_world_grid_from_mesh stages in LDS at a time."""
    return int(lib().optik_hip_mesh_tile())


class mesh_pairs_per_launch:
    """``with mesh_pairs_per_launch(pairs): ...`` -- a test hook (include/optik_hip.h: optik_hip_mesh_pairs_per_launch):
    within the block optik_hip_world_grid_from_mesh splits its nodes into launches of at most `pairs` (node, triangle)
    pairs each instead of MESH_PAIRS_PER_LAUNCH; restored after it.  No result depends on it."""

    def __init__(self, pairs):
        self.pairs = int(pairs)
        if self.pairs < 1:
            raise ValueError("pairs must be >= 1")

    def __enter__(self):
        self.prev = int(lib().optik_hip_mesh_pairs_per_launch(-1))
        lib().optik_hip_mesh_pairs_per_launch(self.pairs)
        return self

    def __exit__(self, *exc):
        lib().optik_hip_mesh_pairs_per_launch(self.prev)
        return False


MAX_FIT_SPHERES = 256     # include/optik_hip.h: OPTIK_HIP_MAX_FIT_SPHERES
MAX_FIT_POINTS = 1 << 20  # include/optik_hip.h: OPTIK_HIP_MAX_FIT_POINTS


def fit_tile():
    """FIT_TILE of csrc/spherefit_measure.hpp: the points optik_hip_sphere_fit stages in LDS at a time."""
    return int(lib().optik_hip_fit_tile())


class fit_pairs_per_launch:
    """``with fit_pairs_per_launch(pairs): ...`` -- a test hook (include/optik_hip.h: optik_hip_fit_pairs_per_launch):
    within the block optik_hip_sphere_fit cuts its candidates into launches of at most `pairs` (candidate, point) pair
    tests each instead of FIT_PAIRS_PER_LAUNCH; restored after it.  No result depends on it."""

    def __init__(self, pairs):
        self.pairs = int(pairs)
        if self.pairs < 1:
            raise ValueError("pairs must be >= 1")

    def __enter__(self):
        self.prev = int(lib().optik_hip_fit_pairs_per_launch(-1))
        lib().optik_hip_fit_pairs_per_launch(self.pairs)
        return self

    def __exit__(self, *exc):
        lib().optik_hip_fit_pairs_per_launch(self.prev)
        return False


PATH_OPTIMIZE_MAX_WAYPOINTS = 64  # include/optik_hip.h: OPTIK_HIP_PATH_OPTIMIZE_MAX_WAYPOINTS
# The values with which the host reference (csrc/path_optimize.hpp under g++) clears the L = 16 scene of
# tests/test_path_optimize_host.py: that and nothing more.
PATH_OPTIMIZE_ITERS, PATH_OPTIMIZE_STEP, PATH_OPTIMIZE_W_SMOOTH, PATH_OPTIMIZE_W_OBS = 100, 0.05, 1.0, 1.0


# include/optik_hip.h: OPTIK_HIP_REPAIR_MAX_ITERS and the statuses of optik_hip_collision_repair_batch
REPAIR_MAX_ITERS = 4096
REPAIR_FREE, REPAIR_LIMIT, REPAIR_STUCK, REPAIR_NAN = 0, 1, 2, 3
# The values with which the host reference (csrc/repair_measure.hpp) clears the scene of examples/ik_repair.py: its
# start state in 2 steps and 9 in 10 of the colliding configurations of its cell (177 steps at the 90th percentile);
# a quarter of the budget frees fewer than half of them (tests/test_repair_host.py asserts both).  That and nothing more.
REPAIR_STEP, REPAIR_ITERS = 0.05, 256


class RepairOutputs(C.Structure):
    """optik_hip_collision_repair_outputs (include/optik_hip.h)."""
    _fields_ = [(k, C.c_void_p) for k in ("d_x", "d_clearance", "d_violation", "d_moved", "d_status", "d_iterations")]


class RegionRepair(C.Structure):
    """optik_hip_region_repair (include/optik_hip.h)."""
    _fields_ = [("influence", C.c_double), ("safety", C.c_double), ("step", C.c_double), ("max_move", C.c_double),
                ("iters", C.c_int32), ("d_repaired", C.c_void_p)]


def region_repair_args(repair):
    """ik_region's repair=dict(influence, safety, step=REPAIR_STEP, iters=REPAIR_ITERS, max_move=inf), checked:
    (influence, safety, step, iters, max_move).  ValueError for another key, a missing one or a bad value."""
    if not isinstance(repair, dict) or set(repair) - {"influence", "safety", "step", "iters", "max_move"} \
            or not {"influence", "safety"} <= set(repair):
        raise ValueError("repair must be a dict with influence and safety, and optionally step, iters and max_move")
    return check_repair_args(repair["influence"], repair["safety"], repair.get("step", REPAIR_STEP),
                             repair.get("iters", REPAIR_ITERS), repair.get("max_move", math.inf))


def check_repair_args(influence, safety, step, iters, max_move):
    """The argument rules of optik_hip_collision_repair_batch, checked on the host."""
    if isinstance(iters, bool) or int(iters) != iters or not 0 <= int(iters) <= REPAIR_MAX_ITERS:
        raise ValueError(f"iters must be an integer in 0 .. {REPAIR_MAX_ITERS}, got {iters!r}")
    influence, safety, step, max_move = float(influence), float(safety), float(step), float(max_move)
    if not (math.isfinite(influence) and math.isfinite(step) and influence > safety >= 0.0 and step > 0.0):
        raise ValueError("collision_repair: needs influence > safety >= 0 and step > 0, all finite")
    if not max_move >= 0.0:
        raise ValueError(f"max_move must be >= 0 (inf: no bound), got {max_move!r}")
    return influence, safety, step, int(iters), max_move


def check_path_optimize_args(L, iters, step, w_smooth, w_obs, influence, safety):
    """The argument rules of optik_hip_path_optimize, checked on the host."""
    if not 3 <= int(L) <= PATH_OPTIMIZE_MAX_WAYPOINTS:
        raise ValueError(f"a path has 3 .. {PATH_OPTIMIZE_MAX_WAYPOINTS} waypoints, got {L}")
    if isinstance(iters, bool) or int(iters) != iters or int(iters) < 0 or int(iters) >= 1 << 31:
        raise ValueError(f"iters must be an integer >= 0, got {iters!r}")
    vals = [float(v) for v in (step, w_smooth, w_obs, influence, safety)]
    if not (all(math.isfinite(v) for v in vals) and vals[0] > 0.0 and vals[1] >= 0.0 and vals[2] >= 0.0
            and vals[3] > vals[4] >= 0.0):
        raise ValueError("path_optimize: needs step > 0, w_smooth >= 0, w_obs >= 0 and influence > safety >= 0, "
                         "all finite")


# include/optik_hip.h: OPTIK_HIP_ROADMAP_MAX_NODES, OPTIK_HIP_ROADMAP_MAX_K; the statuses of optik_hip_roadmap_query
ROADMAP_MAX_NODES, ROADMAP_MAX_K = 8192, 16
ROADMAP_FOUND, ROADMAP_NO_ROUTE, ROADMAP_TOO_LONG, ROADMAP_NAN = 0, 1, 2, 3
# The values with which Robot.build_roadmap / plan_paths plan the wall scene of examples/plan_path.py on a Panda: that
# and nothing more.
ROADMAP_NODES, ROADMAP_K, ROADMAP_RESOLUTION = 512, 8, 0.05
# include/optik_hip.h: OPTIK_HIP_ROADMAP_UNKNOWN .. _BLOCKED, the verdicts of a lazy roadmap's slots; the one more
# status of optik_hip_roadmap_lazy_plan; OPTIK_HIP_ROADMAP_LAZY_MAX_ROUNDS
ROADMAP_SLOT_UNKNOWN, ROADMAP_SLOT_FREE, ROADMAP_SLOT_BLOCKED = 0, 1, 2
ROADMAP_UNSETTLED = 4
ROADMAP_LAZY_MAX_ROUNDS = 4096
# Twice the larger number of rounds that the wall scene of the tests and the scene of examples/plan_lazy.py took on
# a Panda, rounded up to a power of two (DESIGN.md section 5.24 has the two figures): that and nothing more.
ROADMAP_LAZY_ROUNDS = 8


# include/optik_hip.h: OPTIK_HIP_ROADMAP_MAX_GOALS, the goal slots of a goal-set query
ROADMAP_MAX_GOALS = 16


def check_roadmap_goals(G):
    """The number of goal slots of a goal-set plan as an int: an integer in 1 .. ROADMAP_MAX_GOALS."""
    if isinstance(G, bool) or int(G) != G or not 1 <= int(G) <= ROADMAP_MAX_GOALS:
        raise ValueError(f"a goal set has 1 .. {ROADMAP_MAX_GOALS} goals per query, got {G!r}")
    return int(G)


def check_lazy_rounds(rounds):
    """`rounds` of a lazy plan as an int: None is ROADMAP_LAZY_ROUNDS; an integer in 0 .. 4096."""
    if rounds is None:
        return ROADMAP_LAZY_ROUNDS
    if isinstance(rounds, bool) or int(rounds) != rounds or not 0 <= int(rounds) <= ROADMAP_LAZY_MAX_ROUNDS:
        raise ValueError(f"rounds must be an integer in 0 .. {ROADMAP_LAZY_MAX_ROUNDS}, got {rounds!r}")
    return int(rounds)


def check_roadmap_args(N=1, k=1, max_waypoints=2):
    """The argument rules of the roadmap entry points, checked on the host."""
    for name, v, lo, hi in (("N", N, 1, ROADMAP_MAX_NODES), ("k", k, 1, ROADMAP_MAX_K),
                            ("max_waypoints", max_waypoints, 2, PATH_OPTIMIZE_MAX_WAYPOINTS)):
        if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
            raise ValueError(f"{name} must be an integer in {lo} .. {hi}, got {v!r}")


# include/optik_hip.h: OPTIK_HIP_RRT_MAX_ITERS, _MAX_NODES, _MAX_POLL; the statuses of optik_hip_rrt_plan are the
# roadmap query's (ROADMAP_FOUND .. ROADMAP_NAN)
RRT_MAX_ITERS, RRT_MIN_NODES, RRT_MAX_NODES, RRT_MAX_POLL = 65536, 2, 4096, 65536
# The values with which Robot.plan_rrt plans the pair of examples/plan_rrt.py on a Panda, a route the example's small
# roadmap misses -- the serial reference joins the trees there after 33 iterations with 17 and 15 nodes, and the
# budgets are the next powers of two times four: that and nothing more.
RRT_ITERS, RRT_STEP, RRT_NODES, RRT_POLL = 256, 0.5, 256, 32


def check_rrt_args(iters=1, step=1.0, max_nodes=2, max_waypoints=2, poll=1, first=0):
    """The argument rules of optik_hip_rrt_plan, checked on the host; returns (iters, step, max_nodes, poll, first)
    with None replaced by RRT_ITERS, RRT_STEP, RRT_NODES and RRT_POLL."""
    iters = RRT_ITERS if iters is None else iters
    max_nodes = RRT_NODES if max_nodes is None else max_nodes
    poll = RRT_POLL if poll is None else poll
    for name, v, lo, hi in (("iters", iters, 1, RRT_MAX_ITERS), ("max_nodes", max_nodes, RRT_MIN_NODES, RRT_MAX_NODES),
                            ("max_waypoints", max_waypoints, 2, PATH_OPTIMIZE_MAX_WAYPOINTS),
                            ("poll", poll, 1, RRT_MAX_POLL), ("first", first, 0, (1 << 64) - 1)):
        if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
            raise ValueError(f"{name} must be an integer in {lo} .. {hi}, got {v!r}")
    step = RRT_STEP if step is None else float(step)
    if not (math.isfinite(step) and step > 0.0):
        raise ValueError(f"step must be finite and > 0, got {step!r}")
    return int(iters), step, int(max_nodes), int(poll), int(first)


# include/optik_hip.h: OPTIK_HIP_RRT_MAX_GOALS, the goal slots of optik_hip_rrt_plan_goals
RRT_MAX_GOALS = 16


def check_rrt_goals(G, max_nodes):
    """The goal slots of a tree plan with a goal set as an int: an integer in 1 .. RRT_MAX_GOALS, and no more than
    max_nodes (already checked by check_rrt_args), since every goal may be a root of tree 1."""
    if isinstance(G, bool) or int(G) != G or not 1 <= int(G) <= RRT_MAX_GOALS:
        raise ValueError(f"a goal set has 1 .. {RRT_MAX_GOALS} goals per query, got {G!r}")
    if max_nodes < int(G):
        raise ValueError(f"max_nodes must be an integer in max(2, G) = {max(2, int(G))} .. {RRT_MAX_NODES}, "
                         f"got {max_nodes!r}")
    return int(G)


# include/optik_hip.h: OPTIK_HIP_RRT_PROJECT_ITERS, the default budget of a projection inside the constrained tree
# planner's extension (the table, and nothing more)
RRT_PROJECT_ITERS = 16


def rrt_chunk(chain_handle, max_nodes):
    """The queries optik_hip_rrt_plan processes per chunk of its workspace for this chain and tree size."""
    c = int(lib().optik_hip_rrt_chunk(chain_handle, int(max_nodes)))
    if c < 1:
        raise ValueError(f"max_nodes must be an integer in {RRT_MIN_NODES} .. {RRT_MAX_NODES}, got {max_nodes!r}")
    return c


# include/optik_hip.h: OPTIK_HIP_PATH_SHORTCUT_MAX_VERTICES; the statuses of optik_hip_path_shortcut / _path_resample
PATH_SHORTCUT_MAX_VERTICES = 64
SHORTCUT_FOUND, SHORTCUT_NO_ROUTE, SHORTCUT_BAD_LENGTH, SHORTCUT_NAN = 0, 1, 2, 3
# OPTIK_HIP_PATH_RESAMPLE_UNPROJECTED: optik_hip_path_resample_constrained left an interior waypoint as interpolated
RESAMPLE_UNPROJECTED = 4
# All-pairs visibility samples about V^2 / 6 times the path's own length: 32 vertices cost a quarter of 64
# (profiles/shortcut_cost.txt).
SHORTCUT_VERTICES, SHORTCUT_RESOLUTION, RESAMPLE_WAYPOINTS = 32, 0.05, 32


def check_shortcut_args(L=2, vertices=2, max_waypoints=2, resolution=1.0, hop_penalty=0.0):
    """The argument rules of optik_hip_path_shortcut and optik_hip_path_resample, checked on the host; returns
    (resolution, hop_penalty) as floats, hop_penalty None meaning the resolution: a length difference below what the
    check samples is not one the check can see."""
    for name, v in (("L", L), ("vertices", vertices), ("max_waypoints", max_waypoints)):
        if isinstance(v, bool) or int(v) != v or not 2 <= int(v) <= PATH_SHORTCUT_MAX_VERTICES:
            raise ValueError(f"{name} must be an integer in 2 .. {PATH_SHORTCUT_MAX_VERTICES}, got {v!r}")
    h = check_resolution(resolution)
    hop = h if hop_penalty is None else float(hop_penalty)
    if not (math.isfinite(hop) and hop >= 0.0):
        raise ValueError(f"hop_penalty must be finite and >= 0, got {hop_penalty!r}")
    return h, hop


def path_shortcut_chunk(chain_handle, vertices):
    """The paths optik_hip_path_shortcut processes per chunk of its workspace for this chain and vertex budget."""
    c = int(lib().optik_hip_path_shortcut_chunk(chain_handle, int(vertices)))
    if c < 1:
        check(c)
    return c


def path_shortcut_constrained_chunk(chain_handle, vertices):
    """The paths optik_hip_path_shortcut_constrained processes per chunk of its workspace for this chain and vertex
    budget."""
    c = int(lib().optik_hip_path_shortcut_constrained_chunk(chain_handle, int(vertices)))
    if c < 1:
        check(c)
    return c


# include/optik_hip.h: OPTIK_HIP_PATH_TIME_MAX_WAYPOINTS, OPTIK_HIP_TRAJECTORY_MAX_SAMPLES; optik_hip_path_time's statuses
PATH_TIME_MIN_WAYPOINTS, PATH_TIME_MAX_WAYPOINTS, TRAJECTORY_MAX_SAMPLES = 3, 64, 65536
TIME_TIMED, TIME_STALLED, TIME_BAD_LENGTH, TIME_NAN = 0, 1, 2, 3


def check_time_args(n, L=3, a_max=1.0, v_max=math.inf, scale=1.0):
    """The argument rules of optik_hip_path_time, checked on the host; returns (v_max [n], a_max [n]) as float64
    arrays, each a scalar or n values, both multiplied by `scale` in (0, 1].  a_max must be finite and > 0, v_max > 0
    (+inf: no velocity limit)."""
    import numpy as np
    if isinstance(L, bool) or int(L) != L or not PATH_TIME_MIN_WAYPOINTS <= int(L) <= PATH_TIME_MAX_WAYPOINTS:
        raise ValueError(f"L must be an integer in {PATH_TIME_MIN_WAYPOINTS} .. {PATH_TIME_MAX_WAYPOINTS}, got {L!r}")
    scale = float(scale)
    if not 0.0 < scale <= 1.0:
        raise ValueError(f"scale must be in (0, 1], got {scale!r}")
    out = []
    for name, v in (("v_max", v_max), ("a_max", a_max)):
        a = np.asarray(v, dtype=np.float64)
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != n):
            raise ValueError(f"{name} must be a scalar or [n] with n = {n}, got shape {list(a.shape)}")
        out.append(np.ascontiguousarray(np.broadcast_to(a, (n,))) * scale)
    v, a = out
    if not np.all(v > 0.0):
        raise ValueError(f"v_max must be > 0 (inf: no limit), got {v_max!r}")
    if not np.all(np.isfinite(a) & (a > 0.0)):
        raise ValueError(f"a_max must be finite and > 0, got {a_max!r}")
    return v, a


def check_time_tool_args(tool_v_max=math.inf, tool_a_tangential=math.inf, tool_a_normal=math.inf,
                         tool_w_max=math.inf, scale=1.0):
    """The tool limits of optik_hip_path_time_tool, checked on the host; returns them as a float64 array of 4 in the
    order the entry takes them.  Each is a number > 0 (+inf: no limit).  `scale` in (0, 1] multiplies the velocity-like
    ones (the speed, the angular speed) as it multiplies v_max and the acceleration-like ones (tangential, normal) as
    it multiplies a_max."""
    import numpy as np
    scale = float(scale)
    if not 0.0 < scale <= 1.0:
        raise ValueError(f"scale must be in (0, 1], got {scale!r}")
    out = np.empty(4, dtype=np.float64)
    for i, (name, v) in enumerate((("tool_v_max", tool_v_max), ("tool_a_tangential", tool_a_tangential),
                                   ("tool_a_normal", tool_a_normal), ("tool_w_max", tool_w_max))):
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a number, got {v!r}") from None
        if not v > 0.0:
            raise ValueError(f"{name} must be > 0 (inf: no limit), got {v!r}")
        out[i] = v * scale
    return out


# optik_hip_path_time_spline's statuses (csrc/time_spline_measure.hpp)
SPLINE_SMOOTH, SPLINE_BAD_TIMES, SPLINE_BAD_LENGTH, SPLINE_NOT_FINITE, SPLINE_OVER_LIMIT = 0, 1, 2, 3, 4


def check_time_spline_args(n, L=3, j_max=math.inf, a_max=math.inf, v_max=math.inf):
    """The argument rules of optik_hip_path_time_spline, checked on the host; returns (v_max [n], a_max [n], j_max [n])
    as float64 arrays, each a scalar or n values.  Every limit must be > 0; +inf means "no limit" (for a_max too, unlike
    optik_hip_path_time's, which needs one to bound the profile)."""
    import numpy as np
    if isinstance(L, bool) or int(L) != L or not PATH_TIME_MIN_WAYPOINTS <= int(L) <= PATH_TIME_MAX_WAYPOINTS:
        raise ValueError(f"L must be an integer in {PATH_TIME_MIN_WAYPOINTS} .. {PATH_TIME_MAX_WAYPOINTS}, got {L!r}")
    out = []
    for name, v in (("v_max", v_max), ("a_max", a_max), ("j_max", j_max)):
        try:
            a = np.asarray(v, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a number or [n] numbers, got {v!r}") from None
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != n):
            raise ValueError(f"{name} must be a scalar or [n] with n = {n}, got shape {list(a.shape)}")
        a = np.ascontiguousarray(np.broadcast_to(a, (n,)))
        if not np.all(a > 0.0):
            raise ValueError(f"{name} must be > 0 (inf: no limit), got {v!r}")
        out.append(a.copy())
    return tuple(out)


def check_sample_args(dt, T=1):
    """The argument rules of optik_hip_trajectory_sample; returns dt as a float."""
    dt = float(dt)
    if not (math.isfinite(dt) and dt > 0.0):
        raise ValueError(f"dt must be finite and > 0, got {dt!r}")
    if isinstance(T, bool) or int(T) != T or not 1 <= int(T) <= TRAJECTORY_MAX_SAMPLES:
        raise ValueError(f"a trajectory has 1 .. {TRAJECTORY_MAX_SAMPLES} samples, got {T!r}: raise dt")
    return dt


def check(rc: int):
    if rc != 0:
        msg = lib().optik_hip_last_error()
        raise OptikHipError(f"optik_hip error {rc}: {msg.decode() if msg else '?'}")


# optik_solver_config.solution_mode (include/optik_hip.h: OPTIK_MODE_*).  quality and speed are the reference's;
# manipulability and condition rank the successes by -w / -c of their body Jacobian (csrc/manip_measure.hpp)
SOLUTION_MODES = {"quality": 1, "speed": 2, "manipulability": 3, "condition": 4}
MEASURE_MODES = ("manipulability", "condition")


def solution_mode_code(solution_mode):
    """The OPTIK_MODE_* value of a mode name; ValueError for anything else."""
    if not isinstance(solution_mode, str) or solution_mode not in SOLUTION_MODES:
        raise ValueError("solution_mode must be one of " + ", ".join(repr(m) for m in SOLUTION_MODES)
                         + f", got {solution_mode!r}")
    return SOLUTION_MODES[solution_mode]


def make_config(solution_mode="speed", max_time=0.0, max_restarts=0, tol_f=1e-6, tol_df=-1.0,
                tol_dx=-1.0, linear_weight=(1.0, 1.0, 1.0), angular_weight=(1.0, 1.0, 1.0)):
    cfg = SolverConfigC()
    cfg.solution_mode = solution_mode_code(solution_mode)
    cfg.max_time = float(max_time)
    cfg.max_restarts = int(max_restarts)
    cfg.tol_f, cfg.tol_df, cfg.tol_dx = float(tol_f), float(tol_df), float(tol_dx)
    cfg.linear_weight[:] = [float(v) for v in linear_weight]
    cfg.angular_weight[:] = [float(v) for v in angular_weight]
    return cfg


SOLVE_KERNELS = {"auto": 0, "quad": 1, "lane64": 2, "general": 3}
WIDE_FORMS = {"lds": 0, "hbm": 1}


def set_option(name, value):
    """Tuning option of the kernel layer (include/optik_hip.h: optik_hip_set_option) -- tests and tools.  `value`: an
    integer, or for solve_kernel / wide_form one of their names."""
    if isinstance(value, str):
        value = {"solve_kernel": SOLVE_KERNELS, "wide_form": WIDE_FORMS}[name][value]
    check(lib().optik_hip_set_option(name.encode(), int(value)))


def get_option(name):
    return int(lib().optik_hip_get_option(name.encode()))


class options:
    """``with options(solve_kernel="lane64"): ...`` -- set for the block, restored after it.  The names are those of
    optik_hip_set_option: solve_kernel, wide_form, range_rule, stop_x_legacy and grid_cap -- a test hook,
    ``options(grid_cap=1)`` launches every grid-stride kernel with at most one block (0: the device's own cap), so
    that a few hundred rows take the later trips of its loop; no result depends on it."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.prev = {k: get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            set_option(k, v)
        return False
