"""Python front end with the surface of the reference's `optik` module
(/root/reference/optik.pyi:9-49; implementation crates/optik-py/src/lib.rs:17-155),
bound with ctypes to the `optik_robot_*` C ABI of liboptik_amd.so (include/optik.h).

Poses are 4x4 homogeneous matrices given as nested lists / arrays in row-major
order (optik-py/src/lib.rs:8-15); results come back as Python lists, as in the
reference (`diff_ik` included: a small LP solved exactly on the host).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as nat
from .constraint import checked_constraint_arrays, constraint_arrays

U64_MAX = 0xFFFFFFFFFFFFFFFF


def _bind(L):
    if getattr(L, "_robot_bound", False):
        return L
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    L.optik_robot_try_from_urdf_str.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(vp)]
    L.optik_robot_last_error.restype = C.c_char_p
    L.optik_robot_free.argtypes = [vp]
    L.optik_robot_set_parallelism.argtypes = [vp, C.c_uint]
    L.optik_robot_num_positions.argtypes = [vp]
    L.optik_robot_num_positions.restype = C.c_uint
    L.optik_robot_ik_ex.argtypes = [vp, C.POINTER(nat.SolverConfigC), dp, dp, dp, dp, dp,
                                    C.POINTER(C.c_uint64)]
    L.optik_robot_ik_batch_ex.argtypes = [vp, C.POINTER(nat.SolverConfigC), C.c_int32, dp, dp, dp, dp, dp,
                                          C.POINTER(C.c_int32)]
    L.optik_robot_ik_batch_poses.argtypes = [vp, C.POINTER(nat.SolverConfigC), C.c_int32, dp, C.c_uint32, dp, dp,
                                             dp, dp, C.POINTER(C.c_int32)]
    L.optik_robot_ik_solutions.argtypes = [vp, C.POINTER(nat.SolverConfigC), C.c_int32, dp, C.c_uint32, dp, dp,
                                           C.c_int32, C.c_double, C.POINTER(C.c_int32), dp, dp,
                                           C.POINTER(C.c_uint64)]
    L.optik_robot_ik_path.argtypes = [vp, C.POINTER(nat.SolverConfigC), C.c_int32, C.c_int32, dp, C.c_uint32, dp, dp,
                                      C.c_double, dp, dp, C.POINTER(C.c_uint64), dp, C.POINTER(C.c_int32)]
    L.optik_robot_manipulability_batch.argtypes = [vp, C.c_int64, dp, dp, dp, dp]
    L.optik_robot_fk_ex.argtypes = [vp, dp, dp, dp]
    ip = C.POINTER(C.c_int32)
    L.optik_robot_set_collision_model.argtypes = [vp, ip, dp, dp, C.c_int32, ip, C.c_int32, C.c_double]
    L.optik_robot_set_world.argtypes = [vp, dp, C.c_int32, dp, C.c_int32]
    L.optik_robot_set_world_grid.argtypes = [vp, dp, C.c_double, C.c_int32, C.c_int32, C.c_int32, vp]
    L.optik_robot_world_grid_bake.argtypes = [vp, dp, C.c_double, C.c_int32, C.c_int32, C.c_int32, vp]
    L.optik_robot_world_grid_from_occupancy.argtypes = [vp, C.c_double, C.c_int32, C.c_int32, C.c_int32, vp, C.c_double,
                                                        vp]
    L.optik_robot_occupancy_from_points.argtypes = [vp, dp, C.c_double, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int64,
                                                    vp, C.c_int32, vp]
    L.optik_robot_depth_integrate.argtypes = [vp, dp, C.c_double, C.c_int32, C.c_int32, C.c_int32, vp, vp, C.c_int32,
                                              C.c_int32, C.c_int32, dp, dp, vp, C.c_int32, C.c_double, C.c_double,
                                              C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.optik_robot_occupancy_from_map.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32,
                                                 C.c_int32, vp]
    L.optik_robot_world_grid_from_mesh.argtypes = [vp, dp, C.c_double, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32,
                                                   C.c_double, vp]
    L.optik_robot_sphere_fit.argtypes = [vp, dp, C.c_double, C.c_int32, C.c_int32, C.c_int32, vp, dp, C.c_int64,
                                         C.c_double, C.c_double, C.c_int32, ip, dp, dp, ip, ip]
    L.optik_robot_link_frames_batch.argtypes = [vp, C.c_int64, dp, dp, dp]
    L.optik_robot_collision_batch.argtypes = [vp, C.c_int64, dp, dp, dp, C.POINTER(C.c_uint8)]
    L.optik_robot_collision_motion_batch.argtypes = [vp, C.c_int64, dp, dp, C.c_double, dp, dp, C.POINTER(C.c_uint8),
                                                     ip, ip]
    L.optik_robot_set_motion_resolution.argtypes = [vp, C.c_double]
    L.optik_robot_constraint_batch.argtypes = [vp, C.c_int64, dp, dp, dp, dp, dp, dp, dp]
    L.optik_robot_constraint_project_batch.argtypes = [vp, C.c_int64, dp, dp, dp, dp, C.c_double, C.c_int32,
                                                       C.c_double, C.c_double, dp, dp, dp, ip, ip]
    L.optik_robot_ik_region.argtypes = [vp, C.c_int32, dp, dp, C.c_uint64, C.c_double, C.c_int32, C.c_double, C.c_double,
                                        C.c_int32, dp, dp, dp, C.c_double, C.c_int32, C.c_double, dp, ip, dp, dp,
                                        C.POINTER(C.c_uint64), dp]
    L.optik_robot_ik_region_repair.argtypes = [vp, C.c_int32, dp, dp, C.c_uint64, C.c_double, C.c_int32, C.c_double,
                                               C.c_double, C.c_int32, dp, dp, dp, C.c_double, C.c_int32, C.c_double, dp,
                                               dp, ip, dp, dp, C.POINTER(C.c_uint64), dp, ip]
    L.optik_robot_constraint_motion_batch.argtypes = [vp, C.c_int64, dp, dp, C.c_double, dp, dp, dp, C.c_double, dp,
                                                      dp, C.POINTER(C.c_uint8), ip, ip]
    L.optik_robot_collision_motion_certify_batch.argtypes = [vp, C.c_int64, dp, dp, C.c_double, C.c_double, C.c_int32,
                                                             dp, ip, ip, dp, dp]
    L.optik_robot_diff_ik_ex.argtypes = [vp, dp, dp, dp, dp, C.POINTER(C.c_double), dp]
    L.optik_robot_diff_ik_batch.argtypes = [vp, C.c_int64, dp, dp, dp, dp, dp, dp, C.POINTER(C.c_int32)]
    L.optik_robot_collision_witness_batch.argtypes = [vp, C.c_int64, dp, dp, dp, dp, C.POINTER(C.c_int32)]
    L.optik_robot_diff_ik_avoid.argtypes = [vp, dp, dp, dp, C.c_double, C.c_double, C.c_double, dp,
                                            C.POINTER(C.c_double), dp]
    L.optik_robot_diff_ik_avoid_batch.argtypes = [vp, C.c_int64, dp, dp, dp, C.c_double, C.c_double, C.c_double, dp,
                                                  dp, dp, C.POINTER(C.c_int32)]
    L.optik_robot_path_optimize.argtypes = [vp, C.c_int64, C.c_int32, dp, C.c_int32, C.c_double, C.c_double, C.c_double,
                                            C.c_double, C.c_double, dp, dp, dp, dp, dp, C.POINTER(C.c_int32)]
    L.optik_robot_roadmap_build.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, C.c_uint64]
    L.optik_robot_roadmap_build.restype = C.c_int64
    L.optik_robot_roadmap_plan.argtypes = [vp, dp, dp, C.c_int64, C.c_int32, dp, ip, dp, ip]
    L.optik_robot_roadmap_plan_goals.argtypes = [vp, dp, dp, ip, C.c_int32, C.c_int64, C.c_int32, dp, ip, dp, ip, ip]
    L.optik_robot_roadmap_plan_goals_lazy.argtypes = [vp, dp, dp, ip, C.c_int32, C.c_int64, C.c_int32, C.c_int32, dp, ip,
                                                      dp, ip, ip, ip, C.POINTER(C.c_int64)]
    L.optik_robot_roadmap_build_lazy.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, C.c_uint64]
    L.optik_robot_roadmap_build_lazy.restype = C.c_int64
    L.optik_robot_roadmap_plan_lazy.argtypes = [vp, dp, dp, C.c_int64, C.c_int32, C.c_int32, dp, ip, dp, ip, ip,
                                                C.POINTER(C.c_int64)]
    L.optik_robot_rrt_plan.argtypes = [vp, dp, dp, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_uint64, C.c_int32,
                                       C.c_int32, C.c_int32, dp, dp, ip, dp, ip, ip, ip]
    L.optik_robot_rrt_plan_goals.argtypes = [vp, dp, dp, ip, C.c_int32, C.c_int64, C.c_int32, C.c_double, C.c_double,
                                             C.c_uint64, C.c_int32, C.c_int32, C.c_int32, dp, dp, ip, dp, ip, ip, ip, ip]
    L.optik_robot_rrt_plan_constrained.argtypes = [vp, dp, dp, ip, C.c_int32, C.c_int64, dp, dp, dp, C.c_double,
                                                   C.c_double, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double,
                                                   C.c_double, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, dp, dp, ip,
                                                   dp, ip, ip, ip, ip, ip]
    L.optik_robot_path_shortcut.argtypes = [vp, C.c_int64, C.c_int32, dp, ip, C.c_int32, C.c_double, C.c_double, C.c_int32,
                                            dp, dp, ip, dp, dp, ip]
    L.optik_robot_path_resample.argtypes = [vp, C.c_int64, C.c_int32, dp, ip, C.c_int32, dp, ip]
    L.optik_robot_path_shortcut_constrained.argtypes = [vp, C.c_int64, C.c_int32, dp, ip, C.c_int32, C.c_double,
                                                        C.c_double, C.c_int32, dp, dp, dp, C.c_double, C.c_double,
                                                        C.c_int32, C.c_double, C.c_double, dp, dp, ip, dp, dp, ip, ip]
    L.optik_robot_path_resample_constrained.argtypes = [vp, C.c_int64, C.c_int32, dp, ip, C.c_int32, dp, dp, dp,
                                                        C.c_double, C.c_int32, C.c_double, C.c_double, dp, dp, ip, ip]
    L.optik_robot_path_optimize_constrained.argtypes = [vp, C.c_int64, C.c_int32, dp, C.c_int32, C.c_double, C.c_double,
                                                        C.c_double, C.c_double, C.c_double, dp, dp, dp, C.c_double,
                                                        C.c_int32, C.c_double, C.c_double, dp, dp, dp, dp, dp, ip, dp, ip]
    L.optik_robot_collision_repair_batch.argtypes = [vp, C.c_int64, dp, C.c_double, C.c_double, C.c_double, C.c_int32,
                                                     C.c_double, dp, dp, dp, C.c_double, C.c_int32, C.c_double,
                                                     C.c_double, dp, dp, dp, dp, dp, ip, ip]
    L.optik_robot_path_time.argtypes = [vp, C.c_int64, C.c_int32, dp, ip, dp, dp, dp, dp, dp, dp, ip]
    L.optik_robot_trajectory_sample.argtypes = [vp, C.c_int64, C.c_int32, dp, ip, dp, dp, ip, C.c_double, C.c_int32, dp,
                                                dp]
    L.optik_robot_path_time_tool.argtypes = [vp, C.c_int64, C.c_int32, dp, ip, dp, dp, dp, dp, dp, dp, dp, dp, ip, dp,
                                             dp, dp]
    L.optik_robot_path_time_spline.argtypes = [vp, C.c_int64, C.c_int32, dp, ip, dp, ip, dp, dp, dp, dp, dp, dp, dp, dp,
                                               dp, ip]
    L.optik_robot_velocity_limits.argtypes = [vp]
    L.optik_robot_velocity_limits.restype = C.POINTER(C.c_double)
    L.optik_robot_joint_jacobian_ex.argtypes = [vp, dp, dp, dp]
    L.optik_robot_set_devices.argtypes = [vp, C.POINTER(C.c_int32), C.c_int32]
    L.optik_robot_num_devices.argtypes = [vp]
    L.optik_robot_last_parts.argtypes = [vp]
    L.optik_robot_last_parts.restype = C.c_int32
    L.optik_robot_chain_tables.argtypes = [vp, C.POINTER(C.c_int32), dp, dp, C.POINTER(C.c_int32)]
    L.optik_robot_chain_tables_n.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32), dp, dp, C.POINTER(C.c_int32)]
    L.optik_robot_hip_chain.argtypes = [vp]
    L.optik_robot_hip_chain.restype = vp
    L.optik_robot_joint_limits.argtypes = [vp]
    L.optik_robot_joint_limits.restype = dp
    L._robot_bound = True
    return L


BATCH_ROW_MAJOR, BATCH_VALIDATE_POSES = 1, 2  # include/optik.h: OPTIK_BATCH_*


def _err(L):
    m = L.optik_robot_last_error()
    return m.decode() if m else "unknown error"


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _pose16(m):
    """Row-major nested 4x4 -> column-major flat (parse_pose, optik-py/src/lib.rs:8-15).

    parse_pose converts with nalgebra's ``try_convert::<Matrix4, Isometry3>`` and panics with
    "invalid target transform specified" unless the matrix is an isometry: bottom row exactly
    (0, 0, 0, 1) and the 3x3 block special-orthogonal -- R^T R equal to the identity within
    100 * f64::EPSILON per entry (``is_special_orthogonal``) and det R > 0.  Host-side input
    validation, the same message."""
    a = np.asarray(m, dtype=np.float64)
    if a.shape != (4, 4):
        raise ValueError("pose must be a 4x4 homogeneous matrix")
    R = a[:3, :3]
    eps = 100.0 * np.finfo(np.float64).eps
    ok = (a[3, 0] == 0.0 and a[3, 1] == 0.0 and a[3, 2] == 0.0 and a[3, 3] == 1.0
          and np.all(np.abs(R.T @ R - np.eye(3)) <= eps) and np.linalg.det(R) > 0.0)
    if not ok:
        raise ValueError("invalid target transform specified")
    return np.ascontiguousarray(a.T).ravel()


class SolverConfig:
    """optik.pyi:9-20; defaults of optik-py/src/lib.rs:24-31 / config.rs:52-65."""

    def __init__(self, solution_mode="speed", max_time=0.1, max_restarts=U64_MAX, tol_f=1e-6,
                 tol_df=-1.0, tol_dx=-1.0, linear_weight=(1.0, 1.0, 1.0),
                 angular_weight=(1.0, 1.0, 1.0)):
        # config.rs:10-20; "manipulability" and "condition" are extensions (include/optik_hip.h: OPTIK_MODE_*):
        # every restart runs, as under "quality", and the success with the largest measure of Robot.manipulability
        # wins (w, resp. c)
        if solution_mode not in nat.SOLUTION_MODES:
            raise ValueError("solution_mode must be 'speed', 'quality', 'manipulability' or 'condition'")
        if max_time == 0.0 and max_restarts == 0:
            # optik-py/src/lib.rs:45-47
            raise ValueError("no time or restart limit applied (solver would run forever)")
        self.solution_mode = solution_mode
        self.max_time = float(max_time)
        self.max_restarts = int(max_restarts)
        self.tol_f, self.tol_df, self.tol_dx = float(tol_f), float(tol_df), float(tol_dx)
        self.linear_weight = [float(v) for v in linear_weight]
        self.angular_weight = [float(v) for v in angular_weight]

    def to_c(self):
        return nat.make_config(self.solution_mode, self.max_time,
                               0 if self.max_restarts >= U64_MAX else self.max_restarts,
                               self.tol_f, self.tol_df, self.tol_dx, self.linear_weight,
                               self.angular_weight)


def _check_damper(influence, safety, gain):
    if not (np.isfinite([influence, safety, gain]).all() and influence > safety >= 0.0 and gain > 0.0):
        raise ValueError("diff_ik_avoid: needs influence > safety >= 0 and gain > 0, all finite")


class Robot:
    """optik.pyi:22-49."""

    def __init__(self, handle):
        self._L = _bind(nat.lib())
        self._h = handle
        self._hip = {}

    @staticmethod
    def from_urdf_str(urdf: str, base_link: str, ee_link: str) -> "Robot":
        L = _bind(nat.lib())
        h = C.c_void_p()
        rc = L.optik_robot_try_from_urdf_str(urdf.encode(), base_link.encode(), ee_link.encode(),
                                             C.byref(h))
        if rc:
            raise RuntimeError(_err(L))
        return Robot(h)

    @staticmethod
    def from_urdf_file(path: str, base_link: str, ee_link: str) -> "Robot":
        try:
            with open(path) as fh:
                text = fh.read()
        except OSError as e:
            raise RuntimeError("error parsing URDF file!") from e  # lib.rs:55
        return Robot.from_urdf_str(text, base_link, ee_link)

    def __del__(self):
        try:
            if self._h:
                self._L.optik_robot_free(self._h)
                self._h = None
        except Exception:
            pass

    def set_parallelism(self, n: int) -> None:
        """lib.rs:66-72.  The GPU needs no thread count; what n keeps from the reference is Speed
        mode's early-exit rule.  n = 1 returns the lowest successful restart -- the reference's
        deterministic 1-thread answer (its own determinism test sets 1, tests/test_ik.rs:45-89).
        Never calling this (the reference's default pool has every core) or n > 1 stops at the
        first success of any restart, like rayon's find_any with several threads (README.md:17,
        96): lower latency, a valid but timing-dependent choice among the solutions."""
        self._L.optik_robot_set_parallelism(self._h, int(n))

    def set_devices(self, device_ids) -> None:
        """GPUs of this node the robot spreads restart ranges (ik) and targets (ik_batch) over
        (extension; include/optik.h: optik_robot_set_devices).  Before the first GPU call."""
        ids = (C.c_int32 * len(device_ids))(*[int(d) for d in device_ids])
        if self._L.optik_robot_set_devices(self._h, ids, len(device_ids)):
            raise RuntimeError(_err(self._L))

    def num_devices(self) -> int:
        return int(self._L.optik_robot_num_devices(self._h))

    def last_parts(self) -> int:
        """Over how many of the robot's devices the last ik / ik_batch call was actually cut."""
        return int(self._L.optik_robot_last_parts(self._h))

    def num_positions(self) -> int:
        return int(self._L.optik_robot_num_positions(self._h))

    def joint_limits(self):
        n = self.num_positions()
        p = self._L.optik_robot_joint_limits(self._h)
        vals = [p[i] for i in range(2 * n)]
        C.CDLL(None).free(p)
        return vals[:n], vals[n:]

    def _check_x(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        if x.size != self.num_positions():
            # kinematics.rs:129-133
            raise ValueError("generalized position vector `q` is of incorrect length")
        return x

    def fk(self, x, ee_offset=None):
        x = self._check_x(x)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        out = np.zeros(16)
        if self._L.optik_robot_fk_ex(self._h, _dp(x), _dp(ee) if ee is not None else None, _dp(out)):
            raise RuntimeError(_err(self._L))
        return out.reshape(4, 4).T.tolist()

    def joint_jacobian(self, x, ee_offset=None):
        x = self._check_x(x)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        n = self.num_positions()
        out = np.zeros(6 * n)
        if self._L.optik_robot_joint_jacobian_ex(self._h, _dp(x), _dp(ee) if ee is not None else None,
                                                 _dp(out)):
            raise RuntimeError(_err(self._L))
        return out.reshape(n, 6).T.tolist()

    def ik(self, config: SolverConfig, target, x0, ee_offset=None, return_index=False):
        """Returns (x, c) or None (optik.pyi:36-42).  `return_index=True` appends the winning
        restart index (an extension used by the parity tests)."""
        x0 = self._check_x(x0)
        tgt = _pose16(target)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        cfg = config.to_c()
        n = self.num_positions()
        x, f, idx = np.zeros(n), C.c_double(0.0), C.c_uint64(0)
        rc = self._L.optik_robot_ik_ex(self._h, C.byref(cfg), _dp(tgt), _dp(x0),
                                       _dp(ee) if ee is not None else None, _dp(x), C.byref(f),
                                       C.byref(idx))
        if rc < 0:
            raise RuntimeError(_err(self._L))  # e.g. "seed joint position outside of joint limits"
        if rc == 1:
            return None
        return (x.tolist(), f.value, idx.value) if return_index else (x.tolist(), f.value)

    def ik_batch_arrays(self, config: SolverConfig, targets, x0s, ee_offset=None):
        """Many ik() calls at once (extension), array form: `targets` [T, 4, 4] row-major poses,
        `x0s` [T, n] seeds -> (x [T, n], c [T], found [T] bool); rows with found False are zero.
        Each target gets the semantics of ik() with the same config (poses validated the same way)."""
        tg = np.asarray(targets, dtype=np.float64)
        if tg.ndim != 3 or tg.shape[1:] != (4, 4):
            raise ValueError("targets must be [T, 4, 4]")
        T = tg.shape[0]
        n = self.num_positions()
        x0s = np.ascontiguousarray(x0s, dtype=np.float64).reshape(T, n)
        tg16 = np.ascontiguousarray(tg).reshape(T, 16)  # row-major as given; the host layer transposes
        ee = _pose16(ee_offset) if ee_offset is not None else None
        cfg = config.to_c()
        x = np.zeros((T, n))
        f = np.zeros(T)
        found = np.zeros(T, dtype=np.int32)
        # BATCH_VALIDATE_POSES: parse_pose's isometry test (see _pose16) on every target, in C++
        rc = self._L.optik_robot_ik_batch_poses(self._h, C.byref(cfg), T, _dp(tg16),
                                                BATCH_ROW_MAJOR | BATCH_VALIDATE_POSES, _dp(x0s),
                                                _dp(ee) if ee is not None else None, _dp(x), _dp(f),
                                                found.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc == -3:
            raise ValueError(_err(self._L))
        if rc < 0:
            raise RuntimeError(_err(self._L))
        return x, f, found.astype(bool)

    def ik_batch(self, config: SolverConfig, targets, x0s, ee_offset=None):
        """ik_batch_arrays as a list: (x, c) or None per target, like T calls of ik()."""
        x, f, found = self.ik_batch_arrays(config, targets, x0s, ee_offset)
        # Building ~10 Python objects per target trips the cyclic collector every few hundred targets, and
        # each of its passes walks what has been built so far: 65 536 targets take 105 ms instead of 41.
        # For large batches the collector is paused while the list is built (none of these objects can be
        # garbage).  Its state is process-global: a thread that changes it at the same moment may find it
        # re-enabled -- callers for whom that matters (or who want arrays anyway) use ik_batch_arrays.
        import gc
        pause = len(found) >= 2048 and gc.isenabled()
        if pause:
            gc.disable()
        try:
            xs, fs = x.tolist(), f.tolist()
            return [(xs[t], fs[t]) if ok else None for t, ok in enumerate(found.tolist())]
        finally:
            if pause:
                gc.enable()

    def ik_solutions_batch_arrays(self, config: SolverConfig, targets, x0s, k=8, min_dist=0.1, ee_offset=None):
        """Up to k distinct solutions per target (extension; include/optik.h: optik_robot_ik_solutions), array form:
        `targets` [T, 4, 4] row-major poses, `x0s` [T, n] seeds -> (x [T, k, n], c [T, k], idx [T, k] int64,
        count [T]).  Every restart index in [0, config.max_restarts) runs to its end; the successes are taken best
        first (Quality: nearest to the seed, Speed: lowest index), each kept only if its largest joint difference to
        every solution kept before it is > min_dist.  Slots past count: x and c NaN, idx -1.  On a redundant arm the
        successes form a continuum and min_dist sets the spacing of the returned samples."""
        k, min_dist = nat.check_solutions_args(k, min_dist)
        R = config.max_restarts
        if R <= 0 or R >= U64_MAX:
            raise ValueError("ik_solutions needs a finite max_restarts: every restart index in [0, max_restarts) runs")
        if R > nat.MAX_SOLUTION_RESTARTS:
            raise ValueError(f"ik_solutions: max_restarts must be at most {nat.MAX_SOLUTION_RESTARTS}")
        tg = np.asarray(targets, dtype=np.float64)
        if tg.ndim != 3 or tg.shape[1:] != (4, 4) or tg.shape[0] < 1:
            raise ValueError("targets must be [T, 4, 4]")
        T = tg.shape[0]
        n = self.num_positions()
        x0s = np.asarray(x0s, dtype=np.float64)
        if x0s.shape != (T, n):
            raise ValueError(f"x0s must be [T, n] = [{T}, {n}], got {list(x0s.shape)}")
        x0s = np.ascontiguousarray(x0s)
        tg16 = np.ascontiguousarray(tg).reshape(T, 16)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        cfg = config.to_c()
        x = np.empty((T, k, n))
        f = np.empty((T, k))
        idx = np.empty((T, k), dtype=np.uint64)
        count = np.empty(T, dtype=np.int32)
        rc = self._L.optik_robot_ik_solutions(self._h, C.byref(cfg), T, _dp(tg16), BATCH_ROW_MAJOR | BATCH_VALIDATE_POSES,
                                              _dp(x0s), _dp(ee) if ee is not None else None, k, min_dist,
                                              count.ctypes.data_as(C.POINTER(C.c_int32)), _dp(x), _dp(f),
                                              idx.ctypes.data_as(C.POINTER(C.c_uint64)))
        if rc == -3:
            raise ValueError(_err(self._L))
        if rc < 0:
            raise RuntimeError(_err(self._L))
        return x, f, idx.view(np.int64), count

    def ik_solutions(self, config: SolverConfig, target, x0, k=8, min_dist=0.1, ee_offset=None, return_index=False):
        """Up to k distinct solutions of one target, best first: a list of (x, c) (or (x, c, restart index)),
        empty when no restart succeeded.  See ik_solutions_batch_arrays."""
        x0 = self._check_x(x0)
        tgt = np.asarray(target, dtype=np.float64)
        _pose16(tgt)  # (the single call's checks and messages)
        x, f, idx, count = self.ik_solutions_batch_arrays(config, tgt[None], x0[None], k, min_dist, ee_offset)
        m = int(count[0])
        xs, fs, ids = x[0, :m].tolist(), f[0, :m].tolist(), idx[0, :m].tolist()
        if return_index:
            return [(xs[i], fs[i], ids[i]) for i in range(m)]
        return [(xs[i], fs[i]) for i in range(m)]

    def ik_paths_arrays(self, config: SolverConfig, targets, x0s, max_step=float("inf"), ee_offset=None):
        """Warm-started IK along P paths of L waypoints (extension; include/optik.h: optik_robot_ik_path), array
        form: `targets` [P, L, 4, 4] row-major poses, `x0s` [P, n] start configurations -> (x [P, L, n], c [P, L],
        idx [P, L] int64 (-1 = none), step [P, L], found [P, L] bool).  Each waypoint is solved over restarts
        [0, config.max_restarts) (at most 4096) from the path's current configuration: the start, then the last
        accepted solution.  Accepted is the best success (Quality: nearest, Speed: lowest restart index) whose largest
        joint change from that configuration is <= max_step; a waypoint without one leaves the path where it was
        (x, c and step NaN).  step: the largest joint change of the accepted solution.  max_time, if set, is each
        waypoint's deadline."""
        max_step = nat.check_max_step(max_step)
        R = config.max_restarts
        if R <= 0 or R >= U64_MAX:
            raise ValueError("ik_path needs a finite max_restarts: every waypoint runs restarts [0, max_restarts)")
        if R > nat.PATH_MAX_RESTARTS:
            raise ValueError(f"ik_path: max_restarts must be at most {nat.PATH_MAX_RESTARTS}")
        tg = np.asarray(targets, dtype=np.float64)
        if tg.ndim != 4 or tg.shape[2:] != (4, 4) or tg.shape[0] < 1 or tg.shape[1] < 1:
            raise ValueError("targets must be [P, L, 4, 4]")
        P, L = tg.shape[:2]
        n = self.num_positions()
        x0s = np.asarray(x0s, dtype=np.float64)
        if x0s.shape != (P, n):
            raise ValueError(f"x0s must be [P, n] = [{P}, {n}], got {list(x0s.shape)}")
        x0s = np.ascontiguousarray(x0s)
        tg16 = np.ascontiguousarray(tg).reshape(P * L, 16)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        cfg = config.to_c()
        x = np.empty((P, L, n))
        f = np.empty((P, L))
        idx = np.empty((P, L), dtype=np.uint64)
        step = np.empty((P, L))
        found = np.empty((P, L), dtype=np.int32)
        rc = self._L.optik_robot_ik_path(self._h, C.byref(cfg), P, L, _dp(tg16), BATCH_ROW_MAJOR | BATCH_VALIDATE_POSES,
                                         _dp(x0s), _dp(ee) if ee is not None else None, max_step, _dp(x), _dp(f),
                                         idx.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(step),
                                         found.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc in (-2, -3):  # a start configuration outside the limits, an invalid transform
            raise ValueError(_err(self._L))
        if rc < 0:
            raise RuntimeError(_err(self._L))
        return x, f, idx.view(np.int64), step, found.astype(bool)

    def ik_path(self, config: SolverConfig, targets, x0, max_step=float("inf"), ee_offset=None):
        """One path of L waypoints (`targets` [L, 4, 4]) from x0: a list of L entries, (x, c) or None where the
        waypoint had no accepted solution (the path then carries on from its last configuration).  See
        ik_paths_arrays."""
        x0 = self._check_x(x0)
        tg = np.asarray(targets, dtype=np.float64)
        if tg.ndim != 3 or tg.shape[1:] != (4, 4):
            raise ValueError("targets must be [L, 4, 4]")
        x, f, _, _, found = self.ik_paths_arrays(config, tg[None], x0[None], max_step, ee_offset)
        xs, fs = x[0].tolist(), f[0].tolist()
        return [(xs[w], fs[w]) if ok else None for w, ok in enumerate(found[0].tolist())]

    def diff_ik(self, x0, V_WE, v_max, ee_offset=None):
        """Returns (alpha, v) or None (optik.pyi:43-49; lib.rs:123-239): the joint velocities
        realising alpha * V_WE for the largest feasible 0 <= alpha <= 1 under |v_i| <= v_max_i."""
        x0 = self._check_x(x0)
        n = self.num_positions()
        V = np.ascontiguousarray(V_WE, dtype=np.float64).reshape(6)
        vm = np.ascontiguousarray(v_max, dtype=np.float64).reshape(n)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        alpha, v = C.c_double(0.0), np.zeros(n)
        rc = self._L.optik_robot_diff_ik_ex(self._h, _dp(x0), _dp(V), _dp(vm),
                                            _dp(ee) if ee is not None else None, C.byref(alpha), _dp(v))
        if rc < 0:
            raise RuntimeError(_err(self._L))
        if rc == 1:
            return None
        return alpha.value, v.tolist()

    def diff_ik_batch_arrays(self, x0s, V_WE, v_max, ee_offset=None):
        """Many diff_ik() calls at once (extension), array form: `x0s` [B, n], `V_WE` [B, 6] or one twist [6],
        `v_max` [B, n] or one limit vector [n] -> (alpha [B], v [B, n], found [B] bool).  Row b is what
        diff_ik(x0s[b], V_WE[b], v_max[b], ee_offset) returns, bit for bit; rows with found False are zero.
        One kernel launch per 262 144 rows (include/optik.h: optik_robot_diff_ik_batch)."""
        n = self.num_positions()
        x0s = np.asarray(x0s, dtype=np.float64)
        if x0s.ndim != 2 or x0s.shape[1] != n:
            raise ValueError("x0s must be [B, n]")
        B = x0s.shape[0]
        x0s = np.ascontiguousarray(x0s)
        # (a shared twist / limit vector is repeated here: the host layer takes one row per configuration)
        V = np.ascontiguousarray(np.broadcast_to(np.asarray(V_WE, dtype=np.float64), (B, 6)))
        vm = np.ascontiguousarray(np.broadcast_to(np.asarray(v_max, dtype=np.float64), (B, n)))
        ee = _pose16(ee_offset) if ee_offset is not None else None
        alpha, v = np.zeros(B), np.zeros((B, n))
        status = np.zeros(B, dtype=np.int32)
        rc = self._L.optik_robot_diff_ik_batch(self._h, B, _dp(x0s), _dp(V), _dp(vm),
                                               _dp(ee) if ee is not None else None, _dp(alpha), _dp(v),
                                               status.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc < 0:
            raise RuntimeError(_err(self._L))
        return alpha, v, status == 0

    def diff_ik_batch(self, x0s, V_WE, v_max, ee_offset=None):
        """diff_ik_batch_arrays as a list: (alpha, v) or None per row, like B calls of diff_ik()."""
        alpha, v, found = self.diff_ik_batch_arrays(x0s, V_WE, v_max, ee_offset)
        al, vs = alpha.tolist(), v.tolist()
        return [(al[b], vs[b]) if ok else None for b, ok in enumerate(found.tolist())]

    def diff_ik_avoid(self, x0, V_WE, v_max, influence, safety, gain=1.0, ee_offset=None):
        """diff_ik() that does not drive into obstacles (extension): with the robot's collision model and world, every
        frame whose closest term is within `influence` adds the velocity damper grad . v >= -gain * (dist - safety) /
        (influence - safety) to the LP (the 4 closest frames at most).  Returns (alpha, v), or None when no velocity
        within v_max meets the dampers (a configuration already inside `safety` that cannot back out).  Without a
        collision model it returns what diff_ik() returns, bit for bit.  ValueError unless influence > safety >= 0
        and gain > 0, all finite."""
        x0 = self._check_x(x0)
        n = self.num_positions()
        V = np.ascontiguousarray(V_WE, dtype=np.float64).reshape(6)
        vm = np.ascontiguousarray(v_max, dtype=np.float64).reshape(n)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        _check_damper(influence, safety, gain)
        alpha, v = C.c_double(0.0), np.zeros(n)
        rc = self._L.optik_robot_diff_ik_avoid(self._h, _dp(x0), _dp(V), _dp(vm), influence, safety, gain,
                                               _dp(ee) if ee is not None else None, C.byref(alpha), _dp(v))
        if rc < 0:
            raise RuntimeError(_err(self._L))
        if rc == 1:
            return None
        return alpha.value, v.tolist()

    def diff_ik_avoid_batch_arrays(self, x0s, V_WE, v_max, influence, safety, gain=1.0, ee_offset=None):
        """Many diff_ik_avoid() calls at once, array form, as diff_ik_batch_arrays: -> (alpha [B], v [B, n], found [B]
        bool); row b is what diff_ik_avoid(x0s[b], V_WE[b], v_max[b], ...) returns, bit for bit."""
        n = self.num_positions()
        x0s = np.asarray(x0s, dtype=np.float64)
        if x0s.ndim != 2 or x0s.shape[1] != n:
            raise ValueError("x0s must be [B, n]")
        B = x0s.shape[0]
        x0s = np.ascontiguousarray(x0s)
        V = np.ascontiguousarray(np.broadcast_to(np.asarray(V_WE, dtype=np.float64), (B, 6)))
        vm = np.ascontiguousarray(np.broadcast_to(np.asarray(v_max, dtype=np.float64), (B, n)))
        ee = _pose16(ee_offset) if ee_offset is not None else None
        _check_damper(influence, safety, gain)
        alpha, v = np.zeros(B), np.zeros((B, n))
        status = np.zeros(B, dtype=np.int32)
        rc = self._L.optik_robot_diff_ik_avoid_batch(self._h, B, _dp(x0s), _dp(V), _dp(vm), influence, safety, gain,
                                                     _dp(ee) if ee is not None else None, _dp(alpha), _dp(v),
                                                     status.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc < 0:
            raise RuntimeError(_err(self._L))
        return alpha, v, status == 0

    def collision_witness_batch_arrays(self, xs, ee_offset=None):
        """Which term gives each frame its clearance, and which way is out (extension): `xs` [B, n] -> (dist [B, n + 2],
        grad [B, n + 2, n], witness [B, n + 2, 3] int32).  Row f of a configuration is the smallest term of the
        clearance on frame f: its distance, d dist / d q, and (robot sphere, kind, index) with kind 0 world sphere,
        1 box, 2 grid, 3 self pair (robot sphere a, index of the pair).  dist.min(axis=1) is the clearance of
        collision_clearance_batch_arrays bit for bit; a frame without a term has dist +inf, grad 0, witness -1."""
        n = self.num_positions()
        xs = np.ascontiguousarray(xs, dtype=np.float64)
        if xs.ndim != 2 or xs.shape[1] != n:
            raise ValueError("xs must be [B, n]")
        B = xs.shape[0]
        ee = _pose16(ee_offset) if ee_offset is not None else None
        dist, grad = np.zeros((B, n + 2)), np.zeros((B, n + 2, n))
        wit = np.zeros((B, n + 2, 3), dtype=np.int32)
        if self._L.optik_robot_collision_witness_batch(self._h, B, _dp(xs), _dp(ee) if ee is not None else None,
                                                       _dp(dist), _dp(grad), wit.ctypes.data_as(C.POINTER(C.c_int32))):
            raise RuntimeError(_err(self._L))
        return dist, grad, wit

    def manipulability_batch_arrays(self, xs, ee_offset=None):
        """The measures of solution modes "manipulability" and "condition" (extension) for B configurations:
        `xs` [B, n] -> (w [B], c [B]).  w = sqrt(det G) is the product of the min(n, 6) largest singular values of
        the body Jacobian, c = sigma_min / sigma_max in [0, 1] (G = J^T J for n <= 6, J J^T otherwise); both 0
        where G is not numerically positive definite.  The Jacobian is joint_jacobian's, unscaled (metres and
        radians); TRAC-IK's joint-limit penalty is not applied.  The IK modes rank successes by exactly these
        numbers (include/optik.h: optik_robot_manipulability_batch)."""
        n = self.num_positions()
        xs = np.asarray(xs, dtype=np.float64)
        if xs.ndim != 2 or xs.shape[1] != n:
            raise ValueError(f"xs must be [B, n] with n = {n}, got {list(xs.shape)}")
        B = xs.shape[0]
        xs = np.ascontiguousarray(xs)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        w, c = np.zeros(B), np.zeros(B)
        rc = self._L.optik_robot_manipulability_batch(self._h, B, _dp(xs), _dp(ee) if ee is not None else None,
                                                      _dp(w), _dp(c))
        if rc < 0:
            raise RuntimeError(_err(self._L))
        return w, c

    def manipulability(self, x, ee_offset=None):
        """(w, c) of one configuration: see manipulability_batch_arrays."""
        x = self._check_x(x)
        w, c = self.manipulability_batch_arrays(x[None], ee_offset)
        return float(w[0]), float(c[0])

    # -- the collision filter (extension; include/optik.h) --------------------------------
    def set_collision_model(self, frames, centers, radii, self_pairs="auto", margin=0.0):
        """Robot spheres for the collision filter: frames [S] (0 the base, k = 1 .. n after joint k, n + 1 the end
        effector), centers [S, 3] in those frames, radii [S] (or one radius); self_pairs "auto" (every pair whose
        frames differ by >= 2), None, or [P, 2] sphere indices; margin >= 0.  While a model is set, ik, ik_batch*,
        ik_solutions* and ik_path* return only solutions whose clearance (collision_clearance) is >= margin; Speed
        then returns the lowest-index free success (every restart of a launch runs).  Applied to every GPU of the
        robot.  ValueError for a refused model (before any device work)."""
        from .collision import model_arrays
        f, c, r, p, m = model_arrays(frames, centers, radii, self_pairs, margin)
        if self._L.optik_robot_set_collision_model(self._h, f.ctypes.data_as(C.POINTER(C.c_int32)), _dp(c), _dp(r),
                                                   len(f), p.ctypes.data_as(C.POINTER(C.c_int32)), len(p), m):
            raise ValueError(_err(self._L))

    def clear_collision_model(self):
        """No model: every IK path runs exactly as without the filter."""
        if self._L.optik_robot_set_collision_model(self._h, None, None, None, 0, None, 0, 0.0):
            raise RuntimeError(_err(self._L))

    def set_world(self, spheres=None, boxes=None):
        """Replaces the obstacles, in the base frame: spheres [M, 4] (centre, radius), boxes [M, 10] (t, unit
        quaternion i, j, k, w, half extents).  ValueError for a refused world."""
        from .collision import world_arrays
        sph, box = world_arrays(spheres, boxes)
        if self._L.optik_robot_set_world(self._h, _dp(sph), len(sph), _dp(box), len(box)):
            raise ValueError(_err(self._L))

    # -- the distance-field world (extension; include/optik.h) ----------------------------
    def set_world_grid(self, origin, voxel, values):
        """A sampled signed distance field as a third obstacle kind: values [nx, ny, nz] (anything convertible to
        float32; z fastest), node (i, j, k) at origin + voxel * (i, j, k) in the base frame.  Every robot sphere whose
        centre lies inside the grid adds (trilinear value - radius) to the clearance minimum; spheres outside it add
        nothing.  The interpolated field is within sqrt(3) * voxel of a true distance field: add that to the margin
        for a conservative answer.  set_world leaves the grid alone and this leaves the spheres and boxes alone.
        Applied to every GPU of the robot.  ValueError for a refused grid."""
        from .collision import grid_arrays
        o, v, vals, (nx, ny, nz) = grid_arrays(origin, voxel, values)
        if self._L.optik_robot_set_world_grid(self._h, _dp(o), v, nx, ny, nz, C.c_void_p(vals.ctypes.data)):
            raise ValueError(_err(self._L))

    def clear_world_grid(self):
        """No grid: every call returns what it returns with the spheres and boxes alone."""
        if self._L.optik_robot_set_world_grid(self._h, None, 0.0, 0, 0, 0, None):
            raise RuntimeError(_err(self._L))

    def bake_world_grid(self, origin, voxel, shape):
        """The signed distance of the robot's current spheres and boxes at every node of the grid (origin, voxel,
        shape = (nx, ny, nz)), computed on the GPU: np.float32 [nx, ny, nz].  Installs nothing (hand the result to
        set_world_grid).  ValueError for a refused grid or an empty world."""
        from .collision import grid_arrays
        o, v, _, (nx, ny, nz) = grid_arrays(origin, voxel, shape=shape)
        nodes = nx * ny * nz
        out = np.zeros(nodes if 0 < nodes <= (1 << 24) else 1, dtype=np.float32)
        if self._L.optik_robot_world_grid_bake(self._h, _dp(o), v, nx, ny, nz, C.c_void_p(out.ctypes.data)):
            raise ValueError(_err(self._L))
        return out.reshape(nx, ny, nz)

    # -- from sensor data to that grid (extension; include/optik.h) --------------------------
    def world_grid_from_occupancy(self, voxel, occupied, max_distance=None):
        """The signed field of an occupancy grid `occupied` [nx, ny, nz] (non-zero = occupied), by an exact Euclidean
        distance transform on the GPU: np.float32 [nx, ny, nz], voxel * (distance in voxels to the nearest occupied
        node - 0.5) at a free node and minus voxel * (distance to the nearest free node - 0.5) at an occupied one,
        clamped to +-max_distance (default: the grid diagonal, which never clamps while both kinds of node exist).
        The field takes a voxel for its node: it is optimistic by up to (sqrt(3) - 1) / 2 * voxel on top of
        set_world_grid's sqrt(3) * voxel.  Installs nothing.  ValueError for a refused grid or max_distance."""
        from .collision import default_max_distance, occupancy_array
        occ = occupancy_array(occupied)
        nx, ny, nz = occ.shape
        md = default_max_distance(voxel, occ.shape) if max_distance is None else float(max_distance)
        nodes = nx * ny * nz
        out = np.zeros(nodes if 0 < nodes <= (1 << 24) else 1, dtype=np.float32)
        if self._L.optik_robot_world_grid_from_occupancy(self._h, float(voxel), nx, ny, nz, C.c_void_p(occ.ctypes.data),
                                                         md, C.c_void_p(out.ctypes.data)):
            raise ValueError(_err(self._L))
        return out.reshape(nx, ny, nz)

    def occupancy_from_points(self, origin, voxel, shape, points, exclude=None, into=None):
        """The occupancy grid of a point cloud, on the GPU: a bool array [nx, ny, nz] that is True at the nearest node
        of every point of `points` [N, 3] (base frame) that lies within half a voxel of the grid and inside none of
        the spheres of `exclude` [E, 4] (centre, radius: the self-filter, optik_amd.collision.spheres_at).  NaN and
        infinite points are skipped.  `into`: an earlier result to accumulate into (it is not modified).
        ValueError for a refused grid, more than 1024 exclusion spheres or a non-finite one."""
        from .collision import cloud_arrays, grid_arrays, occupancy_array
        o, v, _, (nx, ny, nz) = grid_arrays(origin, voxel, shape=shape)
        pts, exc = cloud_arrays(points, exclude)
        nodes = nx * ny * nz
        if into is not None:
            occ = occupancy_array(into).copy()
            if occ.shape != (nx, ny, nz):
                raise ValueError("into does not have the grid's shape")
        else:
            occ = np.zeros((nx, ny, nz) if 0 < nodes <= (1 << 24) else (1, 1, 1), dtype=np.uint8)
        if self._L.optik_robot_occupancy_from_points(self._h, _dp(o), v, nx, ny, nz, C.c_void_p(pts.ctypes.data),
                                                     len(pts), C.c_void_p(exc.ctypes.data) if len(exc) else None,
                                                     len(exc), C.c_void_p(occ.ctypes.data)):
            raise ValueError(_err(self._L))
        return occ.view(bool)

    def set_world_points(self, origin, voxel, shape, points, exclude=None, max_distance=None):
        """From a point cloud to the installed distance-field world: occupancy_from_points, then
        world_grid_from_occupancy, then set_world_grid.  Returns the values it installed."""
        occ = self.occupancy_from_points(origin, voxel, shape, points, exclude)
        values = self.world_grid_from_occupancy(voxel, occ, max_distance)
        self.set_world_grid(origin, voxel, values)
        return values

    # -- depth-image worlds: the evidence map (extension; include/optik.h) --------------------
    @staticmethod
    def new_depth_map(shape):
        """An evidence map in which nothing has been observed: np.int16 [nx, ny, nz], all
        optik_amd.collision.MAP_UNKNOWN (-32768).  The caller owns it; depth_integrate returns the next one."""
        from .collision import MAP_UNKNOWN
        shape = tuple(int(v) for v in shape)
        if len(shape) != 3:
            raise ValueError("shape must be (nx, ny, nz)")
        return np.full(shape, MAP_UNKNOWN, dtype=np.int16)

    def depth_integrate(self, map, origin, voxel, depth, intrinsics, poses, exclude=None, z_near=None, z_far=None,
                        band=None, hit=None, miss=None, e_min=None, e_max=None):
        """The evidence map after `depth` has been seen, on the GPU: a new np.int16 [nx, ny, nz] (`map` is not
        modified).  map: an earlier result or new_depth_map(shape), on the node lattice of set_world_grid (origin,
        voxel); depth: [F, H, W] or one [H, W] image, z-depth in metres along the optical axis (what ROS and RealSense
        depth images hold), rectified, pixel centres at integer coordinates; intrinsics: (fx, fy, cx, cy), [F, 4] or
        one row for all frames; poses: the camera in the base frame, [F, 4, 4] or one [4, 4] as fk returns it (x
        right, y down, z forward); exclude: [E, 4] spheres (centre, radius) in the base frame, the self-filter
        (optik_amd.collision.spheres_at): a pixel on one of them sees the robot, which frees the space in front of it
        and is no obstacle.

        Per frame, in order, every node is projected into the image and reads its nearest pixel: a node more than
        `band` in front of the surface loses `miss` (carved free; never below e_min), a node within `band` of it gains
        `hit` (never above e_max), and a node behind the surface, outside the image, outside (z_near, z_far] or under
        an invalid pixel (NaN, infinite, <= z_near) keeps what it has -- unknown (-32768) if it was never observed.  A
        pixel beyond z_far carves up to z_far and marks nothing.  An unknown node counts from 0.

        band defaults to voxel: a band of at least sqrt(3)/2 * voxel = 0.87 * voxel is needed for every surface point
        to have a node within it (the farthest a point can be from its nearest node is half a cell diagonal), and
        anything thinner than the band can be carved by a camera that sees behind it.  The other defaults
        (optik_amd.collision.DEPTH_DEFAULTS: z_near 0.1, z_far 4.0, hit 2, miss 1, e_min -4, e_max 6) are the values
        with which examples/ik_world_depth.py clears and re-marks its scene, and nothing more.
        ValueError for a refused grid, image stack, range, constant, camera or exclusion sphere."""
        from .collision import DEPTH_DEFAULTS, camera_arrays, cloud_arrays, depth_arrays, grid_arrays
        m = np.array(map, dtype=np.int16, order="C")  # (a copy: the C layer reads it, then writes it back)
        if m.ndim != 3:
            raise ValueError(f"map must be [nx, ny, nz], got {list(m.shape)}")
        o, v, _, (nx, ny, nz) = grid_arrays(origin, voxel, shape=m.shape)
        d = depth_arrays(depth)
        F, H, W = d.shape
        k4, p16 = camera_arrays(intrinsics, poses, F)
        _, exc = cloud_arrays(np.zeros((0, 3)), exclude)
        a = {k: (DEPTH_DEFAULTS[k] if val is None else val) for k, val in
             dict(z_near=z_near, z_far=z_far, hit=hit, miss=miss, e_min=e_min, e_max=e_max).items()}
        if self._L.optik_robot_depth_integrate(
                self._h, _dp(o), v, nx, ny, nz, C.c_void_p(m.ctypes.data), C.c_void_p(d.ctypes.data), F, H, W, _dp(k4),
                _dp(p16), C.c_void_p(exc.ctypes.data) if len(exc) else None, len(exc), float(a["z_near"]),
                float(a["z_far"]), v if band is None else float(band), int(a["hit"]), int(a["miss"]), int(a["e_min"]),
                int(a["e_max"])):
            raise ValueError(_err(self._L))
        return m

    def occupancy_from_map(self, map, threshold=None, unknown_occupied=False, into=None):
        """The occupancy of an evidence map, on the GPU: a bool array [nx, ny, nz], True where the evidence is >=
        threshold (default optik_amd.collision.DEPTH_THRESHOLD = 2: one hit at the default constants) and
        `unknown_occupied` where nothing was ever observed.  `into`: an earlier occupancy to OR into (it is not
        modified), as occupancy_from_points has: a map and a point cloud then feed one world_grid_from_occupancy."""
        from .collision import DEPTH_THRESHOLD, occupancy_array
        m = np.ascontiguousarray(map, dtype=np.int16)
        if m.ndim != 3:
            raise ValueError(f"map must be [nx, ny, nz], got {list(m.shape)}")
        nx, ny, nz = m.shape
        if into is not None:
            occ = occupancy_array(into).copy()
            if occ.shape != m.shape:
                raise ValueError("into does not have the map's shape")
        else:
            occ = np.zeros(m.shape, dtype=np.uint8)
        if self._L.optik_robot_occupancy_from_map(self._h, nx, ny, nz, C.c_void_p(m.ctypes.data),
                                                  int(DEPTH_THRESHOLD if threshold is None else threshold),
                                                  1 if unknown_occupied else 0, 1 if into is not None else 0,
                                                  C.c_void_p(occ.ctypes.data)):
            raise ValueError(_err(self._L))
        return occ.view(bool)

    def set_world_depth(self, map, origin, voxel, depth, intrinsics, poses, exclude=None, z_near=None, z_far=None,
                        band=None, hit=None, miss=None, e_min=None, e_max=None, threshold=None,
                        unknown_occupied=False, max_distance=None):
        """From depth images to the installed distance-field world: depth_integrate, then occupancy_from_map, then
        world_grid_from_occupancy, then set_world_grid.  Returns (map, values): the next evidence map, to be handed
        back with the next images, and the values it installed.  The error bounds of set_world_grid and
        world_grid_from_occupancy apply to that field as they stand."""
        map = self.depth_integrate(map, origin, voxel, depth, intrinsics, poses, exclude, z_near, z_far, band, hit, miss,
                                   e_min, e_max)
        occ = self.occupancy_from_map(map, threshold, unknown_occupied)
        values = self.world_grid_from_occupancy(voxel, occ, max_distance)
        self.set_world_grid(origin, voxel, values)
        return map, values

    # -- from a triangle mesh to that grid (extension; include/optik.h) ------------------------
    def world_grid_from_mesh(self, origin, voxel, shape, vertices, triangles=None, max_distance=None):
        """The signed distance field of a triangle mesh on the grid (origin, voxel, shape = (nx, ny, nz)), computed on
        the GPU: np.float32 [nx, ny, nz].  The mesh is `vertices` [V, 3] with `triangles` [M, 3] integer indices, or
        `vertices` [M, 3, 3] as a soup when `triangles` is None (optik_amd.collision.load_stl returns that), in the
        base frame.  Every value is the exact distance to the nearest triangle, negative where the generalized winding
        number has magnitude >= 1/2: holes, unwelded vertices and inward-oriented files are fine, and an open sheet
        reads as unsigned.  Clamped to +-max_distance (default: the grid diagonal).  This is the true distance, so a
        conservative caller adds only set_world_grid's sqrt(3) * voxel to the margin.  No culling: the cost is
        nx * ny * nz * M pair evaluations.  Installs nothing.  ValueError for a refused grid, mesh (no triangle, more
        than 2^20, an index out of range, a NaN or infinite coordinate) or max_distance."""
        from .collision import default_max_distance, grid_arrays, mesh_arrays
        o, v, _, (nx, ny, nz) = grid_arrays(origin, voxel, shape=shape)
        tris = mesh_arrays(vertices, triangles)
        md = default_max_distance(v, (nx, ny, nz)) if max_distance is None else float(max_distance)
        nodes = nx * ny * nz
        out = np.zeros(nodes if 0 < nodes <= (1 << 24) else 1, dtype=np.float32)
        M = len(tris) if len(tris) < (1 << 31) else (1 << 31) - 1
        if self._L.optik_robot_world_grid_from_mesh(self._h, _dp(o), v, nx, ny, nz,
                                                    C.c_void_p(tris.ctypes.data) if len(tris) else _dp(np.zeros(9)),
                                                    M, md, C.c_void_p(out.ctypes.data)):
            raise ValueError(_err(self._L))
        return out.reshape(nx, ny, nz)

    def set_world_mesh(self, origin, voxel, shape, vertices, triangles=None, max_distance=None):
        """From a triangle mesh to the installed distance-field world: world_grid_from_mesh, then set_world_grid.
        Returns the values it installed.  To combine the mesh with another field on the same grid (a bake of the
        primitives, a point cloud's field, a second mesh), take np.minimum of the two value arrays and install that
        with set_world_grid: the minimum of signed distances is the signed distance of the union outside it."""
        values = self.world_grid_from_mesh(origin, voxel, shape, vertices, triangles, max_distance)
        self.set_world_grid(origin, voxel, values)
        return values

    # -- sphere models from collision geometry (extension; include/optik.h) --------------------
    def sphere_fit_arrays(self, values, origin, voxel, points, pad, slack, k):
        """optik_robot_sphere_fit on host arrays (csrc/spherefit_measure.hpp): values [nx, ny, nz] float32, a signed
        distance field on the grid (origin, voxel); points [P, 3] on the solid's surface.  Returns (chosen int32 [k],
        centers [k, 3], radii [k], gains int32 [k], count, uncovered).  ValueError for a refusal."""
        from .collision import cloud_arrays, grid_arrays
        o, v, vals, (nx, ny, nz) = grid_arrays(origin, voxel, values)
        pts, _ = cloud_arrays(points)
        K = int(k)
        kk = K if 1 <= K <= nat.MAX_FIT_SPHERES else 1
        chosen, gains, cu = np.zeros(kk, dtype=np.int32), np.zeros(kk, dtype=np.int32), np.zeros(2, dtype=np.int32)
        centers, radii = np.zeros((kk, 3)), np.zeros(kk)
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_sphere_fit(self._h, _dp(o), v, nx, ny, nz, C.c_void_p(vals.ctypes.data),
                                          _dp(pts) if len(pts) else _dp(np.zeros(3)), len(pts), float(pad),
                                          float(slack), K, chosen.ctypes.data_as(ip), _dp(centers), _dp(radii),
                                          gains.ctypes.data_as(ip), cu.ctypes.data_as(ip)):
            raise ValueError(_err(self._L))
        return chosen, centers, radii, gains, int(cu[0]), int(cu[1])

    def fit_spheres(self, vertices, triangles=None, count=8, voxel=None, pad=None, spacing=None):
        """From a closed triangle mesh (as world_grid_from_mesh takes it, in any frame) to at most `count` spheres
        that contain its surface and stay within `pad` of the solid, on the GPU: (centers [S, 3], radii [S], info).
        The steps: optik_amd.collision.surface_points samples the surface at `spacing`; the grid is the bounding box
        grown by `pad` at `voxel`; world_grid_from_mesh gives the solid's signed distance there; the greedy cover of
        csrc/spherefit_measure.hpp picks the spheres -- centres on grid nodes, radius pad - (the distance at the
        node), each round the sphere that holds the most samples not held yet at least slack = spacing inside.

        Defaults (optik_amd.collision.fit_defaults; nobody has measured better ones): voxel = the bounding box's
        longest side / 10, spacing = voxel / 2, pad = 1.01 * (sqrt(3) * voxel + spacing) = 0.225 of that side: coarse,
        so that a handful of spheres covers a simple solid (a bar 4, a cylinder 5, a cube 25 for uncovered == 0); a
        smaller voxel hugs the solid and needs many more spheres.
        pad >= sqrt(3) * voxel + spacing is required: with it every sample can be covered, and info["uncovered"] == 0
        then means that the whole surface lies inside the spheres (every surface point is within `spacing` of a
        sample that lies `spacing` inside a sphere) while no sphere reaches further than `pad` outside the solid, up
        to the float32 rounding of the field.  With uncovered > 0 the model is NOT conservative: raise `count`, or
        raise `voxel` (fewer, larger spheres that stick out further).  An open sheet has no inside: it gets spheres
        of radius <= pad along it.

        info: uncovered, points (the samples), gains (the samples each sphere newly held), voxel, pad, slack, origin
        and shape of the grid, chosen (the node indices).  The fit does not read the chain.  ValueError for a refused
        mesh, grid (more than 1024 nodes per axis or 2^24 in all: raise voxel), count outside 1..256 or more than
        2^20 samples."""
        from .collision import fit_defaults, fit_grid, mesh_arrays, surface_points
        if not 1 <= int(count) <= nat.MAX_FIT_SPHERES:
            raise ValueError(f"sphere fit: K must be in 1..256, got {count}")
        tris = mesh_arrays(vertices, triangles)
        if len(tris) == 0 or not np.isfinite(tris).all():
            raise ValueError("fit_spheres: the mesh needs at least one triangle and finite coordinates")
        v3 = tris.reshape(-1, 3)
        lo, hi = v3.min(0), v3.max(0)
        voxel, pad, spacing = fit_defaults(float((hi - lo).max()), voxel, pad, spacing)
        origin, shape = fit_grid(lo, hi, voxel, pad)
        pts = surface_points(tris, None, spacing)
        values = self.world_grid_from_mesh(origin, voxel, shape, tris)
        chosen, centers, radii, gains, cnt, unc = self.sphere_fit_arrays(values, origin, voxel, pts, pad, spacing, count)
        info = dict(uncovered=unc, points=len(pts), gains=gains[:cnt].copy(), voxel=voxel, pad=pad, slack=spacing,
                    origin=origin, shape=shape, chosen=chosen[:cnt].copy())
        return centers[:cnt].copy(), radii[:cnt].copy(), info

    def fit_collision_model(self, geometry, per_link=8, voxel=None, pad=None, spacing=None):
        """From collision geometry by frame (optik_amd.collision.urdf_collision_geometry's list of (frame, kind,
        T_frame_geom, data)) to a sphere model: (frames int32 [S], centers [S, 3], radii [S], report) for
        set_collision_model.  All boxes, cylinders and meshes of one frame are merged into one triangle soup (cylinders
        circumscribed: optik_amd.collision.primitive_mesh) and fitted once with fit_spheres(count=per_link; voxel, pad
        and spacing as given, by default from that frame's own bounding box); a <sphere> is passed through as itself.
        report: {frame: fit_spheres' info} under "fits", "uncovered" (the sum), "spheres_per_frame".  ValueError when
        the model would have more than 256 spheres: lower per_link."""
        from .collision import MAX_SPHERES, geometry_soup
        by_frame = {}
        for frame, kind, T, data in geometry:
            by_frame.setdefault(int(frame), []).append((kind, np.asarray(T, dtype=np.float64), data))
        frames, centers, radii = [], [], []
        report = dict(fits={}, uncovered=0, spheres_per_frame={})
        for frame in sorted(by_frame):
            soups, before = [], len(frames)
            for kind, T, data in by_frame[frame]:
                if kind == "sphere":
                    frames.append(frame)
                    centers.append(T[:3, 3].copy())
                    radii.append(float(np.atleast_1d(data)[0]))
                else:
                    soups.append(geometry_soup(kind, T, data))
            if soups:
                c, r, info = self.fit_spheres(np.concatenate(soups), None, per_link, voxel, pad, spacing)
                frames += [frame] * len(r)
                centers += list(c)
                radii += list(r)
                report["fits"][frame] = info
                report["uncovered"] += info["uncovered"]
            report["spheres_per_frame"][frame] = len(frames) - before
        if len(frames) > MAX_SPHERES:
            raise ValueError(f"fit_collision_model: {len(frames)} spheres, more than the {MAX_SPHERES} a collision model "
                             f"may have: lower per_link (now {per_link})")
        return (np.array(frames, dtype=np.int32), np.array(centers, dtype=np.float64).reshape(-1, 3),
                np.array(radii, dtype=np.float64), report)

    def set_collision_model_from_urdf(self, urdf_path, base_link, ee_link, per_link=8, margin=0.0, self_pairs="auto",
                                      reference=None, mesh_dir=None, mesh_resolver=None, on_missing="raise",
                                      voxel=None, pad=None, spacing=None):
        """Reads the URDF's <collision> geometry along the chain (optik_amd.collision.urdf_collision_geometry; meshes
        relative to mesh_dir, by default the URDF's directory), fits spheres to it frame by frame
        (fit_collision_model) and installs them with set_collision_model.  self_pairs "auto": every pair whose frames
        differ by >= 2, without those that overlap at the `reference` configurations ([B, n]; default: the middle of
        the joint range) -- optik_amd.collision.prune_pairs: padded spheres around a joint overlap in every
        configuration; None or [P, 2] as set_collision_model takes them.  Returns (frames, centers, radii, report);
        report adds "geometry" (urdf_collision_geometry's report), "pairs" and "pairs_dropped"."""
        import os
        from .collision import auto_pairs, prune_pairs, urdf_collision_geometry
        with open(urdf_path) as fh:
            text = fh.read()
        if mesh_dir is None:
            mesh_dir = os.path.dirname(os.path.abspath(urdf_path))
        geometry, greport = urdf_collision_geometry(text, base_link, ee_link, mesh_resolver, mesh_dir, on_missing)
        if not geometry:
            raise ValueError("set_collision_model_from_urdf: the chain's links have no collision geometry that was read")
        frames, centers, radii, report = self.fit_collision_model(geometry, per_link, voxel, pad, spacing)
        report["geometry"] = greport
        if isinstance(self_pairs, str) and self_pairs == "auto":
            pairs, dropped = prune_pairs(self, frames, centers, radii, auto_pairs(frames), reference, margin)
        else:
            pairs, dropped = self_pairs, np.zeros((0, 2), dtype=np.int32)
        self.set_collision_model(frames, centers, radii, pairs, margin)
        report["pairs"] = pairs
        report["pairs_dropped"] = dropped
        return frames, centers, radii, report

    def _check_xs(self, xs):
        n = self.num_positions()
        xs = np.asarray(xs, dtype=np.float64)
        if xs.ndim != 2 or xs.shape[1] != n:
            raise ValueError(f"xs must be [B, n] with n = {n}, got {list(xs.shape)}")
        return np.ascontiguousarray(xs)

    def link_frames_batch_arrays(self, xs, ee_offset=None):
        """All n + 2 frames of B configurations xs [B, n] -> [B, n + 2, 4, 4] row-major poses (frame n + 1 is
        fk's pose)."""
        xs = self._check_xs(xs)
        B, n = xs.shape
        ee = _pose16(ee_offset) if ee_offset is not None else None
        out = np.zeros((B, n + 2, 16))
        if self._L.optik_robot_link_frames_batch(self._h, B, _dp(xs), _dp(ee) if ee is not None else None, _dp(out)):
            raise RuntimeError(_err(self._L))
        return out.reshape(B, n + 2, 4, 4).transpose(0, 1, 3, 2).copy()

    def collision_clearance_batch_arrays(self, xs, ee_offset=None):
        """(clearance [B], free [B] bool) of B configurations xs [B, n] against the model and world (+inf clearance
        without a model)."""
        xs = self._check_xs(xs)
        B = xs.shape[0]
        ee = _pose16(ee_offset) if ee_offset is not None else None
        clr, free = np.zeros(B), np.zeros(B, dtype=np.uint8)
        if self._L.optik_robot_collision_batch(self._h, B, _dp(xs), _dp(ee) if ee is not None else None, _dp(clr),
                                               free.ctypes.data_as(C.POINTER(C.c_uint8))):
            raise RuntimeError(_err(self._L))
        return clr, free.astype(bool)

    def collision_clearance(self, x, ee_offset=None):
        """The clearance of one configuration (see collision_clearance_batch_arrays)."""
        x = self._check_x(x)
        clr, _ = self.collision_clearance_batch_arrays(x[None], ee_offset)
        return float(clr[0])

    # -- bending paths out of collision (extension; include/optik.h) ----------------------
    def optimize_paths(self, paths, iters=nat.PATH_OPTIMIZE_ITERS, step=nat.PATH_OPTIMIZE_STEP,
                       w_smooth=nat.PATH_OPTIMIZE_W_SMOOTH, w_obs=nat.PATH_OPTIMIZE_W_OBS, influence=0.2, safety=0.05,
                       resolution=None, ee_offset=None):
        """Covariant gradient smoothing (after CHOMP) of P joint-space paths `paths` [P, L, n], 3 <= L <= 64, against
        the robot's collision model and world: `iters` updates, each a step of -step * Ainv * grad U from the same
        iterate with U = w_smooth * F_smooth + w_obs * F_obs (csrc/path_optimize.hpp), then a clamp to the joint
        limits; the first and the last waypoint never move.  F_obs is a hinge of (witness distance - safety) that is
        zero from `influence` on.  Returns (paths [P, L, n], cost_first [P, 3], cost_last [P, 3], clearance [P],
        status [P] int32): the costs (U, F_smooth, F_obs) of the input and of the result, the smallest witness
        distance over the result's waypoints, and status 1 where the last cost is NaN.  With `resolution` it also
        returns free [P] bool: every one of the L - 1 segments of the result passes collision_motion_batch_arrays at
        that resolution.  Without a collision model the paths relax towards the straight line.
        The defaults of iters, step and the weights are the values with which the host reference clears the L = 16
        scene of tests/test_path_optimize_host.py; they are that and nothing more.  The rows of Ainv sum to about
        L^2 / 8 in the middle of a path, so `step` has to shrink as L^2 grows: the default 0.05 is about 16 times as
        aggressive at L = 64 as at L = 16 and may oscillate there.
        ValueError for L outside 3 .. 64, iters < 0, or unless step > 0, the weights >= 0 and influence > safety
        >= 0, all finite."""
        n = self.num_positions()
        paths = np.ascontiguousarray(paths, dtype=np.float64)
        if paths.ndim != 3 or paths.shape[2] != n:
            raise ValueError(f"paths must be [P, L, n] with n = {n}, got {list(paths.shape)}")
        P, L = paths.shape[0], paths.shape[1]
        nat.check_path_optimize_args(L, iters, step, w_smooth, w_obs, influence, safety)
        if resolution is not None:
            resolution = nat.check_resolution(resolution)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        out = np.zeros((P, L, n))
        first, last, clr = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros(P)
        status = np.zeros(P, dtype=np.int32)
        if self._L.optik_robot_path_optimize(self._h, P, L, _dp(paths), int(iters), float(step), float(w_smooth),
                                             float(w_obs), float(influence), float(safety),
                                             _dp(ee) if ee is not None else None, _dp(out), _dp(first), _dp(last),
                                             _dp(clr), status.ctypes.data_as(C.POINTER(C.c_int32))):
            raise RuntimeError(_err(self._L))
        if resolution is None:
            return out, first, last, clr, status
        seg_free = self.collision_motion_batch_arrays(out[:, :-1].reshape(-1, n), out[:, 1:].reshape(-1, n),
                                                      resolution, ee_offset)[1]
        return out, first, last, clr, status, seg_free.reshape(P, L - 1).all(axis=1)

    # -- roadmap planning (extension; include/optik.h) --------------------------------------
    def build_roadmap(self, N=nat.ROADMAP_NODES, k=nat.ROADMAP_K, resolution=nat.ROADMAP_RESOLUTION, first=0,
                      lazy=False):
        """A probabilistic roadmap over the robot's joint space, kept in the robot: N nodes (1 .. 8192) drawn
        uniformly inside the joint limits -- the IK restart seeds of indices first .. first + N - 1 --, each joined
        to its k (1 .. 16) nearest others (L-infinity) by the motion node -> neighbour, checked at `resolution`
        (radians) against the collision model and world as collision_motion_batch_arrays checks it.  Nodes in
        collision are kept; they have no free edge.  Returns the number of free edges.
        set_collision_model, set_world, set_world_grid and set_world_points make the roadmap stale: plan_paths then
        raises until it is built again.
        lazy=True builds a lazy roadmap instead: the same nodes and neighbours, but no edge
        is checked now.  plan_paths checks the edges its routes use and keeps the verdicts; a change of the model or
        the world only forgets the verdicts, so a lazy roadmap is never stale and plan_paths follows a world that
        changes at camera rate without a rebuild.  Returns the number of edge slots that are not blocked outright
        (empty, or touching a node in collision).
        The defaults are the values with which the wall scene of examples/plan_path.py is planned on a Panda; they
        are that and nothing more.  A cluttered world needs more nodes, a narrow passage a finer resolution.
        ValueError for N, k or a resolution out of range."""
        nat.check_roadmap_args(N=N, k=k)
        h = nat.check_resolution(resolution)
        build = self._L.optik_robot_roadmap_build_lazy if lazy else self._L.optik_robot_roadmap_build
        edges = build(self._h, int(N), int(k), h, int(first))
        if edges < 0:
            raise RuntimeError(_err(self._L))
        self._roadmap_lazy = bool(lazy)
        return int(edges)

    def plan_paths(self, starts, goals, max_waypoints=nat.PATH_OPTIMIZE_MAX_WAYPOINTS, rounds=None):
        """Shortest joint-space paths over the roadmap of build_roadmap for Q pairs starts[q] -> goals[q] ([Q, n]
        each), all on the GPU: each start and each goal is linked to its k nearest nodes by checked motions, the
        direct motion is checked too (and wins ties), and the route of least L-infinity length is walked.  Returns a
        dict: paths [Q, max_waypoints, n] -- start, the nodes of the route, goal, padded with the goal: what
        optimize_paths takes --, len [Q] int32 (the waypoints before the padding), cost [Q] (the route's length in
        radians; the move's duration under equal joint speed limits), status [Q] int32: 0 found, 1 no route (cost
        inf), 2 the route needs more than max_waypoints (the true cost), 3 a NaN in the query (cost NaN); unless 0
        the path is the start, then the goal repeated.  Every one of the len - 1 segments of a found path is a
        motion that was checked free in the direction of travel at the roadmap's resolution.
        On a lazy roadmap (build_roadmap(lazy=True)) `rounds` (0 .. 4096; None: nat.ROADMAP_LAZY_ROUNDS) bounds the
        rounds of checking the unknown edges of the current routes, and the dict gains "rounds" (the rounds made)
        and "checked" (the edges checked).  One more status, 4: unsettled -- the route found last still holds an
        unchecked edge; the path is the start, then the goal repeated, the cost a lower bound (as is the cost of
        status 2 there).  Plans of status 0, 1 and 3 are those of an eager roadmap of the same arguments in the same
        world, bit for bit.  A world that changed since the last call resets the verdicts first.
        RuntimeError without a roadmap or with a stale one; ValueError for max_waypoints outside 2 .. 64, for rounds
        out of range and for rounds on a roadmap that is not lazy."""
        starts, goals = self._check_xs(starts), self._check_xs(goals)
        if starts.shape != goals.shape:
            raise ValueError(f"starts and goals must have the same shape, got {list(starts.shape)} and "
                             f"{list(goals.shape)}")
        nat.check_roadmap_args(max_waypoints=max_waypoints)
        lazy = getattr(self, "_roadmap_lazy", False)
        if rounds is not None and not lazy:
            raise ValueError("rounds is an argument of lazy roadmaps (build_roadmap(lazy=True))")
        Q, n, L = starts.shape[0], starts.shape[1], int(max_waypoints)
        paths, cost = np.zeros((Q, L, n)), np.zeros(Q)
        ln, status = np.zeros(Q, dtype=np.int32), np.zeros(Q, dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        if not lazy:
            if self._L.optik_robot_roadmap_plan(self._h, _dp(starts), _dp(goals), Q, L, _dp(paths),
                                                ln.ctypes.data_as(ip), _dp(cost), status.ctypes.data_as(ip)):
                raise RuntimeError(_err(self._L))
            return dict(paths=paths, len=ln, cost=cost, status=status)
        used, checked = C.c_int32(0), C.c_int64(0)
        if self._L.optik_robot_roadmap_plan_lazy(self._h, _dp(starts), _dp(goals), Q, L, nat.check_lazy_rounds(rounds),
                                                 _dp(paths), ln.ctypes.data_as(ip), _dp(cost),
                                                 status.ctypes.data_as(ip), C.byref(used), C.byref(checked)):
            raise RuntimeError(_err(self._L))
        return dict(paths=paths, len=ln, cost=cost, status=status, rounds=int(used.value), checked=int(checked.value))

    # -- goal-set planning (extension; include/optik.h) --------------------------------------
    _LAZY_GOALS_MSG = ("goal sets are planned over eager roadmaps only: the roadmap is a lazy one "
                       "(build_roadmap(lazy=False), or plan to single goals with plan_paths; over a lazy roadmap goal "
                       "sets are planned by plan_to_goals_lazy, plan_to_poses_lazy and plan_to_region_lazy)")

    def plan_to_goals(self, starts, goals, counts=None, max_waypoints=nat.PATH_OPTIMIZE_MAX_WAYPOINTS):
        """plan_paths to the nearest of several goals per query, in one pass over the roadmap: starts [Q, n], goals
        [Q, G, n] with 1 <= G <= 16, counts [Q] (None: G each) -- query q has the goals g < counts[q] only, nothing
        of the others is read (the NaN rows of ik_solutions_batch_arrays past its count are harmless), and a query
        without goals has status 1.  Returns plan_paths' dict for the cheapest route over the counted goals -- its
        cost is the minimum of plan_paths' costs to each of them, bit for bit -- plus "goal" [Q] int32: the index
        into the goal set of the goal reached for status 0, -1 otherwise.  A found path ends in that goal; any other
        is the start, then goal 0 repeated.  Ties go to the direct motion to the lowest goal.  "paths" and "len" go
        into shortcut_paths, resample_paths and certify_paths as they are.
        RuntimeError without a roadmap, with a stale one and with a lazy one; ValueError for the shapes, for G
        outside 1 .. 16 and for max_waypoints outside 2 .. 64."""
        starts = self._check_xs(starts)
        Q, n = starts.shape
        goals = np.ascontiguousarray(goals, dtype=np.float64)
        if goals.ndim != 3 or goals.shape[0] != Q or goals.shape[2] != n:
            raise ValueError(f"goals must be [Q, G, n] = [{Q}, G, {n}], got {list(goals.shape)}")
        G = nat.check_roadmap_goals(goals.shape[1])
        if counts is not None:
            counts = np.ascontiguousarray(counts, dtype=np.int32)
            if counts.shape != (Q,):
                raise ValueError(f"counts must be [Q] = [{Q}], got {list(counts.shape)}")
        nat.check_roadmap_args(max_waypoints=max_waypoints)
        if getattr(self, "_roadmap_lazy", False):
            raise RuntimeError(self._LAZY_GOALS_MSG)
        L = int(max_waypoints)
        paths, cost = np.zeros((Q, L, n)), np.zeros(Q)
        ln, status, goal = (np.zeros(Q, dtype=np.int32) for _ in range(3))
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_roadmap_plan_goals(self._h, _dp(starts), _dp(goals),
                                                  counts.ctypes.data_as(ip) if counts is not None else None, G, Q, L,
                                                  _dp(paths), ln.ctypes.data_as(ip), _dp(cost),
                                                  status.ctypes.data_as(ip), goal.ctypes.data_as(ip)):
            raise RuntimeError(_err(self._L))
        return dict(paths=paths, len=ln, cost=cost, status=status, goal=goal)

    def plan_to_poses(self, config: SolverConfig, starts, targets, k=8, min_dist=0.1,
                      max_waypoints=nat.PATH_OPTIMIZE_MAX_WAYPOINTS, ee_offset=None):
        """"Move the gripper to this pose": starts [Q, n], targets [Q, 4, 4] row-major poses.  ik_solutions_batch_arrays
        with the starts as seeds gives up to k <= 16 distinct solutions per pose (with a collision model installed:
        the collision-free ones; Quality: solution 0 is the one nearest the start), and plan_to_goals plans to the
        nearest of them over the roadmap.  Returns plan_to_goals' dict plus "goals" [Q, k, n] (NaN past the count)
        and "count" [Q] int32; an unreachable pose has count 0, status 1 and goal -1.  The solutions pass through
        the host here; HipChain.roadmap_plan_poses keeps both stages on the device."""
        k = nat.check_roadmap_goals(k)
        if getattr(self, "_roadmap_lazy", False):
            raise RuntimeError(self._LAZY_GOALS_MSG)
        starts = self._check_xs(starts)
        x, _, _, count = self.ik_solutions_batch_arrays(config, targets, starts, k=k, min_dist=min_dist,
                                                        ee_offset=ee_offset)
        res = self.plan_to_goals(starts, x, counts=count, max_waypoints=max_waypoints)
        res["goals"], res["count"] = x, count
        return res

    # -- goal sets on lazy roadmaps (extension; include/optik.h) -----------------------------
    def _need_lazy_roadmap(self):
        lazy = getattr(self, "_roadmap_lazy", None)
        if lazy is None:
            raise RuntimeError("no roadmap (call build_roadmap(lazy=True) first)")
        if not lazy:
            raise RuntimeError("the roadmap is an eager one: plan goal sets over it with plan_to_goals, plan_to_poses "
                               "and plan_to_region (or build_roadmap(lazy=True))")

    def plan_to_goals_lazy(self, starts, goals, counts=None, max_waypoints=nat.PATH_OPTIMIZE_MAX_WAYPOINTS, rounds=None):
        """plan_to_goals over a lazy roadmap (build_roadmap(lazy=True)): "the world just changed, now plan to these
        goals" without a rebuild.  starts [Q, n], goals [Q, G, n], counts [Q] as plan_to_goals; `rounds` (0 .. 4096;
        None: nat.ROADMAP_LAZY_ROUNDS) bounds the rounds of checking the unknown edges of the current routes, as in
        plan_paths.  The start links, the goal links and the direct motions are checked with the call; the graph's
        edges only where a cheapest route uses them, and after the first pass only the queries that can still change
        are planned again.  Returns plan_to_goals' dict plus "rounds" and "checked".  One more status, 4: unsettled --
        the path is the start, then goal 0 repeated, goal -1, the cost a lower bound (as is the cost of status 2).
        Plans of status 0, 1 and 3 are those of plan_to_goals on an eager roadmap of the same arguments in the same
        world, bit for bit.  A world that changed since the last call resets the verdicts first.
        RuntimeError without a roadmap and with an eager one (plan_to_goals plans over those); ValueError for the
        shapes, G outside 1 .. 16, max_waypoints outside 2 .. 64 and rounds out of range."""
        self._need_lazy_roadmap()
        starts = self._check_xs(starts)
        Q, n = starts.shape
        goals = np.ascontiguousarray(goals, dtype=np.float64)
        if goals.ndim != 3 or goals.shape[0] != Q or goals.shape[2] != n:
            raise ValueError(f"goals must be [Q, G, n] = [{Q}, G, {n}], got {list(goals.shape)}")
        G = nat.check_roadmap_goals(goals.shape[1])
        if counts is not None:
            counts = np.ascontiguousarray(counts, dtype=np.int32)
            if counts.shape != (Q,):
                raise ValueError(f"counts must be [Q] = [{Q}], got {list(counts.shape)}")
        nat.check_roadmap_args(max_waypoints=max_waypoints)
        rounds = nat.check_lazy_rounds(rounds)
        L = int(max_waypoints)
        paths, cost = np.zeros((Q, L, n)), np.zeros(Q)
        ln, status, goal = (np.zeros(Q, dtype=np.int32) for _ in range(3))
        ip = C.POINTER(C.c_int32)
        used, checked = C.c_int32(0), C.c_int64(0)
        if self._L.optik_robot_roadmap_plan_goals_lazy(self._h, _dp(starts), _dp(goals),
                                                       counts.ctypes.data_as(ip) if counts is not None else None, G, Q,
                                                       L, rounds, _dp(paths), ln.ctypes.data_as(ip), _dp(cost),
                                                       status.ctypes.data_as(ip), goal.ctypes.data_as(ip),
                                                       C.byref(used), C.byref(checked)):
            raise RuntimeError(_err(self._L))
        return dict(paths=paths, len=ln, cost=cost, status=status, goal=goal, rounds=int(used.value),
                    checked=int(checked.value))

    def plan_to_poses_lazy(self, config: SolverConfig, starts, targets, k=8, min_dist=0.1,
                           max_waypoints=nat.PATH_OPTIMIZE_MAX_WAYPOINTS, rounds=None, ee_offset=None):
        """plan_to_poses over a lazy roadmap: ik_solutions_batch_arrays with the starts as seeds, then
        plan_to_goals_lazy to the nearest of the solutions.  Returns plan_to_goals_lazy's dict plus "goals" [Q, k, n]
        (NaN past the count) and "count" [Q] int32; an unreachable pose has count 0, status 1 and goal -1."""
        self._need_lazy_roadmap()
        k = nat.check_roadmap_goals(k)
        starts = self._check_xs(starts)
        x, _, _, count = self.ik_solutions_batch_arrays(config, targets, starts, k=k, min_dist=min_dist,
                                                        ee_offset=ee_offset)
        res = self.plan_to_goals_lazy(starts, x, counts=count, max_waypoints=max_waypoints, rounds=rounds)
        res["goals"], res["count"] = x, count
        return res

    # -- the bidirectional tree planner (extension; include/optik.h) --------------------------
    def plan_rrt(self, starts, goals, iters=None, step=None, resolution=nat.ROADMAP_RESOLUTION, first=0, max_nodes=None,
                 max_waypoints=nat.PATH_OPTIMIZE_MAX_WAYPOINTS, poll=nat.RRT_POLL, ee_offset=None):
        """Single-query planning for the pairs a roadmap misses -- the rows plan_paths returns with status 1 because
        the start or the goal sits in a pocket none of its nodes sees: for each of Q pairs starts[q] -> goals[q] ([Q,
        n] each) two trees grow on the GPU, one from the start and one from the goal, towards the same uniform samples
        (the IK restart seeds first, first + 1, ...) in steps of at most `step` radians (L-infinity), and are joined
        by a free motion (bidirectional RRT with one extension per tree and iteration).  Every motion is checked at
        `resolution` against the collision model and world, in the direction the path travels it, as
        collision_motion_batch_arrays checks it.  Returns a dict: paths [Q, max_waypoints, n], len [Q] int32, cost [Q]
        and status [Q] int32 as plan_paths returns them -- 0 found; 1 no junction within `iters` iterations, or a start
        or goal in collision (cost inf); 2 found, but with more than max_waypoints waypoints (the true cost); 3 a NaN or
        an infinity in the query (cost NaN); unless 0 the path is the start, then the goal repeated --, iters [Q] int32
        (the iterations run before the query ended) and nodes [Q, 2] int32 (the sizes of the two trees, at most
        max_nodes each).  "paths" and "len" go into shortcut_paths, resample_paths and certify_paths as they are; a
        tree's path is jagged, so shortcut it.
        It keeps no state in the robot and reads no roadmap, so nothing can be stale.  A query's result does not
        depend on the other queries or on `poll`, the iterations between two looks at the number of unfinished
        queries (each look synchronises with the GPU once).
        The defaults of iters, step and max_nodes (nat.RRT_ITERS, RRT_STEP, RRT_NODES) are the values with which the
        pair of examples/plan_rrt.py is planned on a Panda; they are that and nothing more.
        ValueError for iters outside 1 .. 65536, max_nodes outside 2 .. 4096, max_waypoints outside 2 .. 64, poll
        outside 1 .. 65536, a step or a resolution that is not finite and > 0."""
        starts, goals = self._check_xs(starts), self._check_xs(goals)
        if starts.shape != goals.shape:
            raise ValueError(f"starts and goals must have the same shape, got {list(starts.shape)} and "
                             f"{list(goals.shape)}")
        iters, step, max_nodes, poll, first = nat.check_rrt_args(iters, step, max_nodes, max_waypoints, poll, first)
        h = nat.check_resolution(resolution)
        Q, n, L = starts.shape[0], starts.shape[1], int(max_waypoints)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        paths, cost = np.zeros((Q, L, n)), np.zeros(Q)
        ln, status, it = (np.zeros(Q, dtype=np.int32) for _ in range(3))
        nodes = np.zeros((Q, 2), dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_rrt_plan(self._h, _dp(starts), _dp(goals), Q, iters, step, h, first, max_nodes, L, poll,
                                        _dp(ee) if ee is not None else None, _dp(paths), ln.ctypes.data_as(ip),
                                        _dp(cost), status.ctypes.data_as(ip), it.ctypes.data_as(ip),
                                        nodes.ctypes.data_as(ip)):
            raise RuntimeError(_err(self._L))
        return dict(paths=paths, len=ln, cost=cost, status=status, iters=it, nodes=nodes)

    # -- the tree planner with a goal set (extension; include/optik.h) -----------------------
    def plan_rrt_to_goals(self, starts, goals, counts=None, iters=None, step=None, resolution=nat.ROADMAP_RESOLUTION,
                          first=0, max_nodes=None, max_waypoints=nat.PATH_OPTIMIZE_MAX_WAYPOINTS, poll=nat.RRT_POLL,
                          ee_offset=None):
        """plan_rrt to any of several goals per query: starts [Q, n], goals [Q, G, n] with 1 <= G <= 16, counts [Q]
        (None: G each) -- query q has the goals g < counts[q] only, nothing of the others influences an output (the
        NaN rows of ik_solutions_batch_arrays past its count are the normal input), and a query without goals has
        status 1.  Tree 1 has one root per counted goal that is free, so a goal behind an obstacle costs its root
        node and nothing more, and the query ends at the first junction with any of them.  If direct motions start
        -> goal are free the nearest such goal wins (a tie: the lower index); past that the answer is the goal
        joined FIRST, not the cheapest one.  Returns plan_rrt's dict plus "goal" [Q] int32: the index into the goal
        set of the goal reached for status 0, -1 otherwise.  A found path ends in that goal; any other is the start,
        then goal 0 repeated.  With one goal per query it is plan_rrt, bit for bit.  "paths" and "len" go into
        shortcut_paths, resample_paths and certify_paths as they are.
        It keeps no state in the robot and reads no roadmap: it works whatever roadmap the robot holds -- none, an
        eager one, a lazy one, a stale one.  The defaults are plan_rrt's.
        ValueError for the shapes, for G outside 1 .. 16, for max_nodes outside max(2, G) .. 4096 and for what
        plan_rrt refuses."""
        starts = self._check_xs(starts)
        Q, n = starts.shape
        goals = np.ascontiguousarray(goals, dtype=np.float64)
        if goals.ndim != 3 or goals.shape[0] != Q or goals.shape[2] != n:
            raise ValueError(f"goals must be [Q, G, n] = [{Q}, G, {n}], got {list(goals.shape)}")
        if counts is not None:
            counts = np.ascontiguousarray(counts, dtype=np.int32)
            if counts.shape != (Q,):
                raise ValueError(f"counts must be [Q] = [{Q}], got {list(counts.shape)}")
        iters, step, max_nodes, poll, first = nat.check_rrt_args(iters, step, max_nodes, max_waypoints, poll, first)
        G = nat.check_rrt_goals(goals.shape[1], max_nodes)
        h = nat.check_resolution(resolution)
        L = int(max_waypoints)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        paths, cost = np.zeros((Q, L, n)), np.zeros(Q)
        ln, status, it, goal = (np.zeros(Q, dtype=np.int32) for _ in range(4))
        nodes = np.zeros((Q, 2), dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_rrt_plan_goals(self._h, _dp(starts), _dp(goals),
                                              counts.ctypes.data_as(ip) if counts is not None else None, G, Q, iters,
                                              step, h, first, max_nodes, L, poll, _dp(ee) if ee is not None else None,
                                              _dp(paths), ln.ctypes.data_as(ip), _dp(cost), status.ctypes.data_as(ip),
                                              it.ctypes.data_as(ip), nodes.ctypes.data_as(ip), goal.ctypes.data_as(ip)):
            raise RuntimeError(_err(self._L))
        return dict(paths=paths, len=ln, cost=cost, status=status, iters=it, nodes=nodes, goal=goal)

    def plan_rrt_to_poses(self, config: SolverConfig, starts, targets, k=8, min_dist=0.1, iters=None, step=None,
                          resolution=nat.ROADMAP_RESOLUTION, first=0, max_nodes=None,
                          max_waypoints=nat.PATH_OPTIMIZE_MAX_WAYPOINTS, poll=nat.RRT_POLL, ee_offset=None):
        """"Move the gripper to this pose" without a roadmap: starts [Q, n], targets [Q, 4, 4] row-major poses.
        ik_solutions_batch_arrays with the starts as seeds gives up to k <= 16 distinct solutions per pose (with a
        collision model installed: the collision-free ones), and plan_rrt_to_goals grows one tree from the start and
        one from all of them at once -- what to run on the rows plan_to_poses returns with status 1, and the way to
        plan to a pose beside a lazy roadmap, which plan_to_poses refuses.  Returns plan_rrt_to_goals' dict plus
        "goals" [Q, k, n] (NaN past the count) and "count" [Q] int32; an unreachable pose has count 0, status 1 and
        goal -1.  The goal reached is the one joined first, not the cheapest.  The solutions pass through the host
        here; HipChain.rrt_plan_poses keeps both stages on the device."""
        k = nat.check_roadmap_goals(k)
        starts = self._check_xs(starts)
        x, _, _, count = self.ik_solutions_batch_arrays(config, targets, starts, k=k, min_dist=min_dist,
                                                        ee_offset=ee_offset)
        res = self.plan_rrt_to_goals(starts, x, counts=count, iters=iters, step=step, resolution=resolution,
                                     first=first, max_nodes=max_nodes, max_waypoints=max_waypoints, poll=poll,
                                     ee_offset=ee_offset)
        res["goals"], res["count"] = x, count
        return res

    # -- shortcutting and resampling (extension; include/optik.h) ---------------------------
    def _check_paths(self, paths, lens):
        n = self.num_positions()
        paths = np.ascontiguousarray(paths, dtype=np.float64)
        if paths.ndim != 3 or paths.shape[2] != n:
            raise ValueError(f"paths must be [P, L, n] with n = {n}, got {list(paths.shape)}")
        if lens is not None:
            lens = np.ascontiguousarray(lens, dtype=np.int32)
            if lens.shape != (paths.shape[0],):
                raise ValueError(f"lens must be [P] with P = {paths.shape[0]}, got {list(lens.shape)}")
        return paths, lens

    def shortcut_paths(self, paths, lens=None, resolution=nat.SHORTCUT_RESOLUTION, vertices=nat.SHORTCUT_VERTICES,
                       hop_penalty=None, max_waypoints=None, ee_offset=None):
        """Shortcuts P joint-space paths `paths` [P, L, n] with `lens` [P] waypoints each (None: L each) -- plan_paths'
        "paths" and "len" as they are --, all on the GPU: each polyline is subdivided into at most `vertices` (2 .. 64)
        vertices, its own waypoints among them, EVERY pair of vertices is checked as a motion at `resolution` against
        the collision model and world, and the route of least (L-infinity length + hop_penalty) per hop through that
        visibility graph is walked: the optimum over all vertex shortcuts, deterministic.  hop_penalty (radians; None:
        the resolution) keeps detours of equal length up to a rounding from adding waypoints.  Returns a dict: paths
        [P, max_waypoints, n] (None: L) padded with the goal, len [P] int32, cost [P] and cost_in [P] (the route's
        and the input's length, without penalties), status [P] int32: 0 found -- every segment a motion checked free
        in the direction of travel --, 1 no route (the input is blocked at this resolution), 2 a length outside 2 ..
        min(L, vertices) or a route of more than max_waypoints, 3 a NaN or an infinity; unless 0 the input comes back.
        All-pairs visibility samples about vertices^2 / 6 times the path's own length: 64 vertices cost about four
        times what 32 do (profiles/shortcut_cost.txt).  The stored roadmap is neither read nor required.
        ValueError for L, vertices or max_waypoints outside 2 .. 64, a resolution that is not finite and > 0, a
        hop_penalty that is NaN, negative or infinite."""
        paths, lens = self._check_paths(paths, lens)
        P, L, n = paths.shape
        Lout = L if max_waypoints is None else max_waypoints
        h, hop = nat.check_shortcut_args(L, vertices, Lout, resolution, hop_penalty)
        Lout = int(Lout)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        out, cost, cost_in = np.zeros((P, Lout, n)), np.zeros(P), np.zeros(P)
        ln, status = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_path_shortcut(self._h, P, L, _dp(paths), lens.ctypes.data_as(ip) if lens is not None else None,
                                             int(vertices), h, hop, Lout, _dp(ee) if ee is not None else None,
                                             _dp(out), ln.ctypes.data_as(ip), _dp(cost), _dp(cost_in),
                                             status.ctypes.data_as(ip)):
            raise RuntimeError(_err(self._L))
        return dict(paths=out, len=ln, cost=cost, cost_in=cost_in, status=status)

    def resample_paths(self, paths, lens=None, waypoints=nat.RESAMPLE_WAYPOINTS, resolution=None, ee_offset=None):
        """`waypoints` (2 .. 64) waypoints at equal L-infinity arc length along each of P polylines `paths` [P, L, n]
        with `lens` [P] waypoints each (None: L each): the dense, evenly spaced path optimize_paths and a controller
        take.  The ends are copied; every other waypoint lies on the input.  Returns (paths [P, waypoints, n], status
        [P] int32: 0, 2 for a length outside 2 .. L, 3 for a NaN or infinite length).  The new segments cut the
        input's corners, so they are NOT free by construction: with `resolution` it also returns free [P] bool, whether
        each of the waypoints - 1 new segments passes collision_motion_batch_arrays at that resolution.
        ValueError for L or waypoints outside 2 .. 64 or a bad resolution."""
        paths, lens = self._check_paths(paths, lens)
        P, L, n = paths.shape
        nat.check_shortcut_args(L, max_waypoints=waypoints)
        if resolution is not None:
            resolution = nat.check_resolution(resolution)
        W = int(waypoints)
        out, status = np.zeros((P, W, n)), np.zeros(P, dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_path_resample(self._h, P, L, _dp(paths), lens.ctypes.data_as(ip) if lens is not None else None,
                                             W, _dp(out), status.ctypes.data_as(ip)):
            raise RuntimeError(_err(self._L))
        if resolution is None:
            return out, status
        seg_free = self.collision_motion_batch_arrays(out[:, :-1].reshape(-1, n), out[:, 1:].reshape(-1, n),
                                                      resolution, ee_offset)[1]
        return out, status, seg_free.reshape(P, W - 1).all(axis=1)

    # -- timing and sampling (extension; include/optik.h) -----------------------------------
    def velocity_limits(self):
        """The URDF's <limit velocity=> of the n articulated joints [n]; inf where it is absent, 0 or negative."""
        n = self.num_positions()
        p = self._L.optik_robot_velocity_limits(self._h)
        vals = np.array([p[i] for i in range(n)], dtype=np.float64)
        C.CDLL(None).free(p)
        return vals

    def time_paths(self, paths, lens=None, a_max=None, v_max=None, scale=1.0):
        """Times P joint-space paths `paths` [P, L, n] with `lens` [P] waypoints each (None: L each), 3 <= L <= 64, rest
        to rest under joint velocity and acceleration limits, all on the GPU: time-optimal path parameterisation by
        reachability analysis (TOPP-RA) on the path's own waypoints, so evenly spaced input -- resample_paths' -- is
        what it is meant for.  a_max (rad/s^2; required: a URDF carries none) and v_max (rad/s; None: the URDF's,
        velocity_limits()) are a scalar or [n]; `scale` in (0, 1] multiplies both.  Returns a dict: times [P, L] from
        0, velocities and accelerations [P, L, n] at the waypoints, duration [P], status [P] int32: 0 timed; 1 stalled
        (two neighbouring waypoints both at zero speed: the path is too jagged for its spacing); 2 a length outside 3
        .. L or a waypoint repeated three times (twice at the start); 3 a NaN or an infinity; unless 0 the times and
        the duration are NaN.  The result always respects the limits at the waypoints and is time-optimal where the
        path is dense and gently curved (DESIGN.md section 5.20 says by how much it is longer elsewhere).
        ValueError for an a_max that is not finite and > 0, a v_max that is <= 0 or NaN, L outside 3 .. 64, a scale
        outside (0, 1]."""
        paths, lens = self._check_paths(paths, lens)
        P, L, n = paths.shape
        if a_max is None:
            raise ValueError("a_max is required: a URDF carries no acceleration limits")
        v, a = nat.check_time_args(n, L, a_max, self.velocity_limits() if v_max is None else v_max, scale)
        times, dur = np.zeros((P, L)), np.zeros(P)
        vel, acc = np.zeros((P, L, n)), np.zeros((P, L, n))
        status = np.zeros(P, dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_path_time(self._h, P, L, _dp(paths), lens.ctypes.data_as(ip) if lens is not None else None,
                                         _dp(v), _dp(a), _dp(times), _dp(vel), _dp(acc), _dp(dur),
                                         status.ctypes.data_as(ip)):
            raise RuntimeError(_err(self._L))
        return dict(times=times, velocities=vel, accelerations=acc, duration=dur, status=status)

    def time_paths_tool(self, paths, lens=None, a_max=None, v_max=None, tool_v_max=np.inf, tool_a_tangential=np.inf,
                        tool_a_normal=np.inf, tool_w_max=np.inf, scale=1.0, ee_offset=None):
        """time_paths with limits on the tool as well: `tool_v_max` the speed of the tool centre point (m/s; a
        collaborative cell's reduced speed is 0.25), `tool_a_tangential` and `tool_a_normal` its acceleration along
        and across its path (m/s^2), `tool_w_max` the end effector's angular speed (rad/s); each a number > 0, inf for
        "no limit".  The tool is the end effector with `ee_offset` [4, 4].  `scale` multiplies the speed limits as it
        multiplies v_max and the acceleration limits as it multiplies a_max.  Returns time_paths' dict plus
        "tool_speed" [P, L], "tool_accel" [P, L, 2] (tangential, normal) and "tool_wspeed" [P, L] at the waypoints, to
        check the limits with; the dict goes into sample_trajectories as it is.  Guaranteed at the waypoints: speed <=
        tool_v_max, |tangential| <= tool_a_tangential, normal <= tool_a_normal (so |acceleration| <= their root sum of
        squares), angular speed <= tool_w_max.  NOT bounded: the angular acceleration, and anything between waypoints
        -- resample densely.  With every tool limit inf the result is time_paths'.
        ValueError for what time_paths refuses and for a tool limit that is <= 0 or NaN."""
        paths, lens = self._check_paths(paths, lens)
        P, L, n = paths.shape
        if a_max is None:
            raise ValueError("a_max is required: a URDF carries no acceleration limits")
        v, a = nat.check_time_args(n, L, a_max, self.velocity_limits() if v_max is None else v_max, scale)
        lim = nat.check_time_tool_args(tool_v_max, tool_a_tangential, tool_a_normal, tool_w_max, scale)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        times, dur = np.zeros((P, L)), np.zeros(P)
        vel, acc = np.zeros((P, L, n)), np.zeros((P, L, n))
        status = np.zeros(P, dtype=np.int32)
        speed, taccel, wspeed = np.zeros((P, L)), np.zeros((P, L, 2)), np.zeros((P, L))
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_path_time_tool(self._h, P, L, _dp(paths),
                                              lens.ctypes.data_as(ip) if lens is not None else None, _dp(v), _dp(a),
                                              _dp(lim), _dp(ee) if ee is not None else None, _dp(times), _dp(vel),
                                              _dp(acc), _dp(dur), status.ctypes.data_as(ip), _dp(speed), _dp(taccel),
                                              _dp(wspeed)):
            raise RuntimeError(_err(self._L))
        return dict(times=times, velocities=vel, accelerations=acc, duration=dur, status=status, tool_speed=speed,
                    tool_accel=taccel, tool_wspeed=wspeed)

    def smooth_timing(self, paths, timing, j_max, a_max, v_max=None, lens=None):
        """Spline retiming, the stage between time_paths / time_paths_tool and sample_trajectories: `timing` is their
        result for these `paths` [P, L, n] and `lens`.  The waypoints keep their places and get new times, velocities
        and accelerations: those of the C2 cubic spline through them, rest to rest, with every time multiplied by the
        least factor >= 1 at which |velocity| <= v_max, |acceleration| <= a_max and |jerk| <= j_max hold along the
        WHOLE curve, between the waypoints too.  j_max (rad/s^3), a_max (rad/s^2) and v_max (rad/s; None: the URDF's,
        velocity_limits()) are a scalar or [n], each > 0, inf for "no limit".  Returns time_paths' dict -- times [P, L],
        velocities and accelerations [P, L, n], duration [P], status [P] int32 -- plus factor [P] and ratios [P, 3], the
        final peak velocity, acceleration and jerk over their limits (all <= 1 for status 0).  status: 0; 1 the input
        status was neither 0 nor 4, or its times do not increase strictly from 0; 2 a length outside 3 .. L; 3 a NaN or
        an infinity; 4 a ratio still above 1: rounding of the new times, rare, seen at 1 + 3e-12 with the jerk binding
        at 64 waypoints; unless 0 or 4 the times and the duration are NaN.  sample_trajectories treats every status
        other than 0 as untimed and holds such a path at its start, a 4 included: pass a result that holds a 4 through
        smooth_timing once more (`timing` = that result), which retimes those paths by about 1 + 2e-12 and leaves the
        ones with status 0 at factor 1, bit for bit.  The
        sampler's cubic Hermite curve over (times, waypoints, velocities) IS this spline, so the dict goes into
        sample_trajectories as it is and (q, qd, qdd) are consistent.  Not covered: the
        motion starts and stops with a finite acceleration step -- the jerk is bounded on the open interval --, the
        slow-down is uniform, time_paths_tool's tool limits are only scaled down.
        ValueError for a limit that is <= 0 or NaN, L outside 3 .. 64, a timing of another shape."""
        paths, lens = self._check_paths(paths, lens)
        P, L, n = paths.shape
        v, a, j = nat.check_time_spline_args(n, L, j_max, a_max, self.velocity_limits() if v_max is None else v_max)
        t_in = np.ascontiguousarray(timing["times"], dtype=np.float64)
        s_in = np.ascontiguousarray(timing["status"], dtype=np.int32)
        if t_in.shape != (P, L) or s_in.shape != (P,):
            raise ValueError("timing must be time_paths' result for these paths")
        times, dur, fac, ratios = np.zeros((P, L)), np.zeros(P), np.zeros(P), np.zeros((P, 3))
        vel, acc = np.zeros((P, L, n)), np.zeros((P, L, n))
        status = np.zeros(P, dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_path_time_spline(self._h, P, L, _dp(paths),
                                                lens.ctypes.data_as(ip) if lens is not None else None, _dp(t_in),
                                                s_in.ctypes.data_as(ip), _dp(v), _dp(a), _dp(j), _dp(times), _dp(vel),
                                                _dp(acc), _dp(dur), _dp(fac), _dp(ratios), status.ctypes.data_as(ip)):
            raise RuntimeError(_err(self._L))
        return dict(times=times, velocities=vel, accelerations=acc, duration=dur, status=status, factor=fac,
                    ratios=ratios)

    def sample_trajectories(self, paths, timing, dt, lens=None, resolution=None, ee_offset=None):
        """Samples the trajectories time_paths timed (`timing`: its result for these `paths` and `lens`) every `dt`
        seconds by cubic Hermite interpolation in time over the waypoints' positions and velocities -- what a
        joint-trajectory controller does with them.  Returns (positions [P, T, n], velocities [P, T, n]) with
        T = the largest ceil(duration / dt) + 1 over the paths with status 0 (1 if there is none): past its duration a
        path holds its goal at rest; a path whose status is not 0 holds its start.  The Hermite curve leaves the
        polyline between waypoints, as resample_paths' segments cut corners, so it is NOT free by construction: with
        `resolution` the call also returns free [P] bool, whether every move between consecutive samples passes
        collision_motion_batch_arrays at that resolution.  ValueError for a dt that is not finite and > 0 or a T above
        65 536 (raise dt)."""
        paths, lens = self._check_paths(paths, lens)
        P, L, n = paths.shape
        nat.check_time_args(n, L)
        if resolution is not None:
            resolution = nat.check_resolution(resolution)
        times = np.ascontiguousarray(timing["times"], dtype=np.float64)
        vel = np.ascontiguousarray(timing["velocities"], dtype=np.float64)
        status = np.ascontiguousarray(timing["status"], dtype=np.int32)
        dur = np.asarray(timing["duration"], dtype=np.float64)
        if times.shape != (P, L) or vel.shape != (P, L, n) or status.shape != (P,) or dur.shape != (P,):
            raise ValueError("timing must be time_paths' result for these paths")
        dt = nat.check_sample_args(dt)
        ok = status == nat.TIME_TIMED
        T = int(np.ceil(dur[ok] / dt).max()) + 1 if ok.any() else 1
        nat.check_sample_args(dt, T)
        q, qd = np.zeros((P, T, n)), np.zeros((P, T, n))
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_trajectory_sample(self._h, P, L, _dp(paths),
                                                 lens.ctypes.data_as(ip) if lens is not None else None, _dp(times),
                                                 _dp(vel), status.ctypes.data_as(ip), dt, T, _dp(q), _dp(qd)):
            raise RuntimeError(_err(self._L))
        if resolution is None:
            return q, qd
        if T < 2:
            return q, qd, np.ones(P, dtype=bool)
        seg_free = self.collision_motion_batch_arrays(q[:, :-1].reshape(-1, n), q[:, 1:].reshape(-1, n), resolution,
                                                      ee_offset)[1]
        return q, qd, seg_free.reshape(P, T - 1).all(axis=1)

    # -- the motion check (extension; include/optik.h) ------------------------------------
    def collision_motion_batch_arrays(self, xa, xb, resolution, ee_offset=None):
        """The straight joint-space motions xa[b] -> xb[b] ([B, n] each) sampled at `resolution` (L-infinity,
        radians) against the model and world: (clearance [B], free [B] bool, first [B] int32, steps [B] int32) --
        the minimum clearance over the samples, whether all of them are free, the lowest sample index that is not
        (-1: none), and the number of steps (-1: more than 4096 steps or a non-finite distance: not sampled,
        clearance NaN, free False)."""
        xa, xb = self._check_xs(xa), self._check_xs(xb)
        if xa.shape != xb.shape:
            raise ValueError(f"xa and xb must have the same shape, got {list(xa.shape)} and {list(xb.shape)}")
        h = nat.check_resolution(resolution)
        B = xa.shape[0]
        ee = _pose16(ee_offset) if ee_offset is not None else None
        clr, free = np.zeros(B), np.zeros(B, dtype=np.uint8)
        first, steps = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_collision_motion_batch(self._h, B, _dp(xa), _dp(xb), h,
                                                      _dp(ee) if ee is not None else None, _dp(clr),
                                                      free.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                      first.ctypes.data_as(ip), steps.ctypes.data_as(ip)):
            raise RuntimeError(_err(self._L))
        return clr, free.astype(bool), first, steps

    def collision_motion(self, xa, xb, resolution, ee_offset=None):
        """One motion: (clearance, free, first, steps) as Python scalars (see collision_motion_batch_arrays)."""
        xa, xb = self._check_x(xa), self._check_x(xb)
        clr, free, first, steps = self.collision_motion_batch_arrays(xa[None], xb[None], resolution, ee_offset)
        return float(clr[0]), bool(free[0]), int(first[0]), int(steps[0])

    # -- the certified motion check (extension; include/optik.h) ------------------------------
    def collision_motion_certify_batch_arrays(self, xa, xb, tol, grid_lipschitz=None, max_steps=nat.CERTIFY_STEPS,
                                              ee_offset=None):
        """Conservative advancement along the straight joint-space motions xa[b] -> xb[b] ([B, n] each) against the
        model and world: a dict of status [B] int32, steps [B] int32, t_stop [B], clearance [B].  Where
        collision_motion_batch_arrays says "free at the samples", status 0 (nat.CERTIFY_FREE) says that the clearance
        is >= margin - tol for EVERY t in [0, 1] (and >= margin at the `steps` samples it evaluated); 1
        (CERTIFY_BLOCKED) exhibits q(t_stop) = xa + t_stop (xb - xa), which is not free; 2 (CERTIFY_LIMIT) says
        nothing: max_steps samples were not enough -- a long grazing motion with a small tol, or a sphere outside an
        installed grid creeping up to a boundary behind which the field is low; 3 (CERTIFY_NAN): a NaN or infinite
        joint (steps 0, t_stop NaN) or a NaN frame.  A motion whose true minimum clearance is below margin - tol never
        comes back free, one whose minimum is >= margin never comes back blocked; in between either answer is right.
        clearance is the minimum over the evaluated samples (+inf without a model).  The statement is about the
        library's clearance function: with a grid world it inherits the trilinear field's sqrt(3) * voxel and is only
        as true as grid_lipschitz (None: sqrt(3), valid for every true distance field; collision.grid_lipschitz gives
        the constant of any other grid); floating-point rounding of the bounds is not accounted for, so tol is meant
        to be many orders above 1e-16.  ValueError for a tol or grid_lipschitz that is not finite and > 0 or a
        max_steps outside 2 .. 65 536."""
        xa, xb = self._check_xs(xa), self._check_xs(xb)
        if xa.shape != xb.shape:
            raise ValueError(f"xa and xb must have the same shape, got {list(xa.shape)} and {list(xb.shape)}")
        tol, G, max_steps = nat.check_certify_args(tol, grid_lipschitz, max_steps)
        B = xa.shape[0]
        ee = _pose16(ee_offset) if ee_offset is not None else None
        status, steps = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        t_stop, clr = np.zeros(B), np.zeros(B)
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_collision_motion_certify_batch(self._h, B, _dp(xa), _dp(xb), tol, G, max_steps,
                                                              _dp(ee) if ee is not None else None,
                                                              status.ctypes.data_as(ip), steps.ctypes.data_as(ip),
                                                              _dp(t_stop), _dp(clr)):
            raise RuntimeError(_err(self._L))
        return dict(status=status, steps=steps, t_stop=t_stop, clearance=clr)

    def collision_motion_certify(self, xa, xb, tol, grid_lipschitz=None, max_steps=nat.CERTIFY_STEPS, ee_offset=None):
        """One motion: (status, steps, t_stop, clearance) as Python scalars (see
        collision_motion_certify_batch_arrays)."""
        xa, xb = self._check_x(xa), self._check_x(xb)
        r = self.collision_motion_certify_batch_arrays(xa[None], xb[None], tol, grid_lipschitz, max_steps, ee_offset)
        return int(r["status"][0]), int(r["steps"][0]), float(r["t_stop"][0]), float(r["clearance"][0])

    def certify_paths(self, paths, lens=None, tol=0.01, grid_lipschitz=None, max_steps=nat.CERTIFY_STEPS,
                      ee_offset=None):
        """Certifies P joint-space paths `paths` [P, L, n] with `lens` [P] waypoints each (None: L each) -- plan_paths',
        shortcut_paths' or resample_paths' "paths" and "len" as they are: the len - 1 segments of every path go through
        ONE collision_motion_certify_batch_arrays call.  Returns a dict: status [P] int32, the worst of the path's
        segments in the order CERTIFY_NAN > CERTIFY_BLOCKED > CERTIFY_LIMIT > CERTIFY_FREE (a path of fewer than two
        waypoints has no segment: free); segment [P] int32, the first segment with that status, -1 when all are free;
        clearance [P], the minimum over the path's segments (NaN if one of them is NaN, +inf without segments)."""
        paths, lens = self._check_paths(paths, lens)
        nat.check_certify_args(tol, grid_lipschitz, max_steps)
        P, L, n = paths.shape
        lens = np.full(P, L, dtype=np.int32) if lens is None else lens
        nseg = max(L - 1, 0)
        valid = np.arange(nseg)[None, :] < (np.clip(lens, 0, L)[:, None] - 1)
        status = np.zeros((P, nseg), dtype=np.int32)
        clr = np.full((P, nseg), np.inf)
        if valid.any():
            r = self.collision_motion_certify_batch_arrays(paths[:, :-1][valid], paths[:, 1:][valid], tol,
                                                           grid_lipschitz, max_steps, ee_offset)
            status[valid], clr[valid] = r["status"], r["clearance"]
        # the order of badness: NAN 3 > BLOCKED 2 > LIMIT 1 > FREE 0
        rank_of = np.array([0, 2, 1, 3])
        rank = np.where(valid, rank_of[status], 0)
        worst = rank.max(axis=1) if nseg else np.zeros(P, dtype=np.int64)
        seg = np.where(worst > 0, (rank == worst[:, None]).argmax(axis=1) if nseg else 0, -1).astype(np.int32)
        out_status = np.array([nat.CERTIFY_FREE, nat.CERTIFY_LIMIT, nat.CERTIFY_BLOCKED, nat.CERTIFY_NAN],
                              dtype=np.int32)[worst]
        with np.errstate(invalid="ignore"):
            clearance = np.where(np.isnan(clr).any(axis=1), np.nan, clr.min(axis=1, initial=np.inf))
        return dict(status=out_status, segment=seg, clearance=clearance)

    # -- pose constraints (extension; include/optik.h) -------------------------------------
    def constraint_batch_arrays(self, xs, c, ee_offset=None):
        """(residual [B, 6], violation [B]) of B configurations xs [B, n] against the pose constraint c
        (optik_amd.PoseConstraint): r_i = e_i - min(max(e_i, lo_i), hi_i) of the pose error against c's reference,
        and max_i |r_i| (NaN for a NaN row).  x satisfies c at tol iff its violation is <= tol."""
        xs = self._check_xs(xs)
        ref7, lo, hi = constraint_arrays(c)
        B = xs.shape[0]
        ee = _pose16(ee_offset) if ee_offset is not None else None
        r, v = np.zeros((B, 6)), np.zeros(B)
        if self._L.optik_robot_constraint_batch(self._h, B, _dp(xs), _dp(ref7), _dp(lo), _dp(hi),
                                                _dp(ee) if ee is not None else None, _dp(r), _dp(v)):
            raise RuntimeError(_err(self._L))
        return r, v

    def constraint_project_batch_arrays(self, xs, c, tol=nat.CONSTRAINT_TOL, iters=nat.CONSTRAINT_ITERS,
                                        damping=nat.CONSTRAINT_DAMPING, max_step=nat.CONSTRAINT_MAX_STEP,
                                        ee_offset=None):
        """Projects B configurations xs [B, n] onto the set where c holds at tol, inside the joint limits, by damped
        Gauss-Newton (at most `iters` steps of at most max_step radians per joint): a dict of x [B, n], violation [B]
        (at x), status [B] int32 -- 0 projected: the violation is <= tol and x lies within the limits; 1 the steps
        are spent; 2 a NaN or infinite joint (the row comes back as it went in) or a failed factorisation -- and
        iterations [B] int32.  A row that satisfies c comes back unchanged after 0 iterations.  The defaults of iters,
        damping and max_step are the values read from one table (uniform Panda samples onto
        upright(home, 0.1)); they are that and nothing more.  ValueError for a tol, iters, damping or max_step out of
        range."""
        xs = self._check_xs(xs)
        ref7, lo, hi = constraint_arrays(c)
        tol, iters, damping, max_step = nat.check_project_args(tol, iters, damping, max_step)
        B, n = xs.shape
        ee = _pose16(ee_offset) if ee_offset is not None else None
        x, v = np.zeros((B, n)), np.zeros(B)
        status, its = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_constraint_project_batch(self._h, B, _dp(xs), _dp(ref7), _dp(lo), _dp(hi), tol, iters,
                                                        damping, max_step, _dp(ee) if ee is not None else None,
                                                        _dp(x), _dp(v), status.ctypes.data_as(ip),
                                                        its.ctypes.data_as(ip)):
            raise RuntimeError(_err(self._L))
        return dict(x=x, violation=v, status=status, iterations=its)

    def constraint_motion_batch_arrays(self, xa, xb, resolution, c, tol=nat.CONSTRAINT_TOL, ee_offset=None):
        """The straight joint-space motions xa[b] -> xb[b] ([B, n] each), sampled as collision_motion_batch_arrays
        samples them, against the pose constraint c: (violation [B], ok [B] bool, first [B] int32, steps [B] int32)
        -- the largest violation over the samples (NaN if any sample's is), whether every sample's is <= tol, the
        lowest sample index that is not (-1: none), and the number of steps (-1: not sampled; violation NaN, ok
        False).  Nothing is projected: it says what holds at the samples."""
        xa, xb = self._check_xs(xa), self._check_xs(xb)
        if xa.shape != xb.shape:
            raise ValueError(f"xa and xb must have the same shape, got {list(xa.shape)} and {list(xb.shape)}")
        h = nat.check_resolution(resolution)
        ref7, lo, hi = constraint_arrays(c)
        tol = nat.check_constraint_tol(tol)
        B = xa.shape[0]
        ee = _pose16(ee_offset) if ee_offset is not None else None
        v, ok = np.zeros(B), np.zeros(B, dtype=np.uint8)
        first, steps = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_constraint_motion_batch(self._h, B, _dp(xa), _dp(xb), h, _dp(ref7), _dp(lo), _dp(hi),
                                                       tol, _dp(ee) if ee is not None else None, _dp(v),
                                                       ok.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                       first.ctypes.data_as(ip), steps.ctypes.data_as(ip)):
            raise RuntimeError(_err(self._L))
        return v, ok.astype(bool), first, steps

    def check_paths_constraint(self, paths, lens, c, tol=nat.CONSTRAINT_TOL, resolution=nat.ROADMAP_RESOLUTION,
                               ee_offset=None):
        """Whether P joint-space paths `paths` [P, L, n] with `lens` [P] waypoints each (None: L each) keep the pose
        constraint c: the len - 1 segments of every path go through ONE constraint_motion_batch_arrays call.
        shortcut_paths, resample_paths and optimize_paths know nothing of constraints; this tells whether their output
        can still be used (shortcut_paths_constrained, resample_paths_constrained and optimize_paths_constrained
        keep one).  Returns a dict: violation [P], the largest over the path's segments (NaN if one of them is
        NaN or not sampled, 0 without segments); ok [P] bool, every segment ok; segment [P] int32, the first segment
        that is not, -1 when all are."""
        paths, lens = self._check_paths(paths, lens)
        P, L, n = paths.shape
        lens = np.full(P, L, dtype=np.int32) if lens is None else lens
        nseg = max(L - 1, 0)
        valid = np.arange(nseg)[None, :] < (np.clip(lens, 0, L)[:, None] - 1)
        v, ok = np.zeros((P, nseg)), np.ones((P, nseg), dtype=bool)
        if valid.any():
            sv, sok, _, _ = self.constraint_motion_batch_arrays(paths[:, :-1][valid], paths[:, 1:][valid], resolution,
                                                                c, tol, ee_offset)
            v[valid], ok[valid] = sv, sok
        with np.errstate(invalid="ignore"):
            worst = np.where(np.isnan(v).any(axis=1), np.nan, v.max(axis=1, initial=0.0))
        bad = ~ok
        seg = np.where(bad.any(axis=1), bad.argmax(axis=1) if nseg else 0, -1).astype(np.int32)
        return dict(violation=worst, ok=~bad.any(axis=1), segment=seg)

    def _device_chain(self):
        """The robot's own device chain (optik_robot_hip_chain) behind the HipChain interface: it carries the
        collision model and the world installed in the robot, which hip_chain()'s separate chain does not.  Borrowed:
        the robot owns it."""
        from .device import HipChain
        hc = getattr(self, "_own_chain", None)
        if hc is None:
            import torch
            h = self._L.optik_robot_hip_chain(self._h)
            if not h:
                raise RuntimeError(_err(self._L))

            class _Borrowed(HipChain):
                def close(self):
                    self._h = C.c_void_p()

            hc = _Borrowed.__new__(_Borrowed)
            hc.device = torch.device("cuda", torch.cuda.current_device())
            lb, ub = (np.ascontiguousarray(v, dtype=np.float64) for v in self.joint_limits())
            hc.n, hc.lb, hc.ub, hc._h = len(lb), lb, ub, C.c_void_p(h)
            self._own_chain = hc
        return hc

    def build_constrained_roadmap(self, c, tol=nat.CONSTRAINT_TOL, N=nat.ROADMAP_NODES, k=nat.ROADMAP_K,
                                  resolution=nat.ROADMAP_RESOLUTION, first=0, **project):
        """A roadmap whose every edge keeps the pose constraint c at tol, at the samples of `resolution`: N nodes
        drawn as build_roadmap draws them (the IK restart seeds first .. first + N - 1), each projected onto c
        (constraint_project_batch_arrays' method; **project: iters, damping, max_step), the ones that did not project
        dropped (NaN columns: they join nothing), the rest joined to their k nearest others where the motion node ->
        neighbour passes the collision check against the robot's model and world AND the constraint check.  Edges stay
        straight in joint space; nothing between the samples is projected.
        Returns the roadmap (optik_amd.constraint.ConstrainedRoadmap: device tensors, N, k, resolution, constraint,
        tol, projected).  It is the caller's object, as a depth map is: a change of the world, the collision model or
        the constraint needs a new one, and NO staleness guard exists here -- plan_constrained_paths plans over
        whatever it is given.  It does not touch the roadmap of build_roadmap."""
        import torch
        from .constraint import ConstrainedRoadmap
        nat.check_roadmap_args(N=N, k=k)
        h = nat.check_resolution(resolution)
        hc = self._device_chain()
        seeds = hc.seed_batch(int(first), int(N))
        p = hc.constraint_project_batch(seeds, c, tol, **project)
        okp = p["status"] == nat.CONSTRAINT_PROJECTED
        nodes = torch.where(okp[None, :], p["x"], torch.full_like(p["x"], float("nan"))).contiguous()
        nbr, w = hc.roadmap_build_constrained(nodes, int(k), h, c, tol)
        return ConstrainedRoadmap(nodes, nbr, w, h, c, tol, int(okp.sum().item()))

    def plan_constrained_paths(self, roadmap, starts, goals, max_waypoints=nat.PATH_OPTIMIZE_MAX_WAYPOINTS):
        """plan_paths over a roadmap of build_constrained_roadmap, for Q pairs starts[q] -> goals[q] ([Q, n] each):
        the start links, the goal links and the direct motion pass the collision check and the roadmap's constraint
        check, as its edges did.  So every segment of a found path is a motion that passed both checks in the
        direction of travel, at the samples; a start or a goal that violates the constraint has no link and comes
        back with status 1.  Returns plan_paths' dict (paths [Q, max_waypoints, n], len, cost, status).  The roadmap
        is used as it is: rebuild it after a change of the world or the model."""
        import torch
        starts, goals = self._check_xs(starts), self._check_xs(goals)
        if starts.shape != goals.shape:
            raise ValueError(f"starts and goals must have the same shape, got {list(starts.shape)} and "
                             f"{list(goals.shape)}")
        nat.check_roadmap_args(max_waypoints=max_waypoints)
        hc = self._device_chain()
        dev = roadmap.nodes.device
        s = torch.from_numpy(np.ascontiguousarray(starts.T)).to(dev)
        g = torch.from_numpy(np.ascontiguousarray(goals.T)).to(dev)
        r = hc.roadmap_plan_constrained((roadmap.nodes, roadmap.nbr, roadmap.w), s, g, min(roadmap.k, roadmap.N),
                                        int(max_waypoints), roadmap.resolution, roadmap.constraint, roadmap.tol)
        return dict(paths=np.ascontiguousarray(r["path"].cpu().numpy().transpose(1, 0, 2)),
                    len=r["len"].cpu().numpy(), cost=r["cost"].cpu().numpy(), status=r["status"].cpu().numpy())

    # -- the tree planner under a pose constraint (extension; include/optik.h) --------------
    def plan_rrt_to_goals_constrained(self, starts, goals, c, counts=None, *, tol, iters=None, step=None,
                                      resolution=nat.ROADMAP_RESOLUTION, first=0, max_nodes=None,
                                      max_waypoints=nat.PATH_OPTIMIZE_MAX_WAYPOINTS, poll=nat.RRT_POLL,
                                      ptol=nat.CONSTRAINT_TOL, piters=nat.RRT_PROJECT_ITERS,
                                      damping=nat.CONSTRAINT_DAMPING, max_step=nat.CONSTRAINT_MAX_STEP, ee_offset=None):
        """plan_rrt_to_goals under the pose constraint c ("carry the glass upright"): the fallback for the rows
        plan_constrained_paths returns with status 1.  starts [Q, n], goals [Q, G, n], counts [Q] or None as there.
        Two trees per query grow as plan_rrt's do, but every candidate node is first projected onto c
        (constraint_project_batch_arrays' method at ptol, at most piters iterations, damping, max_step) and a
        projection that fails costs the iteration; every motion a tree or the junction takes has passed the collision
        check AND constraint_motion_batch_arrays at tol, at `resolution`, in the direction the path travels it.  A
        start that violates c at tol gives status 1; a goal that does is no root.  tol has no default: as for
        build_constrained_roadmap it is the caller's statement of how far the straight joint-space motion between two
        nodes on the constraint may leave it -- edge interiors are not projected.
        Returns plan_rrt_to_goals' dict plus "projected" [Q, 2] int32: the projections attempted and the ones that
        ended projected.  With a box that is free on all six axes the shared outputs are plan_rrt_to_goals', bit for
        bit.  "paths" and "len" go into check_paths_constraint, certify_paths and time_paths as they are; a tree's
        path has a corner at every waypoint, so give time_paths a v_max the corners can be taken at (its status 1
        says the limits were too fast for them; DESIGN.md section 5.30 has the example's figures).
        shortcut_paths_constrained, resample_paths_constrained and optimize_paths_constrained shorten, respace and
        smooth it with c kept; shortcut_paths, resample_paths and optimize_paths know nothing of constraints: check
        their output with check_paths_constraint before using it.
        It keeps no state in the robot and reads no roadmap.  The default of piters (nat.RRT_PROJECT_ITERS) is read
        from one table and is that and nothing more; the other defaults are plan_rrt's and
        the projection's.  ValueError for what plan_rrt_to_goals and the constraint calls refuse."""
        starts = self._check_xs(starts)
        Q, n = starts.shape
        goals = np.ascontiguousarray(goals, dtype=np.float64)
        if goals.ndim != 3 or goals.shape[0] != Q or goals.shape[2] != n:
            raise ValueError(f"goals must be [Q, G, n] = [{Q}, G, {n}], got {list(goals.shape)}")
        if counts is not None:
            counts = np.ascontiguousarray(counts, dtype=np.int32)
            if counts.shape != (Q,):
                raise ValueError(f"counts must be [Q] = [{Q}], got {list(counts.shape)}")
        iters, step, max_nodes, poll, first = nat.check_rrt_args(iters, step, max_nodes, max_waypoints, poll, first)
        G = nat.check_rrt_goals(goals.shape[1], max_nodes)
        h = nat.check_resolution(resolution)
        ref7, lo, hi = constraint_arrays(c)
        tol = nat.check_constraint_tol(tol)
        ptol, piters, damping, max_step = nat.check_project_args(ptol, piters, damping, max_step)
        L = int(max_waypoints)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        paths, cost = np.zeros((Q, L, n)), np.zeros(Q)
        ln, status, it, goal = (np.zeros(Q, dtype=np.int32) for _ in range(4))
        nodes, projected = np.zeros((Q, 2), dtype=np.int32), np.zeros((Q, 2), dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_rrt_plan_constrained(
                self._h, _dp(starts), _dp(goals), counts.ctypes.data_as(ip) if counts is not None else None, G, Q,
                _dp(ref7), _dp(lo), _dp(hi), tol, ptol, piters, damping, max_step, iters, step, h, first, max_nodes, L,
                poll, _dp(ee) if ee is not None else None, _dp(paths), ln.ctypes.data_as(ip), _dp(cost),
                status.ctypes.data_as(ip), it.ctypes.data_as(ip), nodes.ctypes.data_as(ip), goal.ctypes.data_as(ip),
                projected.ctypes.data_as(ip)):
            raise RuntimeError(_err(self._L))
        return dict(paths=paths, len=ln, cost=cost, status=status, iters=it, nodes=nodes, goal=goal,
                    projected=projected)

    def plan_rrt_constrained(self, starts, goals, c, *, tol, **kwargs):
        """plan_rrt under the pose constraint c, for Q pairs starts[q] -> goals[q] ([Q, n] each):
        plan_rrt_to_goals_constrained with one goal per query (its keyword arguments, its dict: "goal" is 0 where
        the status is 0).  Its paths go into shortcut_paths_constrained, resample_paths_constrained,
        check_paths_constraint, certify_paths and time_paths as they are, and what resample_paths_constrained makes
        of them into optimize_paths_constrained."""
        starts, goals = self._check_xs(starts), self._check_xs(goals)
        if starts.shape != goals.shape:
            raise ValueError(f"starts and goals must have the same shape, got {list(starts.shape)} and "
                             f"{list(goals.shape)}")
        return self.plan_rrt_to_goals_constrained(starts, goals[:, None, :], c, None, tol=tol, **kwargs)

    # -- IK into pose regions and planning to them (extension; include/optik.h) --------------
    def ik_region_batch_arrays(self, config: SolverConfig, regions, x0s, k=8, min_dist=0.1,
                               restarts=nat.REGION_RESTARTS, tol=nat.CONSTRAINT_TOL, iters=nat.CONSTRAINT_ITERS,
                               damping=nat.CONSTRAINT_DAMPING, max_step=nat.CONSTRAINT_MAX_STEP, keep=None,
                               ee_offset=None, repair=None):
        """Up to k distinct configurations per pose REGION: ik_solutions_batch_arrays whose target is a box on the
        pose error (optik_amd.PoseConstraint -- position_only, axis_free, around, upright or any box) instead of an
        exact pose.  regions: one PoseConstraint, broadcast over the rows of x0s [T, n], or a sequence of T.  Every
        restart index in [0, restarts) runs: restart 0 from x0s[t], restart i > 0 from the IK restart seed i, each
        projected onto the region by constraint_project_batch_arrays' method (tol, iters, damping, max_step).  The
        rows that projected are ranked by config.solution_mode (quality: nearest x0s[t] first; speed: lowest index;
        manipulability / condition), and taken greedily if more than min_dist (L-infinity) from every row taken
        before.  With a collision model installed only free rows are taken; keep = (PoseConstraint, tol) drops the
        rows that violate that second constraint at tol (nothing is projected onto it).  Only solution_mode is read
        of config.
        Returns a dict: count [T] int32, x [T, k, n] (NaN past count), violation [T, k] (NaN), idx [T, k] uint64
        (2^64 - 1), key [T, k] (+inf).  Every returned row satisfies its region at tol, lies within the joint limits,
        is collision-free under a model, and is more than min_dist from the rows before it.  Gauss-Newton from a seed
        is not the SLSQP solver of ik(): it may miss what ik() finds on a pinned region, and nothing is promised
        about how the rows cover the region's solution manifold.  ValueError for a bad region (naming the row), k,
        min_dist, restarts, keep or projection argument.
        repair = dict(influence, safety, step=.., iters=.., max_move=inf) (repair_configurations' parameters; DESIGN.md
        section 5.37): with a collision model, a restart that projected but is in collision is not thrown away at once:
        it is first pushed free under its own region at tol, and takes part in the ranking with its repaired x if that
        ends free (re-measured against keep).  The dict then also has repaired [T] int32, the restarts of each region
        that took a repaired x (zeros without repair).  repair=None is the call without the argument, bit for bit.
        Chains of 1 .. 8 joints with a model."""
        from .constraint import keep_arrays, region_rows
        x0s = self._check_xs(x0s)
        T, n = x0s.shape
        reg = region_rows(regions, T)
        k, min_dist = nat.check_solutions_args(k, min_dist)
        restarts = nat.check_region_restarts(restarts)
        tol, iters, damping, max_step = nat.check_project_args(tol, iters, damping, max_step)
        kp = keep_arrays(keep)
        mode = nat.solution_mode_code(config.solution_mode)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        count = np.zeros(T, dtype=np.int32)
        x, v, key = np.full((T, k, n), np.nan), np.full((T, k), np.nan), np.full((T, k), np.inf)
        idx = np.full((T, k), U64_MAX, dtype=np.uint64)
        repaired = np.zeros(T, dtype=np.int32)
        head = (self._h, T, _dp(reg), _dp(x0s), restarts, tol, iters, damping, max_step, mode,
                _dp(kp[0]) if kp else None, _dp(kp[1]) if kp else None, _dp(kp[2]) if kp else None,
                kp[3] if kp else 0.0, k, min_dist)
        tail = (_dp(ee) if ee is not None else None, count.ctypes.data_as(C.POINTER(C.c_int32)), _dp(x), _dp(v),
                idx.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(key))
        if repair is None:
            rc = self._L.optik_robot_ik_region(*head, *tail)
        else:
            rp = nat.region_repair_args(repair)
            r5 = np.array([rp[0], rp[1], rp[2], rp[3], rp[4]], dtype=np.float64)
            rc = self._L.optik_robot_ik_region_repair(*head, _dp(r5), *tail,
                                                      repaired.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc:
            raise RuntimeError(_err(self._L))
        return dict(count=count, x=x, violation=v, idx=idx, key=key, repaired=repaired)

    def ik_region(self, config: SolverConfig, region, x0, **kwargs):
        """The single-region form of ik_region_batch_arrays (its keyword arguments): a list of up to k
        configurations inside `region`, best first; empty when no restart projected."""
        r = self.ik_region_batch_arrays(config, region, np.asarray(x0, dtype=np.float64)[None], **kwargs)
        return [r["x"][0, j].copy() for j in range(int(r["count"][0]))]

    def _region_goals(self, config, starts, regions, k, min_dist, region_args):
        k = nat.check_roadmap_goals(k)
        starts = self._check_xs(starts)
        r = self.ik_region_batch_arrays(config, regions, starts, k=k, min_dist=min_dist, **region_args)
        return starts, r["x"], r["count"]

    def plan_to_region(self, config: SolverConfig, starts, regions, k=8, min_dist=0.1,
                       max_waypoints=nat.PATH_OPTIMIZE_MAX_WAYPOINTS, ee_offset=None, region_args=None):
        """plan_to_poses with pose regions in the place of the poses ("put it anywhere on this shelf"): starts [Q, n],
        regions one PoseConstraint or Q of them.  ik_region_batch_arrays with the starts as x0s gives up to k <= 16
        goals per region (region_args: a dict of its restarts, tol, iters, damping, max_step, keep), and plan_to_goals
        plans to the nearest of them over the roadmap.  Returns plan_to_goals' dict plus "goals" [Q, k, n] and "count" [Q];
        a region nothing projected onto has count 0, status 1 and goal -1.  Eager roadmaps only, as plan_to_goals."""
        if getattr(self, "_roadmap_lazy", False):
            raise RuntimeError(self._LAZY_GOALS_MSG)
        starts, x, count = self._region_goals(config, starts, regions, k, min_dist,
                                              dict(region_args or {}, ee_offset=ee_offset))
        res = self.plan_to_goals(starts, x, counts=count, max_waypoints=max_waypoints)
        res["goals"], res["count"] = x, count
        return res

    def plan_to_region_lazy(self, config: SolverConfig, starts, regions, k=8, min_dist=0.1,
                            max_waypoints=nat.PATH_OPTIMIZE_MAX_WAYPOINTS, rounds=None, ee_offset=None,
                            region_args=None):
        """plan_to_region over a lazy roadmap: ik_region_batch_arrays with the starts as x0s (region_args: a dict of its
        own arguments), then plan_to_goals_lazy.  Returns plan_to_goals_lazy's dict plus "goals" [Q, k, n] and "count"
        [Q]; a region nothing projected onto has count 0, status 1 and goal -1."""
        self._need_lazy_roadmap()
        starts, x, count = self._region_goals(config, starts, regions, k, min_dist,
                                              dict(region_args or {}, ee_offset=ee_offset))
        res = self.plan_to_goals_lazy(starts, x, counts=count, max_waypoints=max_waypoints, rounds=rounds)
        res["goals"], res["count"] = x, count
        return res

    def plan_rrt_to_region(self, config: SolverConfig, starts, regions, k=8, min_dist=0.1, iters=None, step=None,
                           resolution=nat.ROADMAP_RESOLUTION, first=0, max_nodes=None,
                           max_waypoints=nat.PATH_OPTIMIZE_MAX_WAYPOINTS, poll=nat.RRT_POLL, ee_offset=None,
                           region_args=None):
        """plan_rrt_to_poses with pose regions in the place of the poses: ik_region_batch_arrays with the starts as
        x0s (region_args: a dict of its restarts, tol, iters, damping, max_step, keep), then plan_rrt_to_goals.
        Returns plan_rrt_to_goals' dict plus "goals" [Q, k, n] and "count" [Q] int32; count 0 is status 1 and goal -1."""
        starts, x, count = self._region_goals(config, starts, regions, k, min_dist,
                                              dict(region_args or {}, ee_offset=ee_offset))
        res = self.plan_rrt_to_goals(starts, x, counts=count, iters=iters, step=step, resolution=resolution,
                                     first=first, max_nodes=max_nodes, max_waypoints=max_waypoints, poll=poll,
                                     ee_offset=ee_offset)
        res["goals"], res["count"] = x, count
        return res

    def plan_rrt_to_region_constrained(self, config: SolverConfig, starts, regions, c, *, tol, k=8, min_dist=0.1,
                                       region_args=None, ee_offset=None, **kwargs):
        """plan_rrt_to_region under the path constraint c at tol ("carry the glass upright to anywhere on the
        shelf"): ik_region_batch_arrays with keep = (c, tol), so every goal satisfies the path constraint, then
        plan_rrt_to_goals_constrained (**kwargs: its iters, step, resolution, ptol, piters, ...; region_args: a dict
        of ik_region_batch_arrays' own).  Returns plan_rrt_to_goals_constrained's dict plus "goals" and "count"."""
        starts, x, count = self._region_goals(config, starts, regions, k, min_dist,
                                              dict(region_args or {}, keep=(c, tol), ee_offset=ee_offset))
        res = self.plan_rrt_to_goals_constrained(starts, x, c, count, tol=tol, ee_offset=ee_offset, **kwargs)
        res["goals"], res["count"] = x, count
        return res

    # -- shortcutting and resampling under a pose constraint (extension; include/optik.h) ----
    def shortcut_paths_constrained(self, paths, lens, c, *, tol, resolution=nat.SHORTCUT_RESOLUTION,
                                   vertices=nat.SHORTCUT_VERTICES, hop_penalty=None, max_waypoints=None,
                                   ptol=nat.CONSTRAINT_TOL, iters=nat.CONSTRAINT_ITERS, damping=nat.CONSTRAINT_DAMPING,
                                   max_step=nat.CONSTRAINT_MAX_STEP, ee_offset=None):
        """shortcut_paths under the pose constraint c: what follows plan_rrt_constrained or plan_constrained_paths.
        paths [P, L, n], lens [P] or None as there.  Each polyline is subdivided as shortcut_paths subdivides it; the
        input's own waypoints, the start and the goal among them, are vertices as they are and never move; every other
        vertex is projected onto c (constraint_project_batch_arrays' method at ptol, at most `iters` iterations,
        damping, max_step) and a vertex that does not project is dropped.  A pair of vertices is joined only where the
        motion between them passes the collision check AND constraint_motion_batch_arrays at `resolution`, tol, in the
        direction of travel; the route of least (length + hop_penalty) per hop is walked.  So with status 0 every
        new vertex has violation <= ptol and lies within the joint limits, and every segment has passed both checks at
        the samples -- check_paths_constraint at the same tol and resolution says ok.  tol has no default: as for
        plan_rrt_constrained it is the caller's statement of how far the straight motion between two vertices on the
        constraint may leave it; segment interiors are not projected.
        Returns shortcut_paths' dict plus "projected" [P, 2] int32: the projections attempted and the ones that ended
        projected.  cost can exceed cost_in, because projected vertices leave the input's polyline: compare the two.
        With a box that is free on all six axes and paths within the joint limits the shared outputs are
        shortcut_paths', bit for bit.  ValueError for what shortcut_paths and the constraint calls refuse."""
        paths, lens = self._check_paths(paths, lens)
        P, L, n = paths.shape
        Lout = L if max_waypoints is None else max_waypoints
        h, hop = nat.check_shortcut_args(L, vertices, Lout, resolution, hop_penalty)
        Lout = int(Lout)
        ref7, lo, hi = constraint_arrays(c)
        tol = nat.check_constraint_tol(tol)
        ptol, iters, damping, max_step = nat.check_project_args(ptol, iters, damping, max_step)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        out, cost, cost_in = np.zeros((P, Lout, n)), np.zeros(P), np.zeros(P)
        ln, status = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32)
        projected = np.zeros((P, 2), dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_path_shortcut_constrained(
                self._h, P, L, _dp(paths), lens.ctypes.data_as(ip) if lens is not None else None, int(vertices), h, hop,
                Lout, _dp(ref7), _dp(lo), _dp(hi), tol, ptol, iters, damping, max_step,
                _dp(ee) if ee is not None else None, _dp(out), ln.ctypes.data_as(ip), _dp(cost), _dp(cost_in),
                status.ctypes.data_as(ip), projected.ctypes.data_as(ip)):
            raise RuntimeError(_err(self._L))
        return dict(paths=out, len=ln, cost=cost, cost_in=cost_in, status=status, projected=projected)

    def resample_paths_constrained(self, paths, lens, c, waypoints=nat.RESAMPLE_WAYPOINTS, resolution=None, tol=None,
                                   ptol=nat.CONSTRAINT_TOL, iters=nat.CONSTRAINT_ITERS, damping=nat.CONSTRAINT_DAMPING,
                                   max_step=nat.CONSTRAINT_MAX_STEP, ee_offset=None):
        """resample_paths with every waypoint between the two ends projected onto the pose constraint c
        (constraint_project_batch_arrays' method at ptol, `iters`, damping, max_step): the dense path time_paths and a
        controller take, its waypoints on the constraint.  The ends are copied.  The spacing is equal before the
        projection and only approximately equal after it.  Returns (paths [P, waypoints, n], status [P] int32,
        projected [P, 2] int32): status 0; 2 a length outside 2 .. L; 3 a NaN or infinite length (nothing is
        projected); 4 an interior waypoint could not be projected and kept its interpolated value (it ranks below 2
        and 3); projected as in shortcut_paths_constrained.  The new segments are NOT checked by construction: with
        `resolution` and `tol` (both or neither) it also returns free [P] bool and ok [P] bool, whether each of the
        waypoints - 1 new segments passes collision_motion_batch_arrays and constraint_motion_batch_arrays at tol.
        ValueError for what resample_paths and the constraint calls refuse."""
        paths, lens = self._check_paths(paths, lens)
        P, L, n = paths.shape
        nat.check_shortcut_args(L, max_waypoints=waypoints)
        if (resolution is None) != (tol is None):
            raise ValueError("resolution and tol go together: give both for the two checks of the new segments, or neither")
        if resolution is not None:
            resolution, tol = nat.check_resolution(resolution), nat.check_constraint_tol(tol)
        ref7, lo, hi = constraint_arrays(c)
        ptol, iters, damping, max_step = nat.check_project_args(ptol, iters, damping, max_step)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        W = int(waypoints)
        out, status = np.zeros((P, W, n)), np.zeros(P, dtype=np.int32)
        projected = np.zeros((P, 2), dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_path_resample_constrained(
                self._h, P, L, _dp(paths), lens.ctypes.data_as(ip) if lens is not None else None, W, _dp(ref7), _dp(lo),
                _dp(hi), ptol, iters, damping, max_step, _dp(ee) if ee is not None else None, _dp(out),
                status.ctypes.data_as(ip), projected.ctypes.data_as(ip)):
            raise RuntimeError(_err(self._L))
        if resolution is None:
            return out, status, projected
        qa, qb = out[:, :-1].reshape(-1, n), out[:, 1:].reshape(-1, n)
        seg_free = self.collision_motion_batch_arrays(qa, qb, resolution, ee_offset)[1]
        seg_ok = self.constraint_motion_batch_arrays(qa, qb, resolution, c, tol, ee_offset)[1]
        return out, status, projected, seg_free.reshape(P, W - 1).all(axis=1), seg_ok.reshape(P, W - 1).all(axis=1)

    # -- path optimisation under a pose constraint (extension; include/optik.h) ---------------
    def optimize_paths_constrained(self, paths, c, iters=nat.PATH_OPTIMIZE_ITERS, step=nat.PATH_OPTIMIZE_STEP,
                                   w_smooth=nat.PATH_OPTIMIZE_W_SMOOTH, w_obs=nat.PATH_OPTIMIZE_W_OBS, influence=0.2,
                                   safety=0.05, resolution=None, tol=None, ptol=nat.CONSTRAINT_TOL,
                                   iters_project=nat.CONSTRAINT_ITERS, damping=nat.CONSTRAINT_DAMPING,
                                   max_step=nat.CONSTRAINT_MAX_STEP, ee_offset=None):
        """optimize_paths under the pose constraint c: what follows resample_paths_constrained.  Projected covariant
        gradient smoothing: each of the `iters` updates is optimize_paths' update, the clamp to the joint limits
        included, and then every interior waypoint is projected back onto c (constraint_project_batch_arrays' method at
        ptol, at most `iters_project` iterations, damping, max_step).  A waypoint whose projection does not end
        projected keeps its value of the previous iterate, so an interior waypoint that satisfies c at ptol on input
        satisfies it in the result; the two ends never move and are never projected.
        What it is not: the projection follows the step, it is not constrained CHOMP's projection in the metric, so
        the projected update is no longer the covariant one.  The waypoints satisfy c at ptol; the segments BETWEEN
        them are straight in joint space, are not projected and are only checked on request.  `step` has
        optimize_paths' caveats (it has to shrink as L^2 grows).
        Returns a dict: paths [P, L, n], cost_first [P, 3], cost_last [P, 3], clearance [P], status [P] int32 as
        optimize_paths returns them; violation [P], the largest violation over all L waypoints of the result (NaN if
        one is); projected [P, 2] int32, the projections attempted over all updates and those that ended projected.
        With `resolution` also free [P] bool: every segment of the result passes collision_motion_batch_arrays.  With
        `resolution` and `tol` also keeps [P] bool: every segment passes check_paths_constraint at tol (tol without
        a resolution is a ValueError).  With a box that is free on all six axes nothing is projected and the shared
        outputs are optimize_paths', bit for bit.
        ValueError for what optimize_paths and the constraint calls refuse."""
        n = self.num_positions()
        paths = np.ascontiguousarray(paths, dtype=np.float64)
        if paths.ndim != 3 or paths.shape[2] != n:
            raise ValueError(f"paths must be [P, L, n] with n = {n}, got {list(paths.shape)}")
        P, L = paths.shape[0], paths.shape[1]
        nat.check_path_optimize_args(L, iters, step, w_smooth, w_obs, influence, safety)
        if tol is not None and resolution is None:
            raise ValueError("tol needs a resolution: the segments are checked at its samples")
        if resolution is not None:
            resolution = nat.check_resolution(resolution)
        if tol is not None:
            tol = nat.check_constraint_tol(tol)
        ref7, lo, hi = checked_constraint_arrays(c)
        ptol, piters, damping, max_step = nat.check_project_args(ptol, iters_project, damping, max_step)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        out = np.zeros((P, L, n))
        first, last, clr, viol = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros(P), np.zeros(P)
        status, projected = np.zeros(P, dtype=np.int32), np.zeros((P, 2), dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_path_optimize_constrained(
                self._h, P, L, _dp(paths), int(iters), float(step), float(w_smooth), float(w_obs), float(influence),
                float(safety), _dp(ref7), _dp(lo), _dp(hi), ptol, piters, damping, max_step,
                _dp(ee) if ee is not None else None, _dp(out), _dp(first), _dp(last), _dp(clr),
                status.ctypes.data_as(ip), _dp(viol), projected.ctypes.data_as(ip)):
            raise RuntimeError(_err(self._L))
        res = dict(paths=out, cost_first=first, cost_last=last, clearance=clr, violation=viol, projected=projected,
                   status=status)
        if resolution is not None:
            seg_free = self.collision_motion_batch_arrays(out[:, :-1].reshape(-1, n), out[:, 1:].reshape(-1, n),
                                                          resolution, ee_offset)[1]
            res["free"] = seg_free.reshape(P, L - 1).all(axis=1)
            if tol is not None:
                res["keeps"] = self.check_paths_constraint(out, None, c, tol, resolution, ee_offset)["ok"]
        return res

    # -- collision repair (extension; include/optik.h) --------------------------------------
    def repair_configurations(self, xs, influence, safety, step=nat.REPAIR_STEP, iters=nat.REPAIR_ITERS,
                              region=None, max_move=np.inf, tol=nat.CONSTRAINT_TOL,
                              iters_project=nat.CONSTRAINT_ITERS, damping=nat.CONSTRAINT_DAMPING,
                              max_step=nat.CONSTRAINT_MAX_STEP, ee_offset=None):
        """Pushes configurations out of collision: the start state that sensor noise put a few millimetres inside a
        table, the IK solution that ends a few centimetres inside an obstacle.  Every row of xs [B, n] on its own
        steps by `step` down the gradient of optimize_paths' hinge (influence, safety) of its clearance witnesses,
        clamped to the joint limits, until its clearance -- collision_clearance_batch_arrays' number -- is >= safety,
        at most `iters` steps.  With `region` (a PoseConstraint) every step is projected back onto that pose box
        (constraint_project_batch_arrays' method at tol, at most iters_project iterations, damping, max_step), so a
        redundant arm slides out through its null space while the tool stays inside the box.  max_move bounds the
        L-infinity distance of the result from the input.  A fixed step without a line search; the defaults of step
        and iters are the values that clear the scenes of examples/ik_repair.py, and nothing more.
        Returns a dict: x [B, n], clearance [B], violation [B] (of the region; 0 without one), moved [B], status [B]
        int32 -- 0 free (with iterations > 0 also within the joint limits and inside the region at tol; with
        iterations == 0 the row was free already and is returned bit for bit), 1 iters spent, 2 stuck (no gradient,
        a projection that failed, or max_move reached: x is the last accepted iterate), 3 a NaN -- and iterations [B]
        int32.  Revolute chains of 1 .. 8 joints with a collision model.
        ValueError for what the kernel layer refuses of the parameters and the region."""
        n = self.num_positions()
        xs = np.ascontiguousarray(xs, dtype=np.float64)
        if xs.ndim != 2 or xs.shape[1] != n:
            raise ValueError(f"xs must be [B, n] with n = {n}, got {list(xs.shape)}")
        B = xs.shape[0]
        influence, safety, step, iters, max_move = nat.check_repair_args(influence, safety, step, iters, max_move)
        box = (None, None, None)
        keep = None
        if region is not None:
            keep = checked_constraint_arrays(region)
            box = tuple(_dp(a) for a in keep)
            tol, iters_project, damping, max_step = nat.check_project_args(tol, iters_project, damping, max_step)
        piters = int(iters_project)
        ee = _pose16(ee_offset) if ee_offset is not None else None
        x, clr, viol, moved = np.zeros((B, n)), np.zeros(B), np.zeros(B), np.zeros(B)
        status, iterations = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        if self._L.optik_robot_collision_repair_batch(
                self._h, B, _dp(xs), influence, safety, step, iters, max_move, *box, float(tol), piters, float(damping),
                float(max_step),
                _dp(ee) if ee is not None else None, _dp(x), _dp(clr), _dp(viol), _dp(moved),
                status.ctypes.data_as(ip), iterations.ctypes.data_as(ip)):
            raise RuntimeError(_err(self._L))
        return dict(x=x, clearance=clr, violation=viol, moved=moved, status=status, iterations=iterations)

    def set_motion_resolution(self, h):
        """The resolution of ik_path*'s motion check (0, the default: off).  While it is > 0 and a collision model is
        set, a waypoint's candidates are only the successes whose straight joint-space motion from the path's seed is
        free at this resolution, so consecutive accepted waypoints are joined by checked motions.  A start
        configuration in collision blocks every motion from it.  Applied to every GPU of the robot; ik, ik_batch* and
        ik_solutions* ignore it.  ValueError for a NaN, negative or infinite h."""
        if self._L.optik_robot_set_motion_resolution(self._h, nat.check_resolution(h, allow_zero=True)):
            raise ValueError(_err(self._L))

    # -- extensions ---------------------------------------------------------------
    def chain_tables(self):
        """Flat chain (types, origins[J,7], axes[J,3], lb, ub) as loaded by the C++ URDF loader."""
        nj = C.c_int32(0)
        # first call: joint count only (NULL buffers), then buffers of exactly that size
        if self._L.optik_robot_chain_tables_n(self._h, 0, C.byref(nj), None, None, None):
            raise RuntimeError(_err(self._L))
        origins, axes = np.zeros(nj.value * 7), np.zeros(nj.value * 3)
        types = np.zeros(nj.value, dtype=np.int32)
        if self._L.optik_robot_chain_tables_n(self._h, nj.value, C.byref(nj), _dp(origins), _dp(axes),
                                              types.ctypes.data_as(C.POINTER(C.c_int32))):
            raise RuntimeError(_err(self._L))
        J = nj.value
        lb, ub = self.joint_limits()
        return dict(types=types[:J].copy(), origins=origins[:J * 7].reshape(J, 7).copy(),
                    axes=axes[:J * 3].reshape(J, 3).copy(), lb=np.array(lb), ub=np.array(ub))

    def hip_chain(self, device="cuda:0"):
        """Device-buffer interface (optik_amd.device.HipChain) for this robot."""
        from .device import HipChain
        key = str(device)
        if key not in self._hip:
            self._hip[key] = HipChain(device=device, **self.chain_tables())
        return self._hip[key]
