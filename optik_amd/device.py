"""Device-buffer front end over the kernel-layer C ABI (``include/optik_hip.h``).

PyTorch is used only as plumbing: HBM allocation, streams, and (in ``bench.py``)
``torch.distributed``.  All arithmetic happens in the HIP kernels of
``csrc/ik_capi.hip``; nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _native as nat
from .constraint import checked_constraint_arrays, constraint_arrays, keep_arrays


def _stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _dpn(a):
    """_dp, or a null pointer for None (an end-effector offset that was not given)."""
    return _dp(a) if a is not None else None


def _box_ptrs(arrays):
    """The three pointers a constraint entry takes (ref7, lo6, hi6), of a PoseConstraint's arrays
    (constraint.constraint_arrays); each keeps its array alive."""
    ref7, lo, hi = arrays
    return _dp(ref7), _dp(lo), _dp(hi)


class LazyRoadmap:
    """The state of a lazy roadmap (HipChain.roadmap_build_lazy), device tensors: nodes
    [n, N], nbr [k, N] int32, the unchecked weights w0 [k, N], the working weights w [k, N] (w0, +inf where blocked:
    the graph roadmap_query sees), verdict [k, N] int32 (nat.ROADMAP_SLOT_UNKNOWN / _FREE / _BLOCKED), and the
    resolution its edges are checked at.  roadmap_plan_lazy updates w and verdict in place."""

    def __init__(self, nodes, nbr, w0, w, verdict, resolution):
        self.nodes, self.nbr, self.w0, self.w, self.verdict = nodes, nbr, w0, w, verdict
        self.resolution = float(resolution)


class HipChain:
    """A flat kinematic chain uploaded to the GPU (optik_hip_chain).

    Every batch operator is stream-ordered on the current stream and returns without waiting for the device, with
    one exception: roadmap_plan_lazy and roadmap_plan_goals_lazy (and their test hooks, and the _poses_lazy and
    _region_lazy forms) run their loop on the host and read one or two int32 per round, so they synchronise the
    current stream once per round of checks they make.
    roadmap_plan keeps its promise of no host synchronisation."""

    def __init__(self, types, origins, axes, lb, ub, device="cuda:0"):
        if not torch.cuda.is_available():
            raise nat.OptikHipError("no GPU visible to torch; optik_amd has no CPU fallback")
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        types = np.ascontiguousarray(types, dtype=np.int32)
        origins = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 7)
        axes = np.ascontiguousarray(axes, dtype=np.float64).reshape(-1, 3)
        lb = np.ascontiguousarray(lb, dtype=np.float64)
        ub = np.ascontiguousarray(ub, dtype=np.float64)
        self.n = int(len(lb))
        self.lb, self.ub = lb, ub
        self._h = C.c_void_p()
        nat.check(nat.lib().optik_hip_chain_create(
            _dp(origins), _dp(axes), types.ctypes.data_as(C.POINTER(C.c_int32)), len(types),
            _dp(lb), _dp(ub), self.n, C.byref(self._h)))

    def close(self):
        if self._h:
            nat.lib().optik_hip_chain_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_range_rule(self, rule):
        """Which rand 0.9.2 code path the restart seeds follow (nat.RANGE_*; optik_hip.h)."""
        nat.check(nat.lib().optik_hip_chain_set_range_rule(self._h, int(rule)))

    # -- batched primitives ----------------------------------------------------
    def eval_batch(self, q, target7, cfg=None, ee_offset7=None, grad=True):
        """q: [n, B] float64 cuda tensor -> (f [B], g [n, B])."""
        cfg = cfg or nat.make_config()
        assert q.is_cuda and q.dtype == torch.float64 and q.shape[0] == self.n and q.is_contiguous()
        B = q.shape[1]
        f = torch.empty(B, dtype=torch.float64, device=q.device)
        g = torch.empty_like(q) if grad else None
        t7 = np.ascontiguousarray(target7, dtype=np.float64)
        ee = np.ascontiguousarray(ee_offset7, dtype=np.float64) if ee_offset7 is not None else None
        nat.check(nat.lib().optik_hip_eval_batch(self._h, C.byref(cfg), _dp(t7),
                                                 _dpn(ee), _ptr(q), B,
                                                 _ptr(f), _ptr(g), _stream_ptr()))
        return f, g

    def fk_batch(self, q, ee_offset7=None, jacobian=False):
        """q: [n, B] -> pose [7, B] (and jac [6n, B], column-major 6 x n per column)."""
        assert q.is_cuda and q.dtype == torch.float64 and q.shape[0] == self.n and q.is_contiguous()
        B = q.shape[1]
        pose = torch.empty((7, B), dtype=torch.float64, device=q.device)
        jac = torch.empty((6 * self.n, B), dtype=torch.float64, device=q.device) if jacobian else None
        ee = np.ascontiguousarray(ee_offset7, dtype=np.float64) if ee_offset7 is not None else None
        nat.check(nat.lib().optik_hip_fk_batch(self._h, _dpn(ee), _ptr(q),
                                               B, _ptr(pose), _ptr(jac), _stream_ptr()))
        return (pose, jac) if jacobian else pose

    def diff_ik_batch(self, q, V, v_max, ee_offset7=None):
        """Robot.diff_ik for every column of q [n, B] (float64 cuda tensors): V [6, B] or one twist [6], v_max
        [n, B] or one limit vector [n].  Stream-ordered on the current stream; returns (alpha [B], v [n, B],
        status [B] int32: 0 solved, 1 no solution with alpha and v zero)."""
        assert q.is_cuda and q.dtype == torch.float64 and q.dim() == 2 and q.shape[0] == self.n and q.is_contiguous()
        B = q.shape[1]
        for t, rows in ((V, 6), (v_max, self.n)):
            assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.device == q.device
            assert tuple(t.shape) in ((rows,), (rows, B)), f"expected [{rows}] or [{rows}, {B}], got {tuple(t.shape)}"
        alpha = torch.empty(B, dtype=torch.float64, device=q.device)
        v = torch.empty((self.n, B), dtype=torch.float64, device=q.device)
        status = torch.empty(B, dtype=torch.int32, device=q.device)
        ee = np.ascontiguousarray(ee_offset7, dtype=np.float64) if ee_offset7 is not None else None
        nat.check(nat.lib().optik_hip_diff_ik_batch(
            self._h, _dpn(ee), _ptr(q), _ptr(V), B if V.dim() == 2 else 0,
            _ptr(v_max), B if v_max.dim() == 2 else 0, B, _ptr(alpha), _ptr(v), _ptr(status), _stream_ptr()))
        return alpha, v, status

    def diff_ik_avoid_batch(self, q, V, v_max, influence, safety, gain=1.0, ee_offset7=None):
        """diff_ik_batch with velocity dampers against the chain's collision model and world (optik_hip.h:
        optik_hip_diff_ik_avoid_batch): the same arguments and returns; status 1 also where the dampers cannot be
        met."""
        assert q.is_cuda and q.dtype == torch.float64 and q.dim() == 2 and q.shape[0] == self.n and q.is_contiguous()
        B = q.shape[1]
        for t, rows in ((V, 6), (v_max, self.n)):
            assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.device == q.device
            assert tuple(t.shape) in ((rows,), (rows, B)), f"expected [{rows}] or [{rows}, {B}], got {tuple(t.shape)}"
        alpha = torch.empty(B, dtype=torch.float64, device=q.device)
        v = torch.empty((self.n, B), dtype=torch.float64, device=q.device)
        status = torch.empty(B, dtype=torch.int32, device=q.device)
        ee = np.ascontiguousarray(ee_offset7, dtype=np.float64) if ee_offset7 is not None else None
        nat.check(nat.lib().optik_hip_diff_ik_avoid_batch(
            self._h, _dpn(ee), _ptr(q), _ptr(V), B if V.dim() == 2 else 0,
            _ptr(v_max), B if v_max.dim() == 2 else 0, B, float(influence), float(safety), float(gain),
            _ptr(alpha), _ptr(v), _ptr(status), _stream_ptr()))
        return alpha, v, status

    def collision_witness_batch(self, q, ee_offset7=None):
        """The witness table of every column of q [n, B] (optik_hip.h: optik_hip_collision_witness_batch):
        (dist [n + 2, B], grad [n + 2, n, B], witness [n + 2, 3, B] int32).  Stream-ordered."""
        assert q.is_cuda and q.dtype == torch.float64 and q.dim() == 2 and q.shape[0] == self.n and q.is_contiguous()
        B, F = q.shape[1], self.n + 2
        dist = torch.empty((F, B), dtype=torch.float64, device=q.device)
        grad = torch.empty((F, self.n, B), dtype=torch.float64, device=q.device)
        wit = torch.empty((F, 3, B), dtype=torch.int32, device=q.device)
        ee = np.ascontiguousarray(ee_offset7, dtype=np.float64) if ee_offset7 is not None else None
        nat.check(nat.lib().optik_hip_collision_witness_batch(self._h, _dpn(ee), _ptr(q), B,
                                                              _ptr(dist), _ptr(grad), _ptr(wit), _stream_ptr()))
        return dist, grad, wit

    def manip_batch(self, q, ee_offset7=None):
        """The measures of solution modes "manipulability" / "condition" for every column of q [n, B] (float64 cuda
        tensor): (w [B], c [B]) -- w = product of the min(n, 6) largest singular values of the body Jacobian, c =
        sigma_min / sigma_max (csrc/manip_measure.hpp; include/optik_hip.h: optik_hip_manip_batch).  Stream-ordered.
        The keys ik_batch / ik_solutions / ik_path report in these modes are -w / -c."""
        if not (isinstance(q, torch.Tensor) and q.is_cuda and q.dtype == torch.float64 and q.dim() == 2
                and q.shape[0] == self.n and q.is_contiguous()):
            raise ValueError(f"q must be a contiguous float64 cuda tensor [n, B] with n = {self.n}")
        B = q.shape[1]
        w = torch.empty(B, dtype=torch.float64, device=q.device)
        c = torch.empty(B, dtype=torch.float64, device=q.device)
        ee = np.ascontiguousarray(ee_offset7, dtype=np.float64) if ee_offset7 is not None else None
        if ee is not None and ee.shape != (7,):
            raise ValueError("ee_offset7 must be 7 numbers: t, then the quaternion i, j, k, w")
        nat.check(nat.lib().optik_hip_manip_batch(self._h, _dpn(ee), _ptr(q), B,
                                                  _ptr(w), _ptr(c), _stream_ptr()))
        return w, c

    # -- the collision filter (include/optik_hip.h) --------------------------------------
    def set_collision_model(self, frames, centers, radii, self_pairs="auto", margin=0.0):
        """The chain's robot spheres (frame index in 0 .. n + 1, centre in that frame, radius), self pairs ("auto":
        every pair whose frames differ by >= 2; None: none; or [P, 2] indices) and margin.  While a model with at
        least one sphere is set, ik_batch / ik_host / ik_solutions / ik_path return free successes only (Speed: the
        lowest-index one; every restart runs to its end).  Waits for the device; host arrays."""
        from .collision import model_arrays
        f, c, r, p, m = model_arrays(frames, centers, radii, self_pairs, margin)
        nat.check(nat.lib().optik_hip_chain_set_collision_model(
            self._h, f.ctypes.data_as(C.POINTER(C.c_int32)), _dp(c), _dp(r), len(f),
            p.ctypes.data_as(C.POINTER(C.c_int32)), len(p), m))

    def clear_collision_model(self):
        """No model: every path runs exactly as without the filter."""
        nat.check(nat.lib().optik_hip_chain_set_collision_model(self._h, None, None, None, 0, None, 0, 0.0))

    def set_world(self, spheres=None, boxes=None):
        """Replaces the world: spheres [M, 4] (centre, radius), boxes [M, 10] (t, unit quaternion i, j, k, w, half
        extents), in the base frame."""
        from .collision import world_arrays
        sph, box = world_arrays(spheres, boxes)
        nat.check(nat.lib().optik_hip_chain_set_world(self._h, _dp(sph), len(sph), _dp(box), len(box)))

    # -- the distance-field world (include/optik_hip.h) ------------------------------------
    def set_world_grid(self, origin, voxel, values):
        """A sampled signed distance field next to the spheres and boxes: values [nx, ny, nz] (a host array or a
        tensor, converted to float32), node (i, j, k) at origin + voxel * (i, j, k) in the base frame.  Replaces the
        whole grid and leaves the spheres and boxes alone.  Waits for the device; the values are checked on the host
        (a tensor is copied there first)."""
        from .collision import grid_arrays
        if isinstance(values, torch.Tensor):
            values = values.detach().to(torch.float32).cpu().numpy()
        o, v, vals, (nx, ny, nz) = grid_arrays(origin, voxel, values)
        nat.check(nat.lib().optik_hip_chain_set_world_grid(self._h, _dp(o), v, nx, ny, nz,
                                                           C.c_void_p(vals.ctypes.data)))

    def clear_world_grid(self):
        """No grid: every call returns what it returns with the spheres and boxes alone."""
        nat.check(nat.lib().optik_hip_chain_set_world_grid(self._h, None, 0.0, 0, 0, 0, None))

    def bake_world_grid(self, origin, voxel, shape):
        """The signed distance of the chain's current spheres and boxes at every node: a float32 cuda tensor
        [nx, ny, nz].  Stream-ordered; installs nothing."""
        from .collision import grid_arrays
        o, v, _, (nx, ny, nz) = grid_arrays(origin, voxel, shape=shape)
        nodes = nx * ny * nz
        out = torch.empty(nodes if 0 < nodes <= (1 << 24) else 1, dtype=torch.float32, device=self.device)
        nat.check(nat.lib().optik_hip_world_grid_bake(self._h, _dp(o), v, nx, ny, nz, _ptr(out), _stream_ptr()))
        return out.view(nx, ny, nz)

    # -- from sensor data to that grid (include/optik_hip.h) --------------------------------
    def world_grid_from_occupancy(self, voxel, occupied, max_distance=None):
        """The signed field of an occupancy grid (a uint8 or bool cuda tensor [nx, ny, nz], non-zero = occupied) by an
        exact Euclidean distance transform: a float32 cuda tensor [nx, ny, nz], clamped to +-max_distance (default:
        the grid diagonal).  Stream-ordered; installs nothing.  The chain's workspace grows on demand."""
        from .collision import default_max_distance
        if not (isinstance(occupied, torch.Tensor) and occupied.is_cuda and occupied.dim() == 3
                and occupied.dtype in (torch.uint8, torch.bool) and occupied.is_contiguous()):
            raise ValueError("occupied must be a contiguous uint8 or bool cuda tensor [nx, ny, nz]")
        nx, ny, nz = (int(v) for v in occupied.shape)
        md = default_max_distance(voxel, (nx, ny, nz)) if max_distance is None else float(max_distance)
        out = torch.empty((nx, ny, nz) if nx * ny * nz <= (1 << 24) else (1, 1, 1), dtype=torch.float32,
                          device=self.device)
        nat.check(nat.lib().optik_hip_world_grid_from_occupancy(self._h, float(voxel), nx, ny, nz, _ptr(occupied), md,
                                                                _ptr(out), _stream_ptr()))
        return out

    def occupancy_from_points(self, origin, voxel, shape, points, exclude=None, into=None):
        """Marks the nodes of a point cloud (a float64 cuda tensor [N, 3], base frame) that none of the spheres of
        `exclude` (float64 cuda tensor [E, 4], E <= 1024) holds: a uint8 cuda tensor [nx, ny, nz].  `into`: a tensor of
        that kind to accumulate into, in place (it is also what is returned).  Stream-ordered."""
        from .collision import grid_arrays
        o, v, _, (nx, ny, nz) = grid_arrays(origin, voxel, shape=shape)

        def f64(t, cols, name):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.dim() == 2
                    and t.shape[1] == cols and t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous float64 cuda tensor [*, {cols}]")
            return t
        points = f64(points, 3, "points")
        E = 0 if exclude is None else int(f64(exclude, 4, "exclude").shape[0])
        nodes = nx * ny * nz
        if into is None:
            into = torch.zeros((nx, ny, nz) if 0 < nodes <= (1 << 24) else (1, 1, 1), dtype=torch.uint8,
                               device=self.device)
        elif not (isinstance(into, torch.Tensor) and into.is_cuda and into.dtype == torch.uint8
                  and tuple(into.shape) == (nx, ny, nz) and into.is_contiguous()):
            raise ValueError("into must be a contiguous uint8 cuda tensor of the grid's shape")
        nat.check(nat.lib().optik_hip_occupancy_from_points(self._h, _dp(o), v, nx, ny, nz, _ptr(points),
                                                            int(points.shape[0]), _ptr(exclude) if E else None, E,
                                                            _ptr(into), _stream_ptr()))
        return into

    # -- depth-image worlds: the evidence map (include/optik_hip.h) ---------------------------
    def depth_integrate(self, map, origin, voxel, depth, intrinsics, poses, exclude=None, z_near=None, z_far=None,
                        band=None, hit=None, miss=None, e_min=None, e_max=None):
        """Applies depth images to an evidence map, in place, and returns it.  map: a contiguous int16 cuda tensor
        [nx, ny, nz], -32768 (optik_amd.collision.MAP_UNKNOWN) where nothing was ever observed; depth: a contiguous
        float32 cuda tensor [F, H, W] or [H, W], z-depth in metres; intrinsics (fx, fy, cx, cy) [F, 4] or one row and
        poses [F, 4, 4] or one [4, 4] (row-major, the camera in the base frame: x right, y down, z forward) are host
        arrays; exclude: a float64 cuda tensor [E, 4], the self-filter's spheres.  Per frame every node gathers its
        nearest pixel: more than `band` in front of the surface it loses `miss` (floor e_min), within `band` of it it
        gains `hit` (ceiling e_max), behind it, out of view or under an invalid pixel it keeps its value.  band
        defaults to voxel and the rest to optik_amd.collision.DEPTH_DEFAULTS (Robot.depth_integrate says what those
        are).  Stream-ordered; the chain's workspace for the cleaned images grows on demand."""
        from .collision import DEPTH_DEFAULTS, camera_arrays, grid_arrays
        if not (isinstance(map, torch.Tensor) and map.is_cuda and map.dtype == torch.int16 and map.dim() == 3
                and map.is_contiguous()):
            raise ValueError("map must be a contiguous int16 cuda tensor [nx, ny, nz]")
        o, v, _, (nx, ny, nz) = grid_arrays(origin, voxel, shape=tuple(map.shape))
        if not (isinstance(depth, torch.Tensor) and depth.is_cuda and depth.dtype == torch.float32
                and depth.dim() in (2, 3) and depth.is_contiguous()):
            raise ValueError("depth must be a contiguous float32 cuda tensor [F, H, W] or [H, W]")
        F, H, W = (1, *depth.shape) if depth.dim() == 2 else (int(s) for s in depth.shape)
        k4, p16 = camera_arrays(intrinsics, poses, F)
        E = 0
        if exclude is not None:
            if not (isinstance(exclude, torch.Tensor) and exclude.is_cuda and exclude.dtype == torch.float64
                    and exclude.dim() == 2 and exclude.shape[1] == 4 and exclude.is_contiguous()):
                raise ValueError("exclude must be a contiguous float64 cuda tensor [E, 4]")
            E = int(exclude.shape[0])
        a = {k: (DEPTH_DEFAULTS[k] if val is None else val) for k, val in
             dict(z_near=z_near, z_far=z_far, hit=hit, miss=miss, e_min=e_min, e_max=e_max).items()}
        nat.check(nat.lib().optik_hip_depth_integrate(
            self._h, _dp(o), v, nx, ny, nz, _ptr(map), _ptr(depth), F, int(H), int(W), _dp(k4), _dp(p16),
            _ptr(exclude) if E else None, E, float(a["z_near"]), float(a["z_far"]), v if band is None else float(band),
            int(a["hit"]), int(a["miss"]), int(a["e_min"]), int(a["e_max"]), _stream_ptr()))
        return map

    def occupancy_from_map(self, map, threshold, unknown_occupied=False, into=None):
        """The occupancy of an evidence map (a contiguous int16 cuda tensor [nx, ny, nz]): a uint8 cuda tensor of that
        shape, 1 where the evidence is >= threshold, `unknown_occupied` where nothing was ever observed.  `into`: a
        tensor of that kind to OR into, in place (it is also what is returned), as occupancy_from_points has -- a map
        and a point cloud then feed one world_grid_from_occupancy.  Stream-ordered."""
        if not (isinstance(map, torch.Tensor) and map.is_cuda and map.dtype == torch.int16 and map.dim() == 3
                and map.is_contiguous()):
            raise ValueError("map must be a contiguous int16 cuda tensor [nx, ny, nz]")
        nx, ny, nz = (int(s) for s in map.shape)
        accumulate = into is not None
        if into is None:
            into = torch.empty((nx, ny, nz), dtype=torch.uint8, device=map.device)
        elif not (isinstance(into, torch.Tensor) and into.is_cuda and into.dtype == torch.uint8
                  and tuple(into.shape) == (nx, ny, nz) and into.is_contiguous()):
            raise ValueError("into must be a contiguous uint8 cuda tensor of the map's shape")
        nat.check(nat.lib().optik_hip_occupancy_from_map(self._h, nx, ny, nz, _ptr(map), int(threshold),
                                                         1 if unknown_occupied else 0, 1 if accumulate else 0,
                                                         _ptr(into), _stream_ptr()))
        return into

    # -- from a triangle mesh to that grid (include/optik_hip.h) ------------------------------
    def world_grid_from_mesh(self, origin, voxel, shape, triangles, max_distance=None):
        """The signed distance field of a triangle soup (a contiguous float64 cuda tensor [M, 3, 3] or [M, 9]: the
        vertices a, b, c of each triangle, base frame; finite coordinates are the caller's promise here) on the grid:
        a float32 cuda tensor [nx, ny, nz], clamped to +-max_distance (default: the grid diagonal).  Stream-ordered;
        installs nothing.  nx * ny * nz * M pair evaluations, no culling."""
        from .collision import default_max_distance, grid_arrays
        o, v, _, (nx, ny, nz) = grid_arrays(origin, voxel, shape=shape)
        t = triangles
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
                and ((t.dim() == 3 and tuple(t.shape[1:]) == (3, 3)) or (t.dim() == 2 and t.shape[1] == 9))):
            raise ValueError("triangles must be a contiguous float64 cuda tensor [M, 3, 3] or [M, 9]")
        M = int(t.shape[0])
        md = default_max_distance(v, (nx, ny, nz)) if max_distance is None else float(max_distance)
        nodes = nx * ny * nz
        out = torch.empty((nx, ny, nz) if 0 < nodes <= (1 << 24) else (1, 1, 1), dtype=torch.float32,
                          device=self.device)
        nat.check(nat.lib().optik_hip_world_grid_from_mesh(self._h, _dp(o), v, nx, ny, nz, _ptr(t) if M else None,
                                                           min(M, (1 << 31) - 1), md, _ptr(out), _stream_ptr()))
        return out

    # -- from a solid to a sphere model (include/optik_hip.h) ---------------------------------
    def sphere_fit(self, values, origin, voxel, points, pad, slack, k):
        """A greedy sphere cover (csrc/spherefit_measure.hpp) of the solid whose signed distance field is `values` (a
        contiguous float32 cuda tensor [nx, ny, nz] on the grid (origin, voxel): what world_grid_from_mesh returns)
        and whose surface is sampled by `points` (a contiguous float64 cuda tensor [P, 3]): up to k spheres with their
        centres on grid nodes, each reaching at most `pad` beyond the solid, chosen one after the other to hold the
        most points not held yet at least `slack` inside.  Returns a dict of cuda tensors: chosen int32 [k] (node
        indices, -1 past the count), centers [k, 3], radii [k] (NaN past the count), gains int32 [k], count_uncovered
        int32 [2].  Stream-ordered, no host synchronisation; the workspace is a torch allocation."""
        from .collision import grid_arrays
        v_t, p_t = values, points
        if not (isinstance(v_t, torch.Tensor) and v_t.is_cuda and v_t.dtype == torch.float32 and v_t.dim() == 3
                and v_t.is_contiguous()):
            raise ValueError("values must be a contiguous float32 cuda tensor [nx, ny, nz]")
        if not (isinstance(p_t, torch.Tensor) and p_t.is_cuda and p_t.dtype == torch.float64 and p_t.dim() == 2
                and p_t.shape[1] == 3 and p_t.is_contiguous()):
            raise ValueError("points must be a contiguous float64 cuda tensor [P, 3]")
        o, v, _, (nx, ny, nz) = grid_arrays(origin, voxel, shape=tuple(v_t.shape))
        P, K = int(p_t.shape[0]), int(k)
        kk = K if 1 <= K <= nat.MAX_FIT_SPHERES else 1
        out = dict(chosen=torch.empty(kk, dtype=torch.int32, device=self.device),
                   centers=torch.empty((kk, 3), dtype=torch.float64, device=self.device),
                   radii=torch.empty(kk, dtype=torch.float64, device=self.device),
                   gains=torch.empty(kk, dtype=torch.int32, device=self.device),
                   count_uncovered=torch.empty(2, dtype=torch.int32, device=self.device))
        return self.sphere_fit_into(v_t, o, v, p_t, pad, slack, K, out)

    def sphere_fit_into(self, values, origin, voxel, points, pad, slack, k, out):
        """sphere_fit into the caller's tensors (`out`: the dict sphere_fit returns); returns `out`."""
        nx, ny, nz = (int(s) for s in values.shape)
        P = int(points.shape[0])
        o = np.ascontiguousarray(origin, dtype=np.float64)
        ws_bytes = int(nat.lib().optik_hip_sphere_fit_workspace_bytes(nx, ny, nz, P))
        ws = torch.empty(max(ws_bytes, 4) // 4, dtype=torch.int32, device=self.device)
        nat.check(nat.lib().optik_hip_sphere_fit(
            self._h, _dp(o), float(voxel), nx, ny, nz, _ptr(values), _ptr(points) if P else None, P, float(pad),
            float(slack), int(k), _ptr(out["chosen"]), _ptr(out["centers"]), _ptr(out["radii"]), _ptr(out["gains"]),
            _ptr(out["count_uncovered"]), _ptr(ws), ws_bytes, _stream_ptr()))
        return out

    def _check_q(self, q):
        if not (isinstance(q, torch.Tensor) and q.is_cuda and q.dtype == torch.float64 and q.dim() == 2
                and q.shape[0] == self.n and q.is_contiguous()):
            raise ValueError(f"q must be a contiguous float64 cuda tensor [n, B] with n = {self.n}")
        return q.shape[1]

    @staticmethod
    def _ee7(ee_offset7):
        ee = np.ascontiguousarray(ee_offset7, dtype=np.float64) if ee_offset7 is not None else None
        if ee is not None and ee.shape != (7,):
            raise ValueError("ee_offset7 must be 7 numbers: t, then the quaternion i, j, k, w")
        return ee

    def link_frames_batch(self, q, ee_offset7=None):
        """All n + 2 frames of every column of q [n, B]: [B, n + 2, 7] (t, quaternion i, j, k, w); frame n + 1 is
        fk_batch's pose.  Stream-ordered."""
        B = self._check_q(q)
        ee = self._ee7(ee_offset7)
        frames = torch.empty((B, self.n + 2, 7), dtype=torch.float64, device=q.device)
        nat.check(nat.lib().optik_hip_link_frames_batch(self._h, _dpn(ee), _ptr(q), B,
                                                        _ptr(frames), _stream_ptr()))
        return frames

    def collision_batch(self, q, ee_offset7=None):
        """(clearance [B], free [B] bool) of every column of q [n, B] against the chain's model and world
        (csrc/collision_measure.hpp).  Stream-ordered."""
        B = self._check_q(q)
        ee = self._ee7(ee_offset7)
        clearance = torch.empty(B, dtype=torch.float64, device=q.device)
        free = torch.empty(B, dtype=torch.uint8, device=q.device)
        nat.check(nat.lib().optik_hip_collision_batch(self._h, _dpn(ee), _ptr(q), B,
                                                      _ptr(clearance), _ptr(free), _stream_ptr()))
        return clearance, free.bool()

    # -- the motion check (include/optik_hip.h) ------------------------------------------
    def collision_motion_batch(self, qa, qb, resolution, ee_offset=None, clearance=True):
        """The straight joint-space motions qa[:, b] -> qb[:, b] (float64 cuda tensors [n, B]) sampled at
        `resolution` (L-infinity, radians; csrc/motion_measure.hpp) against the chain's model and world: (clearance
        [B], free [B] bool, first [B] int32, steps [B] int32) -- the minimum of the samples' clearances, whether every
        sample is free, the lowest sample index that is not (-1: none) and the number of steps K (-1: not sampled,
        then clearance NaN and free False).  clearance=False only classifies (faster for blocked motions) and returns
        None in its place.  ee_offset: 7 numbers, as collision_batch.  Stream-ordered."""
        B = self._check_q(qa)
        if self._check_q(qb) != B or qb.device != qa.device:
            raise ValueError(f"qa and qb must have the same shape and device, got {tuple(qa.shape)} and {tuple(qb.shape)}")
        h = nat.check_resolution(resolution)
        ee = self._ee7(ee_offset)
        clr = torch.empty(B, dtype=torch.float64, device=qa.device) if clearance else None
        free = torch.empty(B, dtype=torch.uint8, device=qa.device)
        first = torch.empty(B, dtype=torch.int32, device=qa.device)
        steps = torch.empty(B, dtype=torch.int32, device=qa.device)
        nat.check(nat.lib().optik_hip_collision_motion_batch(
            self._h, _dpn(ee), _ptr(qa), _ptr(qb), B, h, _ptr(clr), _ptr(free),
            _ptr(first), _ptr(steps), _stream_ptr()))
        return clr, free.bool(), first, steps

    # -- the certified motion check (include/optik_hip.h) ----------------------------------
    def collision_motion_certify(self, qa, qb, tol, grid_lipschitz=None, max_steps=nat.CERTIFY_STEPS, ee_offset=None):
        """Conservative advancement along the straight joint-space motions qa[:, b] -> qb[:, b] (float64 cuda tensors
        [n, B]; csrc/advance_measure.hpp) against the chain's model and world: a dict of device tensors, status [B]
        int32 (nat.CERTIFY_FREE: the clearance is >= margin - tol for EVERY t in [0, 1]; CERTIFY_BLOCKED: q(t_stop)
        is not free; CERTIFY_LIMIT: max_steps samples were not enough, nothing is said; CERTIFY_NAN), steps [B] int32
        (samples evaluated), t_stop [B] and clearance [B] (the minimum over the evaluated samples).  grid_lipschitz:
        the Lipschitz constant of the installed grid's trilinear field (default sqrt(3): any true distance field;
        collision.grid_lipschitz for another grid).  ee_offset: 7 numbers, as collision_batch.  Stream-ordered."""
        B = self._check_q(qa)
        if self._check_q(qb) != B or qb.device != qa.device:
            raise ValueError(f"qa and qb must have the same shape and device, got {tuple(qa.shape)} and {tuple(qb.shape)}")
        tol, G, max_steps = nat.check_certify_args(tol, grid_lipschitz, max_steps)
        ee = self._ee7(ee_offset)
        out = dict(status=torch.empty(B, dtype=torch.int32, device=qa.device),
                   steps=torch.empty(B, dtype=torch.int32, device=qa.device),
                   t_stop=torch.empty(B, dtype=torch.float64, device=qa.device),
                   clearance=torch.empty(B, dtype=torch.float64, device=qa.device))
        nat.check(nat.lib().optik_hip_collision_motion_certify_batch(
            self._h, _dpn(ee), _ptr(qa), _ptr(qb), B, tol, G, max_steps,
            _ptr(out["status"]), _ptr(out["steps"]), _ptr(out["t_stop"]), _ptr(out["clearance"]), _stream_ptr()))
        return out

    def set_motion_resolution(self, h):
        """The resolution of ik_path's motion check between a path's seed and every candidate within max_step (0:
        off, the default); it acts while a collision model is set.  Waits for the device."""
        nat.check(nat.lib().optik_hip_chain_set_motion_resolution(self._h, nat.check_resolution(h, allow_zero=True)))

    # -- bending paths out of collision (include/optik_hip.h) -----------------------------
    def path_optimize(self, q, iters, step, w_smooth, w_obs, influence, safety, ee_offset7=None, out=None):
        """Covariant gradient smoothing of P paths of L waypoints (optik_hip_path_optimize): q [L, P, n] float64 cuda
        tensor -- ik_path's "x" as it is --, 3 <= L <= 64.  `out`: the tensor that receives the waypoints (q itself:
        in place; default: a new one).  Stream-ordered on the current stream; returns a dict of device tensors: q
        [L, P, n], cost_first [P, 3], cost_last [P, 3] = (U, F_smooth, F_obs), clearance [P], status [P] int32."""
        if not (isinstance(q, torch.Tensor) and q.is_cuda and q.dtype == torch.float64 and q.dim() == 3
                and q.shape[2] == self.n and q.is_contiguous()):
            raise ValueError(f"q must be a contiguous float64 cuda tensor [L, P, n] with n = {self.n}")
        L, P = int(q.shape[0]), int(q.shape[1])
        nat.check_path_optimize_args(L, iters, step, w_smooth, w_obs, influence, safety)
        if out is None:
            out = torch.empty_like(q)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and out.is_contiguous()
                  and out.shape == q.shape and out.device == q.device):
            raise ValueError("out must be a contiguous float64 cuda tensor of q's shape and device")
        ee = self._ee7(ee_offset7)
        res = dict(q=out, cost_first=torch.empty((P, 3), dtype=torch.float64, device=q.device),
                   cost_last=torch.empty((P, 3), dtype=torch.float64, device=q.device),
                   clearance=torch.empty(P, dtype=torch.float64, device=q.device),
                   status=torch.empty(P, dtype=torch.int32, device=q.device))
        nat.check(nat.lib().optik_hip_path_optimize(
            self._h, _dpn(ee), _ptr(q), L, P, int(iters), float(step), float(w_smooth),
            float(w_obs), float(influence), float(safety), _ptr(out), _ptr(res["cost_first"]), _ptr(res["cost_last"]),
            _ptr(res["clearance"]), _ptr(res["status"]), _stream_ptr()))
        return res

    def path_optimize_constrained(self, q, c, iters, step, w_smooth, w_obs, influence, safety, ptol=nat.CONSTRAINT_TOL,
                                  piters=nat.CONSTRAINT_ITERS, damping=nat.CONSTRAINT_DAMPING,
                                  max_step=nat.CONSTRAINT_MAX_STEP, ee_offset7=None, out=None):
        """path_optimize under the pose constraint c (optik_hip_path_optimize_constrained; csrc/path_optimize.hpp step
        7): after every update each interior waypoint is projected back onto c
        (constraint_project_batch's method at ptol, piters, damping, max_step) and keeps its value of the previous
        iterate, bit for bit, where the projection does not end CONSTRAINT_PROJECTED.  The ends never move.  Projection
        after the step, not in the metric; the segments between the waypoints are not checked.  q, out and the
        other arguments as path_optimize takes them.  Returns path_optimize's dict plus violation [P] (the largest
        over the L waypoints of the result) and projected [2, P] int32 (attempted, ended projected).  With a box
        that is free on all six axes the shared outputs are path_optimize's, bit for bit.  Stream-ordered."""
        if not (isinstance(q, torch.Tensor) and q.is_cuda and q.dtype == torch.float64 and q.dim() == 3
                and q.shape[2] == self.n and q.is_contiguous()):
            raise ValueError(f"q must be a contiguous float64 cuda tensor [L, P, n] with n = {self.n}")
        L, P = int(q.shape[0]), int(q.shape[1])
        nat.check_path_optimize_args(L, iters, step, w_smooth, w_obs, influence, safety)
        box = _box_ptrs(checked_constraint_arrays(c))
        ptol, piters, damping, max_step = nat.check_project_args(ptol, piters, damping, max_step)
        if out is None:
            out = torch.empty_like(q)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and out.is_contiguous()
                  and out.shape == q.shape and out.device == q.device):
            raise ValueError("out must be a contiguous float64 cuda tensor of q's shape and device")
        ee = self._ee7(ee_offset7)
        res = dict(q=out, cost_first=torch.empty((P, 3), dtype=torch.float64, device=q.device),
                   cost_last=torch.empty((P, 3), dtype=torch.float64, device=q.device),
                   clearance=torch.empty(P, dtype=torch.float64, device=q.device),
                   status=torch.empty(P, dtype=torch.int32, device=q.device),
                   violation=torch.empty(P, dtype=torch.float64, device=q.device),
                   projected=torch.empty((2, P), dtype=torch.int32, device=q.device))
        nat.check(nat.lib().optik_hip_path_optimize_constrained(
            self._h, _dpn(ee), _ptr(q), L, P, int(iters), float(step), float(w_smooth),
            float(w_obs), float(influence), float(safety), *box, ptol, piters, damping, max_step,
            _ptr(out), _ptr(res["cost_first"]), _ptr(res["cost_last"]), _ptr(res["clearance"]), _ptr(res["status"]),
            _ptr(res["violation"]), _ptr(res["projected"]), _stream_ptr()))
        return res

    # -- collision repair (include/optik_hip.h) -------------------------------------------
    def collision_repair_batch(self, q, influence, safety, step=nat.REPAIR_STEP, iters=nat.REPAIR_ITERS, c=None,
                               max_move=math.inf, ptol=nat.CONSTRAINT_TOL, piters=nat.CONSTRAINT_ITERS,
                               damping=nat.CONSTRAINT_DAMPING, max_step=nat.CONSTRAINT_MAX_STEP, ee_offset7=None,
                               out=None):
        """Every column of q [n, B] pushed out of collision on its own (optik_hip_collision_repair_batch;
        csrc/repair_measure.hpp): steps of `step` down the gradient of path_optimize's hinge (influence, safety) of
        the column's witness rows, clamped to the joint limits, until its clearance is >= safety or `iters` steps are
        spent; with the pose constraint c every step is projected back onto c (constraint_project_batch's method at
        ptol, piters, damping, max_step).  max_move bounds the L-infinity distance from the input.  `out`: the
        tensor that receives the configurations (q itself: in place; default: a new one).  Returns a dict of device
        tensors: x [n, B], clearance [B], violation [B] (0 without c), moved [B], status [B] int32 (nat.REPAIR_FREE,
        REPAIR_LIMIT, REPAIR_STUCK, REPAIR_NAN) and iterations [B] int32.  A column that was free already comes back
        bit for bit with 0 iterations.  Stream-ordered."""
        B = self._check_q(q)
        influence, safety, step, iters, max_move = nat.check_repair_args(influence, safety, step, iters, max_move)
        box = (None, None, None)
        if c is not None:
            box = _box_ptrs(checked_constraint_arrays(c))
            ptol, piters, damping, max_step = nat.check_project_args(ptol, piters, damping, max_step)
        if out is None:
            out = torch.empty_like(q)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and out.is_contiguous()
                  and out.shape == q.shape and out.device == q.device):
            raise ValueError("out must be a contiguous float64 cuda tensor of q's shape and device")
        ee = self._ee7(ee_offset7)
        res = dict(x=out, clearance=torch.empty(B, dtype=torch.float64, device=q.device),
                   violation=torch.empty(B, dtype=torch.float64, device=q.device),
                   moved=torch.empty(B, dtype=torch.float64, device=q.device),
                   status=torch.empty(B, dtype=torch.int32, device=q.device),
                   iterations=torch.empty(B, dtype=torch.int32, device=q.device))
        return self.collision_repair_into(q, influence, safety, step, iters, max_move, box, ptol, piters, damping,
                                          max_step, ee, res)

    def collision_repair_into(self, q, influence, safety, step, iters, max_move, box, ptol, piters, damping, max_step,
                              ee, res):
        """collision_repair_batch's call into the caller's tensors (`res`: the dict it returns, an entry None: that
        output is not wanted); the arguments as the C entry takes them, box = three pointers or Nones."""
        o = nat.RepairOutputs(*(res[k].data_ptr() if res.get(k) is not None else None
                                for k in ("x", "clearance", "violation", "moved", "status", "iterations")))
        nat.check(nat.lib().optik_hip_collision_repair_batch(
            self._h, _dpn(ee), _ptr(q), int(q.shape[1]), float(influence), float(safety), float(step), int(iters),
            float(max_move), *box, float(ptol), int(piters), float(damping), float(max_step), C.byref(o),
            _stream_ptr()))
        return res

    # -- roadmap planning (include/optik_hip.h) -------------------------------------------
    def _check_slots(self, t, Q, name, dtype):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.shape[1] == Q
                and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous {dtype} cuda tensor [k, {Q}]")
        nat.check_roadmap_args(k=int(t.shape[0]))
        return int(t.shape[0])

    def roadmap_knn(self, q, nodes, k, exclude_self=False):
        """The k nearest nodes (L-infinity) of every query (optik_hip_roadmap_knn): q [n, Q], nodes [n, N] float64
        cuda tensors -> (idx [k, Q] int32, dist [k, Q]), best first in the order (distance, index), a NaN distance
        after every number; -1 / +inf past the candidates.  exclude_self skips node j for query j.  Stream-ordered."""
        Q, N = self._check_q(q), self._check_q(nodes)
        nat.check_roadmap_args(N=N, k=k)
        idx = torch.empty((int(k), Q), dtype=torch.int32, device=q.device)
        dist = torch.empty((int(k), Q), dtype=torch.float64, device=q.device)
        nat.check(nat.lib().optik_hip_roadmap_knn(self._h, _ptr(q), Q, _ptr(nodes), N, int(k), 1 if exclude_self else 0,
                                                  _ptr(idx), _ptr(dist), _stream_ptr()))
        return idx, dist

    def roadmap_edges(self, frm, nodes, idx, resolution, reverse=False, ee_offset7=None):
        """The weights w [k, Q] of the motions frm[:, q] -> nodes[:, idx[s, q]] (reverse: node -> frm), checked at
        `resolution` by the motion check against the chain's model and world (optik_hip_roadmap_edges): max_i of the
        joint differences where the motion is free, +inf elsewhere and for index -1.  idx None pairs frm[:, q] with
        nodes[:, q] ([1, Q]).  Stream-ordered; one call per chain at a time."""
        Q, N = self._check_q(frm), self._check_q(nodes)
        h = nat.check_resolution(resolution)
        if idx is None:
            if N != Q:
                raise ValueError("without idx, frm and nodes must have the same shape")
            k = 1
        else:
            k = self._check_slots(idx, Q, "idx", torch.int32)
        ee = self._ee7(ee_offset7)
        w = torch.empty((k, Q), dtype=torch.float64, device=frm.device)
        nat.check(nat.lib().optik_hip_roadmap_edges(self._h, _dpn(ee), _ptr(frm), Q,
                                                    _ptr(nodes), N, _ptr(idx), k, h, 1 if reverse else 0, _ptr(w),
                                                    _stream_ptr()))
        return w

    def roadmap_query(self, nodes, nbr, w, start, goal, sidx, sw, gidx, gw, direct, Lmax, _route=(None, None)):
        """Shortest joint paths over one graph for Q (start, goal) pairs (optik_hip_roadmap_query): nodes [n, N], the
        out-edges nbr [k, N] int32 and w [k, N], start and goal [n, Q], the start links sidx, sw [ks, Q], the goal
        links gidx, gw [kg, Q], direct [Q].  Returns a dict of device tensors: path [Lmax, Q, n] (what path_optimize
        takes), len [Q] int32, cost [Q], status [Q] int32 (nat.ROADMAP_*).  Stream-ordered."""
        N, Q = self._check_q(nodes), self._check_q(start)
        if self._check_q(goal) != Q:
            raise ValueError("start and goal must have the same shape")
        nat.check_roadmap_args(N=N, max_waypoints=Lmax)
        k = self._check_slots(nbr, N, "nbr", torch.int32)
        if self._check_slots(w, N, "w", torch.float64) != k:
            raise ValueError("nbr and w must have the same shape")
        ks, kg = self._check_slots(sidx, Q, "sidx", torch.int32), self._check_slots(gidx, Q, "gidx", torch.int32)
        if self._check_slots(sw, Q, "sw", torch.float64) != ks or self._check_slots(gw, Q, "gw", torch.float64) != kg:
            raise ValueError("a link's indices and weights must have the same shape")
        if not (isinstance(direct, torch.Tensor) and direct.is_cuda and direct.dtype == torch.float64
                and direct.numel() == Q and direct.is_contiguous()):
            raise ValueError(f"direct must be a contiguous float64 cuda tensor of {Q} weights")
        dev = nodes.device
        res = dict(path=torch.empty((int(Lmax), Q, self.n), dtype=torch.float64, device=dev),
                   len=torch.empty(Q, dtype=torch.int32, device=dev),
                   cost=torch.empty(Q, dtype=torch.float64, device=dev),
                   status=torch.empty(Q, dtype=torch.int32, device=dev))
        nat.check(nat.lib().optik_hip_roadmap_query_route(
            self._h, _ptr(nodes), N, _ptr(nbr), _ptr(w), k, _ptr(start), _ptr(goal), Q, _ptr(sidx), _ptr(sw), ks,
            _ptr(gidx), _ptr(gw), kg, _ptr(direct), int(Lmax), _ptr(res["path"]), _ptr(res["len"]), _ptr(res["cost"]),
            _ptr(res["status"]), _ptr(_route[0]), _ptr(_route[1]), _stream_ptr()))
        return res

    def roadmap_build(self, nodes, k, resolution, ee_offset7=None):
        """The roadmap over nodes [n, N]: every node's k nearest others (roadmap_knn with exclude_self) and the
        checked weights of the motions node -> neighbour (roadmap_edges).  Returns (nbr [k, N] int32, w [k, N])."""
        nbr, _ = self.roadmap_knn(nodes, nodes, k, exclude_self=True)
        return nbr, self.roadmap_edges(nodes, nodes, nbr, resolution, ee_offset7=ee_offset7)

    def roadmap_plan(self, roadmap, starts, goals, ks, Lmax, resolution, ee_offset7=None):
        """Plans starts[:, q] -> goals[:, q] ([n, Q]) over roadmap = (nodes, nbr, w): each start's and each goal's
        ks nearest nodes, the links start -> node and node -> goal and the direct motion start -> goal checked at
        `resolution`, then roadmap_query.  Six launches' worth of kernels on the current stream, no host
        synchronisation in between.  Returns roadmap_query's dict."""
        nodes, nbr, w = roadmap
        sidx, _ = self.roadmap_knn(starts, nodes, ks)
        gidx, _ = self.roadmap_knn(goals, nodes, ks)
        sw = self.roadmap_edges(starts, nodes, sidx, resolution, ee_offset7=ee_offset7)
        gw = self.roadmap_edges(goals, nodes, gidx, resolution, reverse=True, ee_offset7=ee_offset7)
        direct = self.roadmap_edges(starts, goals, None, resolution, ee_offset7=ee_offset7)
        return self.roadmap_query(nodes, nbr, w, starts, goals, sidx, sw, gidx, gw, direct, Lmax)

    # -- pose constraints (include/optik_hip.h) -------------------------------------------
    def constraint_batch(self, q, c, ee_offset7=None):
        """The residual [6, B] and the violation [B] of every column of q [n, B] against the pose constraint c
        (optik_amd.PoseConstraint; csrc/constraint_measure.hpp).  Stream-ordered."""
        B = self._check_q(q)
        box = _box_ptrs(constraint_arrays(c))
        ee = self._ee7(ee_offset7)
        r = torch.empty((6, B), dtype=torch.float64, device=q.device)
        v = torch.empty(B, dtype=torch.float64, device=q.device)
        nat.check(nat.lib().optik_hip_constraint_batch(self._h, _dpn(ee), *box, _ptr(q), B, _ptr(r), _ptr(v), _stream_ptr()))
        return r, v

    def constraint_project_batch(self, q, c, tol=nat.CONSTRAINT_TOL, iters=nat.CONSTRAINT_ITERS,
                                 damping=nat.CONSTRAINT_DAMPING, max_step=nat.CONSTRAINT_MAX_STEP, ee_offset7=None):
        """Damped Gauss-Newton from every column of q [n, B] onto the set where c holds at tol, inside the joint
        limits: a dict of device tensors x [n, B], violation [B] (at x), status [B] int32 (nat.CONSTRAINT_PROJECTED:
        the violation is <= tol and x lies within the limits; CONSTRAINT_BUDGET: `iters` steps were not enough;
        CONSTRAINT_FAILED: a NaN or infinite joint, or a failed factorisation) and iterations [B] int32.  A column
        that satisfies c comes back unchanged after 0 iterations.  Stream-ordered."""
        B = self._check_q(q)
        box = _box_ptrs(constraint_arrays(c))
        tol, iters, damping, max_step = nat.check_project_args(tol, iters, damping, max_step)
        ee = self._ee7(ee_offset7)
        out = dict(x=torch.empty_like(q), violation=torch.empty(B, dtype=torch.float64, device=q.device),
                   status=torch.empty(B, dtype=torch.int32, device=q.device),
                   iterations=torch.empty(B, dtype=torch.int32, device=q.device))
        nat.check(nat.lib().optik_hip_constraint_project_batch(
            self._h, _dpn(ee), *box, _ptr(q), B, tol, iters, damping,
            max_step, _ptr(out["x"]), _ptr(out["violation"]), _ptr(out["status"]), _ptr(out["iterations"]),
            _stream_ptr()))
        return out

    def constraint_motion_batch(self, qa, qb, resolution, c, tol=nat.CONSTRAINT_TOL, ee_offset7=None):
        """The straight joint-space motions qa[:, b] -> qb[:, b] ([n, B]) sampled as collision_motion_batch samples
        them, against the pose constraint c: (violation [B], ok [B] bool, first [B] int32, steps [B] int32) -- the
        largest violation over the samples (NaN if any sample's is), whether every sample's is <= tol, the lowest
        sample index that is not (-1: none), the number of steps K (-1: not sampled, then NaN and False).  One pass,
        no projection: it says what holds at the samples.  Stream-ordered."""
        B = self._check_q(qa)
        if self._check_q(qb) != B or qb.device != qa.device:
            raise ValueError(f"qa and qb must have the same shape and device, got {tuple(qa.shape)} and {tuple(qb.shape)}")
        h = nat.check_resolution(resolution)
        box = _box_ptrs(constraint_arrays(c))
        tol = nat.check_constraint_tol(tol)
        ee = self._ee7(ee_offset7)
        v = torch.empty(B, dtype=torch.float64, device=qa.device)
        ok = torch.empty(B, dtype=torch.uint8, device=qa.device)
        first = torch.empty(B, dtype=torch.int32, device=qa.device)
        steps = torch.empty(B, dtype=torch.int32, device=qa.device)
        nat.check(nat.lib().optik_hip_constraint_motion_batch(
            self._h, _dpn(ee), *box, _ptr(qa), _ptr(qb), B, h, tol,
            _ptr(v), _ptr(ok), _ptr(first), _ptr(steps), _stream_ptr()))
        return v, ok.bool(), first, steps

    def _constraint_mask(self, w, frm, nodes, idx, resolution, c, tol, reverse=False, ee_offset7=None):
        """w [k, Q] with +inf wherever the motion frm[:, q] -> nodes[:, idx[s, q]] (reverse: node -> frm; idx None:
        frm[:, q] -> nodes[:, q]) does not pass constraint_motion_batch.  Slots without a node (-1) keep their +inf;
        device gathers, no host synchronisation."""
        n, Q = frm.shape
        if idx is None:
            a, b = frm, nodes
        else:
            k = idx.shape[0]
            a = frm.unsqueeze(1).expand(n, k, Q).reshape(n, k * Q).contiguous()
            b = nodes[:, idx.clamp(min=0).reshape(-1).long()].contiguous()
        if reverse:
            a, b = b, a
        ok = self.constraint_motion_batch(a, b, resolution, c, tol, ee_offset7=ee_offset7)[1].reshape(w.shape)
        return torch.where(ok, w, torch.full_like(w, float("inf")))

    def roadmap_build_constrained(self, nodes, k, resolution, c, tol=nat.CONSTRAINT_TOL, ee_offset7=None):
        """roadmap_build with w = +inf wherever the motion node -> neighbour does not pass constraint_motion_batch at
        tol.  The nodes are the caller's -- projected onto c, say; a NaN column joins nothing: roadmap_knn orders it
        last and neither check samples it.  Returns (nbr [k, N] int32, w [k, N]).  No host synchronisation."""
        nbr, w = self.roadmap_build(nodes, k, resolution, ee_offset7=ee_offset7)
        return nbr, self._constraint_mask(w, nodes, nodes, nbr, resolution, c, tol, ee_offset7=ee_offset7)

    def roadmap_plan_constrained(self, roadmap, starts, goals, ks, Lmax, resolution, c, tol=nat.CONSTRAINT_TOL,
                                 ee_offset7=None):
        """roadmap_plan's sequence over roadmap = (nodes, nbr, w) of roadmap_build_constrained, with the same mask
        on the start links (start -> node), the goal links (node -> goal) and the direct motion.  So every segment of
        a found path is a motion that passed the collision check and the constraint check in the direction of
        travel, at the samples; a start or goal that violates c has no link and comes back with status 1.  Returns
        roadmap_query's dict.  No host synchronisation."""
        nodes, nbr, w = roadmap
        sidx, _ = self.roadmap_knn(starts, nodes, ks)
        gidx, _ = self.roadmap_knn(goals, nodes, ks)
        sw = self.roadmap_edges(starts, nodes, sidx, resolution, ee_offset7=ee_offset7)
        gw = self.roadmap_edges(goals, nodes, gidx, resolution, reverse=True, ee_offset7=ee_offset7)
        direct = self.roadmap_edges(starts, goals, None, resolution, ee_offset7=ee_offset7)
        sw = self._constraint_mask(sw, starts, nodes, sidx, resolution, c, tol, ee_offset7=ee_offset7)
        gw = self._constraint_mask(gw, goals, nodes, gidx, resolution, c, tol, reverse=True, ee_offset7=ee_offset7)
        direct = self._constraint_mask(direct, starts, goals, None, resolution, c, tol, ee_offset7=ee_offset7)
        return self.roadmap_query(nodes, nbr, w, starts, goals, sidx, sw, gidx, gw, direct.reshape(-1), Lmax)

    # -- goal-set planning (include/optik_hip.h) -------------------------------------------
    def _check_goal_slots(self, t, G, Q, name, dtype):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.dim() == 3 and t.shape[0] == G
                and t.shape[2] == Q and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous {dtype} cuda tensor [{G}, kg, {Q}]")
        nat.check_roadmap_args(k=int(t.shape[1]))
        return int(t.shape[1])

    def roadmap_query_goals(self, nodes, nbr, w, start, goals, gcount, sidx, sw, gidx, gw, direct, Lmax, route=False):
        """roadmap_query with G goal slots per query (optik_hip_roadmap_query_goals): goals [G, n, Q], gcount [Q]
        int32 -- only the goals g < gcount exist, nothing of the others is read --, the goal links gidx, gw [G, kg, Q]
        and the direct weights direct [G, Q]; nodes, nbr, w, start and the start links sidx, sw [ks, Q] as there.
        Returns roadmap_query's dict for the cheapest route to any counted goal plus which [Q] int32, the goal reached
        (-1 unless status 0); route=True adds route and hop [Lmax, Q] int32 as roadmap_query_route.  Stream-ordered."""
        N, Q = self._check_q(nodes), self._check_q(start)
        if not (isinstance(goals, torch.Tensor) and goals.is_cuda and goals.dtype == torch.float64 and goals.dim() == 3
                and goals.shape[1] == self.n and goals.shape[2] == Q and goals.is_contiguous()):
            raise ValueError(f"goals must be a contiguous float64 cuda tensor [G, n, Q] = [G, {self.n}, {Q}]")
        G = nat.check_roadmap_goals(int(goals.shape[0]))
        nat.check_roadmap_args(N=N, max_waypoints=Lmax)
        if not (isinstance(gcount, torch.Tensor) and gcount.is_cuda and gcount.dtype == torch.int32
                and tuple(gcount.shape) == (Q,) and gcount.is_contiguous()):
            raise ValueError(f"gcount must be a contiguous int32 cuda tensor [{Q}]")
        k = self._check_slots(nbr, N, "nbr", torch.int32)
        if self._check_slots(w, N, "w", torch.float64) != k:
            raise ValueError("nbr and w must have the same shape")
        ks = self._check_slots(sidx, Q, "sidx", torch.int32)
        kg = self._check_goal_slots(gidx, G, Q, "gidx", torch.int32)
        if self._check_slots(sw, Q, "sw", torch.float64) != ks or self._check_goal_slots(gw, G, Q, "gw",
                                                                                       torch.float64) != kg:
            raise ValueError("a link's indices and weights must have the same shape")
        if not (isinstance(direct, torch.Tensor) and direct.is_cuda and direct.dtype == torch.float64
                and tuple(direct.shape) == (G, Q) and direct.is_contiguous()):
            raise ValueError(f"direct must be a contiguous float64 cuda tensor [{G}, {Q}]")
        dev = nodes.device
        res = dict(path=torch.empty((int(Lmax), Q, self.n), dtype=torch.float64, device=dev),
                   len=torch.empty(Q, dtype=torch.int32, device=dev),
                   cost=torch.empty(Q, dtype=torch.float64, device=dev),
                   status=torch.empty(Q, dtype=torch.int32, device=dev),
                   which=torch.empty(Q, dtype=torch.int32, device=dev))
        if route:
            res["route"] = torch.empty((int(Lmax), Q), dtype=torch.int32, device=dev)
            res["hop"] = torch.empty((int(Lmax), Q), dtype=torch.int32, device=dev)
        nat.check(nat.lib().optik_hip_roadmap_query_goals(
            self._h, _ptr(nodes), N, _ptr(nbr), _ptr(w), k, _ptr(start), _ptr(goals), _ptr(gcount), G, Q, _ptr(sidx),
            _ptr(sw), ks, _ptr(gidx), _ptr(gw), kg, _ptr(direct), int(Lmax), _ptr(res["path"]), _ptr(res["len"]),
            _ptr(res["cost"]), _ptr(res["status"]), _ptr(res["which"]), _ptr(res.get("route")), _ptr(res.get("hop")),
            _stream_ptr()))
        return res

    def roadmap_plan_goals(self, roadmap, starts, goals, gcount, ks, Lmax, resolution, ee_offset7=None):
        """Plans starts[:, q] ([n, Q]) to the nearest of goals[:gcount[q], :, q] ([G, n, Q], gcount [Q] int32) over
        roadmap = (nodes, nbr, w): roadmap_plan's steps with the G * Q goal columns in one batch each -- the ks
        nearest nodes of every start and every goal, the links start -> node and node -> goal, the direct motions
        start -> goal g (the starts repeated G times) --, then roadmap_query_goals.  Existing entry points and the
        goal-set query on the current stream, torch reshapes between them, no host synchronisation.  A goal past
        gcount (the NaN rows of ik_solutions) goes through the searches and the motion check as it is -- a NaN segment
        is not sampled and costs nothing -- and its results are never read.  Returns roadmap_query_goals' dict."""
        nodes, nbr, w = roadmap
        Q = self._check_q(starts)
        if not (isinstance(goals, torch.Tensor) and goals.is_cuda and goals.dtype == torch.float64 and goals.dim() == 3
                and goals.shape[1] == self.n and goals.shape[2] == Q and goals.is_contiguous()):
            raise ValueError(f"goals must be a contiguous float64 cuda tensor [G, n, Q] = [G, {self.n}, {Q}]")
        G = nat.check_roadmap_goals(int(goals.shape[0]))
        # [n, G * Q]: goal g of query q is column g * Q + q (for Q = 1 the reshape is a transposed view: a copy then)
        cols = goals.permute(1, 0, 2).reshape(self.n, G * Q).contiguous()
        sidx, _ = self.roadmap_knn(starts, nodes, ks)
        gidx, _ = self.roadmap_knn(cols, nodes, ks)
        sw = self.roadmap_edges(starts, nodes, sidx, resolution, ee_offset7=ee_offset7)
        gw = self.roadmap_edges(cols, nodes, gidx, resolution, reverse=True, ee_offset7=ee_offset7)
        direct = self.roadmap_edges(starts.repeat(1, G), cols, None, resolution, ee_offset7=ee_offset7)
        ks = int(ks)
        return self.roadmap_query_goals(nodes, nbr, w, starts, goals, gcount, sidx, sw,
                                        gidx.reshape(ks, G, Q).permute(1, 0, 2).contiguous(),
                                        gw.reshape(ks, G, Q).permute(1, 0, 2).contiguous(), direct.reshape(G, Q), Lmax)

    def roadmap_plan_poses(self, roadmap, cfg, targets, starts, restart_begin, restart_end, K, min_dist, ks, Lmax,
                           resolution, ee_offset7=None):
        """Plans starts[:, q] ([n, Q]) to the poses targets [Q, 7]: ik_solutions with x0 = the starts and up to K <=
        16 solutions per pose, whose count is the goal count and whose x [Q, K, n] becomes the goal set [K, n, Q],
        then roadmap_plan_goals -- back to back on the current stream, no host synchronisation, the solutions never
        leave the device.  With a collision model installed the solutions are the collision-free ones (DESIGN.md
        section 5.12); in the Quality mode solution 0 is the one nearest the start.  Returns roadmap_plan_goals' dict
        plus goals [K, n, Q] and count [Q] int32."""
        K = nat.check_roadmap_goals(K)
        Q = self._check_q(starts)
        sol = self.ik_solutions(cfg, targets, starts.t().contiguous(), restart_begin, restart_end, K, min_dist,
                                ee_offset7=ee_offset7)
        goals = sol["x"].permute(1, 2, 0).contiguous()
        res = self.roadmap_plan_goals(roadmap, starts, goals, sol["count"], ks, Lmax, resolution,
                                      ee_offset7=ee_offset7)
        res["goals"], res["count"] = goals, sol["count"]
        return res

    # -- lazy roadmaps (include/optik_hip.h) ------------------------------------------------
    def roadmap_query_route(self, nodes, nbr, w, start, goal, sidx, sw, gidx, gw, direct, Lmax):
        """roadmap_query with two more tensors in its dict (optik_hip_roadmap_query_route): route [Lmax, Q] int32,
        the node of waypoint t for 1 <= t < len - 1 and -1 elsewhere, and hop [Lmax, Q] int32, the slot of the graph
        hop that leaves waypoint t (-1 for the route's last node and elsewhere).  Stream-ordered."""
        Q = self._check_q(start)
        route = torch.empty((int(Lmax), Q), dtype=torch.int32, device=nodes.device)
        hop = torch.empty((int(Lmax), Q), dtype=torch.int32, device=nodes.device)
        res = self.roadmap_query(nodes, nbr, w, start, goal, sidx, sw, gidx, gw, direct, Lmax, _route=(route, hop))
        res["route"], res["hop"] = route, hop
        return res

    def roadmap_build_lazy(self, nodes, k, resolution, ee_offset7=None):
        """A lazy roadmap over nodes [n, N]: every node's k nearest others, the lengths of the motions to them in
        place of their check, and the reset against the chain's model and world.  Returns a LazyRoadmap: the device
        tensors nodes, nbr [k, N] int32, w0 [k, N], verdict [k, N] int32 (nat.ROADMAP_SLOT_*) and w [k, N], with k and
        the resolution.  Stream-ordered."""
        h = nat.check_resolution(resolution)
        nbr, _ = self.roadmap_knn(nodes, nodes, k, exclude_self=True)
        rm = LazyRoadmap(nodes, nbr, torch.empty(nbr.shape, dtype=torch.float64, device=nodes.device),
                         torch.empty(nbr.shape, dtype=torch.float64, device=nodes.device), torch.empty_like(nbr), h)
        self.roadmap_lazy_reset(rm, ee_offset7=ee_offset7, lengths=True)
        return rm

    def roadmap_lazy_reset(self, roadmap, ee_offset7=None, node_free=None, lengths=False):
        """Forgets the verdicts of a LazyRoadmap (optik_hip_roadmap_lazy_reset): what to call after the chain's model
        or world changed.  A slot is blocked if it is empty or touches a node that is not free, unknown otherwise.
        node_free [N] uint8 stands for the classification of the nodes (the tests); lengths=True writes w0 first.
        Stream-ordered; returns the roadmap."""
        rm = roadmap
        N, k = self._check_q(rm.nodes), self._check_slots(rm.nbr, rm.nodes.shape[1], "nbr", torch.int32)
        nat.check_roadmap_args(N=N, k=k)
        for name, t, dt in (("w0", rm.w0, torch.float64), ("w", rm.w, torch.float64), ("verdict", rm.verdict, torch.int32)):
            if self._check_slots(t, N, name, dt) != k:
                raise ValueError(f"{name} must have nbr's shape")
        if node_free is not None and not (isinstance(node_free, torch.Tensor) and node_free.is_cuda
                                          and node_free.dtype == torch.uint8 and node_free.numel() == N
                                          and node_free.is_contiguous()):
            raise ValueError(f"node_free must be a contiguous uint8 cuda tensor of {N} flags")
        ee = self._ee7(ee_offset7)
        nat.check(nat.lib().optik_hip_roadmap_lazy_reset(
            self._h, _dpn(ee), _ptr(rm.nodes), N, _ptr(rm.nbr), k, 1 if lengths else 0,
            _ptr(rm.w0), _ptr(node_free), _ptr(rm.verdict), _ptr(rm.w), _stream_ptr()))
        return rm

    def _lazy_loop(self, rm, q, Lmax, rounds, call):
        start, goal, sidx, sw, gidx, gw, direct = q
        N, Q = self._check_q(rm.nodes), self._check_q(start)
        if self._check_q(goal) != Q:
            raise ValueError("start and goal must have the same shape")
        nat.check_roadmap_args(N=N, max_waypoints=Lmax)
        rounds = nat.check_lazy_rounds(rounds)
        k = self._check_slots(rm.nbr, N, "nbr", torch.int32)
        ks, kg = self._check_slots(sidx, Q, "sidx", torch.int32), self._check_slots(gidx, Q, "gidx", torch.int32)
        if self._check_slots(sw, Q, "sw", torch.float64) != ks or self._check_slots(gw, Q, "gw", torch.float64) != kg:
            raise ValueError("a link's indices and weights must have the same shape")
        if not (isinstance(direct, torch.Tensor) and direct.is_cuda and direct.dtype == torch.float64
                and direct.numel() == Q and direct.is_contiguous()):
            raise ValueError(f"direct must be a contiguous float64 cuda tensor of {Q} weights")
        dev = rm.nodes.device
        res = dict(path=torch.empty((int(Lmax), Q, self.n), dtype=torch.float64, device=dev),
                   len=torch.empty(Q, dtype=torch.int32, device=dev),
                   cost=torch.empty(Q, dtype=torch.float64, device=dev),
                   status=torch.empty(Q, dtype=torch.int32, device=dev))
        used, checked = C.c_int32(0), C.c_int64(0)
        nat.check(call(k, N, (_ptr(start), _ptr(goal), Q, _ptr(sidx), _ptr(sw), ks, _ptr(gidx), _ptr(gw), kg,
                              _ptr(direct), int(Lmax), rounds, _ptr(res["path"]), _ptr(res["len"]), _ptr(res["cost"]),
                              _ptr(res["status"]), C.byref(used), C.byref(checked), _stream_ptr())))
        res["rounds"], res["checked"] = int(used.value), int(checked.value)
        return res

    def roadmap_plan_lazy(self, roadmap, starts, goals, ks, Lmax, rounds=None, ee_offset7=None):
        """roadmap_plan over a LazyRoadmap (optik_hip_roadmap_lazy_plan): the links and the direct motion are checked
        as roadmap_plan checks them, then passes of the query alternate with checks of the unknown edges that the
        found routes use, at most `rounds` times (None: nat.ROADMAP_LAZY_ROUNDS); the verdicts stay in the roadmap.
        Returns roadmap_query's dict with status 4 (nat.ROADMAP_UNSETTLED) for a route that still holds an unchecked
        edge, and "rounds" and "checked" as Python ints.
        Unlike roadmap_plan this call synchronises with the host: the loop reads one int32, the number of edges to
        check, after every pass -- one stream synchronise per round made."""
        rm = roadmap
        h = rm.resolution
        sidx, _ = self.roadmap_knn(starts, rm.nodes, ks)
        gidx, _ = self.roadmap_knn(goals, rm.nodes, ks)
        sw = self.roadmap_edges(starts, rm.nodes, sidx, h, ee_offset7=ee_offset7)
        gw = self.roadmap_edges(goals, rm.nodes, gidx, h, reverse=True, ee_offset7=ee_offset7)
        direct = self.roadmap_edges(starts, goals, None, h, ee_offset7=ee_offset7)
        ee = self._ee7(ee_offset7)
        return self._lazy_loop(rm, (starts, goals, sidx, sw, gidx, gw, direct), Lmax, rounds,
                               lambda k, N, q: nat.lib().optik_hip_roadmap_lazy_plan(
                                   self._h, _dpn(ee), _ptr(rm.nodes), N, _ptr(rm.nbr),
                                   _ptr(rm.w), _ptr(rm.verdict), k, h, *q))

    def roadmap_plan_lazy_from_flags(self, roadmap, edge_free, node_free, start, goal, sidx, sw, gidx, gw, direct,
                                     Lmax, rounds):
        """The loop of roadmap_plan_lazy with edge_free [k, N] uint8 in place of the motion check (a test hook:
        optik_hip_roadmap_lazy_plan_from_flags); node_free [N] uint8 not None resets the roadmap from it first.  The
        links and the direct weights are given, as for roadmap_query."""
        rm = roadmap
        if self._check_slots(edge_free, rm.nodes.shape[1], "edge_free", torch.uint8) != rm.nbr.shape[0]:
            raise ValueError("edge_free must have nbr's shape")
        return self._lazy_loop(rm, (start, goal, sidx, sw, gidx, gw, direct), Lmax, rounds,
                               lambda k, N, q: nat.lib().optik_hip_roadmap_lazy_plan_from_flags(
                                   self._h, _ptr(rm.nodes), N, _ptr(rm.nbr), _ptr(rm.w0), _ptr(rm.w), _ptr(rm.verdict),
                                   k, _ptr(edge_free), _ptr(node_free), *q))

    # -- goal sets on lazy roadmaps (include/optik_hip.h) ------------------------------------
    def _goals_lazy_loop(self, rm, q, Lmax, rounds, skip_settled, call):
        start, goals, gcount, sidx, sw, gidx, gw, direct = q
        N, Q = self._check_q(rm.nodes), self._check_q(start)
        if not (isinstance(goals, torch.Tensor) and goals.is_cuda and goals.dtype == torch.float64 and goals.dim() == 3
                and goals.shape[1] == self.n and goals.shape[2] == Q and goals.is_contiguous()):
            raise ValueError(f"goals must be a contiguous float64 cuda tensor [G, n, Q] = [G, {self.n}, {Q}]")
        G = nat.check_roadmap_goals(int(goals.shape[0]))
        nat.check_roadmap_args(N=N, max_waypoints=Lmax)
        rounds = nat.check_lazy_rounds(rounds)
        if not (isinstance(gcount, torch.Tensor) and gcount.is_cuda and gcount.dtype == torch.int32
                and tuple(gcount.shape) == (Q,) and gcount.is_contiguous()):
            raise ValueError(f"gcount must be a contiguous int32 cuda tensor [{Q}]")
        k = self._check_slots(rm.nbr, N, "nbr", torch.int32)
        ks = self._check_slots(sidx, Q, "sidx", torch.int32)
        kg = self._check_goal_slots(gidx, G, Q, "gidx", torch.int32)
        if self._check_slots(sw, Q, "sw", torch.float64) != ks or self._check_goal_slots(gw, G, Q, "gw",
                                                                                       torch.float64) != kg:
            raise ValueError("a link's indices and weights must have the same shape")
        if not (isinstance(direct, torch.Tensor) and direct.is_cuda and direct.dtype == torch.float64
                and tuple(direct.shape) == (G, Q) and direct.is_contiguous()):
            raise ValueError(f"direct must be a contiguous float64 cuda tensor [{G}, {Q}]")
        dev = rm.nodes.device
        res = dict(path=torch.empty((int(Lmax), Q, self.n), dtype=torch.float64, device=dev),
                   len=torch.empty(Q, dtype=torch.int32, device=dev),
                   cost=torch.empty(Q, dtype=torch.float64, device=dev),
                   status=torch.empty(Q, dtype=torch.int32, device=dev),
                   which=torch.empty(Q, dtype=torch.int32, device=dev))
        used, checked = C.c_int32(0), C.c_int64(0)
        nat.check(call(k, N, (_ptr(start), _ptr(goals), _ptr(gcount), G, Q, _ptr(sidx), _ptr(sw), ks, _ptr(gidx),
                              _ptr(gw), kg, _ptr(direct), int(Lmax), rounds, 1 if skip_settled else 0,
                              _ptr(res["path"]), _ptr(res["len"]), _ptr(res["cost"]), _ptr(res["status"]),
                              _ptr(res["which"]), C.byref(used), C.byref(checked), _stream_ptr())))
        res["rounds"], res["checked"] = int(used.value), int(checked.value)
        return res

    def roadmap_plan_goals_lazy(self, roadmap, starts, goals, gcount, ks, Lmax, rounds=None, ee_offset7=None,
                                _skip_settled=True):
        """roadmap_plan_goals over a LazyRoadmap (optik_hip_roadmap_lazy_plan_goals): the start links, the G * ks goal
        links and the G direct motions are checked as roadmap_plan_goals checks them, then passes of the goal-set
        query alternate with checks of the unknown edges that the found routes use, at most `rounds` times (None:
        nat.ROADMAP_LAZY_ROUNDS); the verdicts stay in the roadmap.  Every pass after the first runs only the queries
        that can still change (_skip_settled=False runs all of them every time: the same outputs, for measurements).
        Returns roadmap_query_goals' dict with status 4 (nat.ROADMAP_UNSETTLED) for a route that still holds an
        unchecked edge (which -1, the start and then goal 0), and "rounds" and "checked" as Python ints.  Like
        roadmap_plan_lazy this call synchronises the current stream once per round made."""
        rm = roadmap
        h = rm.resolution
        Q = self._check_q(starts)
        if not (isinstance(goals, torch.Tensor) and goals.is_cuda and goals.dtype == torch.float64 and goals.dim() == 3
                and goals.shape[1] == self.n and goals.shape[2] == Q and goals.is_contiguous()):
            raise ValueError(f"goals must be a contiguous float64 cuda tensor [G, n, Q] = [G, {self.n}, {Q}]")
        G = nat.check_roadmap_goals(int(goals.shape[0]))
        # [n, G * Q]: goal g of query q is column g * Q + q (for Q = 1 the reshape is a transposed view: a copy then)
        cols = goals.permute(1, 0, 2).reshape(self.n, G * Q).contiguous()
        sidx, _ = self.roadmap_knn(starts, rm.nodes, ks)
        gidx, _ = self.roadmap_knn(cols, rm.nodes, ks)
        sw = self.roadmap_edges(starts, rm.nodes, sidx, h, ee_offset7=ee_offset7)
        gw = self.roadmap_edges(cols, rm.nodes, gidx, h, reverse=True, ee_offset7=ee_offset7)
        direct = self.roadmap_edges(starts.repeat(1, G), cols, None, h, ee_offset7=ee_offset7)
        ks = int(ks)
        ee = self._ee7(ee_offset7)
        return self._goals_lazy_loop(
            rm, (starts, goals, gcount, sidx, sw, gidx.reshape(ks, G, Q).permute(1, 0, 2).contiguous(),
                 gw.reshape(ks, G, Q).permute(1, 0, 2).contiguous(), direct.reshape(G, Q)), Lmax, rounds, _skip_settled,
            lambda k, N, q: nat.lib().optik_hip_roadmap_lazy_plan_goals(
                self._h, _dpn(ee), _ptr(rm.nodes), N, _ptr(rm.nbr), _ptr(rm.w), _ptr(rm.verdict), k, h, *q))

    def roadmap_plan_goals_lazy_from_flags(self, roadmap, edge_free, node_free, start, goals, gcount, sidx, sw, gidx,
                                           gw, direct, Lmax, rounds, skip_settled=True):
        """The loop of roadmap_plan_goals_lazy with edge_free [k, N] uint8 in place of the motion check (a test hook:
        optik_hip_roadmap_lazy_plan_goals_from_flags); node_free [N] uint8 not None resets the roadmap from it first.
        The links and the direct weights are given, as for roadmap_query_goals."""
        rm = roadmap
        if self._check_slots(edge_free, rm.nodes.shape[1], "edge_free", torch.uint8) != rm.nbr.shape[0]:
            raise ValueError("edge_free must have nbr's shape")
        return self._goals_lazy_loop(rm, (start, goals, gcount, sidx, sw, gidx, gw, direct), Lmax, rounds, skip_settled,
                                     lambda k, N, q: nat.lib().optik_hip_roadmap_lazy_plan_goals_from_flags(
                                         self._h, _ptr(rm.nodes), N, _ptr(rm.nbr), _ptr(rm.w0), _ptr(rm.w),
                                         _ptr(rm.verdict), k, _ptr(edge_free), _ptr(node_free), *q))

    def roadmap_plan_poses_lazy(self, roadmap, cfg, targets, starts, restart_begin, restart_end, K, min_dist, ks, Lmax,
                                rounds=None, ee_offset7=None):
        """roadmap_plan_poses over a LazyRoadmap: ik_solutions with x0 = the starts in front of roadmap_plan_goals_lazy
        on the same stream.  Returns roadmap_plan_goals_lazy's dict plus goals [K, n, Q] and count [Q] int32."""
        K = nat.check_roadmap_goals(K)
        self._check_q(starts)
        sol = self.ik_solutions(cfg, targets, starts.t().contiguous(), restart_begin, restart_end, K, min_dist,
                                ee_offset7=ee_offset7)
        goals = sol["x"].permute(1, 2, 0).contiguous()
        res = self.roadmap_plan_goals_lazy(roadmap, starts, goals, sol["count"], ks, Lmax, rounds=rounds,
                                           ee_offset7=ee_offset7)
        res["goals"], res["count"] = goals, sol["count"]
        return res

    def roadmap_plan_region_lazy(self, roadmap, regions, starts, restart_begin, restart_end, K, min_dist, ks, Lmax,
                                 rounds=None, ee_offset7=None, region_args=None):
        """roadmap_plan_region over a LazyRoadmap: ik_region with x0 = the starts (region_args: a dict of its own
        arguments) in front of roadmap_plan_goals_lazy on the same stream.  Returns roadmap_plan_goals_lazy's dict
        plus goals [K, n, Q] and count [Q] int32."""
        goals, count = self._region_goals(regions, starts, restart_begin, restart_end, K, min_dist,
                                          dict(region_args or {}, ee_offset7=ee_offset7))
        res = self.roadmap_plan_goals_lazy(roadmap, starts, goals, count, ks, Lmax, rounds=rounds,
                                           ee_offset7=ee_offset7)
        res["goals"], res["count"] = goals, count
        return res

    # -- the bidirectional tree planner (include/optik_hip.h) -----------------------------
    def rrt_plan(self, starts, goals, iters, step, resolution, first=0, max_nodes=nat.RRT_NODES, Lmax=64,
                 poll=nat.RRT_POLL, ee_offset7=None):
        """Plans starts[:, q] -> goals[:, q] ([n, Q] each) without a roadmap (optik_hip_rrt_plan): two trees per
        query, grown from its own start and goal towards the samples first, first + 1, ... of seed_batch, every motion
        checked at `resolution` in the direction the path travels it.  Returns a dict of device tensors: path [Lmax, Q,
        n] (what path_shortcut, path_resample and path_optimize take), len [Q] int32, cost [Q], status [Q] int32
        (nat.ROADMAP_FOUND .. ROADMAP_NAN), iters [Q] int32 and nodes [2, Q] int32.
        Unlike roadmap_plan this call synchronises with the host: the loop over the iterations reads one int32, the
        number of queries that have not ended, every `poll` iterations."""
        Q = self._check_q(starts)
        if self._check_q(goals) != Q:
            raise ValueError("starts and goals must have the same shape")
        iters, step, max_nodes, poll, first = nat.check_rrt_args(iters, step, max_nodes, Lmax, poll, first)
        h = nat.check_resolution(resolution)
        dev = starts.device
        res = dict(path=torch.empty((int(Lmax), Q, self.n), dtype=torch.float64, device=dev),
                   len=torch.empty(Q, dtype=torch.int32, device=dev),
                   cost=torch.empty(Q, dtype=torch.float64, device=dev),
                   status=torch.empty(Q, dtype=torch.int32, device=dev),
                   iters=torch.empty(Q, dtype=torch.int32, device=dev),
                   nodes=torch.empty((2, Q), dtype=torch.int32, device=dev))
        ee = self._ee7(ee_offset7)
        nat.check(nat.lib().optik_hip_rrt_plan(
            self._h, _dpn(ee), _ptr(starts), _ptr(goals), Q, iters, step, h, first,
            max_nodes, int(Lmax), poll, _ptr(res["path"]), _ptr(res["len"]), _ptr(res["cost"]), _ptr(res["status"]),
            _ptr(res["iters"]), _ptr(res["nodes"]), _stream_ptr()))
        return res

    # -- the tree planner with a goal set (include/optik_hip.h) ----------------------------
    def rrt_plan_goals(self, starts, goals, gcount, iters, step, resolution, first=0, max_nodes=nat.RRT_NODES, Lmax=64,
                       poll=nat.RRT_POLL, ee_offset7=None):
        """rrt_plan with G goal slots per query (optik_hip_rrt_plan_goals): starts [n, Q], goals [G, n, Q], gcount [Q]
        int32 -- only the goals g < gcount exist, nothing of the others influences an output (the NaN rows of
        ik_solutions past its count are the normal input); gcount None: G each.  Tree 1 has one root per counted goal that is free and the
        query ends at the first junction with any of them: past the direct motions (the nearest free one wins) the
        answer is the goal joined first, not the cheapest.  Returns rrt_plan's dict plus which [Q] int32, the goal
        reached (-1 unless status 0); a found path ends in that goal.  With G = 1 and gcount = 1 it is rrt_plan, bit
        for bit.  max_nodes must be at least G.  Synchronises with the host as rrt_plan does, every `poll`
        iterations."""
        Q = self._check_q(starts)
        if not (isinstance(goals, torch.Tensor) and goals.is_cuda and goals.dtype == torch.float64 and goals.dim() == 3
                and goals.shape[1] == self.n and goals.shape[2] == Q and goals.is_contiguous()):
            raise ValueError(f"goals must be a contiguous float64 cuda tensor [G, n, Q] = [G, {self.n}, {Q}]")
        if gcount is not None and not (isinstance(gcount, torch.Tensor) and gcount.is_cuda
                                       and gcount.dtype == torch.int32 and tuple(gcount.shape) == (Q,)
                                       and gcount.is_contiguous()):
            raise ValueError(f"gcount must be a contiguous int32 cuda tensor [{Q}]")
        iters, step, max_nodes, poll, first = nat.check_rrt_args(iters, step, max_nodes, Lmax, poll, first)
        G = nat.check_rrt_goals(int(goals.shape[0]), max_nodes)
        h = nat.check_resolution(resolution)
        dev = starts.device
        res = dict(path=torch.empty((int(Lmax), Q, self.n), dtype=torch.float64, device=dev),
                   len=torch.empty(Q, dtype=torch.int32, device=dev),
                   cost=torch.empty(Q, dtype=torch.float64, device=dev),
                   status=torch.empty(Q, dtype=torch.int32, device=dev),
                   iters=torch.empty(Q, dtype=torch.int32, device=dev),
                   nodes=torch.empty((2, Q), dtype=torch.int32, device=dev),
                   which=torch.empty(Q, dtype=torch.int32, device=dev))
        ee = self._ee7(ee_offset7)
        nat.check(nat.lib().optik_hip_rrt_plan_goals(
            self._h, _dpn(ee), _ptr(starts), _ptr(goals), _ptr(gcount), Q, G, iters, step, h,
            first, max_nodes, int(Lmax), poll, _ptr(res["path"]), _ptr(res["len"]), _ptr(res["cost"]),
            _ptr(res["status"]), _ptr(res["iters"]), _ptr(res["nodes"]), _ptr(res["which"]), _stream_ptr()))
        return res

    # -- the tree planner under a pose constraint (include/optik_hip.h) --------------------
    def rrt_plan_constrained(self, starts, goals, gcount, c, tol, iters, step, resolution, first=0,
                             max_nodes=nat.RRT_NODES, Lmax=64, poll=nat.RRT_POLL, ptol=nat.CONSTRAINT_TOL,
                             piters=nat.RRT_PROJECT_ITERS, damping=nat.CONSTRAINT_DAMPING,
                             max_step=nat.CONSTRAINT_MAX_STEP, ee_offset7=None):
        """rrt_plan_goals under the pose constraint c (optik_hip_rrt_plan_constrained; csrc/rrt_constrained_measure.hpp):
        starts [n, Q], goals [G, n, Q], gcount [Q] int32 or None (G each).  Every node a tree takes is first projected
        onto c (constraint_project_batch's method at ptol, piters, damping, max_step) and every motion has passed
        collision_motion_batch and constraint_motion_batch at tol, in the direction the path travels it; a start that
        violates c at tol gives status 1, a goal that does is not a root.  Returns rrt_plan_goals' dict plus projected
        [2, Q] int32: the projections attempted and those that ended CONSTRAINT_PROJECTED.  With a box that is free on
        all six axes every shared output is rrt_plan_goals', bit for bit.  tol has no default: it says how far the
        straight motion between two projected nodes may leave c.  Synchronises with the host as rrt_plan does."""
        Q = self._check_q(starts)
        if not (isinstance(goals, torch.Tensor) and goals.is_cuda and goals.dtype == torch.float64 and goals.dim() == 3
                and goals.shape[1] == self.n and goals.shape[2] == Q and goals.is_contiguous()):
            raise ValueError(f"goals must be a contiguous float64 cuda tensor [G, n, Q] = [G, {self.n}, {Q}]")
        if gcount is not None and not (isinstance(gcount, torch.Tensor) and gcount.is_cuda
                                       and gcount.dtype == torch.int32 and tuple(gcount.shape) == (Q,)
                                       and gcount.is_contiguous()):
            raise ValueError(f"gcount must be a contiguous int32 cuda tensor [{Q}]")
        iters, step, max_nodes, poll, first = nat.check_rrt_args(iters, step, max_nodes, Lmax, poll, first)
        G = nat.check_rrt_goals(int(goals.shape[0]), max_nodes)
        h = nat.check_resolution(resolution)
        box = _box_ptrs(constraint_arrays(c))
        tol = nat.check_constraint_tol(tol)
        ptol, piters, damping, max_step = nat.check_project_args(ptol, piters, damping, max_step)
        dev = starts.device
        res = dict(path=torch.empty((int(Lmax), Q, self.n), dtype=torch.float64, device=dev),
                   len=torch.empty(Q, dtype=torch.int32, device=dev),
                   cost=torch.empty(Q, dtype=torch.float64, device=dev),
                   status=torch.empty(Q, dtype=torch.int32, device=dev),
                   iters=torch.empty(Q, dtype=torch.int32, device=dev),
                   nodes=torch.empty((2, Q), dtype=torch.int32, device=dev),
                   which=torch.empty(Q, dtype=torch.int32, device=dev),
                   projected=torch.empty((2, Q), dtype=torch.int32, device=dev))
        ee = self._ee7(ee_offset7)
        nat.check(nat.lib().optik_hip_rrt_plan_constrained(
            self._h, _dpn(ee), *box, tol, ptol, piters, damping,
            max_step, _ptr(starts), _ptr(goals), _ptr(gcount), Q, G, iters, step, h, first, max_nodes, int(Lmax), poll,
            _ptr(res["path"]), _ptr(res["len"]), _ptr(res["cost"]), _ptr(res["status"]), _ptr(res["iters"]),
            _ptr(res["nodes"]), _ptr(res["which"]), _ptr(res["projected"]), _stream_ptr()))
        return res

    def rrt_plan_poses(self, cfg, targets, starts, restart_begin, restart_end, K, min_dist, iters, step, resolution,
                       first=0, max_nodes=nat.RRT_NODES, Lmax=64, poll=nat.RRT_POLL, ee_offset7=None):
        """Plans starts[:, q] ([n, Q]) to the poses targets [Q, 7] without a roadmap: ik_solutions with x0 = the starts
        and up to K <= 16 solutions per pose, whose count is the goal count and whose x [Q, K, n] becomes the goal set
        [K, n, Q], then rrt_plan_goals -- back to back on the current stream, no host synchronisation between the two
        stages, the solutions never leave the device.  It mirrors roadmap_plan_poses.  Returns rrt_plan_goals' dict
        plus goals [K, n, Q] and count [Q] int32."""
        K = nat.check_roadmap_goals(K)
        self._check_q(starts)
        sol = self.ik_solutions(cfg, targets, starts.t().contiguous(), restart_begin, restart_end, K, min_dist,
                                ee_offset7=ee_offset7)
        goals = sol["x"].permute(1, 2, 0).contiguous()
        res = self.rrt_plan_goals(starts, goals, sol["count"], iters, step, resolution, first=first,
                                  max_nodes=max_nodes, Lmax=Lmax, poll=poll, ee_offset7=ee_offset7)
        res["goals"], res["count"] = goals, sol["count"]
        return res

    # -- shortcutting and resampling (include/optik_hip.h) --------------------------------
    def _check_paths(self, path, lens):
        if not (isinstance(path, torch.Tensor) and path.is_cuda and path.dtype == torch.float64 and path.dim() == 3
                and path.shape[2] == self.n and path.is_contiguous()):
            raise ValueError(f"path must be a contiguous float64 cuda tensor [L, P, n] with n = {self.n}")
        L, P = int(path.shape[0]), int(path.shape[1])
        if lens is not None and not (isinstance(lens, torch.Tensor) and lens.is_cuda and lens.dtype == torch.int32
                                     and lens.numel() == P and lens.is_contiguous() and lens.device == path.device):
            raise ValueError(f"lens must be a contiguous int32 cuda tensor of {P} lengths on path's device")
        return L, P

    def path_shortcut(self, path, lens=None, resolution=nat.SHORTCUT_RESOLUTION, vertices=nat.SHORTCUT_VERTICES,
                      hop_penalty=None, max_waypoints=None, ee_offset7=None):
        """Shortcuts P paths over the all-pairs visibility of at most `vertices` vertices each
        (optik_hip_path_shortcut): path [L, P, n] float64 cuda tensor and lens [P] int32 (None: L each) -- roadmap_plan's
        "path" and "len" as they are.  hop_penalty None: the resolution.  max_waypoints None: L.  Stream-ordered on the
        current stream; returns a dict of device tensors: path [max_waypoints, P, n] (what path_optimize takes), len
        [P] int32, cost [P], cost_in [P], status [P] int32 (nat.SHORTCUT_*)."""
        L, P = self._check_paths(path, lens)
        Lout = L if max_waypoints is None else max_waypoints
        h, hop = nat.check_shortcut_args(L, vertices, Lout, resolution, hop_penalty)
        ee = self._ee7(ee_offset7)
        dev = path.device
        res = dict(path=torch.empty((int(Lout), P, self.n), dtype=torch.float64, device=dev),
                   len=torch.empty(P, dtype=torch.int32, device=dev),
                   cost=torch.empty(P, dtype=torch.float64, device=dev),
                   cost_in=torch.empty(P, dtype=torch.float64, device=dev),
                   status=torch.empty(P, dtype=torch.int32, device=dev))
        nat.check(nat.lib().optik_hip_path_shortcut(
            self._h, _dpn(ee), _ptr(path), _ptr(lens), L, P, int(vertices), h, hop,
            int(Lout), _ptr(res["path"]), _ptr(res["len"]), _ptr(res["cost"]), _ptr(res["cost_in"]),
            _ptr(res["status"]), _stream_ptr()))
        return res

    def path_resample(self, path, lens=None, waypoints=nat.RESAMPLE_WAYPOINTS):
        """`waypoints` waypoints at equal arc length (L-infinity) along each of P polylines
        (optik_hip_path_resample): path [L, P, n], lens [P] int32 or None as path_shortcut takes them.  Returns (path
        [waypoints, P, n], status [P] int32).  The new segments cut the input's corners and are not checked.
        Stream-ordered."""
        L, P = self._check_paths(path, lens)
        nat.check_shortcut_args(L, max_waypoints=waypoints)
        out = torch.empty((int(waypoints), P, self.n), dtype=torch.float64, device=path.device)
        status = torch.empty(P, dtype=torch.int32, device=path.device)
        nat.check(nat.lib().optik_hip_path_resample(self._h, _ptr(path), _ptr(lens), L, P, int(waypoints), _ptr(out),
                                                    _ptr(status), _stream_ptr()))
        return out, status

    def path_shortcut_chunk(self, vertices):
        """The paths path_shortcut processes per chunk of its workspace (tests cross it)."""
        return nat.path_shortcut_chunk(self._h, vertices)

    # -- shortcutting and resampling under a pose constraint (include/optik_hip.h) ---------
    def path_shortcut_constrained(self, path, lens, c, tol, ptol=nat.CONSTRAINT_TOL, piters=nat.CONSTRAINT_ITERS,
                                  damping=nat.CONSTRAINT_DAMPING, max_step=nat.CONSTRAINT_MAX_STEP,
                                  resolution=nat.SHORTCUT_RESOLUTION, vertices=nat.SHORTCUT_VERTICES, hop_penalty=None,
                                  max_waypoints=None, ee_offset7=None):
        """path_shortcut under the pose constraint c (optik_hip_path_shortcut_constrained;
        csrc/shortcut_constrained_measure.hpp): every subdivision vertex that is not one of the input's own waypoints
        is projected onto c (constraint_project_batch's method at ptol, piters, damping, max_step; a vertex that does
        not project is dead), and a pair of vertices is open only where the motion between them passes
        collision_motion_batch AND constraint_motion_batch at `resolution`, tol, in the direction of travel.  The
        input's waypoints never move.  Returns path_shortcut's dict plus projected [2, P] int32: the projections
        attempted and those that ended CONSTRAINT_PROJECTED.  cost may exceed cost_in.  With a box that is free on all
        six axes and paths within the joint limits every shared output is path_shortcut's, bit for bit.  tol has no
        default: it says how far the straight motion between two vertices may leave c.  Stream-ordered."""
        L, P = self._check_paths(path, lens)
        Lout = L if max_waypoints is None else max_waypoints
        h, hop = nat.check_shortcut_args(L, vertices, Lout, resolution, hop_penalty)
        box = _box_ptrs(constraint_arrays(c))
        tol = nat.check_constraint_tol(tol)
        ptol, piters, damping, max_step = nat.check_project_args(ptol, piters, damping, max_step)
        ee = self._ee7(ee_offset7)
        dev = path.device
        res = dict(path=torch.empty((int(Lout), P, self.n), dtype=torch.float64, device=dev),
                   len=torch.empty(P, dtype=torch.int32, device=dev),
                   cost=torch.empty(P, dtype=torch.float64, device=dev),
                   cost_in=torch.empty(P, dtype=torch.float64, device=dev),
                   status=torch.empty(P, dtype=torch.int32, device=dev),
                   projected=torch.empty((2, P), dtype=torch.int32, device=dev))
        nat.check(nat.lib().optik_hip_path_shortcut_constrained(
            self._h, _dpn(ee), _ptr(path), _ptr(lens), L, P, int(vertices), h, hop,
            int(Lout), *box, tol, ptol, piters, damping, max_step, _ptr(res["path"]),
            _ptr(res["len"]), _ptr(res["cost"]), _ptr(res["cost_in"]), _ptr(res["status"]), _ptr(res["projected"]),
            _stream_ptr()))
        return res

    def path_resample_constrained(self, path, lens, c, waypoints=nat.RESAMPLE_WAYPOINTS, ptol=nat.CONSTRAINT_TOL,
                                  piters=nat.CONSTRAINT_ITERS, damping=nat.CONSTRAINT_DAMPING,
                                  max_step=nat.CONSTRAINT_MAX_STEP, ee_offset7=None):
        """path_resample with every waypoint between the two ends projected onto the pose constraint c
        (optik_hip_path_resample_constrained): returns (path [waypoints, P, n], status [P] int32, projected [2, P]
        int32).  Status nat.RESAMPLE_UNPROJECTED (4): a projection did not end CONSTRAINT_PROJECTED and the waypoint
        kept its interpolated value; it ranks below 2 and 3, and a path of status 3 is not projected.  The spacing is
        equal before the projection and only approximately equal after it; the new segments are not checked.
        Stream-ordered."""
        L, P = self._check_paths(path, lens)
        nat.check_shortcut_args(L, max_waypoints=waypoints)
        box = _box_ptrs(constraint_arrays(c))
        ptol, piters, damping, max_step = nat.check_project_args(ptol, piters, damping, max_step)
        ee = self._ee7(ee_offset7)
        out = torch.empty((int(waypoints), P, self.n), dtype=torch.float64, device=path.device)
        status = torch.empty(P, dtype=torch.int32, device=path.device)
        projected = torch.empty((2, P), dtype=torch.int32, device=path.device)
        nat.check(nat.lib().optik_hip_path_resample_constrained(
            self._h, _dpn(ee), _ptr(path), _ptr(lens), L, P, int(waypoints), *box, ptol, piters, damping, max_step, _ptr(out), _ptr(status), _ptr(projected),
            _stream_ptr()))
        return out, status, projected

    def constraint_motion_mask(self, qa, qb, resolution, c, tol, flag, ee_offset7=None):
        """Masks flag [B] uint8 in place with constraint_motion_batch's verdicts of qa[:, b] -> qb[:, b] ([n, B]): a
        segment whose flag is 0 is not sampled and stays 0, every other flag becomes the ok byte
        (optik_hip_constraint_motion_mask: what path_shortcut_constrained runs behind the motion check).  Returns
        flag.  Stream-ordered."""
        B = self._check_q(qa)
        if self._check_q(qb) != B or qb.device != qa.device:
            raise ValueError(f"qa and qb must have the same shape and device, got {tuple(qa.shape)} and {tuple(qb.shape)}")
        if not (isinstance(flag, torch.Tensor) and flag.is_cuda and flag.dtype == torch.uint8 and flag.numel() == B
                and flag.is_contiguous() and flag.device == qa.device):
            raise ValueError(f"flag must be a contiguous uint8 cuda tensor of {B} flags on qa's device")
        h = nat.check_resolution(resolution)
        box = _box_ptrs(constraint_arrays(c))
        tol = nat.check_constraint_tol(tol)
        ee = self._ee7(ee_offset7)
        nat.check(nat.lib().optik_hip_constraint_motion_mask(
            self._h, _dpn(ee), *box, _ptr(qa), _ptr(qb), B, h, tol,
            _ptr(flag), _stream_ptr()))
        return flag

    def path_shortcut_constrained_chunk(self, vertices):
        """The paths path_shortcut_constrained processes per chunk of its workspace (tests cross it)."""
        return nat.path_shortcut_constrained_chunk(self._h, vertices)

    # -- timing and sampling (include/optik_hip.h) ------------------------------------------
    def _limits(self, v, name, device):
        if not (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float64 and v.numel() == self.n
                and v.is_contiguous() and v.device == device):
            raise ValueError(f"{name} must be a contiguous float64 cuda tensor of {self.n} limits on path's device")
        return v

    def path_time(self, path, lens=None, v_max=None, a_max=None):
        """Times P paths rest to rest under the joint velocity limits v_max [n] (> 0, inf allowed) and acceleration
        limits a_max [n] (finite, > 0), both float64 cuda tensors (optik_hip_path_time): path [L, P, n] float64 cuda
        tensor and lens [P] int32 (None: L each) -- path_resample's output as it is, 3 <= L <= 64.  Stream-ordered on
        the current stream; returns a dict of device tensors: t [L, P], qd [L, P, n], qdd [L, P, n], x [L, P] (the
        squared path speed), duration [P], status [P] int32 (nat.TIME_*)."""
        L, P = self._check_paths(path, lens)
        nat.check_time_args(self.n, L)
        dev = path.device
        v_max, a_max = self._limits(v_max, "v_max", dev), self._limits(a_max, "a_max", dev)
        res = dict(t=torch.empty((L, P), dtype=torch.float64, device=dev),
                   qd=torch.empty((L, P, self.n), dtype=torch.float64, device=dev),
                   qdd=torch.empty((L, P, self.n), dtype=torch.float64, device=dev),
                   x=torch.empty((L, P), dtype=torch.float64, device=dev),
                   duration=torch.empty(P, dtype=torch.float64, device=dev),
                   status=torch.empty(P, dtype=torch.int32, device=dev))
        nat.check(nat.lib().optik_hip_path_time(self._h, _ptr(path), _ptr(lens), L, P, _ptr(v_max), _ptr(a_max),
                                                _ptr(res["t"]), _ptr(res["qd"]), _ptr(res["qdd"]), _ptr(res["x"]),
                                                _ptr(res["duration"]), _ptr(res["status"]), _stream_ptr()))
        return res

    def path_time_tool(self, path, lens=None, v_max=None, a_max=None, tool_v_max=math.inf,
                       tool_a_tangential=math.inf, tool_a_normal=math.inf, tool_w_max=math.inf, ee_offset7=None):
        """path_time with limits on the tool as well (optik_hip_path_time_tool): the tool
        centre point's speed tool_v_max (m/s), its tangential and normal acceleration (m/s^2) and the end effector's
        angular speed tool_w_max (rad/s), host numbers > 0, inf for "no limit"; the tool is fk_batch's pose with
        ee_offset7.  Returns path_time's dict plus tool_speed [L, P], tool_accel [L, P, 2] (tangential, normal) and
        tool_wspeed [L, P] at the waypoints; it goes into trajectory_sample as it is.  With every tool limit inf the
        shared entries are path_time's bit for bit.  Stream-ordered."""
        L, P = self._check_paths(path, lens)
        nat.check_time_args(self.n, L)
        lim = nat.check_time_tool_args(tool_v_max, tool_a_tangential, tool_a_normal, tool_w_max)
        ee = self._ee7(ee_offset7)
        dev = path.device
        v_max, a_max = self._limits(v_max, "v_max", dev), self._limits(a_max, "a_max", dev)
        res = dict(t=torch.empty((L, P), dtype=torch.float64, device=dev),
                   qd=torch.empty((L, P, self.n), dtype=torch.float64, device=dev),
                   qdd=torch.empty((L, P, self.n), dtype=torch.float64, device=dev),
                   x=torch.empty((L, P), dtype=torch.float64, device=dev),
                   duration=torch.empty(P, dtype=torch.float64, device=dev),
                   status=torch.empty(P, dtype=torch.int32, device=dev),
                   tool_speed=torch.empty((L, P), dtype=torch.float64, device=dev),
                   tool_accel=torch.empty((L, P, 2), dtype=torch.float64, device=dev),
                   tool_wspeed=torch.empty((L, P), dtype=torch.float64, device=dev))
        nat.check(nat.lib().optik_hip_path_time_tool(
            self._h, _ptr(path), _ptr(lens), L, P, _ptr(v_max), _ptr(a_max), _dp(lim), _dpn(ee), _ptr(res["t"]),
            _ptr(res["qd"]), _ptr(res["qdd"]), _ptr(res["x"]), _ptr(res["duration"]), _ptr(res["status"]),
            _ptr(res["tool_speed"]), _ptr(res["tool_accel"]), _ptr(res["tool_wspeed"]), _stream_ptr()))
        return res

    def path_time_spline(self, path, timing, j_max, a_max, v_max, lens=None):
        """Spline retiming of timed paths (optik_hip_path_time_spline): path and lens as
        path_time took them, timing its result (or path_time_tool's; "t" and "status" are read); j_max, a_max, v_max
        float64 cuda tensors [n] (> 0, inf allowed).  Returns a dict of device tensors: t [L, P], qd and qdd [L, P, n]
        -- the clamped C2 cubic spline through the waypoints at the times factor * t, slowed uniformly until the three
        limits hold along the whole curve --, duration [P], factor [P], ratios [P, 3] (peak velocity, acceleration,
        jerk over their limits), status [P] int32 (nat.SPLINE_*).  It goes into trajectory_sample as it is; a path
        with status 4 (nat.SPLINE_OVER_LIMIT: rare, rounding) is held at its start there like every status other than
        0, and is cleared by passing the result in again as `timing`.  As in path_time the limits' VALUES are not
        checked here -- they are device tensors --: a limit that is 0, negative or NaN gives status 1 or ratios without
        meaning, not a refusal; Robot.smooth_timing checks them on the host.  Stream-ordered."""
        L, P = self._check_paths(path, lens)
        nat.check_time_spline_args(self.n, L)
        dev = path.device
        t_in, status_in = timing["t"], timing["status"]
        if not (isinstance(t_in, torch.Tensor) and isinstance(status_in, torch.Tensor) and t_in.shape == (L, P)
                and status_in.shape == (P,) and t_in.is_contiguous() and status_in.is_contiguous()
                and t_in.dtype == torch.float64 and status_in.dtype == torch.int32
                and t_in.device == status_in.device == dev):
            raise ValueError("timing must be path_time's result for this path")
        v_max, a_max, j_max = (self._limits(v_max, "v_max", dev), self._limits(a_max, "a_max", dev),
                               self._limits(j_max, "j_max", dev))
        res = dict(t=torch.empty((L, P), dtype=torch.float64, device=dev),
                   qd=torch.empty((L, P, self.n), dtype=torch.float64, device=dev),
                   qdd=torch.empty((L, P, self.n), dtype=torch.float64, device=dev),
                   duration=torch.empty(P, dtype=torch.float64, device=dev),
                   factor=torch.empty(P, dtype=torch.float64, device=dev),
                   ratios=torch.empty((P, 3), dtype=torch.float64, device=dev),
                   status=torch.empty(P, dtype=torch.int32, device=dev))
        nat.check(nat.lib().optik_hip_path_time_spline(
            self._h, _ptr(path), _ptr(lens), L, P, _ptr(t_in), _ptr(status_in), _ptr(v_max), _ptr(a_max), _ptr(j_max),
            _ptr(res["t"]), _ptr(res["qd"]), _ptr(res["qdd"]), _ptr(res["duration"]), _ptr(res["factor"]),
            _ptr(res["ratios"]), _ptr(res["status"]), _stream_ptr()))
        return res

    def trajectory_sample(self, path, timing, dt, samples, lens=None):
        """`samples` samples of each timed path at k * dt by cubic Hermite interpolation over the waypoints' times,
        positions and velocities (optik_hip_trajectory_sample): path and lens as path_time took them, timing its
        result.  Returns (q [samples, P, n], qd [samples, P, n]); past a path's duration its goal at rest, for a status
        other than 0 its start at rest.  The curve leaves the polyline between waypoints and is not checked.
        Stream-ordered."""
        L, P = self._check_paths(path, lens)
        nat.check_time_args(self.n, L)
        dt = nat.check_sample_args(dt, samples)
        t, qd, status = timing["t"], timing["qd"], timing["status"]
        if not (t.shape == (L, P) and qd.shape == (L, P, self.n) and status.shape == (P,) and t.is_contiguous()
                and qd.is_contiguous() and status.is_contiguous() and t.dtype == torch.float64
                and qd.dtype == torch.float64 and status.dtype == torch.int32
                and t.device == qd.device == status.device == path.device):
            raise ValueError("timing must be path_time's result for this path")
        q = torch.empty((int(samples), P, self.n), dtype=torch.float64, device=path.device)
        v = torch.empty_like(q)
        nat.check(nat.lib().optik_hip_trajectory_sample(self._h, _ptr(path), _ptr(lens), L, P, _ptr(t), _ptr(qd),
                                                        _ptr(status), dt, int(samples), _ptr(q), _ptr(v),
                                                        _stream_ptr()))
        return q, v

    def seed_batch(self, first, count):
        q = torch.empty((self.n, count), dtype=torch.float64, device=self.device)
        nat.check(nat.lib().optik_hip_seed_batch(self._h, int(first), int(count), _ptr(q), _stream_ptr()))
        return q

    # -- the hot path -------------------------------------------------------------
    def alloc_ik_buffers(self, T, R, per_restart=True):
        dev = self.device
        bufs = dict(
            win_x=torch.empty((T, self.n), dtype=torch.float64, device=dev),
            win_f=torch.empty(T, dtype=torch.float64, device=dev),
            win_idx=torch.empty(T, dtype=torch.int64, device=dev),
            win_key=torch.empty(T, dtype=torch.float64, device=dev))
        if per_restart:
            bufs.update(
                x=torch.empty((self.n, T * R), dtype=torch.float64, device=dev),
                f=torch.empty(T * R, dtype=torch.float64, device=dev),
                status=torch.empty(T * R, dtype=torch.int32, device=dev),
                evals=torch.empty(T * R, dtype=torch.int32, device=dev))
        return bufs

    def ik_batch(self, cfg, targets, x0, restart_begin, restart_end, flags=0, deadline_s=0.0,
                 ee_offset7=None, bufs=None, per_restart=True):
        """targets [T, 7], x0 [T, n] float64 cuda tensors.  Stream-ordered; returns the
        buffer dict (win_idx is int64 with -1 = UINT64_MAX = no solution)."""
        assert targets.is_cuda and targets.dtype == torch.float64 and targets.is_contiguous()
        assert x0.is_cuda and x0.dtype == torch.float64 and x0.is_contiguous()
        T = targets.shape[0]
        assert targets.shape == (T, 7) and x0.shape == (T, self.n)
        R = int(restart_end - restart_begin)
        if bufs is None:
            bufs = self.alloc_ik_buffers(T, R, per_restart)
        o = nat.IkOutputs()
        o.d_x, o.d_f = _ptr(bufs.get("x")), _ptr(bufs.get("f"))
        o.d_status, o.d_evals = _ptr(bufs.get("status")), _ptr(bufs.get("evals"))
        o.d_win_x, o.d_win_f = _ptr(bufs["win_x"]), _ptr(bufs["win_f"])
        o.d_win_idx, o.d_win_key = _ptr(bufs["win_idx"]), _ptr(bufs["win_key"])
        ee = np.ascontiguousarray(ee_offset7, dtype=np.float64) if ee_offset7 is not None else None
        nat.check(nat.lib().optik_hip_ik_batch(
            self._h, C.byref(cfg), _ptr(targets), _ptr(x0), T, _dpn(ee),
            int(restart_begin), int(restart_end), int(flags), float(deadline_s), C.byref(o),
            _stream_ptr()))
        return bufs

    def ik_solutions(self, cfg, targets, x0, restart_begin, restart_end, k, min_dist, deadline_s=0.0,
                     ee_offset7=None, bufs=None):
        """Up to k distinct solutions per target (optik_hip_ik_solutions): every restart of [restart_begin,
        restart_end) runs to its end, the successes are taken in (key, index) order and kept if their largest joint
        difference to every solution kept before is > min_dist.  targets [T, 7], x0 [T, n] float64 cuda tensors.
        Stream-ordered on the current stream; returns a dict of device tensors: count [T] int32, x [T, k, n],
        f [T, k], idx [T, k] int64 (-1 past count), key [T, k] (+inf past count)."""
        k, min_dist = nat.check_solutions_args(k, min_dist)
        if not (targets.is_cuda and targets.dtype == torch.float64 and targets.is_contiguous()
                and targets.dim() == 2 and targets.shape[1] == 7):
            raise ValueError("targets must be a contiguous float64 cuda tensor [T, 7]")
        T = targets.shape[0]
        if not (x0.is_cuda and x0.dtype == torch.float64 and x0.is_contiguous() and tuple(x0.shape) == (T, self.n)):
            raise ValueError(f"x0 must be a contiguous float64 cuda tensor [T, n] = [{T}, {self.n}]")
        if int(restart_end) <= int(restart_begin) or int(restart_begin) < 0:
            raise ValueError("empty restart range")
        if bufs is None:
            dev = targets.device
            bufs = dict(count=torch.empty(T, dtype=torch.int32, device=dev),
                        x=torch.empty((T, k, self.n), dtype=torch.float64, device=dev),
                        f=torch.empty((T, k), dtype=torch.float64, device=dev),
                        idx=torch.empty((T, k), dtype=torch.int64, device=dev),
                        key=torch.empty((T, k), dtype=torch.float64, device=dev))
        o = nat.IkSolutionsOutputs()
        o.d_count, o.d_x, o.d_f = _ptr(bufs.get("count")), _ptr(bufs.get("x")), _ptr(bufs.get("f"))
        o.d_idx, o.d_key = _ptr(bufs.get("idx")), _ptr(bufs.get("key"))
        ee = np.ascontiguousarray(ee_offset7, dtype=np.float64) if ee_offset7 is not None else None
        nat.check(nat.lib().optik_hip_ik_solutions(
            self._h, C.byref(cfg), _ptr(targets), _ptr(x0), T, _dpn(ee),
            int(restart_begin), int(restart_end), float(deadline_s), k, min_dist, C.byref(o), _stream_ptr()))
        return bufs

    # -- IK into pose regions (include/optik_hip.h) ----------------------------------------
    def ik_region(self, regions, x0, restart_begin, restart_end, k, min_dist, tol=nat.CONSTRAINT_TOL,
                  iters=nat.CONSTRAINT_ITERS, damping=nat.CONSTRAINT_DAMPING, max_step=nat.CONSTRAINT_MAX_STEP,
                  mode="quality", keep=None, ee_offset7=None, per_restart=False, repair=None):
        """Up to k distinct configurations per pose region (optik_hip_ik_region; csrc/region_measure.hpp): regions
        [T, 19] (per row ref7, lo, hi -- optik_amd.constraint.region_rows makes it; device data, not validated here:
        a NaN in a row's reference gives it count 0) and x0 [T, n], float64 cuda tensors.  Restart i of [restart_begin,
        restart_end) starts at x0[t] (i = 0) or at seed_batch's row i and is projected onto the region as
        constraint_project_batch projects (tol, iters, damping, max_step); the rows that projected are taken in (key,
        index) order -- mode "quality": ||x - x0[t]||, "speed": the index, "manipulability" / "condition": -w / -c --,
        without the ones in collision when a model is installed and without the ones that violate keep = (constraint,
        tol), and kept if their largest joint difference to every row kept before is > min_dist.  Stream-ordered;
        returns a dict of device tensors: count [T] int32, x [T, k, n] (NaN past count), violation [T, k] (NaN), idx
        [T, k] int64 (-1), key [T, k] (+inf); with per_restart also restart_x [n, T * R], restart_violation,
        restart_key [T * R], restart_status, restart_iterations [T * R] int32 (column t * R + i - restart_begin).
        repair = dict(influence, safety, step, iters, max_move) (optik_hip_ik_region_repair):
        between the projection and the key passes every projected restart that is in collision is pushed free by
        collision_repair_batch's loop under its own region at tol; one that ends free takes the repaired x, violation
        and key, every other one is left as it was and is dropped by the collision filter as before.  The dict then
        also has "repaired" [T] int32, the restarts of each region that took a repaired x.  repair=None is the call
        without the argument, bit for bit and with not one launch more: the dict then has no "repaired" (a tensor of
        zeros would be a fill on the stream)."""
        k, min_dist = nat.check_solutions_args(k, min_dist)
        rp = nat.region_repair_args(repair) if repair is not None else None
        tol, iters, damping, max_step = nat.check_project_args(tol, iters, damping, max_step)
        mode = nat.solution_mode_code(mode) if isinstance(mode, str) else int(mode)
        kp = keep_arrays(keep)
        if not (isinstance(regions, torch.Tensor) and regions.is_cuda and regions.dtype == torch.float64
                and regions.is_contiguous() and regions.dim() == 2 and regions.shape[1] == nat.REGION_DOUBLES):
            raise ValueError("regions must be a contiguous float64 cuda tensor [T, 19]")
        T = int(regions.shape[0])
        if not (isinstance(x0, torch.Tensor) and x0.is_cuda and x0.dtype == torch.float64 and x0.is_contiguous()
                and tuple(x0.shape) == (T, self.n)):
            raise ValueError(f"x0 must be a contiguous float64 cuda tensor [T, n] = [{T}, {self.n}]")
        b, e = int(restart_begin), int(restart_end)
        if b < 0 or e <= b:
            raise ValueError("empty restart range")
        dev, cols = regions.device, T * (e - b)
        res = dict(count=torch.empty(T, dtype=torch.int32, device=dev),
                   x=torch.empty((T, k, self.n), dtype=torch.float64, device=dev),
                   violation=torch.empty((T, k), dtype=torch.float64, device=dev),
                   idx=torch.empty((T, k), dtype=torch.int64, device=dev),
                   key=torch.empty((T, k), dtype=torch.float64, device=dev))
        o = nat.IkRegionOutputs()
        if per_restart:
            res.update(restart_x=torch.empty((self.n, cols), dtype=torch.float64, device=dev),
                       restart_violation=torch.empty(cols, dtype=torch.float64, device=dev),
                       restart_status=torch.empty(cols, dtype=torch.int32, device=dev),
                       restart_iterations=torch.empty(cols, dtype=torch.int32, device=dev),
                       restart_key=torch.empty(cols, dtype=torch.float64, device=dev))
            o.d_x, o.d_violation = _ptr(res["restart_x"]), _ptr(res["restart_violation"])
            o.d_status, o.d_iterations = _ptr(res["restart_status"]), _ptr(res["restart_iterations"])
            o.d_key = _ptr(res["restart_key"])
        o.d_count, o.d_sol_x, o.d_sol_violation = _ptr(res["count"]), _ptr(res["x"]), _ptr(res["violation"])
        o.d_sol_idx, o.d_sol_key = _ptr(res["idx"]), _ptr(res["key"])
        ee = self._ee7(ee_offset7)
        head = (self._h, _dpn(ee), _ptr(regions), _ptr(x0), T, b, e, tol, iters, damping, max_step, mode,
                _dp(kp[0]) if kp else None, _dp(kp[1]) if kp else None, _dp(kp[2]) if kp else None,
                kp[3] if kp else 0.0, k, min_dist)
        if rp is None:
            nat.check(nat.lib().optik_hip_ik_region(*head, C.byref(o), _stream_ptr()))
            return res
        res["repaired"] = torch.empty(T, dtype=torch.int32, device=dev)
        rs = nat.RegionRepair(rp[0], rp[1], rp[2], rp[4], rp[3], res["repaired"].data_ptr())
        nat.check(nat.lib().optik_hip_ik_region_repair(*head, C.byref(rs), C.byref(o), _stream_ptr()))
        return res

    def _region_goals(self, regions, starts, restart_begin, restart_end, K, min_dist, region_args):
        K = nat.check_roadmap_goals(K)
        self._check_q(starts)
        sol = self.ik_region(regions, starts.t().contiguous(), restart_begin, restart_end, K, min_dist, **region_args)
        return sol["x"].permute(1, 2, 0).contiguous(), sol["count"]

    def rrt_plan_region(self, regions, starts, restart_begin, restart_end, K, min_dist, iters, step, resolution,
                        first=0, max_nodes=nat.RRT_NODES, Lmax=64, poll=nat.RRT_POLL, ee_offset7=None,
                        region_args=None):
        """rrt_plan_poses with pose regions [Q, 19] in the place of the poses: ik_region with x0 = the starts and up
        to K <= 16 rows per region (region_args: a dict of its tol, iters, damping, max_step, mode, keep), then
        rrt_plan_goals
        -- back to back on the current stream, no host synchronisation between the two stages.  Returns
        rrt_plan_goals' dict plus goals [K, n, Q] and count [Q] int32."""
        goals, count = self._region_goals(regions, starts, restart_begin, restart_end, K, min_dist,
                                          dict(region_args or {}, ee_offset7=ee_offset7))
        res = self.rrt_plan_goals(starts, goals, count, iters, step, resolution, first=first, max_nodes=max_nodes,
                                  Lmax=Lmax, poll=poll, ee_offset7=ee_offset7)
        res["goals"], res["count"] = goals, count
        return res

    def roadmap_plan_region(self, roadmap, regions, starts, restart_begin, restart_end, K, min_dist, ks, Lmax,
                            resolution, ee_offset7=None, region_args=None):
        """roadmap_plan_poses with pose regions [Q, 19] in the place of the poses: ik_region with x0 = the starts
        (region_args: a dict of its own arguments), then roadmap_plan_goals, back to back on the current stream.
        Returns roadmap_plan_goals' dict plus goals [K, n, Q] and count [Q] int32."""
        goals, count = self._region_goals(regions, starts, restart_begin, restart_end, K, min_dist,
                                          dict(region_args or {}, ee_offset7=ee_offset7))
        res = self.roadmap_plan_goals(roadmap, starts, goals, count, ks, Lmax, resolution, ee_offset7=ee_offset7)
        res["goals"], res["count"] = goals, count
        return res

    def rrt_plan_region_constrained(self, regions, starts, c, tol, restart_begin, restart_end, K, min_dist, iters,
                                    step, resolution, first=0, max_nodes=nat.RRT_NODES, Lmax=64, poll=nat.RRT_POLL,
                                    ee_offset7=None, region_args=None, **constrained_args):
        """rrt_plan_region under the path constraint c at tol: ik_region with keep = (c, tol), so every goal
        satisfies the path constraint, then rrt_plan_constrained (**constrained_args: its ptol, piters, damping,
        max_step; region_args: a dict of ik_region's own).  Returns rrt_plan_constrained's dict plus goals [K, n, Q]
        and count [Q] int32."""
        goals, count = self._region_goals(regions, starts, restart_begin, restart_end, K, min_dist,
                                          dict(region_args or {}, keep=(c, tol), ee_offset7=ee_offset7))
        res = self.rrt_plan_constrained(starts, goals, count, c, tol, iters, step, resolution, first=first,
                                        max_nodes=max_nodes, Lmax=Lmax, poll=poll, ee_offset7=ee_offset7,
                                        **constrained_args)
        res["goals"], res["count"] = goals, count
        return res

    def ik_path(self, cfg, targets, x0, restart_begin, restart_end, max_step=float("inf"), flags=0, deadline_s=0.0,
                ee_offset7=None, bufs=None):
        """Warm-started IK along P paths of L waypoints (optik_hip_ik_path): waypoint l of path p is solved from the
        path's current seed (x0[p], then the last accepted solution), its accepted solution being the (key, index)
        minimum of the successes within max_step (L-infinity) of that seed.  targets [L, P, 7] (waypoint-major),
        x0 [P, n] float64 cuda tensors; restart_end - restart_begin <= 4096.  Stream-ordered on the current stream;
        returns a dict of device tensors: x [L, P, n], f [L, P], idx [L, P] int64 (-1 = none), key [L, P] (+inf =
        none), step [L, P] (NaN = none), last [P, n] (each path's final seed)."""
        max_step = nat.check_max_step(max_step)
        if not (targets.is_cuda and targets.dtype == torch.float64 and targets.is_contiguous()
                and targets.dim() == 3 and targets.shape[2] == 7 and targets.shape[0] >= 1 and targets.shape[1] >= 1):
            raise ValueError("targets must be a contiguous float64 cuda tensor [L, P, 7]")
        L, P = int(targets.shape[0]), int(targets.shape[1])
        if not (x0.is_cuda and x0.dtype == torch.float64 and x0.is_contiguous() and tuple(x0.shape) == (P, self.n)):
            raise ValueError(f"x0 must be a contiguous float64 cuda tensor [P, n] = [{P}, {self.n}]")
        b, e = int(restart_begin), int(restart_end)
        if b < 0 or e <= b:
            raise ValueError("empty restart range")
        if e - b > nat.PATH_MAX_RESTARTS:
            raise ValueError(f"ik_path runs at most {nat.PATH_MAX_RESTARTS} restarts per waypoint, got {e - b}")
        if int(flags) & ~nat.IK_RESTART_MAJOR:
            raise ValueError("ik_path: flags may only hold IK_RESTART_MAJOR")
        if bufs is None:
            dev = targets.device
            bufs = dict(x=torch.empty((L, P, self.n), dtype=torch.float64, device=dev),
                        f=torch.empty((L, P), dtype=torch.float64, device=dev),
                        idx=torch.empty((L, P), dtype=torch.int64, device=dev),
                        key=torch.empty((L, P), dtype=torch.float64, device=dev),
                        step=torch.empty((L, P), dtype=torch.float64, device=dev),
                        last=torch.empty((P, self.n), dtype=torch.float64, device=dev))
        o = nat.IkPathOutputs()
        o.d_x, o.d_f, o.d_idx = _ptr(bufs.get("x")), _ptr(bufs.get("f")), _ptr(bufs.get("idx"))
        o.d_key, o.d_step, o.d_last = _ptr(bufs.get("key")), _ptr(bufs.get("step")), _ptr(bufs.get("last"))
        ee = np.ascontiguousarray(ee_offset7, dtype=np.float64) if ee_offset7 is not None else None
        nat.check(nat.lib().optik_hip_ik_path(
            self._h, C.byref(cfg), _ptr(targets), _ptr(x0), P, L, _dpn(ee), b, e,
            int(flags), float(deadline_s), max_step, C.byref(o), _stream_ptr()))
        return bufs

    def ik_host(self, cfg, targets, x0, restart_begin, restart_end, flags=0, deadline_s=0.0, ee_offset7=None):
        """optik_hip_ik_host: host arrays in (targets [T, 7], x0 [T, n]), the winners back as numpy arrays; blocking.
        With IK_EARLY_EXIT | IK_FIND_ANY and one target the call returns when the first restart has succeeded."""
        targets = np.ascontiguousarray(targets, dtype=np.float64)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        T = targets.shape[0]
        assert targets.shape == (T, 7) and x0.shape == (T, self.n)
        win_x = np.zeros((T, self.n)); win_f = np.zeros(T); win_key = np.zeros(T)
        win_idx = np.zeros(T, dtype=np.uint64)
        ee = np.ascontiguousarray(ee_offset7, dtype=np.float64) if ee_offset7 is not None else None
        nat.check(nat.lib().optik_hip_ik_host(
            self._h, C.byref(cfg), _dp(targets), _dp(x0), T, _dpn(ee),
            int(restart_begin), int(restart_end), int(flags), float(deadline_s), _dp(win_x), _dp(win_f),
            win_idx.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(win_key)))
        return dict(win_x=win_x, win_f=win_f, win_idx=win_idx.astype(np.int64), win_key=win_key)

    def set_timing(self, enabled=True):
        nat.lib().optik_hip_set_timing(self._h, 1 if enabled else 0)

    def timing_mean(self):
        """(mean solve-kernel ms, launches) since set_timing(True); HIP events on the launch stream."""
        ms, cnt = C.c_double(0.0), C.c_int32(0)
        nat.check(nat.lib().optik_hip_timing_mean(self._h, C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    def last_launch(self):
        info = nat.LaunchInfo()
        nat.check(nat.lib().optik_hip_last_launch(self._h, C.byref(info)))
        return dict(grid=info.grid, block=info.block, lds_bytes=info.lds_bytes, tiles=info.tiles,
                    kernel_ms=info.kernel_ms)


def probe(op, a, b=None):
    """Elementary device functions (test hook).  numpy in, numpy out."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b if b is not None else a, dtype=np.float64)
    out = np.empty_like(a)
    nat.check(nat.lib().optik_hip_probe(int(op), _dp(a), _dp(b), a.size, _dp(out)))
    return out


_MATH_STRIDE = {0: 3, 1: 9, 2: 6, 3: 36}


def probe_math(op, poses7):
    """math.rs functions on the device (test hook): poses7 [count, 7] = t[3], quat[i,j,k,w].
    op 0 so3::log -> [count, 3]; 1 so3::right_jacobian(so3::log(q)) -> [count, 3, 3]; 2 se3::log ->
    [count, 6]; 3 se3::right_jacobian -> [count, 6, 6] (row-major matrices)."""
    p = np.ascontiguousarray(poses7, dtype=np.float64).reshape(-1, 7)
    out = np.empty((p.shape[0], _MATH_STRIDE[int(op)]), dtype=np.float64)
    nat.check(nat.lib().optik_hip_probe_math(int(op), _dp(p), p.shape[0], _dp(out)))
    if op == 1:
        return out.reshape(-1, 3, 3)
    if op == 3:
        return out.reshape(-1, 6, 6)
    return out
