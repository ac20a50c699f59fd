#!/usr/bin/env python3
"""IK against a point cloud: a synthetic depth-camera cloud of a table and a post, which also sees the arm itself, is
filtered of the arm's own points (the self-filter: the robot's spheres at its current configuration, padded),
voxelized and turned into a signed distance field on the GPU (Robot.set_world_points); then a target is solved with ik
and a short path with ik_path against that field:

    python examples/ik_world_points.py <robot.urdf> <base_link> <ee_link> [restarts]"""
import math
import sys

import numpy as np

from optik_amd import Robot, SolverConfig
from optik_amd.collision import spheres_along_chain, spheres_at


def surface_points(lo, hi, step, rng, noise):
    """Points on the six faces of the box [lo, hi], `step` apart, with sensor noise."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    pts = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        gb, gc = np.meshgrid(np.arange(lo[b], hi[b] + step / 2, step), np.arange(lo[c], hi[c] + step / 2, step))
        for v in (lo[a], hi[a]):
            face = np.zeros((gb.size, 3))
            face[:, a], face[:, b], face[:, c] = v, gb.ravel(), gc.ravel()
            pts.append(face)
    pts = np.concatenate(pts)
    return pts + rng.normal(scale=noise, size=pts.shape)


def main():
    if len(sys.argv) < 4:
        print(__doc__)
        return 2
    urdf, base, ee = sys.argv[1:4]
    restarts = int(sys.argv[4]) if len(sys.argv) > 4 else 1024
    robot = Robot.from_urdf_file(urdf, base, ee)
    n = robot.num_positions()
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(2)
    frames, centers, radii = spheres_along_chain(robot, 0.05, 8)
    voxel = 0.04
    # the field is optimistic by up to (sqrt(3) - 1) / 2 voxels (a voxel is taken for its node) and its interpolation
    # is off by up to sqrt(3) voxels: both go into the margin.  (No self pairs: the margin would apply to them too.)
    margin = (math.sqrt(3.0) + (math.sqrt(3.0) - 1.0) / 2.0) * voxel
    robot.set_collision_model(frames, centers, radii, self_pairs=None, margin=margin)

    # the scene as the camera returns it: a table, a post on it, the arm where it stands now, a few invalid returns
    x_now = 0.5 * (lb + ub)
    table = surface_points([0.35, -0.45, 0.16], [0.85, 0.45, 0.20], voxel / 2, rng, 0.002)
    post = surface_points([0.55, 0.20, 0.20], [0.61, 0.26, 0.60], voxel / 2, rng, 0.002)
    own = spheres_at(robot, x_now, frames, centers, radii)
    d = rng.normal(size=(len(own), 60, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    arm = (own[:, None, :3] + own[:, None, 3:] * d).reshape(-1, 3) + rng.normal(scale=0.002, size=(len(own) * 60, 3))
    cloud = np.concatenate([table, post, arm, np.full((16, 3), np.nan)])
    origin, shape = [-1.0, -1.0, -0.2], (51, 51, 41)

    raw = robot.occupancy_from_points(origin, voxel, shape, cloud)
    exclude = spheres_at(robot, x_now, frames, centers, radii, pad=0.03)
    values = robot.set_world_points(origin, voxel, shape, cloud, exclude)
    print(f"{len(cloud)} points -> {int(raw.sum())} occupied voxels, {int((values < 0).sum())} after the self-filter "
          f"({len(exclude)} spheres); field {values.min():.3f} .. {values.max():.3f} m on {values.shape} nodes")
    clr_now = robot.collision_clearance(x_now)
    print(f"the arm where it stands: clearance {clr_now:.3f} (margin {margin:.3f}); "
          "without the self-filter it would stand inside its own image")

    # targets that are known to be reachable without collision: the poses of free configurations with a free straight
    # joint-space move between them
    cand = rng.uniform(np.maximum(lb, x_now - 1.0), np.minimum(ub, x_now + 1.0), size=(256, n))
    clr, free = robot.collision_clearance_batch_arrays(cand)
    cand = cand[free & (clr > margin + 0.02)]
    pair = None
    for k in range(len(cand) - 1):
        if robot.collision_motion(cand[k], cand[k + 1], 0.02)[1]:
            pair = (cand[k], cand[k + 1])
            break
    if pair is None:
        print("no free move among the candidates")
        return 1
    L = 8
    qs = np.array([(1 - s) * pair[0] + s * pair[1] for s in np.linspace(0.0, 1.0, L)])
    targets = np.array([robot.fk(q) for q in qs])

    cfg = SolverConfig("quality", max_time=0.0, max_restarts=restarts)
    sol = robot.ik(cfg, targets[-1], x_now)
    if sol is None:
        print("ik: no collision-free solution")
        return 1
    c_ik = robot.collision_clearance(sol[0])
    print(f"ik against the cloud: error {sol[1]:.2e}, clearance {c_ik:.3f}")
    path = robot.ik_path(cfg, targets, pair[0])
    got = [r for r in path if r is not None]
    c_path, ok = robot.collision_clearance_batch_arrays(np.array([r[0] for r in got]).reshape(-1, n))
    print(f"ik_path against the cloud: {len(got)} of {L} waypoints, least clearance "
          f"{(c_path.min() if len(got) else float('nan')):.3f}")
    all_free = c_ik >= margin and len(got) > 0 and bool(ok.all())
    print(f"all free: {all_free}")
    robot.clear_world_grid()
    robot.clear_collision_model()
    return 0 if all_free else 1


if __name__ == "__main__":
    sys.exit(main())
