#!/usr/bin/env python3
"""IK against a world seen by depth cameras: a synthetic box and the arm itself are rendered to depth images in numpy
from two camera poses and integrated over a few frames into a persistent evidence map on the GPU
(Robot.set_world_depth), self-filtered with the robot's own spheres.  A target on the box's top face is refused while
the box stands there; a free target is solved.  Then the box is taken out of the images: the cameras now see through
where it was, the map carves it away frame by frame, and the same target becomes reachable:

    python examples/ik_world_depth.py <robot.urdf> <base_link> <ee_link> [restarts]"""
import math
import sys

import numpy as np

from optik_amd import Robot, SolverConfig
from optik_amd.collision import spheres_along_chain, spheres_at

H, W = 120, 160
INTRINSICS = np.array([140.0, 140.0, 79.5, 59.5])  # fx, fy, cx, cy
FAR = 10.0  # what a ray that hits nothing returns: beyond z_far, so it carves and marks nothing


def look_at(eye, target):
    """The camera at `eye` looking at `target` as a 4x4: x right, y down, z forward."""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T


def render(T, boxes, spheres):
    """The z-depth image of axis-aligned boxes [(lo, hi)] and spheres [S, 4] from the camera T: one ray per pixel,
    p = eye + s * R (x, y, 1), so the parameter s of the nearest hit is the z-depth itself."""
    fx, fy, cx, cy = INTRINSICS
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones((H, W))], axis=-1) @ T[:3, :3].T
    eye = T[:3, 3]
    depth = np.full((H, W), FAR)
    with np.errstate(divide="ignore", invalid="ignore"):
        for lo, hi in boxes:
            t0, t1 = (np.asarray(lo) - eye) / d, (np.asarray(hi) - eye) / d
            near, far = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
            hit = (near <= far) & (near > 0.0)
            depth = np.where(hit & (near < depth), near, depth)
        for s in spheres:
            oc = eye - s[:3]
            a, b, c = (d * d).sum(-1), (d * oc).sum(-1), oc @ oc - s[3] * s[3]
            disc = b * b - a * c
            near = (-b - np.sqrt(np.maximum(disc, 0.0))) / a
            hit = (disc >= 0.0) & (near > 0.0)
            depth = np.where(hit & (near < depth), near, depth)
    return depth.astype(np.float32)


def main():
    if len(sys.argv) < 4:
        print(__doc__)
        return 2
    urdf, base, ee = sys.argv[1:4]
    restarts = int(sys.argv[4]) if len(sys.argv) > 4 else 512
    robot = Robot.from_urdf_file(urdf, base, ee)
    n = robot.num_positions()
    lb, ub = (np.array(v) for v in robot.joint_limits())
    voxel = 0.04
    # the model: spheres along the links and one on the end effector; the field's two error bounds go into the margin
    # (examples/ik_world_points.py)
    frames, centers, radii = spheres_along_chain(robot, 0.05, 6)
    frames = np.concatenate([frames, [n + 1]]).astype(np.int32)
    centers, radii = np.concatenate([centers, [[0.0, 0.0, 0.0]]]), np.concatenate([radii, [0.04]])
    margin = (math.sqrt(3.0) + (math.sqrt(3.0) - 1.0) / 2.0) * voxel
    robot.set_collision_model(frames, centers, radii, self_pairs=None, margin=margin)

    # the arm stands at x_now; the box's top face is centred on the end effector's position at x_goal
    x_now = 0.5 * (lb + ub)
    x_goal = x_now.copy()
    x_goal[0] = x_now[0] + 0.9
    target = np.array(robot.fk(x_goal))
    p = target[:3, 3]
    box = (p - [0.10, 0.10, 0.30], p + [0.10, 0.10, 0.0])
    origin = np.floor((p - [0.8, 0.8, 0.9]) / voxel) * voxel
    shape = (41, 41, 36)
    out = p + 1.2 * np.array([p[0], p[1], 0.0]) / max(np.hypot(p[0], p[1]), 1e-9)  # beyond the box, seen from the base
    side = np.array([-p[1], p[0], 0.0]) / max(np.hypot(p[0], p[1]), 1e-9)
    poses = np.stack([look_at(out + 0.8 * side + [0.0, 0.0, 0.7], p - [0.0, 0.0, 0.1]),
                      look_at(out - 0.8 * side + [0.0, 0.0, 0.7], p - [0.0, 0.0, 0.1])])
    own = spheres_at(robot, x_now, frames, centers, radii)
    exclude = spheres_at(robot, x_now, frames, centers, radii, pad=0.03)
    cfg = SolverConfig("quality", max_time=0.0, max_restarts=restarts)

    def integrate(map, boxes, rounds):
        for _ in range(rounds):
            depth = np.stack([render(T, boxes, own) for T in poses])
            map, values = robot.set_world_depth(map, origin, voxel, depth, INTRINSICS, poses, exclude)
        return map, values

    map, values = integrate(Robot.new_depth_map(shape), [box], 3)
    occ = robot.occupancy_from_map(map)
    unfiltered = robot.occupancy_from_map(robot.depth_integrate(
        Robot.new_depth_map(shape), origin, voxel, np.stack([render(T, [box], own) for T in poses]), INTRINSICS, poses))
    print(f"3 rounds of 2 images {H} x {W}: {int((map != -32768).sum())} of {map.size} nodes observed, "
          f"{int((map < 0).sum() - (map == -32768).sum())} carved free, {int(occ.sum())} occupied "
          f"({int(unfiltered.sum())} after one round without the self-filter)")
    clr_now = robot.collision_clearance(x_now)
    print(f"the arm where it stands: clearance {clr_now:.3f} (margin {margin:.3f})")

    # a free target: the pose of a configuration that keeps clear of the map
    rng = np.random.default_rng(4)
    cand = rng.uniform(np.maximum(lb, x_now - 0.8), np.minimum(ub, x_now + 0.8), size=(256, n))
    clr, free = robot.collision_clearance_batch_arrays(cand)
    cand = cand[free & (clr > margin + 0.02)]
    if not len(cand):
        print("no free configuration among the candidates")
        return 1
    sol = robot.ik(cfg, np.array(robot.fk(cand[0])), x_now)
    if sol is None:
        print("ik to a free target: no collision-free solution")
        return 1
    c_free = robot.collision_clearance(sol[0])
    print(f"ik to a free target against the map: error {sol[1]:.2e}, clearance {c_free:.3f}")

    blocked = robot.ik(cfg, target, x_now)
    print("ik to the box's top face, with the box: "
          + ("no collision-free solution" if blocked is None else f"clearance {robot.collision_clearance(blocked[0]):.3f}"))

    # the box goes: the same cameras see through where it stood, and every image takes evidence away
    map, values = integrate(map, [], 5)
    left = int(robot.occupancy_from_map(map).sum())
    sol = robot.ik(cfg, target, x_now)
    reachable = sol is not None and robot.collision_clearance(sol[0]) >= margin
    print(f"5 rounds without the box: {left} occupied nodes left")
    print(f"ik to the same target, box removed: reachable: {reachable}"
          + (f" (error {sol[1]:.2e}, clearance {robot.collision_clearance(sol[0]):.3f})" if sol is not None else ""))
    robot.clear_world_grid()
    robot.clear_collision_model()
    return 0 if (blocked is None and reachable and c_free >= margin and clr_now >= margin) else 1


if __name__ == "__main__":
    sys.exit(main())
