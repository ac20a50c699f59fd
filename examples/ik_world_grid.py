#!/usr/bin/env python3
"""IK in a distance-field world: a small world of boxes is baked into a voxel grid on the GPU, the boxes are taken
away and the grid alone is installed, as a perceived scene (an ESDF from a depth camera, say) would be; then one target
is solved and the clearances under the grid and under the boxes it came from are printed side by side:

    python examples/ik_world_grid.py <robot.urdf> <base_link> <ee_link> [restarts]"""
import math
import sys

import numpy as np

from optik_amd import Robot, SolverConfig
from optik_amd.collision import spheres_along_chain


def main():
    if len(sys.argv) < 4:
        print(__doc__)
        return 2
    urdf, base, ee = sys.argv[1:4]
    restarts = int(sys.argv[4]) if len(sys.argv) > 4 else 2048
    robot = Robot.from_urdf_file(urdf, base, ee)
    n = robot.num_positions()
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(0)
    target = robot.fk(rng.uniform(lb, ub))
    x0 = rng.uniform(lb, ub)
    cfg = SolverConfig("quality", max_time=0.0, max_restarts=restarts)
    frames, centers, radii = spheres_along_chain(robot, 0.04, 6)
    voxel = 0.05
    # the interpolated field is within sqrt(3) * voxel of the true distance: that goes into the margin.  (No self
    # pairs here: the margin applies to them too, and spheres of neighbouring links sit closer than 9 cm.)
    margin = math.sqrt(3.0) * voxel
    robot.set_collision_model(frames, centers, radii, self_pairs=None, margin=margin)

    first = robot.ik(cfg, target, x0)
    if first is None:
        print("no solution without obstacles")
        return 1
    # a box on the middle link of that answer and a wall beside the base
    mid = robot.link_frames_batch_arrays(np.array([first[0]]))[0, (n + 1) // 2]
    unit = [0.0, 0.0, 0.0, 1.0]
    boxes = np.array([np.concatenate([mid[:3, 3], unit, [0.06, 0.06, 0.06]]),
                      np.concatenate([[0.0, 0.9, 0.5], unit, [1.0, 0.02, 0.5]])])
    robot.set_world(boxes=boxes)
    origin, shape = [-1.5, -1.5, -1.5], (61, 61, 61)
    field = robot.bake_world_grid(origin, voxel, shape)
    print(f"baked {len(boxes)} boxes into {field.shape} float32 nodes, values {field.min():.3f} .. {field.max():.3f}")

    robot.set_world()                       # the primitives go ...
    robot.set_world_grid(origin, voxel, field)  # ... and the grid alone is the world
    print(f"the first answer under the grid: clearance {robot.collision_clearance(first[0]):.4f} (margin {margin:.4f})")
    sols = robot.ik_solutions(cfg, target, x0, k=8, min_dist=0.1)
    xs = np.array([s[0] for s in sols]).reshape(-1, n)
    clr_grid, ok = robot.collision_clearance_batch_arrays(xs)
    robot.clear_world_grid()
    robot.set_world(boxes=boxes)
    clr_box, _ = robot.collision_clearance_batch_arrays(xs)
    for k in range(len(xs)):
        print(f"  solution {k}: clearance under the grid {clr_grid[k]:.4f}, under the boxes {clr_box[k]:.4f}")
    worst = float(np.abs(clr_grid - clr_box).max()) if len(xs) else 0.0
    print(f"ik_solutions in the grid world: {len(xs)} solutions, all free: {bool(ok.all())}, "
          f"grid vs boxes differ by at most {worst:.4f} (bound {margin:.4f})")
    robot.clear_collision_model()
    return 0


if __name__ == "__main__":
    sys.exit(main())
