#!/usr/bin/env python3
"""Collision-free IK: one target solved without and with a box in the way of the first answer, then up to eight
distinct collision-free answers (ik_solutions).  The robot is modelled by spheres along its links
(optik_amd.collision.spheres_along_chain; the bundled URDFs carry no collision geometry), with "auto" self pairs:

    python examples/ik_collision.py <robot.urdf> <base_link> <ee_link> [restarts]"""
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
    robot.set_collision_model(frames, centers, radii, self_pairs="auto", margin=0.0)
    print(f"model: {len(frames)} spheres on frames {sorted(set(frames.tolist()))}")

    free = robot.ik(cfg, target, x0, return_index=True)
    if free is None:
        print("no collision-free solution without obstacles")
        return 1
    x, f, idx = free
    print(f"no obstacles: restart {idx}  clearance {robot.collision_clearance(x):.4f}  f {f:.3g}")

    # a box around the middle link of that answer: the answer is now in collision, another one is returned
    mid = robot.link_frames_batch_arrays(np.array([x]))[0, (n + 1) // 2]
    robot.set_world(boxes=[np.concatenate([mid[:3, 3], [0.0, 0.0, 0.0, 1.0], [0.06, 0.06, 0.06]])])
    print(f"box at {np.round(mid[:3, 3], 3).tolist()}: the first answer's clearance is "
          f"{robot.collision_clearance(x):.4f}")
    res = robot.ik(cfg, target, x0, return_index=True)
    if res is None:
        print("with the box: no collision-free solution")
    else:
        x2, f2, idx2 = res
        print(f"with the box: restart {idx2}  clearance {robot.collision_clearance(x2):.4f}  f {f2:.3g}")

    sols = robot.ik_solutions(cfg, target, x0, k=8, min_dist=0.1)
    clr, ok = robot.collision_clearance_batch_arrays(np.array([s[0] for s in sols]).reshape(-1, n))
    print(f"ik_solutions with the filter: {len(sols)} solutions, all free: {bool(ok.all())}, "
          f"smallest clearance {clr.min() if len(clr) else float('nan'):.4f}")
    robot.clear_collision_model()
    return 0


if __name__ == "__main__":
    sys.exit(main())
