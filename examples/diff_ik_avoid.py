"""A servo loop that stops in front of a wall instead of crossing it (Robot.diff_ik_avoid).

    python examples/diff_ik_avoid.py robot.urdf base_link ee_link [steps]

The arm starts at the middle of its joint ranges with a sphere model along its links; a wall (a box) stands 10 cm in
front of the end effector along +x, and the loop asks for 0.5 m/s straight into it.  diff_ik would cross the wall;
diff_ik_avoid slows down inside the influence distance and stops at the safety distance."""
import sys

import numpy as np

from optik_amd import Robot
from optik_amd.collision import spheres_along_chain


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    robot = Robot.from_urdf_file(*sys.argv[1:4])
    steps = int(sys.argv[4]) if len(sys.argv) > 4 else 100
    n = robot.num_positions()
    lb, ub = (np.array(v) for v in robot.joint_limits())
    x = 0.5 * (np.maximum(lb, -np.pi) + np.minimum(ub, np.pi))
    frames, centers, radii = spheres_along_chain(robot, 0.04, 2)
    # one more sphere on the end effector itself
    frames = np.concatenate([frames, [n + 1]]).astype(np.int32)
    centers = np.concatenate([centers, np.zeros((1, 3))])
    radii = np.concatenate([radii, [0.04]])
    robot.set_collision_model(frames, centers, radii, self_pairs=None)
    tip = np.array(robot.fk(x.tolist()))[:3, 3]
    wall_x = tip[0] + 0.04 + 0.10
    robot.set_world(boxes=[[wall_x + 0.05, tip[1], tip[2], 0.0, 0.0, 0.0, 1.0, 0.05, 2.0, 2.0]])
    V = [0.5, 0.0, 0.0, 0.0, 0.0, 0.0]
    v_max = np.ones(n)
    influence, safety, dt = 0.08, 0.02, 0.01
    plain = x.copy()
    for _ in range(steps):
        out = robot.diff_ik_avoid(x, V, v_max, influence, safety)
        if out is not None:
            x = x + dt * np.array(out[1])
        ref = robot.diff_ik(plain, V, v_max)
        if ref is not None:
            plain = plain + dt * np.array(ref[1])
    clr = robot.collision_clearance_batch_arrays(np.array([x, plain]))[0]
    print(f"clearance after {steps} steps: {clr[0]:.4f} m with diff_ik_avoid (safety {safety} m), "
          f"{clr[1]:.4f} m with diff_ik")


if __name__ == "__main__":
    main()
