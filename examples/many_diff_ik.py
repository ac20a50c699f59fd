#!/usr/bin/env python3
"""Batched differential IK: B robots (or simulated environments) stepped together through a few control steps,
each asking for the joint velocities that track a fixed Cartesian twist within its speed limits
(Robot.diff_ik_batch_arrays; the batched counterpart of examples/diff_ik.py):

    python examples/many_diff_ik.py <robot.urdf> <base_link> <ee_link> [B] [steps]"""
import sys
import time

import numpy as np

from optik_amd import Robot


def main():
    urdf, base, ee = sys.argv[1:4]
    B = int(sys.argv[4]) if len(sys.argv) > 4 else 65536
    steps = int(sys.argv[5]) if len(sys.argv) > 5 else 5
    robot = Robot.from_urdf_file(urdf, base, ee)
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(1)
    q = rng.uniform(lb, ub, size=(B, len(lb)))
    twist = np.array([0.1, 0.0, 0.05, 0.0, 0.2, 0.0])  # world-frame [v; w] of every end effector
    v_max = np.ones(len(lb))
    dt = 0.01
    robot.diff_ik_batch_arrays(q[:1], twist, v_max)  # first call: device set-up, code objects
    t0 = time.perf_counter()
    for _ in range(steps):
        alpha, v, found = robot.diff_ik_batch_arrays(q, twist, v_max)
        q = np.clip(q + dt * v, lb, ub)
    dt_wall = time.perf_counter() - t0
    print(f"{int(found.sum())} of {B} configurations solved; {steps} steps in {dt_wall * 1e3:.1f} ms: "
          f"{B * steps / dt_wall:.3e} configurations/s; mean alpha {alpha[found].mean():.4f}")


if __name__ == "__main__":
    main()
