#!/usr/bin/env python3
"""Several distinct IK solutions of one target (Robot.ik_solutions): every restart runs to its end, the successes
are taken nearest-to-the-seed first and kept only if they differ from every solution kept before by more than
min_dist in some joint.  On a redundant arm (the Panda) the successes form a continuum and min_dist sets the spacing
of the returned samples:

    python examples/ik_solutions.py <robot.urdf> <base_link> <ee_link> [k] [min_dist] [restarts]"""
import sys

import numpy as np

from optik_amd import Robot, SolverConfig


def main():
    urdf, base, ee = sys.argv[1:4]
    k = int(sys.argv[4]) if len(sys.argv) > 4 else 8
    min_dist = float(sys.argv[5]) if len(sys.argv) > 5 else 0.1
    restarts = int(sys.argv[6]) if len(sys.argv) > 6 else 1024
    robot = Robot.from_urdf_file(urdf, base, ee)
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(3)
    target = robot.fk(rng.uniform(lb, ub))  # a reachable pose
    x0 = (lb + ub) / 2
    config = SolverConfig("quality", max_time=0.0, max_restarts=restarts)
    sols = robot.ik_solutions(config, target, x0, k=k, min_dist=min_dist, return_index=True)
    print(f"{len(sols)} distinct solutions (k = {k}, min_dist = {min_dist}, {restarts} restarts)")
    for j, (x, c, idx) in enumerate(sols):
        pose = np.array(robot.fk(x))
        err = np.abs(pose - np.array(target)).max()
        print(f"solution {j}: restart {idx}, c = {c:.3e}, |fk(x) - target|_max = {err:.1e}, "
              f"x = [{', '.join(f'{v:+.4f}' for v in x)}]")


if __name__ == "__main__":
    main()
