#!/usr/bin/env python3
"""One target solved in all four solution modes (Robot.ik over the same restarts): Speed keeps the lowest successful
restart, Quality the success nearest to the seed, Manipulability the one with the largest w = sqrt(det(J J^T)) (the
product of the Jacobian's singular values), Condition the one with the largest c = sigma_min / sigma_max.  Prints each
winner's restart index, w and c (Robot.manipulability):

    python examples/ik_modes.py <robot.urdf> <base_link> <ee_link> [restarts]"""
import sys

import numpy as np

from optik_amd import Robot, SolverConfig


def main():
    if len(sys.argv) < 4:
        print(__doc__)
        return 2
    urdf, base, ee = sys.argv[1:4]
    restarts = int(sys.argv[4]) if len(sys.argv) > 4 else 1024
    robot = Robot.from_urdf_file(urdf, base, ee)
    robot.set_parallelism(1)  # (Speed: the deterministic lowest successful index)
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(0)
    target = robot.fk(rng.uniform(lb, ub))
    x0 = rng.uniform(lb, ub)
    for mode in ("speed", "quality", "manipulability", "condition"):
        cfg = SolverConfig(mode, max_time=0.0, max_restarts=restarts)
        res = robot.ik(cfg, target, x0, return_index=True)
        if res is None:
            print(f"{mode} no solution in {restarts} restarts")
            return 1
        x, f, idx = res
        w, c = robot.manipulability(x)
        dist = float(np.linalg.norm(np.array(x) - x0))
        print(f"{mode} restart {idx}  w {w:.6g}  c {c:.6g}  |x - x0| {dist:.4f}  f {f:.3g}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
