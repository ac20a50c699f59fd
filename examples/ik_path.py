#!/usr/bin/env python3
"""A straight Cartesian move along warm-started waypoints (Robot.ik_path): the end effector goes from the pose at one
configuration to the pose at another, its position on a straight line and its orientation by slerp.  Each waypoint is
solved from the previous waypoint's solution, so that the joints move continuously; with a finite max_step a
solution that jumps by more than that in some joint (another elbow or wrist branch) is not accepted:

    python examples/ik_path.py <robot.urdf> <base_link> <ee_link> [waypoints] [max_step] [restarts]"""
import sys

import numpy as np

from optik_amd import Robot, SolverConfig


def _log_so3(R):
    """Rotation matrix -> rotation vector (angle below pi)."""
    c = np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)
    a = np.arccos(c)
    if a < 1e-12:
        return np.zeros(3)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return w * (a / (2.0 * np.sin(a)))


def _exp_so3(v):
    a = np.linalg.norm(v)
    if a < 1e-12:
        return np.eye(3)
    k = v / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def straight_line(Ta, Tb, L):
    """L poses from Ta to Tb: linear translation, slerp of the rotation (orthonormalised)."""
    w = _log_so3(Ta[:3, :3].T @ Tb[:3, :3])
    out = []
    for s in np.linspace(0.0, 1.0, L):
        T = np.eye(4)
        u, _, vt = np.linalg.svd(Ta[:3, :3] @ _exp_so3(s * w))
        T[:3, :3] = u @ vt
        T[:3, 3] = (1.0 - s) * Ta[:3, 3] + s * Tb[:3, 3]
        out.append(T)
    return np.array(out)


def main():
    urdf, base, ee = sys.argv[1:4]
    L = int(sys.argv[4]) if len(sys.argv) > 4 else 100
    max_step = float(sys.argv[5]) if len(sys.argv) > 5 else 0.05
    restarts = int(sys.argv[6]) if len(sys.argv) > 6 else 64
    robot = Robot.from_urdf_file(urdf, base, ee)
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(7)
    qa = rng.uniform(lb + 0.25 * (ub - lb), ub - 0.25 * (ub - lb))
    qb = np.clip(qa + rng.uniform(-0.4, 0.4, size=qa.shape), lb, ub)
    targets = straight_line(np.array(robot.fk(qa)), np.array(robot.fk(qb)), L)
    config = SolverConfig("speed", max_time=0.0, max_restarts=restarts)
    for ms in (float("inf"), max_step):
        x, c, idx, step, found = robot.ik_paths_arrays(config, targets[None], qa[None], max_step=ms)
        solved = int(found.sum())
        largest = float(np.nanmax(step)) if solved else float("nan")
        warm = int((idx[0][found[0]] == 0).sum())
        print(f"max_step = {ms}: {solved} of {L} waypoints solved ({warm} from the warm start alone), "
              f"largest joint step {largest:.4f} rad")


if __name__ == "__main__":
    main()
