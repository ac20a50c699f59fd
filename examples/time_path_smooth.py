#!/usr/bin/env python3
"""A timed path made fit for a controller that checks jerk: the straight tool move of ik_path.py, timed by time_paths
(limits at the waypoints only, acceleration jumping at each of them) and then retimed by smooth_timing into the C2
cubic spline through the same waypoints, slowed uniformly until velocity, acceleration and jerk limits hold along the
whole curve:

    python examples/time_path_smooth.py <robot.urdf> <base_link> <ee_link> [waypoints]

Both trajectories are sampled at 1 kHz by sample_trajectories, which needs no change: a C2 cubic spline is the cubic
Hermite curve of its own knot velocities.  The peaks printed for the samples are finite differences of the sampled
velocity, what a controller's own check would see."""
import sys

import numpy as np

from optik_amd import Robot, SolverConfig

from ik_path import straight_line

A_MAX = 7.5     # rad/s^2; a URDF carries no acceleration limits
J_MAX = 500.0   # rad/s^3; nor jerk limits (a Panda's are 3750 .. 10 000)
DT = 0.001      # s


def peaks(v):
    """The largest |acceleration| and |jerk| over the joints by differences of the sampled velocity v [T, n], without
    the last sample: it lies past the end, where the motion stops with an acceleration step."""
    acc = np.diff(v[:-1], axis=0) / DT
    return np.abs(acc).max(), np.abs(np.diff(acc, axis=0) / DT).max()


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    robot = Robot.from_urdf_file(*sys.argv[1:4])
    L = int(sys.argv[4]) if len(sys.argv) > 4 else 48
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(7)
    qa = rng.uniform(lb + 0.25 * (ub - lb), ub - 0.25 * (ub - lb))
    qb = np.clip(qa + rng.uniform(-0.4, 0.4, size=qa.shape), lb, ub)
    targets = straight_line(np.array(robot.fk(qa)), np.array(robot.fk(qb)), L)
    config = SolverConfig("speed", max_time=0.0, max_restarts=64)
    x, _, _, _, found = robot.ik_paths_arrays(config, targets[None], qa[None], max_step=0.1)
    if not found.all():
        print(f"ik_path: {int(found.sum())} of {L} waypoints solved")
        return 1

    timed = robot.time_paths(x, a_max=A_MAX)
    if timed["status"][0] != 0:
        print(f"timed: status {timed['status'][0]}")
        return 1
    smooth = robot.smooth_timing(x, timed, j_max=J_MAX, a_max=A_MAX)
    if smooth["status"][0] != 0:
        print(f"smoothed: status {smooth['status'][0]}")
        return 1
    rv, ra, rj = smooth["ratios"][0]
    print(f"time_paths: duration {timed['duration'][0]:.4f} s")
    print(f"smooth_timing: duration {smooth['duration'][0]:.4f} s, factor {smooth['factor'][0]:.6f}, peak / limit "
          f"along the curve: velocity {rv:.12f}, acceleration {ra:.12f}, jerk {rj:.12f}")
    for name, timing in (("time_paths", timed), ("smooth_timing", smooth)):
        q, v = robot.sample_trajectories(x, timing, DT)
        acc, jerk = peaks(v[0])
        print(f"{name} sampled: {q.shape[1]} samples at {1.0 / DT:.0f} Hz, peak |acceleration| {acc:.4f} rad/s^2, "
              f"peak |jerk| {jerk:.1f} rad/s^3, ends {'at' if np.array_equal(q[0, -1], x[0, -1]) else 'off'} the goal")
    return 0


if __name__ == "__main__":
    sys.exit(main())
