#!/usr/bin/env python3
"""A straight tool move timed for a collaborative cell: the waypoints of ik_path.py's straight Cartesian line, timed
once under the joint limits alone (time_paths) and once with the tool centre point capped at 0.25 m/s, the reduced
speed of a collaborative cell (time_paths_tool):

    python examples/time_path_tool.py <robot.urdf> <base_link> <ee_link> [waypoints]

Both timings are rest to rest within the URDF's velocity limits and A_MAX rad/s^2.  The cap holds at the waypoints; the
trajectory between them is the controller's interpolation, so the line is sampled densely (48 waypoints)."""
import sys

import numpy as np

from optik_amd import Robot, SolverConfig

from ik_path import straight_line

A_MAX = 7.5        # rad/s^2; a URDF carries no acceleration limits
TOOL_V_MAX = 0.25  # m/s
DT = 0.001         # s


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    robot = Robot.from_urdf_file(*sys.argv[1:4])
    L = int(sys.argv[4]) if len(sys.argv) > 4 else 48
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(7)
    qa = rng.uniform(lb + 0.25 * (ub - lb), ub - 0.25 * (ub - lb))
    qb = np.clip(qa + rng.uniform(-0.4, 0.4, size=qa.shape), lb, ub)
    Ta, Tb = np.array(robot.fk(qa)), np.array(robot.fk(qb))
    targets = straight_line(Ta, Tb, L)
    config = SolverConfig("speed", max_time=0.0, max_restarts=64)
    x, _, _, _, found = robot.ik_paths_arrays(config, targets[None], qa[None], max_step=0.1)
    if not found.all():
        print(f"ik_path: {int(found.sum())} of {L} waypoints solved")
        return 1
    print(f"straight move: {np.linalg.norm(Tb[:3, 3] - Ta[:3, 3]):.4f} m in {L} waypoints")

    free = robot.time_paths_tool(x, a_max=A_MAX)
    capped = robot.time_paths_tool(x, a_max=A_MAX, tool_v_max=TOOL_V_MAX)
    if free["status"][0] != 0 or capped["status"][0] != 0:
        print(f"timed: status {free['status'][0]} and {capped['status'][0]}")
        return 1
    print(f"joint limits alone: duration {free['duration'][0]:.4f} s, peak tool speed "
          f"{free['tool_speed'][0].max():.12f} m/s")
    print(f"tool capped at {TOOL_V_MAX} m/s: duration {capped['duration'][0]:.4f} s, peak tool speed "
          f"{capped['tool_speed'][0].max():.12f} m/s")
    q, _ = robot.sample_trajectories(x, capped, DT)
    print(f"samples: {q.shape[1]} at {1.0 / DT:.0f} Hz, "
          f"ends {'at' if np.array_equal(q[0, -1], x[0, -1]) else 'off'} the goal")
    return 0


if __name__ == "__main__":
    sys.exit(main())
