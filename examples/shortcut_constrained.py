"""Carry the glass upright past the wall, then shorten and respace the path with the glass still upright
(Robot.shortcut_paths_constrained, Robot.resample_paths_constrained).

    python examples/shortcut_constrained.py panda.urdf panda_link0 panda_link8

The scene and the plan are examples/plan_rrt_constrained.py's: the Panda, a wall of 2 cm, the end effector's z axis
kept within TILT radians of where it points at the start, and plan_rrt_constrained's path round the wall -- a chain of
0.5 rad steps with a corner at every waypoint.  Without a constraint the pipeline goes on plan -> shortcut -> resample
-> time; with one it used to stop after its first link.  Here:
  - shortcut_paths_constrained subdivides the path, projects every new vertex onto the constraint and joins two
    vertices only where the motion between them passes the collision check AND the constraint's check at TOL.  By
    construction its output has status 0 (the input's own segments are such motions), passes check_paths_constraint
    at the same TOL and resolution, and is not blocked for certify_paths: the example fails on anything else.
  - The costs before and after are printed and not judged: projected vertices leave the input's polyline, so the
    shortcut can be longer than its input in the L-infinity metric.
  - resample_paths_constrained spaces WAYPOINTS waypoints evenly along the shortcut and projects the ones between the
    ends.  Its new segments cut corners and are not free or on the constraint by construction: whether they pass both
    checks is printed.
  - time_paths at the URDF's velocity limits, where the tree's own path stalls (status 1): its status and duration on
    the resampled path are printed, not judged (DESIGN.md section 5.31 records them).
Other 7-joint arms run, but the scene is the Panda's."""
import sys

import numpy as np

from optik_amd import Robot

from plan_rrt_constrained import PLAN, RESOLUTION, START, TOL, setup

WAYPOINTS = 32
A_MAX = 5.0  # rad / s^2 on every joint, as examples/plan_rrt_constrained.py


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    robot = Robot.from_urdf_file(*sys.argv[1:4])
    if robot.num_positions() != len(START):
        sys.exit("the scene of this example is a 7-joint arm's (the Panda's)")
    start, goal, c = setup(robot)
    n = len(start)
    v_max = np.asarray(robot.velocity_limits(), dtype=np.float64)
    a_max = np.full(n, A_MAX)

    def timed(paths, lens):
        t = robot.time_paths(paths, lens, a_max=a_max, v_max=v_max)
        return int(t["status"][0]), float(t["duration"][0])

    tree = robot.plan_rrt_constrained(start[None], goal[None], c, tol=TOL, **PLAN)
    bad = int(tree["status"][0]) != 0
    print(f"plan_rrt_constrained: status {int(tree['status'][0])}, {int(tree['len'][0])} waypoints, length "
          f"{tree['cost'][0]:.3f} rad")
    if not bad:
        st, dur = timed(tree["paths"], tree["len"])
        print(f"  timed at the URDF's velocity limits: status {st}, {dur:.3f} s")
        short = robot.shortcut_paths_constrained(tree["paths"], tree["len"], c, tol=TOL, resolution=RESOLUTION)
        chk = robot.check_paths_constraint(short["paths"], short["len"], c, TOL, RESOLUTION)
        cert = robot.certify_paths(short["paths"], short["len"])
        verdict = {0: "free", 1: "blocked"}.get(int(cert["status"][0]), "undecided")
        print(f"shortcut_paths_constrained: status {int(short['status'][0])}, {int(short['len'][0])} waypoints, length "
              f"{short['cost'][0]:.3f} rad (input {short['cost_in'][0]:.3f} rad); {int(short['projected'][0, 0])} "
              f"projections, {int(short['projected'][0, 1])} ended on the constraint")
        print(f"  constraint {'kept' if chk['ok'][0] else 'broken'} (violation {chk['violation'][0]:.3f}); certified "
              f"{verdict}")
        bad = int(short["status"][0]) != 0 or not chk["ok"][0] or int(cert["status"][0]) == 1
        dense, st, projected, free, ok = robot.resample_paths_constrained(short["paths"], short["len"], c, WAYPOINTS,
                                                                          resolution=RESOLUTION, tol=TOL)
        print(f"resample_paths_constrained: status {int(st[0])}, {WAYPOINTS} waypoints, {int(projected[0, 1])} of "
              f"{int(projected[0, 0])} projected; new segments free: {bool(free[0])}, on the constraint: {bool(ok[0])}")
        st, dur = timed(dense, None)
        print(f"  timed at the URDF's velocity limits: status {st}, {dur:.3f} s")
    robot.clear_collision_model()
    robot.set_world()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
