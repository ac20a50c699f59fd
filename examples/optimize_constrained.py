"""Carry the glass upright past the wall, and push the path away from the wall with the glass still upright
(Robot.optimize_paths_constrained): the whole pipeline, plan -> shortcut -> resample -> optimize -> time, every stage
keeping the pose constraint.

    python examples/optimize_constrained.py panda.urdf panda_link0 panda_link8

The scene and the plan are examples/plan_rrt_constrained.py's, the shortcut and the resampling
examples/shortcut_constrained.py's.  The resampled path passes the wall as closely as the shortcut found it free.
optimize_paths_constrained takes ITERS covariant gradient steps on it and, after each, projects every interior
waypoint back onto the constraint; a waypoint that cannot be projected keeps its previous value.  So:
  - every waypoint of the result satisfies the constraint at PTOL where the input's did (violation before and after
    are printed; the example fails if the one after exceeds PTOL while the one before did not);
  - the clearance and the obstacle cost before and after are printed and not judged: it is projection after the step,
    not a projection in the metric, and it has optimize_paths' step-size caveats (STEP is the default scaled by
    (16 / WAYPOINTS)^2, as the docstring of optimize_paths says it has to be);
  - the segments between the waypoints are straight in joint space and only checked: whether they are free and keep
    the constraint at TOL is printed.
time_paths at the URDF's velocity limits closes the pipeline; its status and duration are printed, not judged.
Other 7-joint arms run, but the scene is the Panda's."""
import sys

import numpy as np

from optik_amd import Robot
from optik_amd import _native as nat

from plan_rrt_constrained import PLAN, RESOLUTION, START, TOL, setup

WAYPOINTS = 32
ITERS, STEP = 100, nat.PATH_OPTIMIZE_STEP * (16.0 / WAYPOINTS) ** 2
PTOL = nat.CONSTRAINT_TOL
A_MAX = 5.0  # rad / s^2 on every joint, as examples/plan_rrt_constrained.py


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    robot = Robot.from_urdf_file(*sys.argv[1:4])
    if robot.num_positions() != len(START):
        sys.exit("the scene of this example is a 7-joint arm's (the Panda's)")
    start, goal, c = setup(robot)
    n = len(start)
    tree = robot.plan_rrt_constrained(start[None], goal[None], c, tol=TOL, **PLAN)
    print(f"plan_rrt_constrained: status {int(tree['status'][0])}, {int(tree['len'][0])} waypoints")
    bad = int(tree["status"][0]) != 0
    if not bad:
        short = robot.shortcut_paths_constrained(tree["paths"], tree["len"], c, tol=TOL, resolution=RESOLUTION)
        print(f"shortcut_paths_constrained: status {int(short['status'][0])}, {int(short['len'][0])} waypoints")
        dense, st, projected = robot.resample_paths_constrained(short["paths"], short["len"], c, WAYPOINTS, ptol=PTOL)
        print(f"resample_paths_constrained: status {int(st[0])}, {WAYPOINTS} waypoints, {int(projected[0, 1])} of "
              f"{int(projected[0, 0])} projected")
        clr_in = robot.collision_clearance_batch_arrays(dense[0])[0].min()
        v_in = robot.constraint_batch_arrays(dense[0], c)[1].max()
        print(f"before: clearance {clr_in:.4f} m, violation {v_in:.3e}")
        res = robot.optimize_paths_constrained(dense, c, iters=ITERS, step=STEP, resolution=RESOLUTION, tol=TOL,
                                               ptol=PTOL)
        print(f"after: clearance {res['clearance'][0]:.4f} m, violation {res['violation'][0]:.3e}")
        print(f"optimize_paths_constrained: status {int(res['status'][0])}, F_obs {res['cost_first'][0, 2]:.4f} -> "
              f"{res['cost_last'][0, 2]:.4f}, length cost {res['cost_first'][0, 1]:.4f} -> {res['cost_last'][0, 1]:.4f}; "
              f"{int(res['projected'][0, 0])} projections, {int(res['projected'][0, 1])} ended on the constraint; "
              f"segments free: {bool(res['free'][0])}, on the constraint: {bool(res['keeps'][0])}")
        bad = int(res["status"][0]) != 0 or (v_in <= PTOL and not res["violation"][0] <= PTOL)
        timed = robot.time_paths(res["paths"], None, a_max=np.full(n, A_MAX),
                                 v_max=np.asarray(robot.velocity_limits(), dtype=np.float64))
        print(f"  timed at the URDF's velocity limits: status {int(timed['status'][0])}, {timed['duration'][0]:.3f} s")
    robot.clear_collision_model()
    robot.set_world()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
