"""IK into a pose region instead of an exact pose (Robot.ik_region, Robot.plan_rrt_to_region).

    python examples/ik_region.py robot.urdf base_link ee_link

The target is the pose the end effector has in a configuration a little off the middle of the joint range.  Three
requests that an exact-pose IK cannot express:
  "reach this point, any orientation"             PoseConstraint.position_only(target)
  "drill here, any angle about the tool axis"     PoseConstraint.axis_free(target, "z")
  "put the glass anywhere on this shelf, upright" a box: 10 cm either way in x and y, the height pinned, the tool's z
                                                  axis within TILT of the target's, any angle about it
Each prints how many distinct configurations came back, the largest violation among them and how far apart they are;
the last is then the goal of the tree planner (Robot.plan_rrt_to_region; plan_rrt_to_region_constrained also keeps
the glass upright on the way).  Exits non-zero if a returned row violates its region."""
import math
import sys

import numpy as np

from optik_amd import PoseConstraint, Robot, SolverConfig

K, MIN_DIST, RESTARTS, TOL = 8, 0.3, 256, 1e-6
TILT, RESOLUTION = 0.3, 0.05


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    robot = Robot.from_urdf_file(*sys.argv[1:4])
    lb, ub = (np.array(v) for v in robot.joint_limits())
    lo, hi = np.maximum(lb, -2.5), np.minimum(ub, 2.5)
    n = len(lb)
    start = lo + (0.5 + 0.2 * np.cos(1.7 * np.arange(n) + 0.4)) * (hi - lo)
    there = np.clip(start + 0.4 * np.sin(np.arange(n) + 1.0), lb, ub)
    target = np.array(robot.fk(list(there)))
    config = SolverConfig("quality", max_time=0.0, max_restarts=RESTARTS)
    b, inf = TILT / math.sqrt(2.0), math.inf
    shelf = PoseConstraint(target, [-0.1, -0.1, 0.0, -b, -b, -inf], [0.1, 0.1, 0.0, b, b, inf])
    bad = 0
    for what, region in (("position_only", PoseConstraint.position_only(target)),
                         ("axis_free z", PoseConstraint.axis_free(target, "z")), ("shelf, upright", shelf)):
        xs = robot.ik_region(config, region, start, k=K, min_dist=MIN_DIST, restarts=RESTARTS, tol=TOL)
        v = robot.constraint_batch_arrays(np.array(xs), region)[1] if xs else np.zeros(0)
        apart = min((np.abs(a - c).max() for i, a in enumerate(xs) for c in xs[:i]), default=math.inf)
        print(f"{what}: {len(xs)} configurations, largest violation {v.max(initial=0.0):.1e}, closest pair "
              f"{apart:.2f} rad apart")
        bad += int(len(xs) == 0 or not (v <= TOL).all() or not apart > MIN_DIST)

    plan = robot.plan_rrt_to_region(config, start[None], shelf, k=K, min_dist=MIN_DIST, resolution=RESOLUTION,
                                    region_args=dict(restarts=RESTARTS, tol=TOL))
    status, length = int(plan["status"][0]), int(plan["len"][0])
    print(f"plan_rrt_to_region: status {status}, goal {int(plan['goal'][0])} of {int(plan['count'][0])}, {length} "
          f"waypoints, length {plan['cost'][0]:.3f} rad")
    if status == 0:
        last = plan["paths"][0, length - 1]
        v = robot.constraint_batch_arrays(last[None], shelf)[1][0]
        print(f"the last waypoint violates the shelf region by {v:.1e}")
        bad += int(not v <= TOL)
    else:
        bad += 1
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
