"""Carry the glass upright past the wall: the tree planner under a pose constraint (Robot.plan_rrt_constrained).

    python examples/plan_rrt_constrained.py panda.urdf panda_link0 panda_link8

The scene is the Panda's of DESIGN.md section 5.18: start and goal differ in the first joint only, the end effector
points straight down at both, and a wall of 2 cm stands where the straight move sweeps the arm through.  The
constraint: the end effector's z axis stays within TILT radians of where it points at the start
(PoseConstraint.upright) -- both ends keep it exactly, and so would the straight move, which the wall blocks.
  - A constrained roadmap of 8 nodes has no route for the pair (status 1): plan_constrained_paths has no answer.
  - plan_rrt finds a way round the wall and tips the glass over on it: check_paths_constraint says so.
  - plan_rrt_constrained projects every node of its trees onto the constraint and checks every motion against it: its
    path passes check_paths_constraint, certify_paths certifies it free and time_paths times it as it is.
time_paths is given V_MAX = 0.5 rad/s, about a quarter of the URDF's limits: a tree's path is a chain of 0.5 rad steps
with a corner at every waypoint, and at the URDF's limits the profile of this path stops at two neighbouring waypoints,
which is time_paths' status 1, "stalled", with the Panda's own acceleration limits too (DESIGN.md sections 5.20 and
5.30).  At 0.5 rad/s and 5 rad/s^2 every corner is taken at the velocity limit, in 9.295 s by the host's timing
reference, and in twice that at half the speed.  Any status but 0 makes this example fail.
The pair, the wall and the tilt were chosen with the serial reference on the host (csrc/rrt_constrained_measure.hpp;
tests/test_rrt_constrained_host.py asserts it): with these parameters it joins the trees after 51 iterations with 20
and 15 nodes and 10 waypoints, all 95 projections ending on the constraint; the unconstrained reference needs 27
iterations and breaks the constraint on 9 of its 10 segments.  The device's forward kinematics may differ from the
host's in the last bit, so its counts may differ from these.  Other 7-joint arms run, but the scene is the Panda's."""
import sys

import numpy as np

from optik_amd import PoseConstraint, Robot
from optik_amd.collision import spheres_along_chain

RESOLUTION = 0.1  # of the motion checks, radians
TILT, TOL = 0.3, 0.05
START = [-0.9, 0.4, 0.0, -1.8, 0.0, 2.2, 0.7]
GOAL = [0.9, 0.4, 0.0, -1.8, 0.0, 2.2, 0.7]
WALL = [0.55, 0.0, 0.45, 0.0, 0.0, 0.0, 1.0, 0.2, 0.01, 0.25]
PLAN = dict(iters=128, step=0.5, first=1, max_nodes=64, resolution=RESOLUTION)
NODES, K = 8, 1
V_MAX, A_MAX = 0.5, 5.0  # rad / s and rad / s^2 on every joint, for time_paths: slowly, the path has corners


def setup(robot):
    """Installs the model and the wall; returns (start, goal, constraint)."""
    frames, centers, radii = spheres_along_chain(robot, 0.05, 2)
    robot.set_collision_model(frames, centers, radii, self_pairs=None)
    robot.set_world(boxes=[np.array(WALL)])
    start, goal = np.array(START), np.array(GOAL)
    return start, goal, PoseConstraint.upright(np.array(robot.fk(list(start))), TILT)


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    robot = Robot.from_urdf_file(*sys.argv[1:4])
    if robot.num_positions() != len(START):
        sys.exit("the scene of this example is a 7-joint arm's (the Panda's)")
    start, goal, c = setup(robot)

    roadmap = robot.build_constrained_roadmap(c, TOL, NODES, K, RESOLUTION)
    plan = robot.plan_constrained_paths(roadmap, start[None], goal[None])
    print(f"constrained roadmap of {NODES} nodes ({roadmap.projected} projected): status {int(plan['status'][0])}")

    def report(name, res):
        status, length = int(res["status"][0]), int(res["len"][0])
        chk = robot.check_paths_constraint(res["paths"], res["len"], c, TOL, RESOLUTION)
        print(f"{name}: status {status}, {length} waypoints, length {res['cost'][0]:.3f} rad, "
              f"{int(res['iters'][0])} iterations, trees of {int(res['nodes'][0, 0])} and {int(res['nodes'][0, 1])} "
              f"nodes; constraint {'kept' if chk['ok'][0] else 'broken'} (violation {chk['violation'][0]:.3f})")
        return status == 0, bool(chk["ok"][0])

    found, kept = report("plan_rrt", robot.plan_rrt(start[None], goal[None], **PLAN))
    bad = (not found) or kept       # (the story needs a path that breaks the constraint)
    tree = robot.plan_rrt_constrained(start[None], goal[None], c, tol=TOL, **PLAN)
    found, kept = report("plan_rrt_constrained", tree)
    print(f"projections: {int(tree['projected'][0, 0])} attempted, {int(tree['projected'][0, 1])} ended on the "
          f"constraint")
    bad = bad or not (found and kept)
    if found:
        cert = robot.certify_paths(tree["paths"], tree["len"])
        verdict = {0: "free", 1: "blocked"}.get(int(cert["status"][0]), "undecided")
        timed = robot.time_paths(tree["paths"], tree["len"], a_max=np.full(len(start), A_MAX),
                                 v_max=np.full(len(start), V_MAX))
        print(f"certified {verdict}; timed: status {int(timed['status'][0])}, {timed['duration'][0]:.3f} s")
        bad = bad or int(cert["status"][0]) != 0 or int(timed["status"][0]) != 0
    robot.clear_collision_model()
    robot.set_world()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
