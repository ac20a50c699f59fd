"""Move the gripper to a pose the roadmap cannot reach: IK solutions as the roots of a tree (Robot.plan_rrt_to_poses).

    python examples/plan_rrt_to_pose.py robot.urdf base_link ee_link

The wall scene of plan_path.py: the arm on one side of a thin wall, and as the target the pose the end effector has
in a configuration on the other side; the roadmap is deliberately small, 8 nodes with one neighbour each.
plan_to_poses plans over the roadmap to the IK solutions of the pose and finds no route (status 1).
plan_rrt_to_poses needs no roadmap: tree 0 grows from the start, tree 1 from ALL the collision-free IK solutions at
once, and the query ends when the two meet -- at the solution joined first, not the cheapest one; a solution that
cannot be reached costs its root node and nothing more.  A tree's path is jagged, so shortcut_paths straightens it."""
import sys

import numpy as np

from optik_amd import Robot, SolverConfig
from plan_path import RESOLUTION, scene

NODES, K = 8, 1
SOLUTIONS, MIN_DIST, RESTARTS = 8, 0.3, 256


def setup(robot):
    """Installs the model and the wall of plan_path.py; returns (start, target [4, 4], config)."""
    start, goal, mid, (frames, centers, radii) = scene(robot)
    robot.set_collision_model(frames, centers, radii, self_pairs=None)

    # a wall of 2 cm across the move of the outermost model sphere, where it is when the arm is halfway
    def point(q):
        link = np.array(robot.link_frames_batch_arrays(q[None]))[0, frames[-1]]
        return (link @ np.append(centers[-1], 1.0))[:3]
    a, b = point(start), point(goal)
    u = (b - a) / np.linalg.norm(b - a)
    quat = np.concatenate([np.cross([1.0, 0.0, 0.0], u), [1.0 + u[0]]])
    quat /= np.linalg.norm(quat)
    robot.set_world(boxes=[np.concatenate([point(mid), quat, [0.01, 0.15, 0.15]])])
    return start, np.array(robot.fk(goal)), SolverConfig("quality", max_time=0.0, max_restarts=RESTARTS)


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    robot = Robot.from_urdf_file(*sys.argv[1:4])
    start, target, config = setup(robot)

    edges = robot.build_roadmap(NODES, K, RESOLUTION)
    plan = robot.plan_to_poses(config, start[None], target[None], k=SOLUTIONS, min_dist=MIN_DIST)
    print(f"roadmap of {NODES} nodes, {edges} free edges: plan_to_poses status {int(plan['status'][0])} "
          f"with {int(plan['count'][0])} IK solutions")

    tree = robot.plan_rrt_to_poses(config, start[None], target[None], k=SOLUTIONS, min_dist=MIN_DIST,
                                   resolution=RESOLUTION)
    status, length, which = int(tree["status"][0]), int(tree["len"][0]), int(tree["goal"][0])
    print(f"plan_rrt_to_poses: status {status}, reached IK solution {which} of {int(tree['count'][0])}, {length} "
          f"waypoints, length {tree['cost'][0]:.3f} rad, {int(tree['iters'][0])} iterations, trees of "
          f"{int(tree['nodes'][0, 0])} and {int(tree['nodes'][0, 1])} nodes")
    bad = 1 if status else 0
    if status == 0:
        short = robot.shortcut_paths(tree["paths"], tree["len"], resolution=RESOLUTION)
        print(f"shortcut: status {int(short['status'][0])}, {int(short['len'][0])} waypoints, length "
              f"{short['cost'][0]:.3f} rad")
        bad += int(short["status"][0]) != 0
    robot.clear_collision_model()
    robot.set_world()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
