"""The pair a roadmap misses: single-query planning with two trees (Robot.plan_rrt).

    python examples/plan_rrt.py robot.urdf base_link ee_link

The scene of plan_lazy.py: the arm's first joint 2 rad to the left and to the right of the middle of its range, and a
thin wall where the outermost sphere of the arm's model passes halfway.  The roadmap is deliberately small -- 8 nodes
with one neighbour each --, so that plan_paths finds no route for the pair (status 1).  plan_rrt needs no roadmap: it
grows one tree from the start and one from the goal and joins them.  A tree's path is jagged, so shortcut_paths
straightens it, and certify_paths says whether every segment of the result is free for every t, not only at the
samples."""
import sys

import numpy as np

from optik_amd import Robot
from optik_amd.collision import spheres_along_chain

RESOLUTION = 0.05  # of the motion check, radians
NODES, K = 8, 1


def scene(robot):
    """(start, goal, mid, model): as examples/plan_lazy.py."""
    lb, ub = (np.array(v) for v in robot.joint_limits())
    mid = 0.5 * (np.maximum(lb, -np.pi) + np.minimum(ub, np.pi))
    start, goal = mid.copy(), mid.copy()
    start[0], goal[0] = max(mid[0] - 2.0, lb[0]), min(mid[0] + 2.0, ub[0])
    return start, goal, mid, spheres_along_chain(robot, 0.05, 2)


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    robot = Robot.from_urdf_file(*sys.argv[1:4])
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

    edges = robot.build_roadmap(NODES, K, RESOLUTION)
    plan = robot.plan_paths(start[None], goal[None])
    print(f"roadmap of {NODES} nodes, {edges} free edges: status {int(plan['status'][0])}")

    tree = robot.plan_rrt(start[None], goal[None], resolution=RESOLUTION)
    status, length = int(tree["status"][0]), int(tree["len"][0])
    print(f"plan_rrt: status {status}, {length} waypoints, length {tree['cost'][0]:.3f} rad, "
          f"{int(tree['iters'][0])} iterations, trees of {int(tree['nodes'][0, 0])} and {int(tree['nodes'][0, 1])} nodes")
    bad = 1 if status else 0
    if status == 0:
        short = robot.shortcut_paths(tree["paths"], tree["len"], resolution=RESOLUTION)
        cert = robot.certify_paths(short["paths"], short["len"])
        verdict = {0: "free", 1: "blocked"}.get(int(cert["status"][0]), "undecided")
        print(f"shortcut: status {int(short['status'][0])}, {int(short['len'][0])} waypoints, length "
              f"{short['cost'][0]:.3f} rad; certified {verdict}")
        bad += int(short["status"][0]) != 0
    robot.clear_collision_model()
    robot.set_world()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
