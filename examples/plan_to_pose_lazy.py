"""The world just changed, now plan to this pose: goal sets on a lazy roadmap (Robot.build_roadmap(lazy=True),
Robot.plan_to_poses_lazy).

    python examples/plan_to_pose_lazy.py robot.urdf base_link ee_link

The scene of plan_lazy.py: the arm's first joint 2 rad to the left of the middle of its range, a thin wall where the
outermost sphere of the arm's model passes halfway, and in the place of the goal configuration the POSE the gripper has
there.  plan_to_poses_lazy solves the pose for up to 8 distinct collision-free configurations and plans to the nearest
of them over the lazy roadmap: it checks only the edges that the cheapest routes use, and after the first pass only
the queries that can still change are planned again.  Then the wall is moved with set_world and the same call plans
again with no rebuild -- plan_to_poses would refuse a lazy roadmap, and an eager one would be stale."""
import sys

import numpy as np

from optik_amd import Robot, SolverConfig
from optik_amd.collision import spheres_along_chain

RESOLUTION = 0.05  # of the motion check, radians
NODES, K = 512, 8


def scene(robot):
    """(start, goal, mid, model): as examples/plan_lazy.py."""
    lb, ub = (np.array(v) for v in robot.joint_limits())
    mid = 0.5 * (np.maximum(lb, -np.pi) + np.minimum(ub, np.pi))
    start, goal = mid.copy(), mid.copy()
    start[0], goal[0] = max(mid[0] - 2.0, lb[0]), min(mid[0] + 2.0, ub[0])
    return start, goal, mid, spheres_along_chain(robot, 0.05, 2)


def report(robot, name, plan):
    status, length, count = int(plan["status"][0]), int(plan["len"][0]), int(plan["count"][0])
    path = plan["paths"][0]
    _, seg_free, _, _ = robot.collision_motion_batch_arrays(path[:length - 1], path[1:length], RESOLUTION)
    print(f"{name}: {count} IK solutions, status {status}, goal {int(plan['goal'][0])}, {length} waypoints, length "
          f"{plan['cost'][0]:.3f} rad, segments {'free' if seg_free.all() else 'blocked'}; rounds {plan['rounds']}, "
          f"checked {plan['checked']} of {NODES * K} edges")
    return status


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    robot = Robot.from_urdf_file(*sys.argv[1:4])
    start, goal, mid, (frames, centers, radii) = scene(robot)
    robot.set_collision_model(frames, centers, radii, self_pairs=None)
    target = np.array(robot.fk(goal))
    cfg = SolverConfig("quality", max_time=0.0, max_restarts=64)

    # a wall of 2 cm across the move of the outermost model sphere, where it is when the arm is halfway
    def point(q):
        link = np.array(robot.link_frames_batch_arrays(q[None]))[0, frames[-1]]
        return (link @ np.append(centers[-1], 1.0))[:3]
    a, b = point(start), point(goal)
    u = (b - a) / np.linalg.norm(b - a)
    quat = np.concatenate([np.cross([1.0, 0.0, 0.0], u), [1.0 + u[0]]])
    quat /= np.linalg.norm(quat)
    wall = np.concatenate([point(mid), quat, [0.01, 0.15, 0.15]])
    robot.set_world(boxes=[wall])

    open_slots = robot.build_roadmap(NODES, K, RESOLUTION, lazy=True)
    print(f"lazy roadmap: {NODES} nodes, {open_slots} of {NODES * K} edge slots open, none checked")
    bad = report(robot, "wall in place", robot.plan_to_poses_lazy(cfg, start[None], target[None]))

    # the world changes: the wall is moved 1 m up, out of the arm's way; the roadmap is not rebuilt
    moved = wall.copy()
    moved[2] += 1.0
    robot.set_world(boxes=[moved])
    bad += report(robot, "wall moved away", robot.plan_to_poses_lazy(cfg, start[None], target[None]))
    again = robot.plan_to_poses_lazy(cfg, start[None], target[None])
    print(f"the same plan again: rounds {again['rounds']}, checked {again['checked']} (the verdicts are kept)")

    robot.clear_collision_model()
    robot.set_world()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
