"""A way round a wall: a roadmap over the joint space, planned on the GPU (Robot.build_roadmap, Robot.plan_paths).

    python examples/plan_path.py robot.urdf base_link ee_link

Two configurations, the arm's first joint 0.9 rad to the left and to the right of the middle of its range, and a
thin wall where the outermost sphere of the arm's model passes halfway between them.  The motion check refuses the
straight joint-space move.  build_roadmap samples configurations inside the joint limits, joins each to its nearest
neighbours and keeps the joins whose motion is free; plan_paths links the two ends to that graph and returns the
shortest route, every segment of it a checked motion.  optimize_paths then smooths the route against the same
world."""
import sys

import numpy as np

from optik_amd import Robot
from optik_amd.collision import spheres_along_chain

RESOLUTION = 0.05  # of the motion check, radians


def scene(robot):
    """(start, goal, mid, model): the two configurations, the one halfway between them (where main() puts the wall)
    and the sphere model (frames, centers, radii)."""
    lb, ub = (np.array(v) for v in robot.joint_limits())
    mid = 0.5 * (np.maximum(lb, -np.pi) + np.minimum(ub, np.pi))
    start, goal = mid.copy(), mid.copy()
    start[0], goal[0] = max(mid[0] - 0.9, lb[0]), min(mid[0] + 0.9, ub[0])
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

    _, free, first, steps = robot.collision_motion(start, goal, RESOLUTION)
    print(f"straight move: {'free' if free else f'blocked at sample {first} of {steps}'}")
    edges = robot.build_roadmap(resolution=RESOLUTION)
    plan = robot.plan_paths(start[None], goal[None])
    status, length = int(plan["status"][0]), int(plan["len"][0])
    if status != 0:
        print(f"roadmap: {edges} free edges; plan: status {status}")
        return 1
    path = plan["paths"][0]
    _, seg_free, _, _ = robot.collision_motion_batch_arrays(path[:length - 1], path[1:length], RESOLUTION)
    print(f"roadmap: {edges} free edges; plan: found, {length} waypoints, length {plan['cost'][0]:.3f} rad, "
          f"segments {'free' if seg_free.all() else 'blocked'}")
    if length >= 3:
        out, cost0, cost1, clearance, _, ok = robot.optimize_paths(path[None, :length], iters=20, step=0.01,
                                                                   resolution=RESOLUTION)
        print(f"optimised plan: {'free' if ok[0] else 'blocked'}, waypoint clearance {clearance[0]:.4f} m, "
              f"length cost {cost0[0, 1]:.4f} -> {cost1[0, 1]:.4f}")
    robot.clear_collision_model()
    robot.set_world()
    return 0


if __name__ == "__main__":
    sys.exit(main())
