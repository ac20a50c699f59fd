"""Move the gripper to a pose behind a wall: IK solutions as a goal set, planned in one pass (Robot.plan_to_poses).

    python examples/plan_to_pose.py robot.urdf base_link ee_link

The wall scene of examples/plan_path.py: the arm starts on one side of a thin wall, and the target is the pose its
end effector has in a configuration on the other side.  A pose is not one goal but several: plan_to_poses asks
ik_solutions for up to 8 distinct collision-free solutions, seeded at the start, and plans over the roadmap to the
NEAREST of them by route length -- one run of the shortest-path search for the whole set, where a loop over the
solutions would take one each.  The solution nearest the start in joint space (solution 0 of the Quality mode) is not
always the one with the shortest free route; both costs are printed."""
import sys

import numpy as np

from optik_amd import Robot, SolverConfig
from plan_path import RESOLUTION, scene


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    robot = Robot.from_urdf_file(*sys.argv[1:4])
    start, goal, mid, (frames, centers, radii) = scene(robot)
    robot.set_collision_model(frames, centers, radii, self_pairs=None)

    # the wall of plan_path.py: 2 cm across the move of the outermost model sphere, where it is when the arm is halfway
    def point(q):
        link = np.array(robot.link_frames_batch_arrays(q[None]))[0, frames[-1]]
        return (link @ np.append(centers[-1], 1.0))[:3]
    a, b = point(start), point(goal)
    u = (b - a) / np.linalg.norm(b - a)
    quat = np.concatenate([np.cross([1.0, 0.0, 0.0], u), [1.0 + u[0]]])
    quat /= np.linalg.norm(quat)
    robot.set_world(boxes=[np.concatenate([point(mid), quat, [0.01, 0.15, 0.15]])])

    target = np.array(robot.fk(goal))
    edges = robot.build_roadmap(resolution=RESOLUTION)
    config = SolverConfig("quality", max_time=0.0, max_restarts=256)
    plan = robot.plan_to_poses(config, start[None], target[None], k=8, min_dist=0.3)
    count, status, which = int(plan["count"][0]), int(plan["status"][0]), int(plan["goal"][0])
    print(f"roadmap: {edges} free edges; the pose has {count} distinct collision-free IK solutions")
    if status != 0:
        print(f"plan: status {status}")
        return 1
    length = int(plan["len"][0])
    path = plan["paths"][0]
    _, seg_free, _, _ = robot.collision_motion_batch_arrays(path[:length - 1], path[1:length], RESOLUTION)
    print(f"plan: reached IK solution {which} of {count}, {length} waypoints, length {plan['cost'][0]:.3f} rad, "
          f"segments {'free' if seg_free.all() else 'blocked'}")
    alone = robot.plan_paths(start[None], plan["goals"][:, 0])
    cost0 = f"length {alone['cost'][0]:.3f} rad" if int(alone["status"][0]) == 0 else f"status {int(alone['status'][0])}"
    print(f"planning to IK solution 0 alone (the one nearest the start): {cost0}")
    robot.clear_collision_model()
    robot.set_world()
    return 0


if __name__ == "__main__":
    sys.exit(main())
