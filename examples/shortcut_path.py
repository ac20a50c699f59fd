"""From a roadmap route to a path a controller takes: plan, shortcut, resample, optimise -- all on the GPU.

    python examples/shortcut_path.py robot.urdf base_link ee_link

The wall scene of plan_path.py: the straight joint-space move between two configurations is blocked by a thin wall.
plan_paths returns a route over roadmap nodes: a handful of random configurations, as far apart as the graph has them.
shortcut_paths subdivides it, checks every pair of vertices as a motion and walks the shortest route through what is
visible: fewer waypoints, never longer, every segment still a checked motion.  resample_paths spaces 32 waypoints
evenly along it -- their segments cut the corners, so they are checked again --, which is what optimize_paths wants."""
import sys

import numpy as np

from optik_amd import Robot

from plan_path import RESOLUTION, scene


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    robot = Robot.from_urdf_file(*sys.argv[1:4])
    start, goal, mid, (frames, centers, radii) = scene(robot)
    robot.set_collision_model(frames, centers, radii, self_pairs=None)

    def point(q):
        link = np.array(robot.link_frames_batch_arrays(q[None]))[0, frames[-1]]
        return (link @ np.append(centers[-1], 1.0))[:3]
    a, b = point(start), point(goal)
    u = (b - a) / np.linalg.norm(b - a)
    quat = np.concatenate([np.cross([1.0, 0.0, 0.0], u), [1.0 + u[0]]])
    quat /= np.linalg.norm(quat)
    robot.set_world(boxes=[np.concatenate([point(mid), quat, [0.01, 0.15, 0.15]])])

    robot.build_roadmap(resolution=RESOLUTION)
    plan = robot.plan_paths(start[None], goal[None])
    if plan["status"][0] != 0:
        print(f"plan: status {plan['status'][0]}")
        return 1
    print(f"plan: {plan['len'][0]} waypoints, length {plan['cost'][0]:.3f} rad")
    cut = robot.shortcut_paths(plan["paths"], plan["len"], resolution=RESOLUTION)
    if cut["status"][0] != 0:
        print(f"shortcut: status {cut['status'][0]}")
        return 1
    n = int(cut["len"][0])
    path = cut["paths"][0]
    _, seg_free, _, _ = robot.collision_motion_batch_arrays(path[:n - 1], path[1:n], RESOLUTION)
    print(f"shortcut: {n} waypoints, length {cut['cost'][0]:.3f} rad, segments {'free' if seg_free.all() else 'blocked'}")
    dense, _, free = robot.resample_paths(cut["paths"], cut["len"], 32, resolution=RESOLUTION)
    length = np.max(np.abs(np.diff(dense[0], axis=0)), axis=1).sum()
    print(f"resampled: {dense.shape[1]} waypoints, length {length:.3f} rad, {'free' if free[0] else 'blocked'}")
    out, cost0, cost1, clearance, _, ok = robot.optimize_paths(dense, iters=20, step=0.0005, resolution=RESOLUTION)
    length = np.max(np.abs(np.diff(out[0], axis=0)), axis=1).sum()
    print(f"optimised: {out.shape[1]} waypoints, length {length:.3f} rad, {'free' if ok[0] else 'blocked'}, "
          f"waypoint clearance {clearance[0]:.4f} m")
    robot.clear_collision_model()
    robot.set_world()
    return 0


if __name__ == "__main__":
    sys.exit(main())
