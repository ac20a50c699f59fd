"""From a planned route to a trajectory a controller executes: plan, shortcut, resample, time, sample -- all on the GPU.

    python examples/time_path.py robot.urdf base_link ee_link

The wall scene of plan_path.py and the chain of shortcut_path.py up to the 32 evenly spaced waypoints of
resample_paths.  time_paths gives every waypoint a time, a velocity and an acceleration within the URDF's velocity
limits and an acceleration limit of A_MAX rad/s^2, rest to rest; sample_trajectories evaluates the cubic Hermite
trajectory through them at 1 kHz, as a joint-trajectory controller would, and checks the moves between samples."""
import sys

import numpy as np

from optik_amd import Robot

from plan_path import RESOLUTION, scene

A_MAX = 7.5   # rad/s^2; a URDF carries no acceleration limits
DT = 0.001    # s


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
    cut = robot.shortcut_paths(plan["paths"], plan["len"], resolution=RESOLUTION)
    if cut["status"][0] != 0:
        print(f"shortcut: status {cut['status'][0]}")
        return 1
    dense, _, free = robot.resample_paths(cut["paths"], cut["len"], 32, resolution=RESOLUTION)
    print(f"resampled: {dense.shape[1]} waypoints, {'free' if free[0] else 'blocked'}")

    v_max = robot.velocity_limits()
    timing = robot.time_paths(dense, a_max=A_MAX)
    if timing["status"][0] != 0:
        print(f"timed: status {timing['status'][0]}")
        return 1
    qd, qdd = timing["velocities"][0], timing["accelerations"][0]
    print(f"timed: duration {timing['duration'][0]:.4f} s")
    print(f"waypoints: peak |qd| / v_max {np.max(np.abs(qd) / v_max):.12f}, "
          f"peak |qdd| / a_max {np.max(np.abs(qdd)) / A_MAX:.12f}")
    q, v, ok = robot.sample_trajectories(dense, timing, DT, resolution=RESOLUTION)
    print(f"samples: {q.shape[1]} at {1.0 / DT:.0f} Hz, peak |qd| / v_max between waypoints "
          f"{np.max(np.abs(v[0]) / v_max):.4f}, moves {'free' if ok[0] else 'blocked'}, "
          f"ends {'at' if np.array_equal(q[0, -1], dense[0, -1]) else 'off'} the goal")
    robot.clear_collision_model()
    robot.set_world()
    return 0


if __name__ == "__main__":
    sys.exit(main())
