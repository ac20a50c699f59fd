"""A joint-space path bent around an obstacle instead of through it (Robot.optimize_paths).

    python examples/optimize_path.py robot.urdf base_link ee_link

Two collision-free IK solutions on either side of a ball, the arm's first joint 0.9 rad to the left and to the right
of the middle of its range; the straight joint-space path between them sweeps a link through the ball.
optimize_paths (covariant gradient smoothing, after CHOMP) bends the 16 waypoints away from it; the motion check
says what each path is worth, before and after."""
import sys

import numpy as np

from optik_amd import Robot, SolverConfig
from optik_amd.collision import spheres_along_chain

RESOLUTION = 0.05  # of the motion check, radians
INFLUENCE, SAFETY = 0.2, 0.05


def scene(robot):
    """(qa, qb, mid, model): the two configurations, the one halfway between them (where main() puts the ball)
    and the sphere model (frames, centers, radii)."""
    lb, ub = (np.array(v) for v in robot.joint_limits())
    mid = 0.5 * (np.maximum(lb, -np.pi) + np.minimum(ub, np.pi))
    qa, qb = mid.copy(), mid.copy()
    qa[0], qb[0] = max(mid[0] - 0.9, lb[0]), min(mid[0] + 0.9, ub[0])
    model = spheres_along_chain(robot, 0.05, 2)
    return qa, qb, mid, model


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    robot = Robot.from_urdf_file(*sys.argv[1:4])
    robot.set_parallelism(1)  # (ik: the lowest successful restart, which starts from x0)
    qa, qb, mid, (frames, centers, radii) = scene(robot)
    robot.set_collision_model(frames, centers, radii, self_pairs=None)
    # the ball sits where the outermost sphere of the model is when the arm is halfway
    link = np.array(robot.link_frames_batch_arrays(mid[None]))[0, frames[-1]]
    ball = np.concatenate([(link @ np.append(centers[-1], 1.0))[:3], [0.08]])
    robot.set_world(spheres=[ball])
    config = SolverConfig(max_time=0.0, max_restarts=64)
    ends = []
    for q in (qa, qb):
        sol = robot.ik(config, np.array(robot.fk(q.tolist())), q.tolist())
        if sol is None:
            sys.exit("no collision-free IK solution for one end of the path")
        ends.append(np.array(sol[0]))
    s = np.linspace(0.0, 1.0, 16)[:, None]
    path = (1.0 - s) * ends[0][None] + s * ends[1][None]
    clr, free, _, _ = robot.collision_motion_batch_arrays(path[:-1], path[1:], RESOLUTION)
    print(f"straight path: {'free' if free.all() else 'blocked'}, clearance {clr.min():.4f} m")
    out, first, last, clearance, status, ok = robot.optimize_paths(path[None], influence=INFLUENCE, safety=SAFETY,
                                                                   resolution=RESOLUTION)
    clr, free, _, _ = robot.collision_motion_batch_arrays(out[0, :-1], out[0, 1:], RESOLUTION)
    print(f"optimised path: {'free' if ok[0] and free.all() else 'blocked'}, clearance {clr.min():.4f} m "
          f"(waypoints {clearance[0]:.4f} m); F_obs {first[0, 2]:.4f} -> {last[0, 2]:.4f}, "
          f"length cost {first[0, 1]:.4f} -> {last[0, 1]:.4f}")


if __name__ == "__main__":
    main()
