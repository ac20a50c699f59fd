#!/usr/bin/env python3
"""Checked motions between waypoints: a path whose waypoints lie on both sides of a thin wall, solved with ik_path
without and with the motion check (Robot.set_motion_resolution).  Without it every waypoint is collision-free and the
move across the wall goes straight through it; with it a waypoint is only accepted if the straight joint-space move
from the previous one is free at the resolution.  The robot is modelled by spheres along its links:

    python examples/ik_motion.py <robot.urdf> <base_link> <ee_link> [restarts]"""
import sys

import numpy as np

from optik_amd import Robot, SolverConfig
from optik_amd.collision import spheres_along_chain


def main():
    if len(sys.argv) < 4:
        print(__doc__)
        return 2
    urdf, base, ee = sys.argv[1:4]
    restarts = int(sys.argv[4]) if len(sys.argv) > 4 else 256
    robot = Robot.from_urdf_file(urdf, base, ee)
    n = robot.num_positions()
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(1)
    frames, centers, radii = spheres_along_chain(robot, 0.04, 6)
    robot.set_collision_model(frames, centers, radii, self_pairs="auto", margin=0.0)
    h, L = 0.02, 8
    qa = 0.5 * (lb + ub) + rng.uniform(-0.3, 0.3, n)
    qb = np.clip(qa + rng.uniform(0.4, 0.8, n) * rng.choice([-1.0, 1.0], n), lb, ub)
    qs = np.array([(1 - s) * qa + s * qb for s in np.linspace(0.0, 1.0, L)])
    targets = np.array([robot.fk(q) for q in qs])

    # a wall of 1 cm across the move of the outermost model sphere between the two middle waypoints
    def point(q):
        fr = robot.link_frames_batch_arrays(np.array([q]))[0, frames[-1]]
        return fr[:3, 3] + fr[:3, :3] @ centers[-1]
    a, b = point(qs[L // 2 - 1]), point(qs[L // 2])
    u = (b - a) / np.linalg.norm(b - a)
    quat = np.concatenate([np.cross([1.0, 0.0, 0.0], u), [1.0 + u[0]]])
    quat /= np.linalg.norm(quat)
    robot.set_world(boxes=[np.concatenate([(a + b) / 2, quat, [0.005, 0.2, 0.2]])])
    print(f"wall of 1 cm at {np.round((a + b) / 2, 3).tolist()}; the sphere travels "
          f"{np.linalg.norm(b - a):.3f} m between waypoints {L // 2 - 1} and {L // 2}")

    cfg = SolverConfig("quality", max_time=0.0, max_restarts=restarts)
    paths = {}
    for name, res in (("off", 0.0), ("on", h)):
        robot.set_motion_resolution(res)
        paths[name] = robot.ik_path(cfg, targets, qa, max_step=float("inf"))
    ok = True
    for name, path in paths.items():
        c, moves = qa, []
        for w, r in enumerate(path):
            if r is None:
                moves.append((w, None))
                continue
            clr, free, first, steps = robot.collision_motion(c, r[0], h)
            moves.append((w, (clr, free, first, steps)))
            c = np.array(r[0])
        line = "  ".join(f"{w}:{'none' if m is None else ('free' if m[1] else f'hit@{m[2]}/{m[3]}')}" for w, m in moves)
        print(f"check {name:3s}: {line}")
        if name == "on":
            ok = all(m is None or m[1] for _, m in moves)
    diff = [w for w, (r0, r1) in enumerate(zip(paths["off"], paths["on"]))
            if (r0 is None) != (r1 is None) or (r0 is not None and r0[0] != r1[0])]
    print(f"waypoints where the two differ: {diff}")
    print(f"every checked move free: {ok}")
    robot.set_motion_resolution(0.0)
    robot.clear_collision_model()
    return 0


if __name__ == "__main__":
    sys.exit(main())
