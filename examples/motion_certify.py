"""What the samples step over: the certified motion check (Robot.collision_motion_certify, Robot.certify_paths).

    python examples/motion_certify.py robot.urdf base_link ee_link

A model of small spheres (5 mm, one per link) and a plate 1 mm thick.  The arm's first joint swings 1.8 rad; the plate
stands where the outermost sphere passes between two samples of the motion check at the roadmap's default resolution
(0.05 rad), so that check calls the move free: free at its samples.  The certified check walks the same segment by
conservative advancement -- every step as long as the clearance at the last sample allows, no longer -- and says
blocked, and where.  Then a route around a wall is planned over a roadmap, whose edges are sampled motions, and
certify_paths says what holds along the whole of it."""
import sys

import numpy as np

from optik_amd import Robot
from optik_amd import _native as nat
from optik_amd.collision import spheres_along_chain

RESOLUTION = nat.ROADMAP_RESOLUTION  # of the sampled check, radians
TOL = 1e-3                           # of the certified check, metres
STATUS = {nat.CERTIFY_FREE: "free", nat.CERTIFY_BLOCKED: "blocked", nat.CERTIFY_LIMIT: "undecided (step limit)",
          nat.CERTIFY_NAN: "NaN"}


def scene(robot):
    """(start, goal, model): the first joint 0.9 rad to either side of the middle of its range, and the sphere model
    (frames, centers, radii)."""
    lb, ub = (np.array(v) for v in robot.joint_limits())
    mid = 0.5 * (np.maximum(lb, -np.pi) + np.minimum(ub, np.pi))
    start, goal = mid.copy(), mid.copy()
    start[0], goal[0] = max(mid[0] - 0.9, lb[0]), min(mid[0] + 0.9, ub[0])
    return start, goal, spheres_along_chain(robot, 0.005, 1)


def plate(robot, model, start, goal, t, half_extents):
    """A box [10] across the path of the model's outermost sphere, centred where that sphere is at q(t), its first
    axis along the sphere's direction of travel."""
    frames, centers, _ = model

    def point(q):
        link = np.array(robot.link_frames_batch_arrays(q[None]))[0, frames[-1]]
        return (link @ np.append(centers[-1], 1.0))[:3]
    q = start + t * (goal - start)
    dq = 1e-3 * (goal - start)
    u = point(q + dq) - point(q - dq)
    u /= np.linalg.norm(u)
    quat = np.concatenate([np.cross([1.0, 0.0, 0.0], u), [1.0 + u[0]]])
    quat /= np.linalg.norm(quat)
    return np.concatenate([point(q), quat, half_extents])


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    robot = Robot.from_urdf_file(*sys.argv[1:4])
    start, goal, model = scene(robot)
    robot.set_collision_model(*model, self_pairs=None)

    # 1. a plate between two samples
    K = int(np.ceil(np.abs(goal - start).max() / RESOLUTION))
    t_plate = (K // 2 + 0.5) / K
    robot.set_world(boxes=[plate(robot, model, start, goal, t_plate, [0.0005, 0.02, 0.02])])
    clr, free, first, steps = robot.collision_motion(start, goal, RESOLUTION)
    print(f"sampled at {RESOLUTION} rad: {'free' if free else f'blocked at sample {first}'} ({steps} steps, lowest "
          f"clearance {clr:.4f} m); the plate stands at t = {t_plate:.4f}")
    status, n, t_stop, clr = robot.collision_motion_certify(start, goal, TOL)
    print(f"certified, tol {TOL} m: {STATUS[status]} at t = {t_stop:.4f} after {n} samples (clearance there "
          f"{clr:.4f} m)")
    sampled_free, certified_blocked = bool(free), status == nat.CERTIFY_BLOCKED

    # 2. a planned route, certified
    robot.set_world(boxes=[plate(robot, model, start, goal, 0.5, [0.01, 0.15, 0.15])])
    edges = robot.build_roadmap(resolution=RESOLUTION)
    plan = robot.plan_paths(start[None], goal[None])
    if int(plan["status"][0]) != 0:
        print(f"roadmap: {edges} free edges; plan: status {int(plan['status'][0])}")
    else:
        cert = robot.certify_paths(plan["paths"], plan["len"], tol=TOL)
        s, seg = int(cert["status"][0]), int(cert["segment"][0])
        print(f"roadmap: {edges} free edges; plan: {int(plan['len'][0])} waypoints; certified: {STATUS[s]}"
              + (f" at segment {seg}" if seg >= 0 else "") + f", clearance {cert['clearance'][0]:.4f} m")
    print(f"the samples stepped over the plate: {sampled_free and certified_blocked}")
    robot.clear_collision_model()
    robot.set_world()
    return 0


if __name__ == "__main__":
    sys.exit(main())
