"""Carry the glass upright: a roadmap whose every edge keeps a pose constraint (Robot.build_constrained_roadmap,
Robot.plan_constrained_paths).

    python examples/plan_constrained.py robot.urdf base_link ee_link [nodes]

The constraint: the end effector's z axis stays within TILT radians of where it points in the middle of the joint
range (PoseConstraint.upright).  A handful of configurations are projected onto it and paired up as starts and goals.
The unconstrained planner joins each pair by the straight joint-space move, which keeps the constraint at its two ends
and nowhere in between; the constrained planner samples nodes, projects them, keeps the joins that pass the constraint
check at every sample, and routes over those.  The tilt along both is printed side by side."""
import sys

import numpy as np

from optik_amd import PoseConstraint, Robot

RESOLUTION = 0.05  # of the motion checks, radians
TILT, TOL = 0.4, 0.05
PAIRS = 16


def tilt_along(robot, path, reference):
    """The largest angle between the end effector's z axis and the reference's over the samples of a path [L, n]."""
    samples = [path[:1]]
    for a, b in zip(path[:-1], path[1:]):
        k = max(1, int(np.ceil(np.max(np.abs(b - a)) / RESOLUTION)))
        samples.append(a + (np.arange(1, k + 1) / k)[:, None] * (b - a))
    ee = np.array(robot.link_frames_batch_arrays(np.concatenate(samples)))[:, -1]
    return float(np.max(np.arccos(np.clip(ee[:, :3, 2] @ reference[:3, 2], -1.0, 1.0))))


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    robot = Robot.from_urdf_file(*sys.argv[1:4])
    nodes = int(sys.argv[4]) if len(sys.argv) > 4 else 1024
    lb, ub = (np.array(v) for v in robot.joint_limits())
    mid = 0.5 * (np.maximum(lb, -np.pi) + np.minimum(ub, np.pi))
    reference = np.array(robot.fk(list(mid)))
    c = PoseConstraint.upright(reference, TILT)

    # starts and goals: uniform configurations projected onto the constraint
    rng = np.random.default_rng(0)
    p = robot.constraint_project_batch_arrays(rng.uniform(np.maximum(lb, -np.pi), np.minimum(ub, np.pi),
                                                          (4 * PAIRS, len(lb))), c)
    ends = p["x"][p["status"] == 0][:2 * PAIRS]
    starts, goals = ends[:len(ends) // 2], ends[len(ends) // 2:2 * (len(ends) // 2)]
    print(f"projected {int((p['status'] == 0).sum())} of {len(p['status'])} configurations onto 'upright within "
          f"{TILT} rad'")

    roadmap = robot.build_constrained_roadmap(c, TOL, nodes, 8, RESOLUTION)
    print(f"constrained roadmap: {roadmap.projected} of {roadmap.N} nodes projected, "
          f"{int(np.isfinite(roadmap.w.cpu().numpy()).sum())} edges keep the constraint")
    plan = robot.plan_constrained_paths(roadmap, starts, goals)
    found = np.nonzero((plan["status"] == 0) & (plan["len"] > 2))[0]
    if not len(found):
        print(f"constrained plan: no route for any of {len(starts)} pairs (status {plan['status'].tolist()})")
        return 1
    j = int(found[0])
    path = plan["paths"][j, :plan["len"][j]]
    chk = robot.check_paths_constraint(path[None], None, c, TOL, RESOLUTION)
    straight = np.stack([starts[j], goals[j]])
    chk0 = robot.check_paths_constraint(straight[None], None, c, TOL, RESOLUTION)
    print(f"unconstrained plan: 2 waypoints, length {np.max(np.abs(goals[j] - starts[j])):.3f} rad, tilt up to "
          f"{tilt_along(robot, straight, reference):.3f} rad, constraint {'kept' if chk0['ok'][0] else 'broken'} "
          f"(violation {chk0['violation'][0]:.3f})")
    print(f"constrained plan: found, {len(path)} waypoints, length {plan['cost'][j]:.3f} rad, tilt up to "
          f"{tilt_along(robot, path, reference):.3f} rad, constraint {'kept' if chk['ok'][0] else 'broken'} "
          f"(violation {chk['violation'][0]:.3f})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
