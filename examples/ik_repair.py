"""Pushing configurations out of collision (Robot.repair_configurations).

    python examples/ik_repair.py robot.urdf base_link ee_link

The scene is made for the Panda (optik_amd/robots/panda.urdf panda_link0 panda_link8): spheres along its links and a
table under its reach.

1. A start state that sensor noise put 8 mm inside the table.  plan_rrt answers such a query "no route" at once, as
   every planner here does; repair_configurations pushes the start out -- a few hundredths of a radian -- and the same
   query is then planned.
2. The same start with the tool kept where it is, PoseConstraint.position_only(fk(start), tolerance): within 2 cm the
   arm slides out through its null space; within 1 mm it does not in the default budget -- the colliding link is the
   one that carries the tool, and a fixed step followed by a projection crawls along such a constraint.  The status
   says so.
3. 256 random configurations of the cell: how many collide, and how many of those the default step and budget free.
4. ik_region low over and inside the table, where many restarts end with a link in the table top: without `repair` the
   collision filter throws those away; with repair=dict(influence, safety) they are first pushed free inside their own
   region, and more distinct configurations come back from the same restarts.
Exits non-zero if a row reported free is not, by collision_clearance_batch_arrays."""
import sys

import numpy as np

from optik_amd import PoseConstraint, Robot, SolverConfig
from optik_amd.collision import spheres_along_chain

INFLUENCE, SAFETY = 0.1, 0.02   # metres: where the hinge starts to push, and the clearance a repaired row has
RESOLUTION = 0.05               # of the planner's motion check, radians
TABLE = [0.5, 0.0, 0.2, 0.0, 0.0, 0.0, 1.0, 0.3, 0.4, 0.02]   # centre, quaternion, half extents: its top at z = 0.22
START = [0.0, 0.8, 0.0, -1.8, 0.0, 2.4, 0.8]                  # the forearm 8 mm inside the table's top
GOAL = [1.2, 0.2, 0.0, -1.6, 0.0, 1.8, 0.8]
POS_TOLS, CELL, SEED = (2e-2, 1e-3), 256, 3
REACH = [([0.7, 0.0, 0.15], 0.02), ([0.55, 0.0, 0.15], 0.02)]   # tool positions and the half width of their boxes
RESTARTS, K, MIN_DIST = 16, 8, 0.1


def model(robot):
    return spheres_along_chain(robot, 0.05, 3)


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    robot = Robot.from_urdf_file(*sys.argv[1:4])
    if robot.num_positions() != len(START):
        sys.exit("the scene of this example is the Panda's (7 joints)")
    robot.set_collision_model(*model(robot), self_pairs="auto")
    robot.set_world(boxes=[TABLE])
    start, goal = np.array(START), np.array(GOAL)
    bad = 0

    clr = robot.collision_clearance_batch_arrays(start[None])[0][0]
    plan = robot.plan_rrt(start[None], goal[None], resolution=RESOLUTION)
    print(f"start: clearance {1e3 * clr:.1f} mm; plan_rrt: status {int(plan['status'][0])}")
    fixed = robot.repair_configurations(start[None], INFLUENCE, SAFETY)
    clr = robot.collision_clearance_batch_arrays(fixed["x"])[0][0]
    print(f"repaired: status {int(fixed['status'][0])} after {int(fixed['iterations'][0])} steps, moved "
          f"{fixed['moved'][0]:.3f} rad, clearance {1e3 * clr:.1f} mm")
    bad += int(fixed["status"][0] != 0 or not clr >= SAFETY)
    plan = robot.plan_rrt(fixed["x"], goal[None], resolution=RESOLUTION)
    print(f"plan_rrt from the repaired start: status {int(plan['status'][0])}, {int(plan['len'][0])} waypoints")
    bad += int(plan["status"][0] != 0)

    for k, pos_tol in enumerate(POS_TOLS):
        region = PoseConstraint.position_only(np.array(robot.fk(list(start))), pos_tol)
        held = robot.repair_configurations(start[None], INFLUENCE, SAFETY, region=region)
        clr = robot.collision_clearance_batch_arrays(held["x"])[0][0]
        print(f"tool held within {1e3 * pos_tol:.0f} mm: status {int(held['status'][0])} after "
              f"{int(held['iterations'][0])} steps, moved {held['moved'][0]:.3f} rad, clearance {1e3 * clr:.1f} mm, "
              f"violation {held['violation'][0]:.1e}")
        bad += int(held["status"][0] == 0 and not (clr >= SAFETY and held["violation"][0] <= 1e-6))
        bad += int(k == 0 and held["status"][0] != 0)

    lb, ub = (np.array(v) for v in robot.joint_limits())
    cell = np.random.default_rng(SEED).uniform(np.maximum(lb, -2.5), np.minimum(ub, 2.5), (CELL, len(lb)))
    before = robot.collision_clearance_batch_arrays(cell)[0]
    out = robot.repair_configurations(cell, INFLUENCE, SAFETY)
    after = robot.collision_clearance_batch_arrays(out["x"])[0]
    hit = before < SAFETY
    freed = hit & (out["status"] == 0)
    print(f"cell: {int(hit.sum())} of {CELL} configurations closer than {1e3 * SAFETY:.0f} mm; {int(freed.sum())} "
          f"repaired, median move {np.median(out['moved'][freed]):.2f} rad; status counts "
          f"{np.bincount(out['status'], minlength=4).tolist()}")
    bad += int(not (after[out["status"] == 0] >= SAFETY).all() or not freed.any())

    config = SolverConfig("quality", max_time=0.0, max_restarts=RESTARTS)
    down = np.diag([1.0, -1.0, -1.0, 1.0])   # the tool pointing down (half a turn about x); the orientation is free
    regions = []
    for pos, half in REACH:
        pose = down.copy()
        pose[:3, 3] = pos
        regions.append(PoseConstraint.position_only(pose, half))
    x0s = np.tile(goal, (len(regions), 1))
    kw = dict(k=K, min_dist=MIN_DIST, restarts=RESTARTS)
    plain = robot.ik_region_batch_arrays(config, regions, x0s, **kw)
    fixed = robot.ik_region_batch_arrays(config, regions, x0s, repair=dict(influence=INFLUENCE, safety=SAFETY), **kw)
    for t in range(len(regions)):
        rows = fixed["x"][t, :fixed["count"][t]]
        clr = robot.collision_clearance_batch_arrays(rows)[0] if len(rows) else np.zeros(0)
        v = robot.constraint_batch_arrays(rows, regions[t])[1] if len(rows) else np.zeros(0)
        print(f"ik_region {t}: {int(plain['count'][t])} configurations without repair, {int(fixed['count'][t])} with "
              f"({int(fixed['repaired'][t])} of {RESTARTS} restarts repaired); smallest clearance "
              f"{1e3 * clr.min(initial=np.inf):.1f} mm, largest violation {v.max(initial=0.0):.1e}")
        bad += int(fixed["count"][t] < plain["count"][t] or not (clr >= 0.0).all() or not (v <= 1e-6).all())
    robot.clear_collision_model()
    robot.set_world()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
