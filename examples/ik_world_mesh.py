#!/usr/bin/env python3
"""IK against a triangle mesh: a small fixture (a table slab and an L-bracket standing on it, as closed triangle boxes)
is written to an STL file, loaded back (optik_amd.collision.load_stl), turned into a signed distance field on the GPU
and installed (Robot.set_world_mesh); then a target is solved with ik against that field and the solution's clearance
is read back with collision_clearance_batch_arrays:

    python examples/ik_world_mesh.py <robot.urdf> <base_link> <ee_link> [restarts]"""
import math
import os
import sys
import tempfile

import numpy as np

from optik_amd import Robot, SolverConfig
from optik_amd.collision import load_stl, spheres_along_chain


def box_triangles(lo, hi):
    """The 12 outward-oriented triangles of the box [lo, hi], [12, 3, 3]."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.array([[(hi if (k >> a) & 1 else lo)[a] for a in range(3)] for k in range(8)])
    quads = [(0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6)]
    return np.array([[v[i], v[j], v[k]] for q in quads for i, j, k in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))])


def write_stl(path, tris):
    """A binary STL file: 80-byte header, the count, then per triangle a normal (left zero: readers recompute it), the
    three vertices as float32 and two attribute bytes."""
    rec = np.zeros(len(tris), dtype=np.dtype([("f", "<f4", (12,)), ("attr", "<u2")]))
    rec["f"][:, 3:] = np.asarray(tris, dtype=np.float32).reshape(-1, 9)
    with open(path, "wb") as fh:
        fh.write(b"optik_amd example fixture".ljust(80))
        fh.write(np.uint32(len(tris)).astype("<u4").tobytes())
        fh.write(rec.tobytes())


def main():
    if len(sys.argv) < 4:
        print(__doc__)
        return 2
    urdf, base, ee = sys.argv[1:4]
    restarts = int(sys.argv[4]) if len(sys.argv) > 4 else 1024
    robot = Robot.from_urdf_file(urdf, base, ee)
    n = robot.num_positions()
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(2)
    frames, centers, radii = spheres_along_chain(robot, 0.05, 8)
    voxel = 0.04
    # the mesh field is the true distance: the only error is the grid's interpolation, sqrt(3) voxels, which goes into
    # the margin.  (No self pairs: the margin would apply to them too.)
    margin = math.sqrt(3.0) * voxel
    robot.set_collision_model(frames, centers, radii, self_pairs=None, margin=margin)

    # the fixture: a table slab, and an L-bracket (a post and an arm over the table) standing on it.  The boxes
    # overlap where they touch, which the winding number does not mind: inside either still reads inside
    fixture = np.concatenate([box_triangles([0.35, -0.45, 0.16], [0.85, 0.45, 0.20]),
                              box_triangles([0.55, 0.20, 0.19], [0.61, 0.26, 0.60]),
                              box_triangles([0.55, -0.05, 0.54], [0.61, 0.26, 0.60])])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "fixture.stl")
        write_stl(path, fixture)
        mesh = load_stl(path)
    origin, shape = [-1.0, -1.0, -0.2], (51, 51, 41)
    values = robot.set_world_mesh(origin, voxel, shape, mesh)
    print(f"{len(mesh)} triangles -> field {values.min():.3f} .. {values.max():.3f} m on {values.shape} nodes, "
          f"{int((values < 0).sum())} of them inside the fixture")

    # a target that is known to be reachable without collision: the pose of a free configuration
    x_now = 0.5 * (lb + ub)
    cand = rng.uniform(np.maximum(lb, x_now - 1.0), np.minimum(ub, x_now + 1.0), size=(256, n))
    clr, free = robot.collision_clearance_batch_arrays(cand)
    cand = cand[free & (clr > margin + 0.02)]
    if len(cand) == 0:
        print("no free configuration among the candidates")
        return 1
    target = robot.fk(cand[0])

    cfg = SolverConfig("quality", max_time=0.0, max_restarts=restarts)
    sol = robot.ik(cfg, target, x_now)
    if sol is None:
        print("ik: no collision-free solution")
        return 1
    c, ok = robot.collision_clearance_batch_arrays(np.asarray(sol[0]).reshape(1, n))
    print(f"ik against the mesh: error {sol[1]:.2e}, clearance {c[0]:.3f} (margin {margin:.3f})")
    all_free = bool(ok[0]) and c[0] >= margin
    print(f"all free: {all_free}")
    robot.clear_world_grid()
    robot.clear_collision_model()
    return 0 if all_free else 1


if __name__ == "__main__":
    sys.exit(main())
