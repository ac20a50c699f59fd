#!/usr/bin/env python3
"""Cost of the way from a triangle mesh to a distance-field world.  The capability is new, so
nothing here is a comparison with the parent.  There is no culling: a field costs nodes * M evaluations of a (node,
triangle) pair, and the figure that describes the kernel is the pair rate.

The mesh is a closed sphere-like surface of M triangles (a latitude / longitude sphere of radius 0.8 around the grid's
centre), the grid --nodes^3 nodes over [-1.28, 1.28]^3.  Timed with device events around HipChain.world_grid_from_mesh
on device buffers, after one warm-up call per shape; medians of --reps with [min, max]:

  field       the whole call at the built-in launch bound: pairs / second
  split       the same with the launch bound forced to 1/16 of the built-in one (_native.mesh_pairs_per_launch): what
              the split into launches costs
  robot       Robot.set_world_mesh of the same mesh on a --robot-nodes^3 grid, end to end from host arrays

One JSON line."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from grid_cost import PANDA, once, stats  # noqa: E402
from optik_amd import Robot, _native  # noqa: E402
from optik_amd.device import HipChain  # noqa: E402


def sphere_mesh(M, radius=0.8):
    """A closed latitude / longitude sphere of exactly M triangles (M even, >= 8), [M, 3, 3], outward oriented."""
    rings = max(2, int(round(math.sqrt(M / 4.0))))
    seg = max(3, M // (2 * rings))
    th = np.linspace(0.0, math.pi, rings + 1)
    ph = np.linspace(0.0, 2.0 * math.pi, seg + 1)

    def pt(i, j):
        return radius * np.array([math.sin(th[i]) * math.cos(ph[j]), math.sin(th[i]) * math.sin(ph[j]), math.cos(th[i])])
    tris = []
    for i in range(rings):
        for j in range(seg):
            a, b, c, d = pt(i, j), pt(i + 1, j), pt(i + 1, j + 1), pt(i, j + 1)
            tris += [[a, b, c], [a, c, d]]  # (at the poles one of the two has zero area: the measure takes it)
    tris = np.array(tris)
    reps = -(-M // len(tris))
    return np.concatenate([tris] * reps)[:M]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nodes", type=int, default=64)
    ap.add_argument("--triangles", type=int, default=4096)
    ap.add_argument("--robot-nodes", type=int, default=64)
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    hc = HipChain(**robot.chain_tables())
    n = a.nodes
    origin, voxel, shape = [-1.28, -1.28, -1.28], 2.56 / (n - 1), (n, n, n)
    mesh = sphere_mesh(a.triangles)
    d_mesh = torch.tensor(mesh, dtype=torch.float64, device="cuda")
    pairs = n ** 3 * len(mesh)
    bound = int(_native.lib().optik_hip_mesh_pairs_per_launch(-1))
    res = {"reps": a.reps, "shape": list(shape), "triangles": len(mesh), "pairs": pairs, "pairs_per_launch": bound,
           "launches": -(-n ** 3 // max(1, bound // len(mesh)))}

    def field():
        return hc.world_grid_from_mesh(origin, voxel, shape, d_mesh)

    def split():
        with _native.mesh_pairs_per_launch(max(1, bound // 16)):
            return hc.world_grid_from_mesh(origin, voxel, shape, d_mesh)

    rn = a.robot_nodes
    r_voxel, r_shape = 2.56 / (rn - 1), (rn, rn, rn)
    calls = {"field": lambda: timed(field), "split": lambda: timed(split),
             "robot": lambda: once(lambda: robot.set_world_mesh(origin, r_voxel, r_shape, mesh))}
    times = {c: [] for c in calls}
    outs = {}
    for rep in range(a.reps + 1):  # (the first round warms up)
        for c, fn in calls.items():
            dt, out = fn()
            outs[c] = out
            if rep:
                times[c].append(dt)
    for c, t in times.items():
        res[c] = stats(t)
    for c in ("field", "split"):
        res[c]["pairs_per_s"] = pairs / (res[c]["median_ms"] * 1e-3)
    res["split_equals_field"] = bool(torch.equal(outs["field"].view(torch.int32), outs["split"].view(torch.int32)))
    res["inside_nodes"] = int((outs["field"] < 0).sum())
    robot.clear_world_grid()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
