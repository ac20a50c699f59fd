#!/usr/bin/env python3
"""Cost of fitting a sphere model to a solid.  The capability is new, so nothing here is a
comparison with the parent, and no time was fixed in advance.

The solid is the cube [-0.5, 0.5]^3 on a --nodes^3 grid over [-0.9, 0.9]^3 (its field from
HipChain.world_grid_from_mesh), sampled at the spacing that gives about 8192 surface points, K = 16.  Medians of --reps
with [min, max], after one warm-up round:

  fit         HipChain.sphere_fit on device buffers, device events around the call: all K rounds
  robot       Robot.fit_spheres of the same cube end to end from host arrays (its own grid: the bounding box grown by
              pad at the same voxel; sampling, field, fit, copies)
  reference   the serial fit_reference of csrc/spherefit_measure.hpp, built with g++ (tests/spherefit_util.py), on the
              input of `fit`, as a process from its input file to its output file -- what `fit` is compared against,
              and it must give the same spheres

Writes profiles/spherefit_cost.txt (--out) and prints one JSON line."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from grid_cost import PANDA, once, stats  # noqa: E402
from mesh_cost import timed  # noqa: E402
from optik_amd import Robot, _native  # noqa: E402
from optik_amd.collision import surface_points  # noqa: E402
from optik_amd.device import HipChain  # noqa: E402
from mesh_util import box_triangles  # noqa: E402
from spherefit_util import build_spherefit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nodes", type=int, default=48)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spherefit_cost.txt"))
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    hc = HipChain(**robot.chain_tables())
    n, K = a.nodes, a.k
    origin, voxel, shape = [-0.9, -0.9, -0.9], 1.8 / (n - 1), (n, n, n)
    tris = box_triangles([-0.5] * 3, [0.5] * 3)
    spacing = math.sqrt(2.0) / 36.0   # 36 subdivisions of a face's diagonal: 12 * 703 = 8436 points
    pts = surface_points(tris, None, spacing)
    pad = 1.01 * (math.sqrt(3.0) * voxel + spacing)
    d_tris = torch.tensor(tris, dtype=torch.float64, device="cuda")
    d_pts = torch.tensor(pts, dtype=torch.float64, device="cuda")
    d_values = hc.world_grid_from_mesh(origin, voxel, shape, d_tris)
    torch.cuda.synchronize()
    values = d_values.cpu().numpy()
    sf = build_spherefit()
    fin, fout = os.path.join(sf.dir, "cost_in.bin"), os.path.join(sf.dir, "cost_out.bin")
    sf.write_input(values, origin, voxel, pts, pad, spacing, K, fin)

    def reference():
        t0 = time.perf_counter()
        subprocess.run([sf.exe, fin, fout], check=True)
        return time.perf_counter() - t0, sf.read_output(fout, K)

    calls = {"fit": lambda: timed(lambda: hc.sphere_fit(d_values, origin, voxel, d_pts, pad, spacing, K)),
             "robot": lambda: once(lambda: robot.fit_spheres(tris, None, count=K, voxel=voxel, pad=pad, spacing=spacing)),
             "reference": reference}
    times = {c: [] for c in calls}
    outs = {}
    for rep in range(a.reps + 1):  # (the first round warms up)
        for c, fn in calls.items():
            dt, out = fn()
            outs[c] = out
            if rep:
                times[c].append(dt)
    res = {"reps": a.reps, "shape": list(shape), "points": len(pts), "K": K, "pad": pad, "slack": spacing,
           "pairs": n ** 3 * len(pts), "pairs_per_launch": int(_native.lib().optik_hip_fit_pairs_per_launch(-1))}
    for c, t in times.items():
        res[c] = stats(t)
    got, want = outs["fit"], outs["reference"]
    res["count"], res["uncovered"] = (int(v) for v in got["count_uncovered"].cpu())
    res["fit_equals_reference"] = bool(np.array_equal(got["chosen"].cpu().numpy(), want["chosen"])
                                       and np.array_equal(got["gains"].cpu().numpy(), want["gains"])
                                       and res["count"] == want["count"] and res["uncovered"] == want["uncovered"])
    res["robot_count"], res["robot_uncovered"] = len(outs["robot"][1]), outs["robot"][2]["uncovered"]
    res["robot_shape"] = list(outs["robot"][2]["shape"])
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("# tools/spherefit_cost.py: the sphere fit on one MI355X (DESIGN.md section 5.27); medians of %d after a "
                 "warm-up round, [min, max], milliseconds\n" % a.reps)
        fh.write("# %s\n" % torch.cuda.get_device_name(0))
        for c in calls:
            fh.write("%-10s %10.3f  [%.3f, %.3f]\n" % (c, res[c]["median_ms"], res[c]["min_ms"], res[c]["max_ms"]))
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
