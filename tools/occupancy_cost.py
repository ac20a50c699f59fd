#!/usr/bin/env python3
"""Cost of the way from sensor data to a distance-field world.  The capability is new, so
nothing here is a comparison with the parent; the context figures are the bake of the same scene from its primitives
(section 5.14) and scipy.ndimage.distance_transform_edt on the host, which is what a user would run without it.

The scene is section 5.12's (tools/grid_cost.py: world_a, 64 spheres and 16 boxes), rasterised as bake <= 0 at 128^3
(voxel 0.02) and 256^3 (voxel 0.01) over the same volume.  Per grid, interleaved in one process, medians of --reps with
[min, max]:

  transform   HipChain.world_grid_from_occupancy of that occupancy (device buffers, default max_distance)
  voxelize    HipChain.occupancy_from_points of N = 2^20 points on the scene's occupied voxels, with the Panda model's
              36 spheres (spheres_along_chain(panda, 0.05, 12)) as exclusion spheres
  points      Robot.set_world_points of the same cloud, end to end from host arrays (copies and installation included)
  bake        HipChain.bake_world_grid of the scene's primitives
  scipy       distance_transform_edt of the occupancy and of its complement (the signed field needs both), on the host
  worst       the transform of a grid with ONE occupied node: every scan runs the whole line

One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from grid_cost import PANDA, once, stats, world_a  # noqa: E402
from optik_amd import Robot  # noqa: E402
from optik_amd.collision import spheres_along_chain, spheres_at  # noqa: E402
from optik_amd.device import HipChain  # noqa: E402

ORIGIN = [-1.28, -1.28, -1.28]
GRIDS = {"128": (0.02, (128, 128, 128)), "256": (0.01, (256, 256, 256))}


def host_once(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--skip-scipy", action="store_true")
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    frames, centers, radii = spheres_along_chain(robot, 0.05, 12)
    robot.set_collision_model(frames, centers, radii, self_pairs="auto", margin=0.0)
    hc = HipChain(**robot.chain_tables())
    sph, box = world_a()
    hc.set_world(sph, box)
    lb, ub = (np.array(v) for v in robot.joint_limits())
    exclude = spheres_at(robot, 0.5 * (lb + ub), frames, centers, radii, pad=0.02)
    d_exclude = torch.tensor(exclude, dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(3)
    res = {"reps": a.reps, "points": a.points, "exclusion_spheres": len(exclude)}

    scenes = {}
    for name, (voxel, shape) in GRIDS.items():
        occ = (hc.bake_world_grid(ORIGIN, voxel, shape) <= 0).to(torch.uint8).contiguous()
        idx = torch.nonzero(occ).cpu().numpy()
        pick = idx[rng.integers(len(idx), size=a.points)]
        pts = np.asarray(ORIGIN) + voxel * (pick + rng.uniform(-0.49, 0.49, pick.shape))
        single = torch.zeros(shape, dtype=torch.uint8, device="cuda")
        single[shape[0] // 2, shape[1] // 2, shape[2] // 2] = 1
        scenes[name] = dict(voxel=voxel, shape=shape, occ=occ, pts=pts, single=single,
                            d_pts=torch.tensor(pts, dtype=torch.float64, device="cuda"),
                            into=torch.zeros(shape, dtype=torch.uint8, device="cuda"))
        res[name] = {"voxel": voxel, "shape": list(shape), "occupied_nodes": int(len(idx))}

    calls = {
        "transform": lambda s: once(lambda: hc.world_grid_from_occupancy(s["voxel"], s["occ"])),
        "voxelize": lambda s: once(lambda: hc.occupancy_from_points(ORIGIN, s["voxel"], s["shape"], s["d_pts"],
                                                                    d_exclude, into=s["into"])),
        "points": lambda s: once(lambda: robot.set_world_points(ORIGIN, s["voxel"], s["shape"], s["pts"], exclude)),
        "bake": lambda s: once(lambda: hc.bake_world_grid(ORIGIN, s["voxel"], s["shape"])),
        "worst": lambda s: once(lambda: hc.world_grid_from_occupancy(s["voxel"], s["single"])),
    }
    times = {(g, c): [] for g in scenes for c in calls}
    for rep in range(a.reps + 1):  # (the first round warms up: workspace growth, first launches)
        for g, s in scenes.items():
            for c, fn in calls.items():
                dt, _ = fn(s)
                if rep:
                    times[(g, c)].append(dt)
    for (g, c), t in times.items():
        res[g][c] = stats(t)
    robot.clear_world_grid()

    if not a.skip_scipy:
        try:
            from scipy.ndimage import distance_transform_edt
        except ImportError:
            distance_transform_edt = None
        for g, s in scenes.items():
            if distance_transform_edt is None:
                res[g]["scipy"] = None
                continue
            occ = s["occ"].cpu().numpy().astype(bool)
            reps = a.reps if g == "128" else 1
            one, both = [], []
            for _ in range(reps):
                t1, _ = host_once(lambda: distance_transform_edt(~occ))
                t2, _ = host_once(lambda: distance_transform_edt(occ))
                one.append(t1)
                both.append(t1 + t2)
            res[g]["scipy"] = {"one_sided": stats(one), "signed": stats(both), "reps": reps}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
