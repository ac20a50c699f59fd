#!/usr/bin/env python3
"""Cost of the distance-field world against the primitives path it stands beside, which is
the parent's code: the baseline of every figure here is a world of spheres and boxes, not the grid against itself.

The model is spheres_along_chain(panda, 0.05, 12) (36 spheres on 3 frames, "auto" pairs), margin 0.  The worlds:

  a        section 5.12's scene: 64 spheres and 16 boxes around the arm (seeded)
  b        --boxes oriented boxes (default 2048) in the same volume
  a_grid   scene a baked at 128^3 (voxel 0.02 over [-1.28, 1.26]^3), the primitives removed
  b_grid   scene b baked likewise
  none     no world at all (the model's self pairs alone): the floor both paths stand on
  sN / bN  the first N spheres / boxes of scene a / b, N = 1 .. 64: where the grid overtakes the primitives

  batch    HipChain.collision_batch at B = 2^20 in every world, interleaved in one process: per repetition each world
           is installed and timed once, so drift hits all of them alike; medians of --reps with [min, max]
  bake     HipChain.bake_world_grid of scenes a and b at 128^3
  key      HipChain.ik_batch, Quality, T = 4096 x R = 256, without a model, with scene a and with a_grid, interleaved:
           the key pass is the difference to the call without a model

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

from optik_amd import Robot  # noqa: E402
from optik_amd import _native as nat  # noqa: E402
from optik_amd.collision import spheres_along_chain  # noqa: E402
from optik_amd.device import HipChain  # noqa: E402

PANDA = (os.path.join(ROOT, "optik_amd", "robots", "panda.urdf"), "panda_link0", "panda_link8")
ORIGIN, VOXEL, SHAPE = [-1.28, -1.28, -1.28], 0.02, (128, 128, 128)


def world_a(seed=0):
    """tools/collision_cost.py's world."""
    rng = np.random.default_rng(seed)
    sph = np.concatenate([rng.uniform(-0.9, 0.9, (64, 3)), rng.uniform(0.03, 0.1, (64, 1))], 1)
    q = rng.normal(size=(16, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    box = np.concatenate([rng.uniform(-0.9, 0.9, (16, 3)), q, rng.uniform(0.02, 0.1, (16, 3))], 1)
    return sph, box


def world_b(count, seed=1):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(count, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate([rng.uniform(-0.9, 0.9, (count, 3)), q, rng.uniform(0.005, 0.02, (count, 3))], 1)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def stats(times):
    return {"median_ms": round(float(np.median(times)) * 1e3, 3), "min_ms": round(min(times) * 1e3, 3),
            "max_ms": round(max(times) * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--boxes", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--skip-key", action="store_true")
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    tables = robot.chain_tables()
    frames, centers, radii = spheres_along_chain(robot, 0.05, 12)
    hc = HipChain(**tables)
    hc.set_collision_model(frames, centers, radii, self_pairs="auto", margin=0.0)
    sph_a, box_a = world_a()
    box_b = world_b(a.boxes)
    res = {"spheres": len(frames), "grid": {"origin": ORIGIN, "voxel": VOXEL, "shape": list(SHAPE)}, "reps": a.reps}

    # the bakes (and their times)
    grids, bake = {}, {}
    for name, prims in (("a", (sph_a, box_a)), ("b", (None, box_b))):
        hc.set_world(*prims)
        hc.bake_world_grid(ORIGIN, VOXEL, SHAPE)  # (warm-up)
        times = []
        for _ in range(a.reps):
            dt, field = once(lambda: hc.bake_world_grid(ORIGIN, VOXEL, SHAPE))
            times.append(dt)
        grids[name] = field.cpu().numpy()
        bake[name] = dict(stats(times), obstacles=int(sum(len(p) for p in prims if p is not None)))
    res["bake"] = bake

    # collision_batch in every world, interleaved
    worlds = [("none", (None, None), None), ("a", (sph_a, box_a), None), ("a_grid", (None, None), grids["a"]),
              ("b", (None, box_b), None), ("b_grid", (None, None), grids["b"])]
    for n in (1, 2, 4, 8, 16, 32, 64):
        worlds.append((f"s{n}", (sph_a[:n], None), None))
        worlds.append((f"b{n}", (None, box_b[:n]), None))
    lb, ub = (np.array(v) for v in robot.joint_limits())
    B = a.batch
    q = torch.tensor(np.random.default_rng(2).uniform(lb, ub, size=(B, 7)).T.copy(), dtype=torch.float64, device="cuda")

    def install(prims, grid):
        hc.set_world(*prims)
        if grid is None:
            hc.clear_world_grid()
        else:
            hc.set_world_grid(ORIGIN, VOXEL, grid)

    times = {name: [] for name, _, _ in worlds}
    free = {}
    for rep in range(a.reps + 1):
        for name, prims, grid in worlds:
            install(prims, grid)
            dt, (clr, fr) = once(lambda: hc.collision_batch(q))
            if rep:
                times[name].append(dt)
            else:
                free[name] = round(float(fr.float().mean()), 4)
    res["batch"] = {name: dict(stats(t), configs_per_s=round(B / float(np.median(t))), free_fraction=free[name])
                    for name, t in times.items()}
    res["batch"]["B"] = B

    # the key pass: the filtered call against the call without a model
    if not a.skip_key:
        T, R = 4096, 256
        plain = HipChain(**tables)
        rng = np.random.default_rng(1)
        tg = plain.fk_batch(torch.tensor(rng.uniform(lb, ub, size=(T, 7)).T.copy(), dtype=torch.float64,
                                         device="cuda")).T.contiguous()
        x0 = torch.tensor(rng.uniform(lb, ub, size=(T, 7)), dtype=torch.float64, device="cuda")
        cfg = nat.make_config(solution_mode="quality")
        variants = [("plain", plain, None), ("a", hc, ((sph_a, box_a), None)), ("a_grid", hc, ((None, None), grids["a"]))]
        ktimes = {name: [] for name, _, _ in variants}
        found = {}
        for rep in range(a.reps + 1):
            for name, chain, setup in variants:
                if setup:
                    install(*setup)
                dt, out = once(lambda: chain.ik_batch(cfg, tg, x0, 0, R, per_restart=False))
                if rep:
                    ktimes[name].append(dt)
                else:
                    found[name] = int((out["win_idx"] >= 0).sum().item())
        res["key"] = {name: dict(stats(t), found=found[name]) for name, t in ktimes.items()}
        res["key"]["T"], res["key"]["R"] = T, R
    print(json.dumps(res))


if __name__ == "__main__":
    main()
