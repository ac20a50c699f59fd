#!/usr/bin/env python3
"""Cost of the clearance witnesses and of collision-avoiding diff_ik, at B = 2^20 Panda
configurations with the model and world of tools/collision_cost.py (36 spheres on 3 frames, "auto" pairs; 64 spheres
and 16 boxes):

  collision_batch            HipChain.collision_batch          configurations / s
  collision_witness_batch    HipChain.collision_witness_batch  (dist, grad and witness)
  diff_ik_batch              HipChain.diff_ik_batch
  diff_ik_avoid_batch        HipChain.diff_ik_avoid_batch      (influence 0.2, safety 0.02)

The four calls run interleaved in one process, --reps rounds after one warm-up round; each rate is B over the median
wall time of a call (6 .. 35 ms each; the HipChain call as a user makes it, so the allocation of its output tensors
is inside), with [min, max] beside it.  One JSON line, and the compiler's resource line of the two new
kernels (python -m optik_amd.build --resources has all of them)."""
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

from collision_cost import PANDA, filtered  # noqa: E402
from optik_amd import Robot, build  # noqa: E402
from optik_amd.device import HipChain  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--log2-b", type=int, default=20)
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    hc = HipChain(**robot.chain_tables())
    S = filtered(robot, hc)
    lb, ub = (np.array(v) for v in robot.joint_limits())
    B = 1 << a.log2_b
    rng = np.random.default_rng(2)
    dev = dict(dtype=torch.float64, device="cuda")
    q = torch.tensor(rng.uniform(lb, ub, size=(B, 7)).T.copy(), **dev)
    V = torch.tensor((rng.normal(size=(B, 6)) * 0.3).T.copy(), **dev)
    vm = torch.tensor(rng.uniform(0.5, 2.0, size=(B, 7)).T.copy(), **dev)
    calls = {"collision_batch": lambda: hc.collision_batch(q),
             "collision_witness_batch": lambda: hc.collision_witness_batch(q),
             "diff_ik_batch": lambda: hc.diff_ik_batch(q, V, vm),
             "diff_ik_avoid_batch": lambda: hc.diff_ik_avoid_batch(q, V, vm, 0.2, 0.02)}
    times = {k: [] for k in calls}
    out = {}
    for rep in range(a.reps + 1):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[name] = fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
    res = {"spheres": S, "B": B, "reps": a.reps}
    for name, ts in times.items():
        res[name] = {"configs_per_s": round(B / float(np.median(ts))),
                     "min_max": [round(B / max(ts)), round(B / min(ts))]}
    dist = out["collision_witness_batch"][0]
    res["rows_within_influence"] = round(float((dist < 0.2).sum(0).clamp(max=4).double().mean()), 3)
    res["avoid_solved_fraction"] = round(float((out["diff_ik_avoid_batch"][2] == 0).double().mean()), 4)
    print(json.dumps(res))
    for name, r in sorted(build.kernel_resources().items()):
        if name.startswith(("collision_witness_kernel<7, true", "diff_ik_avoid_kernel<7, true",
                            "collision_batch_kernel<7, true", "diff_ik_batch_kernel<7, true")):
            print("# %s: %d VGPR, %d AGPR, %d B scratch, %d B LDS, %d waves/SIMD"
                  % (name, r["vgpr"], r["agpr"], r["scratch"], r["lds"], r["occupancy"]))


if __name__ == "__main__":
    main()
