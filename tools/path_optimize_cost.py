#!/usr/bin/env python3
"""Cost of the path optimiser at P = 4096 Panda paths of L = 64 waypoints with the model and
world of tools/collision_cost.py (36 spheres on 3 frames, "auto" pairs; 64 spheres and 16 boxes):

  path_optimize              HipChain.path_optimize, `iters` updates = iters + 1 evaluations in one launch
  collision_witness_batch    HipChain.collision_witness_batch on the same P x L configurations, iters + 1 rounds:
                             what a caller who runs the optimiser's loop on the host would launch for the rows alone

The two run interleaved in one process, --reps rounds after one warm-up round; each figure is from the median wall
time of a call (the HipChain call as a user makes it), with [min, max] beside it.  An evaluation is one waypoint's FK,
distance pass and row gradients: P * L * (iters + 1) per call on both sides.  One JSON line, and the compiler's
resource line of the kernels."""
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
    ap.add_argument("--paths", type=int, default=4096)
    ap.add_argument("--waypoints", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    hc = HipChain(**robot.chain_tables())
    S = filtered(robot, hc)
    lb, ub = (np.array(v) for v in robot.joint_limits())
    P, L, K = a.paths, a.waypoints, a.iters
    rng = np.random.default_rng(2)
    ends = rng.uniform(lb, ub, size=(2, P, 7))
    s = np.linspace(0.0, 1.0, L)[:, None, None]
    q = torch.tensor((1.0 - s) * ends[0][None] + s * ends[1][None], dtype=torch.float64, device="cuda")  # [L, P, 7]
    flat = q.reshape(L * P, 7).T.contiguous()
    # (a step small enough for L = 64: the rows of Ainv sum to about L^2 / 8)
    calls = {"path_optimize": lambda: hc.path_optimize(q, K, 1e-4, 1.0, 1.0, 0.2, 0.02),
             "collision_witness_batch": lambda: [hc.collision_witness_batch(flat) for _ in range(K + 1)]}
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
    evals = P * L * (K + 1)
    res = {"spheres": S, "paths": P, "waypoints": L, "iters": K, "reps": a.reps}
    for name, ts in times.items():
        med = float(np.median(ts))
        res[name] = {"ms": round(med * 1e3, 3), "evaluations_per_s": round(evals / med),
                     "min_max": [round(evals / max(ts)), round(evals / min(ts))]}
    res["path_optimize"]["paths_per_s"] = round(P / float(np.median(times["path_optimize"])))
    res["fused_over_separate_per_evaluation"] = round(
        float(np.median(times["path_optimize"])) / float(np.median(times["collision_witness_batch"])), 3)
    po = out["path_optimize"]
    res["F_obs_first_last"] = [round(float(po["cost_first"][:, 2].mean()), 5), round(float(po["cost_last"][:, 2].mean()), 5)]
    res["status_ok_fraction"] = round(float((po["status"] == 0).double().mean()), 4)
    print(json.dumps(res))
    for name, r in sorted(build.kernel_resources().items()):
        if name.startswith(("path_optimize_kernel<7, true", "collision_witness_kernel<7, true")):
            print("# %s: %d VGPR, %d AGPR, %d B scratch, %d B LDS, %d waves/SIMD"
                  % (name, r["vgpr"], r["agpr"], r["scratch"], r["lds"], r["occupancy"]))


if __name__ == "__main__":
    main()
