#!/usr/bin/env python3
"""Cost of the solution-set stage of HipChain.ik_solutions next to the solve kernel it follows, on the Panda, for the
two shapes of DESIGN.md section 5.9: T = 1024 targets x R = 4096 restarts (one 4 M-item launch, one tile per target:
ik_solutions_small_kernel) and T = 1 x R = 2^20 (256 tiles: ik_solutions_tile_kernel + ik_solutions_pick_kernel per
round), both K = 8, min_dist = 0.1, Quality.  Each shape runs --reps times after one warm-up call.  The kernel times
come from a kernel trace of this process:

    rocprofv3 --kernel-trace --stats -d OUTDIR -o sol -- python tools/ik_solutions_cost.py

Without the profiler it prints the wall time per call and the solution counts (one JSON line)."""
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

SHAPES = {"T1024_R4096": (1024, 4096), "T1_R1M": (1, 1 << 20)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--min-dist", type=float, default=0.1)
    args = ap.parse_args()
    robot = Robot.from_urdf_file(os.path.join(ROOT, "optik_amd", "robots", "panda.urdf"), "panda_link0", "panda_link8")
    hc = robot.hip_chain()
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(0)
    cfg = nat.make_config(solution_mode="quality")
    res = {}
    for name, (T, R) in SHAPES.items():
        q = torch.tensor(rng.uniform(lb, ub, size=(T, len(lb))).T.copy(), dtype=torch.float64, device="cuda")
        tgd = hc.fk_batch(q).T.contiguous()  # reachable targets [T, 7]
        x0d = torch.tensor(rng.uniform(lb, ub, size=(T, len(lb))), dtype=torch.float64, device="cuda")
        out = hc.ik_solutions(cfg, tgd, x0d, 0, R, args.k, args.min_dist)  # warm-up (workspace, code objects)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            out = hc.ik_solutions(cfg, tgd, x0d, 0, R, args.k, args.min_dist, bufs=out)
        torch.cuda.synchronize()
        cnt = out["count"].cpu().numpy()
        res[name] = {"T": T, "R": R, "K": args.k, "min_dist": args.min_dist,
                     "ms_per_call": (time.perf_counter() - t0) / args.reps * 1e3,
                     "mean_count": float(cnt.mean()), "targets_with_K": int((cnt == args.k).sum())}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
