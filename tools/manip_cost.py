#!/usr/bin/env python3
"""Cost of the manipulability / condition solution modes: the key pass that follows the solve
(manip_key_kernel / wide_manip_key_kernel) against the solve kernels, the end-to-end call time of Quality and
Manipulability on the same shape, and the rate of optik_hip_manip_batch.

  panda_T4096_R256   HipChain.ik_batch, 4096 targets x 256 restarts (one launch)
  panda_T1_R1M       HipChain.ik_batch, one target x 2^20 restarts (one launch)
  arm10_T256_R256    HipChain.ik_batch on the general solver, 256 targets x 256 restarts
  batch              HipChain.manip_batch at B = 2^20 on the Panda and the UR3e: configurations / s

Each shape runs --reps times per mode after one warm-up call; the wall times are medians (one JSON line).  The kernel
times come from a kernel trace of this process, in a run of its own:

    rocprofv3 --kernel-trace --stats -d OUTDIR -o manip -- python tools/manip_cost.py --shape panda_T4096_R256"""
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

ROBOTS = {
    "panda": (os.path.join(ROOT, "optik_amd", "robots", "panda.urdf"), "panda_link0", "panda_link8"),
    "ur3e": (os.path.join(ROOT, "tests", "golden", "reference", "ur3e.urdf"), "ur_base_link", "ur_ee_link"),
    "arm10": (os.path.join(ROOT, "tests", "golden", "robots", "arm10.urdf"), "l0", "l11"),
}
SHAPES = {"panda_T4096_R256": ("panda", 4096, 256), "panda_T1_R1M": ("panda", 1, 1 << 20),
          "arm10_T256_R256": ("arm10", 256, 256)}


def _robot(name):
    path, base, ee = ROBOTS[name]
    if not os.path.exists(path):  # (ur3e: the reference fixture's copy)
        raise SystemExit(f"{path} is missing")
    return Robot.from_urdf_file(path, base, ee)


def solve_shape(name, T, R, reps):
    robot = _robot(name)
    hc = robot.hip_chain()
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(1)
    q = rng.uniform(lb, ub, size=(T, len(lb)))
    tg = hc.fk_batch(torch.tensor(q.T.copy(), dtype=torch.float64, device="cuda")).T.contiguous()
    x0 = torch.tensor(rng.uniform(lb, ub, size=(T, len(lb))), dtype=torch.float64, device="cuda")
    out = {}
    for mode in ("quality", "manipulability", "condition"):
        cfg = nat.make_config(solution_mode=mode)
        times, found = [], 0
        for rep in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = hc.ik_batch(cfg, tg, x0, 0, R, per_restart=False)
            torch.cuda.synchronize()
            if rep:
                times.append(time.perf_counter() - t0)
            found = int((res["win_idx"] >= 0).sum())
        out[mode] = dict(ms=1e3 * float(np.median(times)), found=found)
    return out


def batch_rate(reps):
    out = {}
    for name in ("panda", "ur3e"):
        robot = _robot(name)
        hc = robot.hip_chain()
        lb, ub = (np.array(v) for v in robot.joint_limits())
        B = 1 << 20
        q = torch.tensor(np.random.default_rng(2).uniform(lb, ub, size=(B, len(lb))).T.copy(), dtype=torch.float64,
                         device="cuda")
        times = []
        for rep in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hc.manip_batch(q)
            torch.cuda.synchronize()
            if rep:
                times.append(time.perf_counter() - t0)
        out[name] = dict(B=B, ms=1e3 * float(np.median(times)), per_s=B / float(np.median(times)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", choices=sorted(SHAPES) + ["batch", "all"], default="all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    res = {}
    for s in (sorted(SHAPES) if a.shape == "all" else [a.shape] if a.shape != "batch" else []):
        res[s] = solve_shape(*SHAPES[s], a.reps)
    if a.shape in ("batch", "all"):
        res["manip_batch"] = batch_rate(a.reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
