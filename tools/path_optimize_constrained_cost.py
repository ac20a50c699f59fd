#!/usr/bin/env python3
"""Cost of path optimisation under a pose constraint against path_optimize on the same paths
and parameters: P = 1024 Panda paths of L = 32 waypoints in the scene of examples/optimize_constrained.py (the
6-sphere model, the wall), the box upright(fk(START), TILT), the example's ITERS updates at its STEP.

The paths: lines from START to GOAL with the first joint of both ends drawn within +-0.3 rad and 0.01 rad of noise on
every waypoint, resampled onto the constraint with path_resample_constrained, so the input's waypoints satisfy it.

  path_optimize               HipChain.path_optimize (the kernel is the parent commit's, byte for byte)
  path_optimize_constrained   HipChain.path_optimize_constrained

The two run interleaved in one process, --reps rounds after one warm-up round; each figure is the median wall time of
a call as a user makes it (it allocates its outputs), with [min, max].  The Gauss-Newton iterations per projection are
counted in a pass of their own, not timed: the constrained iterate is advanced one update per launch, and at each
iterate path_optimize's own update of it is projected with constraint_project_batch, which reports its iterations --
the projections the fused kernel makes.  One JSON line, and the compiler's resource lines of the two kernels."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

from optik_amd import Robot, build  # noqa: E402
from optimize_constrained import ITERS, PTOL, STEP  # noqa: E402
from plan_rrt_constrained import GOAL, START, setup  # noqa: E402

PANDA = (os.path.join(ROOT, "optik_amd", "robots", "panda.urdf"), "panda_link0", "panda_link8")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--paths", type=int, default=1024)
    ap.add_argument("--waypoints", type=int, default=32)
    ap.add_argument("--iters", type=int, default=ITERS)
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    _, _, c = setup(robot)
    hc = robot._device_chain()  # (the robot's own chain: it carries the model and the wall)
    P, L, K = a.paths, a.waypoints, a.iters
    rng = np.random.default_rng(2)
    ends = np.stack([np.tile(START, (P, 1)), np.tile(GOAL, (P, 1))])
    ends[:, :, 0] += rng.uniform(-0.3, 0.3, size=(2, P))
    s = np.linspace(0.0, 1.0, L)[:, None, None]
    lines = (1.0 - s) * ends[0][None] + s * ends[1][None] + rng.normal(size=(L, P, 7)) * 0.01
    lines[0], lines[-1] = ends[0], ends[1]
    q, st, _ = hc.path_resample_constrained(torch.tensor(lines, dtype=torch.float64, device="cuda"), None, c, L, PTOL)
    prm = (K, STEP, 1.0, 1.0, 0.2, 0.05)
    calls = {"path_optimize": lambda: hc.path_optimize(q, *prm),
             "path_optimize_constrained": lambda: hc.path_optimize_constrained(q, c, *prm, ptol=PTOL)}
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
    res = {"paths": P, "waypoints": L, "iters": K, "step": STEP, "reps": a.reps,
           "resampled_status_0": int((st == 0).sum())}
    for name, ts in times.items():
        res[name] = {"ms": round(float(np.median(ts)) * 1e3, 3),
                     "min_max_ms": [round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)]}
    res["constrained_over_plain"] = round(float(np.median(times["path_optimize_constrained"]))
                                          / float(np.median(times["path_optimize"])), 3)
    con, plain = out["path_optimize_constrained"], out["path_optimize"]
    res["projections"] = [int(v) for v in con["projected"].sum(dim=1).tolist()]
    res["violation_max"] = {"constrained": float(con["violation"].max()),
                            "plain": float(hc.path_optimize_constrained(plain["q"], c, 0, *prm[1:])["violation"].max())}
    res["clearance_min"] = {"constrained": float(con["clearance"].min()), "plain": float(plain["clearance"].min())}
    res["F_obs_mean"] = {"first": float(con["cost_first"][:, 2].mean()), "constrained": float(con["cost_last"][:, 2].mean()),
                         "plain": float(plain["cost_last"][:, 2].mean())}
    # the iterations of the projections, replayed one update at a time (not timed)
    it_sum = it_count = 0
    cur = q.clone()
    for _ in range(K):
        stepped = hc.path_optimize(cur, 1, *prm[1:])["q"][1:-1].reshape(-1, 7).T.contiguous()
        p = hc.constraint_project_batch(stepped, c, PTOL)
        it_sum += int(p["iterations"].sum())
        it_count += int(p["iterations"].numel())
        hc.path_optimize_constrained(cur, c, 1, *prm[1:], ptol=PTOL, out=cur)
    res["gauss_newton_iterations_per_projection"] = round(it_sum / max(it_count, 1), 4)
    res["replay_equals_fused"] = bool(torch.equal(cur, con["q"]))
    print(json.dumps(res))
    for name, r in sorted(build.kernel_resources().items()):
        if name.startswith(("path_optimize_kernel<7, true", "path_optimize_constrained_kernel<7, true")):
            print("# %s: %d VGPR, %d AGPR, %d B scratch, %d B LDS, %d waves/SIMD"
                  % (name, r["vgpr"], r["agpr"], r["scratch"], r["lds"], r["occupancy"]))
    robot.clear_collision_model()
    robot.set_world()


if __name__ == "__main__":
    main()
