#!/usr/bin/env python3
"""Cost of "the world changed, then plan" with an eager and with a lazy roadmap, on the
scene of tools/roadmap_cost.py: a Panda with the model and world of tools/collision_cost.py, N = 8192 nodes, k = 16.

  eager   HipChain.roadmap_build (every node's neighbours, every edge checked) + HipChain.roadmap_plan
  lazy    HipChain.roadmap_lazy_reset (the verdicts forgotten) + HipChain.roadmap_plan_lazy

for Q = 1, 64 and 1024 random (start, goal) pairs, ks = 16, Lmax = 64.  The two run interleaved in one process, --reps
rounds after one warm-up round; each figure is the median wall time of the pair of calls as a user makes them, with
[min, max] beside it, and the lazy plan's rounds and checked edges.  The plans are compared: status 0, 1 and 3 must
be equal bit for bit.  One JSON line per Q, and the compiler's resource line of the new kernels.  No ratio is
promised and none is set here: what is printed is what was measured."""
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
    ap.add_argument("--nodes", type=int, default=8192)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--rounds", type=int, default=4096)
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    hc = HipChain(**robot.chain_tables())
    S = filtered(robot, hc)
    N, k, h = a.nodes, a.k, a.resolution
    nodes = hc.seed_batch(1, N)
    rm = hc.roadmap_build_lazy(nodes, k, h)
    for Q in a.queries:
        starts, goals = hc.seed_batch(1 + N, Q), hc.seed_batch(1 + N + Q, Q)

        def eager():
            nbr, w = hc.roadmap_build(nodes, k, h)
            return hc.roadmap_plan((nodes, nbr, w), starts, goals, k, 64, h)

        def lazy():
            hc.roadmap_lazy_reset(rm)
            return hc.roadmap_plan_lazy(rm, starts, goals, k, 64, a.rounds)

        calls = {"eager": eager, "lazy": lazy}
        times = {name: [] for name in calls}
        out = {}
        for rep in range(a.reps + 1):
            for name, fn in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out[name] = fn()
                torch.cuda.synchronize()
                if rep:
                    times[name].append(time.perf_counter() - t0)
        res = {"spheres": S, "nodes": N, "k": k, "queries": Q, "resolution": h, "reps": a.reps}
        for name, ts in times.items():
            res[name] = {"ms": round(float(np.median(ts)) * 1e3, 3),
                         "min_max_ms": [round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)]}
        e, z = out["eager"], out["lazy"]
        res["rounds_used"], res["checked"] = z["rounds"], z["checked"]
        res["checked_fraction"] = round(z["checked"] / float(N * k), 5)
        res["lazy_status_counts"] = [int((z["status"] == s).sum()) for s in range(5)]
        settled = (z["status"] != 2) & (z["status"] != 4)
        res["settled_plans_equal_eager"] = bool(
            torch.equal(z["status"][settled], e["status"][settled]) and torch.equal(z["len"][settled], e["len"][settled])
            and torch.equal(z["cost"][settled].view(torch.int64), e["cost"][settled].view(torch.int64))
            and torch.equal(z["path"][:, settled].view(torch.int64), e["path"][:, settled].view(torch.int64)))
        print(json.dumps(res))
    for name, r in sorted(build.kernel_resources().items()):
        if name.startswith(("lazy_", "roadmap_query_kernel")):
            print("# %s: %d VGPR, %d AGPR, %d B scratch, %d B LDS, %d waves/SIMD"
                  % (name, r["vgpr"], r["agpr"], r["scratch"], r["lds"], r["occupancy"]))


if __name__ == "__main__":
    main()
