#!/usr/bin/env python3
"""Cost of goal-set planning on the scene of tools/roadmap_cost.py (a Panda with 36 spheres on
3 frames, 64 world spheres and 16 boxes), N = 8192 nodes, k = 16, Q = 1024 queries of G = 8 goals each, ks = kg = 16,
Lmax = 64:

  plan_goals           HipChain.roadmap_plan_goals: the neighbours, links and direct motions of all G * Q goals in one
                       batch each, then ONE goal-set query per start
  plan_each_then_min   what a caller did before: G HipChain.roadmap_plan calls on the same tensors, one per goal slot,
                       and torch.min over the G costs

The two run interleaved in one process, --reps rounds after one warm-up round; each figure is the median wall time
of a call with [min, max] beside it.  The costs of the two must be equal bit for bit (the theorem of section 5.25),
and the tool says so.  The search and edge work is the same on both sides; the difference is G queries against one,
whose sweep count depends on the data.  --profile runs one round of each and nothing else: under
`rocprofv3 --kernel-trace --stats -- python tools/roadmap_goals_cost.py --profile` the query kernels' own times are
in the statistics (roadmap_query_goals_kernel once, roadmap_query_kernel G times).  One JSON line, and the
compiler's resource line of the query kernels."""
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
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--goals", type=int, default=8)
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--profile", action="store_true", help="one round of each call, no timing (for rocprofv3)")
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    hc = HipChain(**robot.chain_tables())
    S = filtered(robot, hc)
    N, k, Q, G, h = a.nodes, a.k, a.queries, a.goals, a.resolution
    nodes = hc.seed_batch(1, N)
    starts = hc.seed_batch(1 + N, Q)
    goals = hc.seed_batch(1 + N + Q, G * Q).reshape(7, G, Q).permute(1, 0, 2).contiguous()  # [G, n, Q]
    each = [goals[g].contiguous() for g in range(G)]
    gcount = torch.full((Q,), G, dtype=torch.int32, device=nodes.device)
    nbr, _ = hc.roadmap_knn(nodes, nodes, k, exclude_self=True)
    w = hc.roadmap_edges(nodes, nodes, nbr, h)
    rm = (nodes, nbr, w)

    def plan_each_then_min():
        plans = [hc.roadmap_plan(rm, starts, each[g], k, 64, h) for g in range(G)]
        cost, which = torch.min(torch.stack([p["cost"] for p in plans]), dim=0)
        return dict(cost=cost, which=which, plans=plans)

    calls = {"plan_goals": lambda: hc.roadmap_plan_goals(rm, starts, goals, gcount, k, 64, h),
             "plan_each_then_min": plan_each_then_min}
    times = {name: [] for name in calls}
    out = {}
    for rep in range(2 if a.profile else a.reps + 1):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[name] = fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
    res = {"spheres": S, "nodes": N, "k": k, "queries": Q, "goals": G, "resolution": h,
           "reps": 1 if a.profile else a.reps, "profile_run": bool(a.profile)}
    for name, ts in times.items():
        res[name] = {"ms": round(float(np.median(ts)) * 1e3, 3),
                     "min_max_ms": [round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)]}
    res["plan_goals_over_plan_each"] = round(res["plan_goals"]["ms"] / res["plan_each_then_min"]["ms"], 3)
    got, base = out["plan_goals"], out["plan_each_then_min"]
    res["costs_equal_bitwise"] = bool(torch.equal(got["cost"].view(torch.int64), base["cost"].view(torch.int64)))
    res["status_counts"] = [int((got["status"] == s).sum()) for s in range(4)]
    found = got["status"] == 0
    res["mean_waypoints_found"] = round(float(got["len"][found].double().mean()), 2) if bool(found.any()) else None
    res["reached_goal_counts"] = [int((got["which"] == g).sum()) for g in range(G)]
    print(json.dumps(res))
    for name, r in sorted(build.kernel_resources().items()):
        if name.startswith(("roadmap_query_goals_kernel", "roadmap_query_kernel")):
            print("# %s: %d VGPR, %d AGPR, %d B scratch, %d B LDS, %d waves/SIMD"
                  % (name, r["vgpr"], r["agpr"], r["scratch"], r["lds"], r["occupancy"]))


if __name__ == "__main__":
    main()
