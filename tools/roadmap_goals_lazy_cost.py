#!/usr/bin/env python3
"""Cost of "the world changed, then plan to goal sets" three ways, on the scene of
tools/roadmap_cost.py: a Panda with the model and world of tools/collision_cost.py, N = 8192 nodes, k = 16.

  eager      HipChain.roadmap_build (every node's neighbours, every edge checked) + HipChain.roadmap_plan_goals
  lazy_all   HipChain.roadmap_lazy_reset + HipChain.roadmap_plan_goals_lazy with every pass on all Q queries
  lazy_live  the same with every pass after the first on the live queries only (what the public layers do)

for Q = 1, 64 and 1024 random starts with G = 8 random goals each, ks = kg = 16, Lmax = 64, rounds = 4096.  The three
run interleaved in one process, --reps rounds after one warm-up round; each figure is the median wall time of the pair
of calls as a user makes them, with [min, max] beside it.  The plans are compared: status 0, 1 and 3 must equal the
eager plan bit for bit, and the two lazy forms each other in everything.  Outside the timed region the loop is run
again with rounds = 0, 1, 2, ... to count the live queries after every pass (status 2 or 4 when the loop is cut
there).  One JSON line per Q, and the compiler's resource line of the new kernels.  No ratio is promised and none is
set here: what is printed is what was measured."""
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

KEYS = ("status", "len", "which", "cost", "path")


def same(a, b, key, cols=None):
    x, y = (a[key], b[key]) if cols is None else ((a[key][:, cols], b[key][:, cols]) if key == "path" else
                                                   (a[key][cols], b[key][cols]))
    if x.dtype == torch.float64:
        return bool(torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64)))
    return bool(torch.equal(x, y))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nodes", type=int, default=8192)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--goals", type=int, default=8)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--rounds", type=int, default=4096)
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    hc = HipChain(**robot.chain_tables())
    S = filtered(robot, hc)
    N, k, h, G = a.nodes, a.k, a.resolution, a.goals
    nodes = hc.seed_batch(1, N)
    rm = hc.roadmap_build_lazy(nodes, k, h)
    for Q in a.queries:
        starts = hc.seed_batch(1 + N, Q)
        goals = hc.seed_batch(1 + N + Q, G * Q).reshape(hc.n, G, Q).permute(1, 0, 2).contiguous()
        gcount = torch.full((Q,), G, dtype=torch.int32, device=starts.device)

        def eager():
            nbr, w = hc.roadmap_build(nodes, k, h)
            return hc.roadmap_plan_goals((nodes, nbr, w), starts, goals, gcount, k, 64, h)

        def lazy(skip, rounds=a.rounds):
            hc.roadmap_lazy_reset(rm)
            return hc.roadmap_plan_goals_lazy(rm, starts, goals, gcount, k, 64, rounds, _skip_settled=skip)

        calls = {"eager": eager, "lazy_all": lambda: lazy(False), "lazy_live": lambda: lazy(True)}
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
        res = {"spheres": S, "nodes": N, "k": k, "queries": Q, "goals": G, "resolution": h, "reps": a.reps}
        for name, ts in times.items():
            res[name] = {"ms": round(float(np.median(ts)) * 1e3, 3),
                         "min_max_ms": [round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)]}
        e, z, y = out["eager"], out["lazy_live"], out["lazy_all"]
        res["rounds_used"], res["checked"] = z["rounds"], z["checked"]
        res["checked_fraction"] = round(z["checked"] / float(N * k), 5)
        res["lazy_status_counts"] = [int((z["status"] == s).sum()) for s in range(5)]
        settled = (z["status"] != 2) & (z["status"] != 4)
        res["settled_plans_equal_eager"] = all(same(z, e, key, settled) for key in KEYS)
        res["lazy_forms_equal"] = bool(all(same(z, y, key) for key in KEYS)
                                       and (z["rounds"], z["checked"]) == (y["rounds"], y["checked"]))
        # the live queries after pass 1, 2, ...: the loop cut after r rounds leaves them as status 2 or 4
        live = []
        for r in range(z["rounds"] + 1):
            cut = lazy(True, r)
            live.append(int(((cut["status"] == 2) | (cut["status"] == 4)).sum()))
        res["live_after_pass"] = live
        res["queries_planned"] = {"lazy_all": Q * (z["rounds"] + 1), "lazy_live": Q + sum(live[:-1])}
        print(json.dumps(res))
    for name, r in sorted(build.kernel_resources().items()):
        if name.startswith(("goals_lazy_", "roadmap_query_goals_kernel")):
            print("# %s: %d VGPR, %d AGPR, %d B scratch, %d B LDS, %d waves/SIMD"
                  % (name, r["vgpr"], r["agpr"], r["scratch"], r["lds"], r["occupancy"]))


if __name__ == "__main__":
    main()
