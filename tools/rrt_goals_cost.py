#!/usr/bin/env python3
"""Cost of the tree planner with a goal set next to what existed before it, on the scene of
tools/rrt_cost.py: a Panda with the model and world of tools/collision_cost.py, iters 1024, step 0.5, max_nodes 512,
poll 32.

  goals   HipChain.rrt_plan_goals at G = 8: the goals are ik_solutions' answers for the poses of Q random
          configurations, seeded at Q random starts (computed once, outside the timing; rows past a pose's count are
          NaN, as ik_solutions leaves them)
  rows    the same goals as 8 Q rows of ONE HipChain.rrt_plan call -- the starts repeated -- and the reduction of its
          8 answers per query on the host: the cheapest found one

for Q = 1, 64 and 1024, interleaved in one process, --reps rounds after one warm-up round; each figure is the median
wall time of the call(s) as a user makes them, with [min, max].  Also: the iterations the host loop launched each way,
and how many queries were found each way.  One JSON line per Q, and the compiler's resource line of the new kernels.
No bar is set here: what is printed is what was measured, including where the new call loses."""
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
from optik_amd import _native as nat  # noqa: E402
from optik_amd.device import HipChain  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def stats(ts):
    return {"ms": round(float(np.median(ts)) * 1e3, 3), "min_max_ms": [round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)]}


def launched(iters_used, status, iters, poll):
    """The iterations the host loop launched: up to the first poll at or after the last query's end."""
    used = int(iters_used.max())
    ended = bool((status != 1).all() or used < iters)
    return min(iters, -(-max(used, 1) // poll) * poll + 1) if ended else iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--goals", type=int, default=8)
    ap.add_argument("--restarts", type=int, default=64)
    ap.add_argument("--min-dist", type=float, default=0.3)
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--iters", type=int, default=1024)
    ap.add_argument("--step", type=float, default=0.5)
    ap.add_argument("--max-nodes", type=int, default=512)
    ap.add_argument("--poll", type=int, default=32)
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    hc = HipChain(**robot.chain_tables())
    S = filtered(robot, hc)
    G, h = a.goals, a.resolution
    cfg = nat.make_config(solution_mode="quality", max_time=0.0, max_restarts=a.restarts)
    for Q in a.queries:
        starts = hc.seed_batch(1 + 8192, Q)
        poses = hc.fk_batch(hc.seed_batch(1 + 8192 + Q, Q)).t().contiguous()          # [Q, 7]
        sol = hc.ik_solutions(cfg, poses, starts.t().contiguous(), 0, a.restarts, G, a.min_dist)
        goals, gcount = sol["x"].permute(1, 2, 0).contiguous(), sol["count"]           # [G, n, Q], [Q]
        rows_s = starts.repeat(1, G).contiguous()                                      # column g Q + q
        rows_g = goals.permute(1, 0, 2).reshape(hc.n, G * Q).contiguous()
        args = dict(first=0, max_nodes=a.max_nodes, Lmax=64, poll=a.poll)

        def goal_set():
            return hc.rrt_plan_goals(starts, goals, gcount, a.iters, a.step, h, **args)

        def rows():
            r = hc.rrt_plan(rows_s, rows_g, a.iters, a.step, h, **args)
            status, cost = r["status"].cpu().numpy().reshape(G, Q), r["cost"].cpu().numpy().reshape(G, Q)
            cost = np.where(status == 0, cost, np.inf)
            which = cost.argmin(axis=0)
            found = np.isfinite(cost.min(axis=0))
            r["which"], r["found"] = np.where(found, which, -1), found
            return r

        calls = {"goals": goal_set, "rows": rows}
        times = {name: [] for name in calls}
        out = {}
        for rep in range(a.reps + 1):
            for name, fn in calls.items():
                out[name], dt = timed(fn)
                if rep:
                    times[name].append(dt)
        res = {"spheres": S, "queries": Q, "goals": G, "resolution": h, "reps": a.reps, "iters": a.iters,
               "step": a.step, "max_nodes": a.max_nodes, "poll": a.poll, "ik_restarts": a.restarts,
               "goal_counts_min_mean_max": [int(gcount.min()), round(float(gcount.double().mean()), 2), int(gcount.max())]}
        for name, ts in times.items():
            res[name] = stats(ts)
        res["goals_over_rows"] = round(res["goals"]["ms"] / res["rows"]["ms"], 3)
        g, r = out["goals"], out["rows"]
        res["goals_status_counts"] = [int((g["status"] == s).sum()) for s in range(4)]
        res["goals_found"] = int(((g["status"] == 0) | (g["status"] == 2)).sum())
        res["rows_found"] = int(r["found"].sum())
        res["rows_status_counts_of_8Q"] = [int((r["status"] == s).sum()) for s in range(4)]
        res["goals_iterations_launched"] = launched(g["iters"], g["status"], a.iters, a.poll)
        res["rows_iterations_launched"] = launched(r["iters"], r["status"], a.iters, a.poll)
        res["goals_tree_nodes_mean"] = [round(float(g["nodes"][t].double().mean()), 1) for t in range(2)]
        print(json.dumps(res), flush=True)
    for name, r in sorted(build.kernel_resources().items()):
        if name.startswith("rrt_"):
            print("# %s: %d VGPR, %d AGPR, %d SGPR, %d B scratch, %d B LDS, %d waves/SIMD"
                  % (name, r["vgpr"], r["agpr"], r["sgpr"], r["scratch"], r["lds"], r["occupancy"]))


if __name__ == "__main__":
    main()
