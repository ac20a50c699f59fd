#!/usr/bin/env python3
"""Cost of the bidirectional tree planner next to "the world changed, then plan" through the
eager and the lazy roadmap, on the scene of tools/roadmap_cost.py: a Panda with the model and world of
tools/collision_cost.py, N = 8192 nodes, k = 16.

  rrt     HipChain.rrt_plan on Q random (start, goal) pairs: no roadmap is built or read
  eager   HipChain.roadmap_build + HipChain.roadmap_plan          (as tools/roadmap_lazy_cost.py)
  lazy    HipChain.roadmap_lazy_reset + HipChain.roadmap_plan_lazy

for Q = 1, 64 and 1024, interleaved in one process, --reps rounds after one warm-up round; each figure is the median
wall time of the call(s) as a user makes them, with [min, max].  For the tree planner also: the iterations the host
loop launched (the largest iters of the batch, up to the next poll), the time per launched iteration, and an ESTIMATE
of the motion check's share of it -- the median time of one optik_hip_collision_motion_batch call on 3 Q segments of
one step each, which is what an iteration hands it while every query is still growing.  Last: the pairs of the largest
batch that the eager roadmap returns as status 1, planned again by the tree planner -- how many it finds and after how
many iterations.  One JSON line each, and the compiler's resource line of the new kernels.  No bar is set here: what
is printed is what was measured."""
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


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def stats(ts):
    return {"ms": round(float(np.median(ts)) * 1e3, 3), "min_max_ms": [round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nodes", type=int, default=8192)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--iters", type=int, default=1024)
    ap.add_argument("--step", type=float, default=0.5)
    ap.add_argument("--max-nodes", type=int, default=512)
    ap.add_argument("--poll", type=int, default=32)
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    hc = HipChain(**robot.chain_tables())
    S = filtered(robot, hc)
    N, k, h = a.nodes, a.k, a.resolution
    nodes = hc.seed_batch(1, N)
    rm = hc.roadmap_build_lazy(nodes, k, h)
    missed = None
    for Q in a.queries:
        starts, goals = hc.seed_batch(1 + N, Q), hc.seed_batch(1 + N + Q, Q)
        # 3 Q segments of one step: from the starts towards the goals
        d = (goals - starts).abs().max(dim=0).values.clamp_min(1e-9)
        ends = starts + (goals - starts) * (a.step / d).clamp_max(1.0)
        qa, qb = starts.repeat(1, 3).contiguous(), ends.repeat(1, 3).contiguous()

        def eager():
            nbr, w = hc.roadmap_build(nodes, k, h)
            return hc.roadmap_plan((nodes, nbr, w), starts, goals, k, 64, h)

        def lazy():
            hc.roadmap_lazy_reset(rm)
            return hc.roadmap_plan_lazy(rm, starts, goals, k, 64, 4096)

        def rrt():
            return hc.rrt_plan(starts, goals, a.iters, a.step, h, first=0, max_nodes=a.max_nodes, Lmax=64, poll=a.poll)

        def motion():
            return hc.collision_motion_batch(qa, qb, h, clearance=False)

        calls = {"rrt": rrt, "eager": eager, "lazy": lazy, "motion_3Q": motion}
        times = {name: [] for name in calls}
        out = {}
        for rep in range(a.reps + 1):
            for name, fn in calls.items():
                out[name], dt = timed(fn)
                if rep:
                    times[name].append(dt)
        res = {"spheres": S, "nodes": N, "k": k, "queries": Q, "resolution": h, "reps": a.reps, "iters": a.iters,
               "step": a.step, "max_nodes": a.max_nodes, "poll": a.poll}
        for name, ts in times.items():
            res[name] = stats(ts)
        r, e = out["rrt"], out["eager"]
        used = int(r["iters"].max())
        ended = bool((r["status"] != 1).all() or used < a.iters)
        launched = min(a.iters, -(-max(used, 1) // a.poll) * a.poll + 1) if ended else a.iters
        res["rrt_status_counts"] = [int((r["status"] == s).sum()) for s in range(4)]
        res["eager_status_counts"] = [int((e["status"] == s).sum()) for s in range(4)]
        res["rrt_iters_max"], res["rrt_iterations_launched"] = used, launched
        res["rrt_ms_per_iteration"] = round(res["rrt"]["ms"] / launched, 4)
        res["motion_share_estimate"] = round(res["motion_3Q"]["ms"] / res["rrt_ms_per_iteration"], 3)
        print(json.dumps(res), flush=True)
        missed = (starts, goals, e["status"] == 1)
    # the pairs the roadmap misses, through the tree planner
    starts, goals, miss = missed
    s, g = starts[:, miss].contiguous(), goals[:, miss].contiguous()
    if s.shape[1]:
        free = hc.collision_batch(s)[1] & hc.collision_batch(g)[1]
        r, dt = timed(lambda: hc.rrt_plan(s, g, 4096, a.step, h, first=0, max_nodes=2048, Lmax=64, poll=a.poll))
        found = (r["status"] == 0) | (r["status"] == 2)
        it = r["iters"][found].cpu().numpy()
        print(json.dumps({"roadmap_status_1": int(miss.sum()), "of_queries": int(miss.numel()),
                          "both_ends_free": int(free.sum()), "rrt_found": int(found.sum()),
                          "rrt_found_too_long": int((r["status"] == 2).sum()), "iters": 4096, "max_nodes": 2048,
                          "found_iters_median_max": [int(np.median(it)), int(it.max())] if len(it) else None,
                          "ms": round(dt * 1e3, 3)}))
    else:
        print(json.dumps({"roadmap_status_1": 0, "of_queries": int(miss.numel())}))
    for name, r in sorted(build.kernel_resources().items()):
        if name.startswith("rrt_"):
            print("# %s: %d VGPR, %d AGPR, %d SGPR, %d B scratch, %d B LDS, %d waves/SIMD"
                  % (name, r["vgpr"], r["agpr"], r["sgpr"], r["scratch"], r["lds"], r["occupancy"]))


if __name__ == "__main__":
    main()
