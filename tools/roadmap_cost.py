#!/usr/bin/env python3
"""Cost of roadmap planning on a Panda with the model and world of tools/collision_cost.py
(36 spheres on 3 frames, "auto" pairs; 64 spheres and 16 boxes), N = 8192 nodes, k = 16:

  roadmap_knn          HipChain.roadmap_knn, every node against every node (exclude_self)
  cdist_topk           torch.cdist(p=inf), 1024 rows a call, + torch.topk on the same tensors: the separate-calls
                       baseline.  Its answers
                       are compared with roadmap_knn's: the distances must be equal, the indices wherever a query's
                       k + 1 smallest distances are distinct (topk breaks ties as it likes)
  roadmap_edges        HipChain.roadmap_edges on the knn result: with roadmap_knn, what roadmap_build costs
  roadmap_plan         HipChain.roadmap_plan for Q = 1024 random (start, goal) pairs, ks = 16, Lmax = 64

The calls run interleaved in one process, --reps rounds after one warm-up round; each figure is the median wall time
of a call (the HipChain call as a user makes it), with [min, max] beside it.  One JSON line, and the compiler's
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
    ap.add_argument("--nodes", type=int, default=8192)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--resolution", type=float, default=0.05)
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    hc = HipChain(**robot.chain_tables())
    S = filtered(robot, hc)
    N, k, Q, h = a.nodes, a.k, a.queries, a.resolution
    nodes = hc.seed_batch(1, N)
    starts, goals = hc.seed_batch(1 + N, Q), hc.seed_batch(1 + N + Q, Q)
    nbr, _ = hc.roadmap_knn(nodes, nodes, k, exclude_self=True)
    w = hc.roadmap_edges(nodes, nodes, nbr, h)
    pts = nodes.T.contiguous()

    def distances():
        # (torch.cdist with p = inf launches one block per pair: 8192 x 8192 is beyond the launch limit, so by rows)
        d = torch.cat([torch.cdist(pts[r0:r0 + 1024], pts, p=float("inf")) for r0 in range(0, N, 1024)])
        d.fill_diagonal_(float("inf"))
        return d

    def cdist_topk():
        return torch.topk(distances(), k, dim=1, largest=False, sorted=True)

    calls = {"roadmap_knn": lambda: hc.roadmap_knn(nodes, nodes, k, exclude_self=True),
             "cdist_topk": cdist_topk,
             "roadmap_edges": lambda: hc.roadmap_edges(nodes, nodes, nbr, h),
             "roadmap_plan": lambda: hc.roadmap_plan((nodes, nbr, w), starts, goals, k, 64, h)}
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
    res["roadmap_build_ms"] = round(res["roadmap_knn"]["ms"] + res["roadmap_edges"]["ms"], 3)
    res["knn_over_cdist_topk"] = round(res["roadmap_knn"]["ms"] / res["cdist_topk"]["ms"], 3)
    res["plans_per_s"] = round(Q / float(np.median(times["roadmap_plan"])))
    # the baseline's answers: equal distances; equal indices wherever the order is decided by the distances alone
    idx, dist = out["roadmap_knn"]
    tv, ti = out["cdist_topk"]
    res["baseline_distances_equal"] = bool(torch.equal(dist.T.contiguous(), tv))
    first = torch.topk(distances(), k + 1, dim=1, largest=False, sorted=True)[0]
    untied = (first[:, 1:] != first[:, :-1]).all(dim=1)
    res["baseline_untied_queries"] = int(untied.sum())
    res["baseline_indices_equal_where_untied"] = bool(torch.equal(idx.T[untied].long(), ti[untied]))
    plan = out["roadmap_plan"]
    res["free_edge_fraction"] = round(float(torch.isfinite(w).double().mean()), 4)
    res["plan_status_counts"] = [int((plan["status"] == s).sum()) for s in range(4)]
    res["plan_mean_waypoints_found"] = round(float(plan["len"][plan["status"] == 0].double().mean()), 2)
    print(json.dumps(res))
    for name, r in sorted(build.kernel_resources().items()):
        if name.startswith(("roadmap_knn_kernel<7>", "roadmap_query_kernel", "roadmap_gather", "roadmap_weight")):
            print("# %s: %d VGPR, %d AGPR, %d B scratch, %d B LDS, %d waves/SIMD"
                  % (name, r["vgpr"], r["agpr"], r["scratch"], r["lds"], r["occupancy"]))


if __name__ == "__main__":
    main()
