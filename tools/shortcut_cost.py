#!/usr/bin/env python3
"""Cost of path shortcutting on a Panda with the model and world of tools/collision_cost.py
(36 spheres on 3 frames, "auto" pairs; 64 spheres and 16 boxes): P = 1024 plans of HipChain.roadmap_plan over an
N = 8192, k = 16 roadmap -- those with status 0, repeated to fill P --, V = 32 and V = 64 vertices, resolution 0.05.

  path_shortcut        HipChain.path_shortcut: vertices, all-pairs visibility and the route on the device
  separate_calls       what the same answer costs without it: the vertices and the pairs built with torch, ONE
                       HipChain.collision_motion_batch call over them (clearance=False), the visibility copied to the
                       host and the route by numpy, vectorised over the paths
  path_resample        HipChain.path_resample of the shortcut paths to 32 waypoints

The calls run interleaved in one process, --reps rounds after one warm-up round; each figure is the median wall time
of a call, with [min, max] beside it.  One JSON line, and the compiler's resource line of the kernels."""
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


def torch_vertices(path, lens, V):
    """The subdivision of csrc/shortcut_measure.hpp step 2 with torch: path [L, P, n], lens [P] -> verts [P, V, n]
    (NaN past a path's count) and the counts [P].  Not bit for bit: the same spacing rule, vectorised."""
    L, P, n = path.shape
    q = path.permute(1, 0, 2)
    seg = torch.arange(L - 1, device=path.device)[None] < (lens[:, None] - 1)
    w = (q[:, 1:] - q[:, :-1]).abs().amax(dim=2) * seg
    T = w.sum(dim=1)
    sp = T / (V - lens).clamp(min=1)
    m = torch.where((V > lens)[:, None] & (T > 0)[:, None], torch.ceil(w / sp[:, None]).clamp(min=1), torch.ones_like(w))
    m = (m * seg).long()
    end = m.cumsum(dim=1)                                   # vertices before the end of segment s
    nv = (end[:, -1] + 1).clamp(max=V)
    v = torch.arange(V, device=path.device)[None].expand(P, V).contiguous()
    s = torch.searchsorted(end, v, right=True).clamp(max=L - 2)
    k = v - (torch.gather(end, 1, s) - torch.gather(m, 1, s))
    t = (k / torch.gather(m, 1, s).clamp(min=1))[..., None]
    idx = s[..., None].expand(P, V, n)
    qa, qb = torch.gather(q, 1, idx), torch.gather(q, 1, idx + 1)
    verts = qa + t * (qb - qa)
    verts[v >= nv[:, None]] = float("nan")
    return verts, nv


def numpy_route(W, nv, hop):
    """d [P, V] and succ [P, V] of step 4 over the weights W [P, V, V] (+inf: no hop), vectorised over the paths."""
    P, V, _ = W.shape
    d = np.full((P, V), np.inf)
    d[np.arange(P), nv - 1] = 0.0
    succ = np.full((P, V), -1)
    for i in range(V - 2, -1, -1):
        c = (W[:, i, :] + hop) + d
        c[:, :i + 1] = np.inf
        j = V - 1 - np.argmin(c[:, ::-1], axis=1)           # ties to the highest j
        best = c[np.arange(P), j]
        live = i < nv - 1
        d[live, i] = best[live]
        succ[live, i] = np.where(np.isfinite(best[live]), j[live], -1)
    return d, succ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nodes", type=int, default=8192)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--paths", type=int, default=1024)
    ap.add_argument("--resolution", type=float, default=0.05)
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    hc = HipChain(**robot.chain_tables())
    S = filtered(robot, hc)
    N, k, P, h = a.nodes, a.k, a.paths, a.resolution
    nodes = hc.seed_batch(1, N)
    nbr, _ = hc.roadmap_knn(nodes, nodes, k, exclude_self=True)
    w = hc.roadmap_edges(nodes, nodes, nbr, h)
    plan = hc.roadmap_plan((nodes, nbr, w), hc.seed_batch(1 + N, P), hc.seed_batch(1 + N + P, P), k, 64, h)
    found = torch.nonzero(plan["status"] == 0).ravel()
    pick = found[torch.arange(P, device=found.device) % len(found)]
    path = plan["path"][:, pick].contiguous()
    lens = plan["len"][pick].contiguous()

    def separate(V):
        verts, nv = torch_vertices(path, lens, V)
        i, j = torch.triu_indices(V, V, 1, device=path.device)
        qa = verts[:, i].reshape(-1, hc.n).T.contiguous()
        qb = verts[:, j].reshape(-1, hc.n).T.contiguous()
        free = hc.collision_motion_batch(qa, qb, h, clearance=False)[1].reshape(P, -1)
        W = torch.full((P, V, V), float("inf"), dtype=torch.float64, device=path.device)
        W[:, i, j] = torch.where(free, (verts[:, j] - verts[:, i]).abs().amax(dim=2), W[:, i, j])
        d, succ = numpy_route(W.cpu().numpy(), nv.cpu().numpy(), h)
        return free, d, succ

    calls = {}
    for V in (32, 64):
        calls[f"path_shortcut_V{V}"] = lambda V=V: hc.path_shortcut(path, lens, h, V)
        calls[f"separate_calls_V{V}"] = lambda V=V: separate(V)
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
    cut = out["path_shortcut_V32"]
    ts = []
    for rep in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hc.path_resample(cut["path"], cut["len"], 32)
        torch.cuda.synchronize()
        if rep:
            ts.append(time.perf_counter() - t0)
    times["path_resample_32"] = ts
    res = {"spheres": S, "nodes": N, "k": k, "paths": P, "plans_found": int(len(found)), "resolution": h, "reps": a.reps}
    for name, ts in times.items():
        res[name] = {"ms": round(float(np.median(ts)) * 1e3, 3),
                     "min_max_ms": [round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)]}
    for V in (32, 64):
        r = out[f"path_shortcut_V{V}"]
        free, d, _ = out[f"separate_calls_V{V}"]
        ok = r["status"] == 0
        res[f"V{V}"] = {
            "shortcut_over_separate": round(res[f"path_shortcut_V{V}"]["ms"] / res[f"separate_calls_V{V}"]["ms"], 3),
            "paths_per_s": round(P / float(np.median(times[f"path_shortcut_V{V}"]))),
            "status_counts": [int((r["status"] == s).sum()) for s in range(4)],
            "pairs_free_share": round(float(free.double().mean()), 4),
            "baseline_routes_found": int(np.isfinite(d[:, 0]).sum()),
            "mean_waypoints_before_after": [round(float(lens[ok].double().mean()), 2),
                                            round(float(r["len"][ok].double().mean()), 2)],
            "mean_cost_before_after": [round(float(r["cost_in"][ok].mean()), 4), round(float(r["cost"][ok].mean()), 4)]}
    res["V64_over_V32"] = round(res["path_shortcut_V64"]["ms"] / res["path_shortcut_V32"]["ms"], 3)
    print(json.dumps(res))
    for name, r in sorted(build.kernel_resources().items()):
        if name.startswith("shortcut_"):
            print("# %s: %d VGPR, %d AGPR, %d B scratch, %d B LDS, %d waves/SIMD"
                  % (name, r["vgpr"], r["agpr"], r["scratch"], r["lds"], r["occupancy"]))


if __name__ == "__main__":
    main()
