#!/usr/bin/env python3
"""Cost of path timing with tool limits against path timing without, on the paths of
tools/time_cost.py: the status-0 plans of a Panda over an N = 8192, k = 16 roadmap, resampled to 32 and to 64
waypoints and repeated to fill P = 1024, 8192 and 65 536 paths.  Limits: the URDF's velocities, 7.5 rad/s^2.

  path_time              optik_hip_path_time, every output written
  path_time_tool_free    optik_hip_path_time_tool with all four tool limits +inf: the forward kinematics, the tool rows
                         and the wider folds, and path_time's result bit for bit (checked here)
  path_time_tool         the same with 0.25 m/s, 2 m/s^2 tangential, 2 m/s^2 normal and 1.5 rad/s

The calls write into tensors allocated beforehand and run interleaved in one process, --reps rounds after one warm-up
round.  Each figure is the median wall time of a call, synchronised before and after, with [min, max] beside it.  One
JSON line per (P, L), and the compiler's resource line of the kernels."""
import argparse
import ctypes as C
import json
import math
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
from optik_amd.device import HipChain, _ptr, _stream_ptr  # noqa: E402

TOOL = (0.25, 2.0, 2.0, 1.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nodes", type=int, default=8192)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--plans", type=int, default=1024)
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--a-max", type=float, default=7.5)
    ap.add_argument("--paths", type=int, nargs="+", default=[1024, 8192, 65536])
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    hc = HipChain(**robot.chain_tables())
    filtered(robot, hc)
    N, k, P0, h = a.nodes, a.k, a.plans, a.resolution
    nodes = hc.seed_batch(1, N)
    nbr, _ = hc.roadmap_knn(nodes, nodes, k, exclude_self=True)
    w = hc.roadmap_edges(nodes, nodes, nbr, h)
    plan = hc.roadmap_plan((nodes, nbr, w), hc.seed_batch(1 + N, P0), hc.seed_batch(1 + N + P0, P0), k, 64, h)
    found = torch.nonzero(plan["status"] == 0).ravel()
    vmax_d = torch.from_numpy(robot.velocity_limits()).cuda()
    amax_d = torch.from_numpy(np.full(hc.n, a.a_max)).cuda()
    work = {}
    for P in a.paths:
        pick = found[torch.arange(P, device=found.device) % len(found)]
        path, lens = plan["path"][:, pick].contiguous(), plan["len"][pick].contiguous()
        for L in (32, 64):
            work[P, L] = hc.path_resample(path, lens, L)[0]
    lib, calls, results = nat.lib(), {}, {}
    free, capped = (C.c_double * 4)(*([math.inf] * 4)), (C.c_double * 4)(*TOOL)

    def time_call(path, r):
        L, P = path.shape[0], path.shape[1]
        nat.check(lib.optik_hip_path_time(hc._h, _ptr(path), None, L, P, _ptr(vmax_d), _ptr(amax_d), _ptr(r["t"]),
                                          _ptr(r["qd"]), _ptr(r["qdd"]), _ptr(r["x"]), _ptr(r["duration"]),
                                          _ptr(r["status"]), _stream_ptr()))

    def tool_call(path, r, lim):
        L, P = path.shape[0], path.shape[1]
        nat.check(lib.optik_hip_path_time_tool(hc._h, _ptr(path), None, L, P, _ptr(vmax_d), _ptr(amax_d), lim, None,
                                               _ptr(r["t"]), _ptr(r["qd"]), _ptr(r["qdd"]), _ptr(r["x"]),
                                               _ptr(r["duration"]), _ptr(r["status"]), _ptr(r["tool_speed"]),
                                               _ptr(r["tool_accel"]), _ptr(r["tool_wspeed"]), _stream_ptr()))
    for key, path in work.items():
        shape = hc.path_time_tool(path, None, vmax_d, amax_d)
        for name in ("path_time", "path_time_tool_free", "path_time_tool"):
            results[(name,) + key] = {kk: torch.empty_like(t) for kk, t in shape.items()}
        calls[("path_time",) + key] = lambda path=path, r=results[("path_time",) + key]: time_call(path, r)
        calls[("path_time_tool_free",) + key] = \
            lambda path=path, r=results[("path_time_tool_free",) + key]: tool_call(path, r, free)
        calls[("path_time_tool",) + key] = \
            lambda path=path, r=results[("path_time_tool",) + key]: tool_call(path, r, capped)
    times = {name: [] for name in calls}
    for rep in range(a.reps + 1):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)

    def row(name, P, L):
        tt = times[name, P, L]
        med = float(np.median(tt))
        return med, {"ms": round(med * 1e3, 3), "min_max_ms": [round(min(tt) * 1e3, 3), round(max(tt) * 1e3, 3)],
                     "paths_per_s": round(P / med)}
    for (P, L) in work:
        base, nolim, lim = (results[name, P, L] for name in ("path_time", "path_time_tool_free", "path_time_tool"))
        same = all(torch.equal(base[kk].view(torch.uint8), nolim[kk].view(torch.uint8))
                   for kk in ("t", "qd", "qdd", "x", "duration", "status"))
        ok = (lim["status"] == 0)
        okb = (base["status"] == 0)
        m0, r0 = row("path_time", P, L)
        m1, r1 = row("path_time_tool_free", P, L)
        m2, r2 = row("path_time_tool", P, L)
        print(json.dumps({
            "paths": P, "waypoints": L, "reps": a.reps, "plans_found": int(len(found)),
            "status_counts": [int((base["status"] == s).sum()) for s in range(4)],
            "status_counts_tool": [int((lim["status"] == s).sum()) for s in range(4)],
            "median_duration_s": round(float(base["duration"][okb].median()), 4),
            "median_duration_tool_s": round(float(lim["duration"][ok].median()), 4),
            "peak_tool_speed": float(lim["tool_speed"][:, ok].max()),
            "peak_tool_speed_unlimited": float(nolim["tool_speed"][:, okb].max()),
            "path_time": r0, "path_time_tool_free": r1, "path_time_tool": r2,
            "tool_free_over_path_time": round(m1 / m0, 2), "tool_over_path_time": round(m2 / m0, 2),
            "free_equals_path_time_bitwise": bool(same)}))
    for name, r in sorted(build.kernel_resources().items()):
        if name.startswith("path_time"):
            print("# %s: %d VGPR, %d AGPR, %d SGPR, %d B scratch, %d B static LDS, %d waves/SIMD"
                  % (name, r["vgpr"], r["agpr"], r["sgpr"], r["scratch"], r["lds"], r["occupancy"]))


if __name__ == "__main__":
    main()
