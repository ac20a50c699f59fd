#!/usr/bin/env python3
"""Cost of warm-started paths (Robot.ik_paths_arrays, HipChain.ik_path) on the Panda, Speed, max_step = inf, for the
two shapes of DESIGN.md section 5.10:

  P1_L256_R64      one path of 256 waypoints, 64 restarts each: wall time per waypoint of Robot.ik_paths_arrays and of
                   HipChain.ik_path, against a host loop of Robot.ik_batch_arrays (T = 1) seeded from the previous
                   result (a launch, a synchronise and copies per waypoint)
  P1024_L64_R256   1024 paths of 64 waypoints, 256 restarts each: waypoints per second of both forms

The paths are FK of joint configurations interpolated between a random start and a nearby end (a warm start usually
converges: the regime the call is for).  Each shape runs --reps times after one warm-up call.  The kernel times
(ik_path_select_kernel next to the solve kernel) come from a kernel trace of this process, in a run of its own:

    rocprofv3 --kernel-trace --stats -d OUTDIR -o path -- python tools/ik_path_cost.py --shape P1024_L64_R256

Without the profiler it prints the wall times and the waypoints solved (one JSON line)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from optik_amd import Robot, SolverConfig  # noqa: E402
from optik_amd import _native as nat  # noqa: E402

SHAPES = {"P1_L256_R64": (1, 256, 64), "P1024_L64_R256": (1024, 64, 256)}


def _mat(p7):
    """pose7 rows [t, qi, qj, qk, qw] -> 4x4 row-major matrices."""
    t, (i, j, k, w) = p7[:, :3], p7[:, 3:].T
    m = np.zeros((len(p7), 4, 4))
    m[:, 0, 0], m[:, 0, 1], m[:, 0, 2] = 1 - 2 * (j * j + k * k), 2 * (i * j - k * w), 2 * (i * k + j * w)
    m[:, 1, 0], m[:, 1, 1], m[:, 1, 2] = 2 * (i * j + k * w), 1 - 2 * (i * i + k * k), 2 * (j * k - i * w)
    m[:, 2, 0], m[:, 2, 1], m[:, 2, 2] = 2 * (i * k - j * w), 2 * (j * k + i * w), 1 - 2 * (i * i + j * j)
    for r in range(len(p7)):  # (orthonormal to the last bit: the isometry test allows 100 eps)
        u, _, vt = np.linalg.svd(m[r, :3, :3])
        m[r, :3, :3] = u @ vt
    m[:, :3, 3] = t
    m[:, 3, 3] = 1.0
    return m


def paths(robot, hc, P, L, rng):
    """-> targets [L, P, 7] on the device, the same as [P, L, 4, 4] matrices, start configurations [P, n]."""
    lb, ub = (np.array(v) for v in robot.joint_limits())
    qa = rng.uniform(lb + 0.2 * (ub - lb), ub - 0.2 * (ub - lb), size=(P, len(lb)))
    qb = np.clip(qa + rng.uniform(-0.5, 0.5, size=qa.shape), lb, ub)
    s = np.linspace(0.0, 1.0, L)[:, None, None]
    q = ((1.0 - s) * qa[None] + s * qb[None]).reshape(L * P, -1)  # [L*P, n], waypoint-major
    pose = hc.fk_batch(torch.tensor(q.T.copy(), dtype=torch.float64, device="cuda")).T.contiguous()  # [L*P, 7]
    mats = _mat(pose.cpu().numpy()).reshape(L, P, 4, 4).transpose(1, 0, 2, 3).copy()
    return pose.reshape(L, P, 7).contiguous(), mats, qa


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append")
    args = ap.parse_args()
    robot = Robot.from_urdf_file(os.path.join(ROOT, "optik_amd", "robots", "panda.urdf"), "panda_link0", "panda_link8")
    hc = robot.hip_chain()
    rng = np.random.default_rng(0)
    res = {}
    for name in args.shape or sorted(SHAPES):
        P, L, R = SHAPES[name]
        tgd, mats, qa = paths(robot, hc, P, L, rng)
        x0d = torch.tensor(qa, dtype=torch.float64, device="cuda")
        ncfg = nat.make_config(solution_mode="speed")
        cfg = SolverConfig("speed", max_time=0.0, max_restarts=R)
        r = {"P": P, "L": L, "R": R}
        # the device form (stream-ordered; one synchronise per call)
        out = hc.ik_path(ncfg, tgd, x0d, 0, R, flags=nat.IK_RESTART_MAJOR)  # warm-up (workspace, code objects)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            out = hc.ik_path(ncfg, tgd, x0d, 0, R, flags=nat.IK_RESTART_MAJOR, bufs=out)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.reps
        idx = out["idx"].cpu().numpy()
        r["device_ms_per_call"] = dt * 1e3
        r["device_us_per_waypoint"] = dt / L * 1e6
        r["device_waypoints_per_s"] = P * L / dt
        r["solved"] = int((idx >= 0).sum())
        r["from_warm_start"] = int((idx == 0).sum())
        # the host form
        robot.ik_paths_arrays(cfg, mats, qa)
        t0 = time.perf_counter()
        for _ in range(args.reps):
            x, f, hidx, step, found = robot.ik_paths_arrays(cfg, mats, qa)
        dt = (time.perf_counter() - t0) / args.reps
        r["robot_ms_per_call"] = dt * 1e3
        r["robot_us_per_waypoint"] = dt / L * 1e6
        r["robot_waypoints_per_s"] = P * L / dt
        r["largest_step"] = float(np.nanmax(step))
        if P == 1:
            # a host loop of ik_batch_arrays, T = 1, each waypoint seeded from the previous result
            def loop():
                c, n_found = qa.copy(), 0
                for w in range(L):
                    bx, _, bfound = robot.ik_batch_arrays(cfg, mats[:, w], c)
                    if bfound[0]:
                        c, n_found = bx.copy(), n_found + 1
                return n_found
            loop()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                n_found = loop()
            dt = (time.perf_counter() - t0) / args.reps
            r["host_loop_us_per_waypoint"] = dt / L * 1e6
            r["host_loop_solved"] = n_found
        res[name] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
