#!/usr/bin/env python3
"""Cost of the collision filter: the key pass that follows the solve (collision_key_kernel)
against the solve kernels, the end-to-end call time with and without the filter on the same shape, the rate of
optik_hip_collision_batch, and what a single Speed ik() call costs with the filter (every restart of a launch runs)
against the first-success rule without it.

The model is spheres_along_chain(panda, 0.05, 12) (36 spheres on 3 frames, "auto" pairs) and the world 64 spheres and
16 boxes around the arm (seeded); a third to a half of the random configurations are free.

  panda_T4096_R256   HipChain.ik_batch, 4096 targets x 256 restarts (one launch), Quality and Speed
  panda_T1_R1M       HipChain.ik_batch, one target x 2^20 restarts (one launch), Quality and Speed
  batch              HipChain.collision_batch at B = 2^20: configurations / s
  single             Robot.ik, Speed, default parallelism, max_time 0.1: median wall time per call

Each shape runs --reps times per variant after one warm-up call; the wall times are medians (one JSON line).  The
kernel times come from a kernel trace of this process, in a run of its own:

    rocprofv3 --kernel-trace --stats -d OUTDIR -o coll -- python tools/collision_cost.py --shape panda_T4096_R256"""
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
from optik_amd.collision import spheres_along_chain  # noqa: E402

PANDA = (os.path.join(ROOT, "optik_amd", "robots", "panda.urdf"), "panda_link0", "panda_link8")
SHAPES = {"panda_T4096_R256": (4096, 256), "panda_T1_R1M": (1, 1 << 20)}


def world(seed=0):
    rng = np.random.default_rng(seed)
    sph = np.concatenate([rng.uniform(-0.9, 0.9, (64, 3)), rng.uniform(0.03, 0.1, (64, 1))], 1)
    q = rng.normal(size=(16, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    box = np.concatenate([rng.uniform(-0.9, 0.9, (16, 3)), q, rng.uniform(0.02, 0.1, (16, 3))], 1)
    return sph, box


def filtered(robot, hc):
    frames, centers, radii = spheres_along_chain(robot, 0.05, 12)
    sph, box = world()
    hc.set_collision_model(frames, centers, radii, self_pairs="auto", margin=0.0)
    hc.set_world(sph, box)
    return len(frames)


def timed(fn, reps):
    times = []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if rep:
            times.append(time.perf_counter() - t0)
    return float(np.median(times)), out


def solve_shape(name, reps):
    T, R = SHAPES[name]
    robot = Robot.from_urdf_file(*PANDA)
    plain = robot.hip_chain()
    from optik_amd.device import HipChain
    filt = HipChain(**robot.chain_tables())
    S = filtered(robot, filt)
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(1)
    q = rng.uniform(lb, ub, size=(T, 7))
    tg = plain.fk_batch(torch.tensor(q.T.copy(), dtype=torch.float64, device="cuda")).T.contiguous()
    x0 = torch.tensor(rng.uniform(lb, ub, size=(T, 7)), dtype=torch.float64, device="cuda")
    out = {"spheres": S}
    for mode in ("quality", "speed"):
        cfg = nat.make_config(solution_mode=mode)
        for what, hc in (("plain", plain), ("filtered", filt)):
            # (Speed without the filter: the deterministic early exit, as ik_batch_arrays' rounds run it)
            flags = nat.IK_EARLY_EXIT | nat.IK_RESTART_MAJOR if mode == "speed" else 0
            ms, res = timed(lambda: hc.ik_batch(cfg, tg, x0, 0, R, flags=flags, per_restart=False), reps)
            out[f"{mode}_{what}_ms"] = round(ms * 1e3, 3)
            out[f"{mode}_{what}_found"] = int((res["win_idx"] >= 0).sum().item())
    return out


def batch_rate(reps):
    robot = Robot.from_urdf_file(*PANDA)
    from optik_amd.device import HipChain
    hc = HipChain(**robot.chain_tables())
    S = filtered(robot, hc)
    lb, ub = (np.array(v) for v in robot.joint_limits())
    B = 1 << 20
    q = torch.tensor(np.random.default_rng(2).uniform(lb, ub, size=(B, 7)).T.copy(), dtype=torch.float64,
                     device="cuda")
    s, (clr, free) = timed(lambda: hc.collision_batch(q), reps)
    return {"spheres": S, "B": B, "configs_per_s": round(B / s), "free_fraction": round(float(free.float().mean()), 4)}


def single_calls(reps):
    robot = Robot.from_urdf_file(*PANDA)
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(3)
    poses = [robot.fk(rng.uniform(lb, ub)) for _ in range(reps)]
    seeds = rng.uniform(lb, ub, size=(reps, 7))
    cfg = SolverConfig("speed")
    out = {}
    for what in ("plain", "filtered"):
        if what == "filtered":
            frames, centers, radii = spheres_along_chain(robot, 0.05, 12)
            robot.set_collision_model(frames, centers, radii, self_pairs="auto", margin=0.0)
            robot.set_world(*world())
        robot.ik(cfg, poses[0], seeds[0])  # (warm-up)
        times, found = [], 0
        for p, s in zip(poses, seeds):
            t0 = time.perf_counter()
            found += robot.ik(cfg, p, s) is not None
            times.append(time.perf_counter() - t0)
        out[f"{what}_us"] = round(float(np.median(times)) * 1e6, 1)
        out[f"{what}_found"] = found
    out["calls"] = reps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES) + ["batch", "single", "all"], default="all")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    res = {}
    for name in (sorted(SHAPES) if a.shape == "all" else [a.shape] if a.shape in SHAPES else []):
        res[name] = solve_shape(name, a.reps)
    if a.shape in ("batch", "all"):
        res["batch"] = batch_rate(a.reps)
    if a.shape in ("single", "all"):
        res["single"] = single_calls(max(a.reps, 50))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
