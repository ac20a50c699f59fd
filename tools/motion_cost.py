#!/usr/bin/env python3
"""Cost of the motion check.

  fused     HipChain.collision_motion_batch against the pipeline it replaces -- the samples materialised on the device
            with torch (in the documented order), HipChain.collision_batch on them, a segmented minimum with torch --
            in one process, interleaved, as medians with the spread of each side (min .. max of the repetitions).  About
            2^20 samples per call, as long segments (K = 256) and as short ones (K = 4).  Next to them
            collision_batch's configurations/s on the pipeline's samples, and the classify-only form against the full
            one on a scene where half the segments are blocked (picked from a larger pool by the full call).
  path      one HipChain.ik_path run with the check on (P = 4096, L = 16, R = 64, h = 0.02): for a kernel trace, in a
            run of its own:

    rocprofv3 --kernel-trace --stats -d OUTDIR -o motion -- python tools/motion_cost.py --shape path

The model is spheres_along_chain(panda, 0.05, 12) with "auto" pairs and the world 64 spheres and 16 boxes: the setup of
tools/collision_cost.py.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from collision_cost import PANDA, filtered, world  # noqa: E402
from optik_amd import Robot  # noqa: E402
from optik_amd import _native as nat  # noqa: E402
from optik_amd.device import HipChain  # noqa: E402


def pipeline(hc, qa, qb, K, margin=0.0):
    """K the same for every segment: samples [n, B * (K + 1)] with torch, collision_batch, segmented min / first."""
    n, B = qa.shape
    t = (torch.arange(K + 1, dtype=torch.float64, device=qa.device) / float(K)).view(1, 1, K + 1)
    s = qa.unsqueeze(2) + t * (qb - qa).unsqueeze(2)
    s[:, :, 0] = qa
    s[:, :, K] = qb
    clr, _ = hc.collision_batch(s.reshape(n, B * (K + 1)).contiguous())
    clr = clr.view(B, K + 1)
    bad = ~(clr >= margin)
    k = torch.arange(K + 1, device=qa.device).expand(B, K + 1)
    first = torch.where(bad, k, torch.full_like(k, K + 1)).min(dim=1).values
    return clr.min(dim=1).values, first == K + 1, torch.where(first == K + 1, torch.full_like(first, -1), first)


def interleaved(fns, reps):
    """Each of fns once per repetition, in turn, after one warm-up round: {name: (median, min, max)} in seconds."""
    times = {k: [] for k in fns}
    for rep in range(reps + 1):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                times[k].append(time.perf_counter() - t0)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in times.items()}


def segments(lb, ub, B, K, h, rng):
    """B segments of exactly K steps at resolution h: d = (K - 0.5) h along a random direction."""
    qa = rng.uniform(lb + 0.3 * (ub - lb), ub - 0.3 * (ub - lb), size=(B, len(lb)))
    u = rng.uniform(-1.0, 1.0, size=qa.shape)
    u /= np.max(np.abs(u), axis=1, keepdims=True)
    qb = qa + u * (K - 0.5) * h
    dev = lambda a: torch.tensor(a.T.copy(), dtype=torch.float64, device="cuda")  # noqa: E731
    return dev(qa), dev(qb)


def fused_shapes(reps):
    robot = Robot.from_urdf_file(*PANDA)
    hc = HipChain(**robot.chain_tables())
    S = filtered(robot, hc)
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(4)
    out = {"spheres": S}
    for name, K, h in (("long_K256", 256, 0.004), ("short_K4", 4, 0.05)):
        B = (1 << 20) // (K + 1)
        qa, qb = segments(lb, ub, B, K, h, rng)
        got = hc.collision_motion_batch(qa, qb, h)
        want = pipeline(hc, qa, qb, K)
        same = bool(torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
                    and torch.equal(got[2].long(), want[2]) and bool((got[3] == K).all()))
        n_s = B * (K + 1)
        flat = (qa.unsqueeze(2) + torch.zeros(1, 1, K + 1, dtype=torch.float64, device="cuda")).reshape(7, n_s).contiguous()
        t = interleaved({"fused": lambda: hc.collision_motion_batch(qa, qb, h),
                         "pipeline": lambda: pipeline(hc, qa, qb, K),
                         "classify": lambda: hc.collision_motion_batch(qa, qb, h, clearance=False),
                         "collision_batch": lambda: hc.collision_batch(flat)}, reps)
        out[name] = {"B": B, "K": K, "samples": n_s, "same_bits": same, "free_fraction": round(float(got[1].float().mean()), 4),
                     **{f"{k}_ms": [round(x * 1e3, 3) for x in v] for k, v in t.items()},
                     "fused_samples_per_s": round(n_s / t["fused"][0]),
                     "collision_batch_configs_per_s": round(n_s / t["collision_batch"][0])}
    # classify-only on a scene where half the segments are blocked: segments of K = 256 steps of 1 mrad, taken from a
    # larger pool by the full call's own verdict, as many free ones as blocked ones
    K, h = 256, 0.001
    B = (1 << 20) // (K + 1)
    pa, pb = segments(lb, ub, 16 * B, K, h, rng)
    pf = hc.collision_motion_batch(pa, pb, h)[1]
    fi, bi = torch.nonzero(pf).flatten(), torch.nonzero(~pf).flatten()
    half = min(B // 2, len(fi), len(bi))
    pick = torch.cat([fi[:half], bi[:half]])[torch.randperm(2 * half, device="cuda", generator=None)]
    qa, qb = pa[:, pick].contiguous(), pb[:, pick].contiguous()
    res = hc.collision_motion_batch(qa, qb, h)
    t = interleaved({"full": lambda: hc.collision_motion_batch(qa, qb, h),
                     "classify": lambda: hc.collision_motion_batch(qa, qb, h, clearance=False)}, reps)
    blocked = ~res[1]
    out["half_blocked_K256"] = {"B": int(2 * half), "K": K, "h": h, "free_fraction": round(float(res[1].float().mean()), 4),
                                "median_first_of_blocked": int(res[2][blocked].median().item()) if bool(blocked.any()) else -1,
                                **{f"{k}_ms": [round(x * 1e3, 3) for x in v] for k, v in t.items()}}
    return out


def path_run(reps):
    robot = Robot.from_urdf_file(*PANDA)
    hc = HipChain(**robot.chain_tables())
    filtered(robot, hc)
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(5)
    P, L, R, h = 4096, 16, 64, 0.02
    qa = rng.uniform(lb, ub, size=(P, 7))
    qb = np.clip(qa + rng.uniform(-0.6, 0.6, size=(P, 7)), lb, ub)
    qs = np.stack([(1 - s) * qa + s * qb for s in np.linspace(0.0, 1.0, L)])  # [L, P, 7]
    tg = hc.fk_batch(torch.tensor(qs.reshape(L * P, 7).T.copy(), dtype=torch.float64, device="cuda")).T.contiguous()
    tg = tg.view(L, P, 7).contiguous()
    x0 = torch.tensor(qa, dtype=torch.float64, device="cuda")
    cfg = nat.make_config(solution_mode="quality")
    out = {"P": P, "L": L, "R": R, "h": h}
    for what, res in (("off", 0.0), ("on", h)):
        hc.set_motion_resolution(res)
        t = interleaved({"ik_path": lambda: hc.ik_path(cfg, tg, x0, 0, R, 0.5)}, reps)["ik_path"]
        got = hc.ik_path(cfg, tg, x0, 0, R, 0.5)
        out[f"{what}_ms"] = [round(x * 1e3, 3) for x in t]
        out[f"{what}_found"] = int((got["idx"] >= 0).sum().item())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["fused", "path", "all"], default="all")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    res = {}
    if a.shape in ("fused", "all"):
        res["fused"] = fused_shapes(a.reps)
    if a.shape in ("path", "all"):
        res["path"] = path_run(a.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
