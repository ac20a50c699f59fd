#!/usr/bin/env python3
"""Cost of the certified motion check beside the sampled one (section 5.13).

The scene is tools/motion_cost.py's: the Panda, spheres_along_chain(panda, 0.05, 12) with "auto" pairs, 64 spheres and
16 boxes, margin 0; 4 080 random segments (qa uniform inside the limits, qb within 0.6 rad of it per joint).  Recorded:

  steps     the distribution of the samples HipChain.collision_motion_certify evaluates per segment at tol = 0.01 and
            0.001 (and the statuses), beside the K of the sampled check at h = 0.05 and 0.01 (K + 1 samples each)
  time      the certified call at both tolerances against HipChain.collision_motion_batch at both resolutions (full
            and classify-only) on the same segments, in one process, interleaved: medians with [min, max] of the
            repetitions, as tools/motion_cost.py does it; and the same for the segments the certificate calls free and
            for those it calls blocked, each as a batch of its own

The sampled check has 64 samples in flight per wave, the certified one has one: whichever is faster where is a result.
One JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from collision_cost import PANDA, filtered  # noqa: E402
from motion_cost import interleaved  # noqa: E402
from optik_amd import Robot  # noqa: E402
from optik_amd.device import HipChain  # noqa: E402

TOLS, RESOLUTIONS, MAX_STEPS = (0.01, 0.001), (0.05, 0.01), 4096


def dist(v):
    v = np.asarray(v)
    return {"min": int(v.min()), "p25": int(np.percentile(v, 25)), "median": int(np.median(v)),
            "p75": int(np.percentile(v, 75)), "p95": int(np.percentile(v, 95)), "max": int(v.max()),
            "mean": round(float(v.mean()), 1), "total": int(v.sum())}


def times(hc, qa, qb, reps):
    fns = {}
    for tol in TOLS:
        fns[f"certify_tol{tol}"] = lambda tol=tol: hc.collision_motion_certify(qa, qb, tol, max_steps=MAX_STEPS)
    for h in RESOLUTIONS:
        fns[f"sampled_h{h}"] = lambda h=h: hc.collision_motion_batch(qa, qb, h)
        fns[f"sampled_h{h}_classify"] = lambda h=h: hc.collision_motion_batch(qa, qb, h, clearance=False)
    return {f"{k}_ms": [round(x * 1e3, 3) for x in v] for k, v in interleaved(fns, reps).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--segments", type=int, default=4080)
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    hc = HipChain(**robot.chain_tables())
    S = filtered(robot, hc)
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(6)
    B = a.segments
    qa = rng.uniform(lb, ub, size=(B, 7))
    qb = np.clip(qa + rng.uniform(-0.6, 0.6, size=(B, 7)), lb, ub)
    dev = lambda x: torch.tensor(x.T.copy(), dtype=torch.float64, device="cuda")  # noqa: E731
    dqa, dqb = dev(qa), dev(qb)
    out = {"spheres": S, "segments": B, "max_steps": MAX_STEPS}
    status = None
    for tol in TOLS:
        r = {k: v.cpu().numpy() for k, v in hc.collision_motion_certify(dqa, dqb, tol, max_steps=MAX_STEPS).items()}
        st = r["status"]
        out[f"certify_tol{tol}"] = {"status_counts": np.bincount(st, minlength=4).tolist(), "steps": dist(r["steps"]),
                                    "steps_free": dist(r["steps"][st == 0]) if (st == 0).any() else None,
                                    "steps_blocked": dist(r["steps"][st == 1]) if (st == 1).any() else None}
        status = st if status is None else status
    for h in RESOLUTIONS:
        _, free, _, steps = hc.collision_motion_batch(dqa, dqb, h)
        out[f"sampled_h{h}"] = {"free": int(free.sum().item()), "samples": dist(steps.cpu().numpy() + 1)}
        # segments the samples call free and the certificate (tol 0.01) blocks
        out[f"sampled_h{h}"]["free_but_certified_blocked"] = int((free.cpu().numpy() & (status == 1)).sum())
    out["all"] = times(hc, dqa, dqb, a.reps)
    for name, pick in (("certified_free", status == 0), ("certified_blocked", status == 1)):
        if pick.sum() >= 64:
            out[name] = {"segments": int(pick.sum()), **times(hc, dev(qa[pick]), dev(qb[pick]), a.reps)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
