#!/usr/bin/env python3
"""Cost of IK into pose regions, written to profiles/ik_region_cost.txt:

  Panda, T = 64 regions, R = 4096 restarts each, axis_free(fk(home), "z"): the time of HipChain.ik_region (one
  optik_hip_ik_region) next to the same rows composed from the calls that existed before it -- seed_batch,
  constraint_project_batch, a torch key, optik_hip_solutions_from_keys --, the mean Gauss-Newton iterations per
  restart and the share of PROJECTED rows;
  for the pinned region, the count of distinct solutions next to ik_solutions' on the same pose and restarts.

Every time is the median of 7 timed calls after one warm-up, with the minimum and the maximum.  Nobody promises a
ratio; the file records what this prints.

    python tools/ik_region_cost.py [--out profiles/ik_region_cost.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from optik_amd import PoseConstraint, Robot  # noqa: E402
from optik_amd import _native as nat  # noqa: E402
from optik_amd import build as optik_build  # noqa: E402
from optik_amd.constraint import region_rows  # noqa: E402

PANDA = (os.path.join(ROOT, "optik_amd", "robots", "panda.urdf"), "panda_link0", "panda_link8")
HOME = [0.0, -0.785398163397, 0.0, -2.35619449019, 0.0, 1.57079632679, 0.785398163397]
REPS, T, R, K, MIN_DIST = 7, 64, 4096, 8, 0.1


def timed(call):
    times = []
    for rep in range(REPS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if rep:
            times.append(time.perf_counter() - t0)
    return float(np.median(times)), min(times), max(times)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ik_region_cost.txt"))
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    hc = robot.hip_chain()
    pose = np.array(robot.fk(HOME))
    c = PoseConstraint.axis_free(pose, "z")
    regions = torch.from_numpy(region_rows(c, T)).cuda()
    x0 = hc.seed_batch(1000, T).t().contiguous()
    lines = [f"# tools/ik_region_cost.py -- {torch.cuda.get_device_name(0)}; {optik_build.toolchain_version()}",
             f"# Panda, T = {T}, R = {R}, K = {K}, min_dist = {MIN_DIST}, axis_free(fk(home), z), Quality; medians of "
             f"{REPS} after a warm-up (min .. max)"]

    def fused():
        return hc.ik_region(regions, x0, 0, R, K, MIN_DIST)

    def composed():
        seeds = hc.seed_batch(0, R)
        starts = seeds.repeat(1, T)
        starts[:, ::R] = x0.t()
        p = hc.constraint_project_batch(starts.contiguous(), c)
        d = p["x"] - x0.t().repeat_interleave(R, dim=1)
        key = torch.where(p["status"] == nat.CONSTRAINT_PROJECTED, torch.sqrt((d * d).sum(dim=0)),
                          torch.full_like(p["violation"], float("inf")))
        o = nat.IkSolutionsOutputs()
        out = dict(count=torch.empty(T, dtype=torch.int32, device="cuda"),
                   x=torch.empty((T, K, hc.n), dtype=torch.float64, device="cuda"))
        o.d_count, o.d_x = out["count"].data_ptr(), out["x"].data_ptr()
        nat.check(nat.lib().optik_hip_solutions_from_keys(hc._h, key.data_ptr(), p["x"].data_ptr(),
                                                          p["violation"].data_ptr(), T, 0, R, K, MIN_DIST, C.byref(o),
                                                          None))
        return out

    for name, call in (("ik_region", fused), ("composed (seed_batch, constraint_project_batch, torch key, "
                                              "solutions_from_keys)", composed)):
        med, lo, hi = timed(call)
        lines.append(f"{name}: {med * 1e3:.3f} ms ({lo * 1e3:.3f} .. {hi * 1e3:.3f}), "
                     f"{T * R / med / 1e6:.2f} M restarts/s")
    a_, b_ = fused(), composed()
    lines.append(f"same counts: {bool(torch.equal(a_['count'], b_['count']))}; same first solutions (the torch key sums "
                 f"in another order): {bool(torch.equal(a_['x'][:, 0], b_['x'][:, 0]))}")
    r = hc.ik_region(regions, x0, 0, R, K, MIN_DIST, per_restart=True)
    ok = r["restart_status"] == nat.CONSTRAINT_PROJECTED
    lines.append(f"mean Gauss-Newton iterations per restart: {r['restart_iterations'].double().mean().item():.2f}; "
                 f"PROJECTED: {ok.double().mean().item() * 100:.1f} %; mean count {r['count'].double().mean().item():.2f}")
    pinned = torch.from_numpy(region_rows(PoseConstraint.around(pose, 0.0, 0.0), T)).cuda()
    pr = hc.ik_region(pinned, x0, 0, R, K, MIN_DIST)
    target = torch.from_numpy(np.tile(PoseConstraint.around(pose, 0.0, 0.0).ref7, (T, 1))).cuda()
    sol = hc.ik_solutions(nat.make_config(solution_mode="quality", max_restarts=R), target, x0, 0, R, K, MIN_DIST)
    lines.append(f"pinned region: mean count {pr['count'].double().mean().item():.2f} of {K}; ik_solutions on the same "
                 f"pose and restarts: {sol['count'].double().mean().item():.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
