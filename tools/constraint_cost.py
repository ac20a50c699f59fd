#!/usr/bin/env python3
"""Cost of pose constraints, written to profiles/constraint_cost.txt:

  rows/s of HipChain.constraint_batch, constraint_project_batch (the default budget) and constraint_motion_batch
  (segments of up to 0.5 rad at resolution 0.05) at B = 2^20 uniform Panda configurations against
  upright(home, 0.1);
  the constrained build (seeds, projection, roadmap_build_constrained) against roadmap_build at N = 8192, k = 16.

Every figure is the median of 7 timed calls after one warm-up, with the minimum and the maximum.  Nobody promises a
ratio; the file records what this prints.

    python tools/constraint_cost.py [--out profiles/constraint_cost.txt]"""
import argparse
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

PANDA = (os.path.join(ROOT, "optik_amd", "robots", "panda.urdf"), "panda_link0", "panda_link8")
HOME = [0.0, -0.785398163397, 0.0, -2.35619449019, 0.0, 1.57079632679, 0.785398163397]
REPS = 7


def timed(call):
    """(median, min, max) seconds of REPS calls after one warm-up, the device idle at both ends of each."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constraint_cost.txt"))
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    hc = robot.hip_chain()
    c = PoseConstraint.upright(np.array(robot.fk(HOME)), 0.1)
    lines = [f"# tools/constraint_cost.py -- {torch.cuda.get_device_name(0)}; {optik_build.toolchain_version()}",
             f"# Panda, upright(home, 0.1); medians of {REPS} after a warm-up (min .. max)"]
    B = 1 << 20
    q = hc.seed_batch(0, B)
    qb = (q + 0.5 * torch.sin(torch.arange(B, device=q.device, dtype=torch.float64))[None, :]
          * torch.linspace(-1.0, 1.0, hc.n, device=q.device, dtype=torch.float64)[:, None]).contiguous()
    ops = [("constraint_batch", lambda: hc.constraint_batch(q, c)),
           ("constraint_project_batch", lambda: hc.constraint_project_batch(q, c)),
           ("constraint_motion_batch", lambda: hc.constraint_motion_batch(q, qb, 0.05, c))]
    for name, call in ops:
        med, lo, hi = timed(call)
        lines.append(f"{name:28s} B = 2^20: {1e3 * med:9.3f} ms ({1e3 * lo:.3f} .. {1e3 * hi:.3f})  "
                     f"{B / med / 1e6:9.3f} M rows/s")
    p = hc.constraint_project_batch(q, c)
    lines.append(f"  projected {100.0 * float((p['status'] == 0).double().mean()):.2f} % of the rows, mean iterations "
                 f"{float(p['iterations'].double().mean()):.1f} (iters = {nat.CONSTRAINT_ITERS}, damping = "
                 f"{nat.CONSTRAINT_DAMPING}, max_step = {nat.CONSTRAINT_MAX_STEP})")
    samples = hc.constraint_motion_batch(q, qb, 0.05, c)[3]
    lines.append(f"  motion: {float((samples + 1).clamp(min=0).double().mean()):.1f} samples per segment")

    N, k, h = 8192, 16, 0.1
    nodes = hc.seed_batch(0, N)

    def constrained():
        pr = hc.constraint_project_batch(hc.seed_batch(0, N), c)
        nd = torch.where((pr["status"] == 0)[None, :], pr["x"], torch.full_like(pr["x"], float("nan"))).contiguous()
        return hc.roadmap_build_constrained(nd, k, h, c, 0.05)

    plain = timed(lambda: hc.roadmap_build(nodes, k, h))
    cons = timed(constrained)
    w = constrained()[1]
    lines.append(f"roadmap_build               N = {N}, k = {k}: {1e3 * plain[0]:9.3f} ms ({1e3 * plain[1]:.3f} .. "
                 f"{1e3 * plain[2]:.3f})")
    lines.append(f"constrained build           N = {N}, k = {k}: {1e3 * cons[0]:9.3f} ms ({1e3 * cons[1]:.3f} .. "
                 f"{1e3 * cons[2]:.3f})  ratio {cons[0] / plain[0]:.2f}, {int(torch.isfinite(w).sum())} of {N * k} "
                 f"edges kept")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
