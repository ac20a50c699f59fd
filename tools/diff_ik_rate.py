#!/usr/bin/env python3
"""Rate of batched diff_ik on one GPU: configurations/s of HipChain.diff_ik_batch (device buffers, the kernel-layer
call) and of Robot.diff_ik_batch_arrays (host arrays, staging included) for Panda (n = 7) and UR3e (n = 6) at
B = 2^16 and 2^20, next to a loop of single Robot.diff_ik calls.  Each figure is the median of repeated calls,
each ended by a device synchronise, after warm-up calls of the same shape.  Prints one JSON line (and writes it to
--out).

    PYTHONPATH=. python tools/diff_ik_rate.py [--reps 20] [--single 300] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from optik_amd import Robot  # noqa: E402

ROBOTS = {
    "panda": (os.path.join(ROOT, "optik_amd", "robots", "panda.urdf"), "panda_link0", "panda_link8"),
    "ur3e": (os.path.join(ROOT, "tests", "golden", "reference", "ur3e.urdf"), "ur_base_link", "ur_ee_link"),
}
HBM_PEAK = 8e12  # B/s, MI355X


def _median_s(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts)


def measure(name, sizes, reps, single):
    robot = Robot.from_urdf_file(*ROBOTS[name])
    n = robot.num_positions()
    lb, ub = (np.array(v) for v in robot.joint_limits())
    hc = robot.hip_chain()
    rng = np.random.default_rng(0)
    out = {"n": n, "batch": {}}
    # bytes a row moves through HBM in the device form: q, V, v_max in; alpha, v, status out
    row_bytes = 8 * (n + 6 + n) + 8 * (1 + n) + 4
    for B in sizes:
        x = rng.uniform(lb, ub, size=(B, n))
        V = rng.normal(size=(B, 6))
        vm = rng.uniform(0.2, 2.0, size=(B, n))
        q_d = torch.tensor(x.T.copy(), device="cuda:0")
        V_d = torch.tensor(V.T.copy(), device="cuda:0")
        vm_d = torch.tensor(vm.T.copy(), device="cuda:0")
        med, best = _median_s(lambda: hc.diff_ik_batch(q_d, V_d, vm_d), reps)
        hmed, hbest = _median_s(lambda: robot.diff_ik_batch_arrays(x, V, vm), max(3, reps // 4), warm=1)
        _, _, found = robot.diff_ik_batch_arrays(x, V, vm)
        out["batch"][str(B)] = {
            "device_call_ms_median": med * 1e3, "device_call_ms_min": best * 1e3,
            "device_configs_per_s": B / med,
            "bytes_per_config": row_bytes,
            "device_GBps": row_bytes * B / med / 1e9,
            "device_share_of_8TBps": row_bytes * B / med / HBM_PEAK,
            "host_call_ms_median": hmed * 1e3, "host_configs_per_s": B / hmed,
            "solved_fraction": float(found.mean()),
        }
    xs = rng.uniform(lb, ub, size=(single, n))
    Vs = rng.normal(size=(single, 6))
    vms = rng.uniform(0.2, 2.0, size=(single, n))
    robot.diff_ik(xs[0], Vs[0], vms[0])
    t0 = time.perf_counter()
    for k in range(single):
        robot.diff_ik(xs[k], Vs[k], vms[k])
    dt = time.perf_counter() - t0
    out["single_call"] = {"rows": single, "us_per_call": dt / single * 1e6, "configs_per_s": single / dt}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--single", type=int, default=300)
    ap.add_argument("--sizes", default=f"{1 << 16},{1 << 20}")
    ap.add_argument("--robots", default="panda,ur3e")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "diff_ik_rate.py measures on the GPU; there is nothing to measure without one"
    sizes = [int(s) for s in args.sizes.split(",")]
    from optik_amd import build
    rec = {"tool": "diff_ik_rate", "device": torch.cuda.get_device_name(0), "toolchain": build.toolchain_version(),
           "reps": args.reps, "robots": {r: measure(r, sizes, args.reps, args.single) for r in args.robots.split(",")}}
    line = json.dumps(rec, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
