#!/usr/bin/env python3
"""Cost of collision repair on the scene of examples/ik_repair.py (a Panda, 9 spheres along
its links, a table; influence 0.1, safety 0.02, the default step and budget):

  repair alone      HipChain.collision_repair_batch on B = 2^16 uniform configurations
  ik_region         HipChain.ik_region at T = 256 targets x 256 restarts -- position-only boxes of 2 cm low over and
                    inside the table -- without `repair` (the parent commit's call: the same entry, bit for bit) and
                    with it, interleaved in one process, with the rows returned both ways

Kernel times come from a `rocprofv3 --kernel-trace --stats` run of its own: without --profile this tool starts
`rocprofv3 ... -- python tools/repair_cost.py --profile` as a child and reads the kernel statistics it leaves; the
calls are told apart by their kernels (region_repair_kernel runs only with `repair`).  Wall times of the calls are
printed beside them (median of --reps after a warm-up).  What it prints goes to profiles/repair_cost.txt."""
import argparse
import csv
import glob
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PANDA = [os.path.join(ROOT, "optik_amd", "robots", "panda.urdf"), "panda_link0", "panda_link8"]


def workload(reps):
    import numpy as np
    import torch
    from optik_amd import Robot
    from optik_amd.device import HipChain
    spec = importlib.util.spec_from_file_location("ik_repair_example", os.path.join(ROOT, "examples", "ik_repair.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    robot = Robot.from_urdf_file(*PANDA)
    hc = HipChain(**robot.chain_tables())
    hc.set_collision_model(*ex.model(robot), self_pairs="auto", margin=0.0)
    hc.set_world(boxes=[ex.TABLE])
    B, T, R, K = 1 << 16, 256, 256, 8
    q = hc.seed_batch(1, B)
    rng = np.random.default_rng(1)
    inf, p = np.inf, 0.02
    regions = np.array([np.concatenate([[rng.uniform(0.35, 0.75), rng.uniform(-0.3, 0.3), rng.uniform(0.12, 0.3)],
                                        [1.0, 0.0, 0.0, 0.0], [-p] * 3 + [-inf] * 3, [p] * 3 + [inf] * 3])
                        for _ in range(T)])
    reg = torch.tensor(regions, device=q.device)
    x0 = torch.tensor(np.tile(np.array(ex.GOAL), (T, 1)), device=q.device)
    rep = dict(influence=ex.INFLUENCE, safety=ex.SAFETY)
    calls = {"repair_alone": lambda: hc.collision_repair_batch(q, ex.INFLUENCE, ex.SAFETY),
             "ik_region": lambda: hc.ik_region(reg, x0, 0, R, K, 0.1),
             "ik_region_repair": lambda: hc.ik_region(reg, x0, 0, R, K, 0.1, repair=rep)}
    times, out = {k: [] for k in calls}, {}
    for r in range(reps + 1):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[name] = fn()
            torch.cuda.synchronize()
            if r:
                times[name].append(time.perf_counter() - t0)
    res = {"B": B, "T": T, "R": R, "K": K, "reps": reps}
    for name, ts in times.items():
        res[name + "_wall_ms"] = {"median": round(float(np.median(ts)) * 1e3, 3),
                                  "min_max": [round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)]}
    st = out["repair_alone"]["status"]
    res["repair_alone_status_counts"] = [int((st == s).sum()) for s in range(4)]
    res["repair_alone_moved_rows"] = int((out["repair_alone"]["iterations"] > 0).sum())
    for name in ("ik_region", "ik_region_repair"):
        c = out[name]["count"]
        res[name + "_rows_returned"] = int(c.sum())
        res[name + "_targets_without_a_row"] = int((c == 0).sum())
    res["restarts_repaired"] = int(out["ik_region_repair"]["repaired"].sum())
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="the workload alone (the child under rocprofv3)")
    a = ap.parse_args()
    if a.profile:
        workload(a.reps)
        return 0
    d = tempfile.mkdtemp(prefix="repair_cost_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "repair_cost", "--",
           sys.executable, os.path.abspath(__file__), "--profile", "--reps", str(a.reps)]
    # (the workload is 4 rounds of about a second of kernels; the limit covers the profiler's start and its reports)
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
    except subprocess.TimeoutExpired:
        sys.stderr.write("the profiled child did not finish within 300 s\n")
        return 1
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        return 1
    print(line[-1])
    calls = a.reps + 1
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.stderr.write("no kernel statistics were written\n" + p.stderr[-2000:])
        return 1
    print("# kernel times (rocprofv3 --kernel-trace --stats), per call = total / launches")
    with open(files[0]) as fh:
        for row in csv.DictReader(fh):
            name = row["Name"]
            if not any(k in name for k in ("repair_kernel", "ik_region_kernel", "collision_key_kernel", "solutions")):
                continue
            n, total = int(row["Calls"]), float(row["TotalDurationNs"])
            print("# %-60s %3d launches, %10.3f ms each (min %.3f, max %.3f)"
                  % (name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][-60:], n, total / n * 1e-6, float(row["MinNs"]) * 1e-6, float(row["MaxNs"]) * 1e-6))
    print(f"# ({calls} calls of each: one warm-up and {a.reps} timed; ik_region's kernels run in both region calls,"
          " region_repair_kernel only with repair)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
