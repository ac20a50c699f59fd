#!/usr/bin/env python3
"""Cost of path timing and trajectory sampling on a Panda with the model and world of
tools/collision_cost.py: the plans of HipChain.roadmap_plan over an N = 8192, k = 16 roadmap with status 0, as
tools/shortcut_cost.py makes them, resampled by HipChain.path_resample to 32 and to 64 waypoints and repeated to fill
P = 1024, 8192 and 65 536 paths.  Limits: the URDF's velocities, 7.5 rad/s^2.

  path_time            optik_hip_path_time on device tensors, every output written
  trajectory_sample    optik_hip_trajectory_sample of its result, 256 samples per path
  host_1, host_16      what a user of the library without it would do: the serial reference of csrc/time_measure.hpp
                       compiled with g++ -O2 for the host, over the same paths on 1 and on 16 threads

The device calls write into tensors allocated beforehand (HipChain.path_time / trajectory_sample allocate theirs per
call, which at a thousand paths costs about as much as the kernel) and run interleaved in one process, --reps rounds
after one warm-up round; the host runs take --reps rounds after one warm-up round too.  Each figure is the median wall
time of a call, synchronised before and after, with [min, max] beside it.  One JSON line per (P, L), and the compiler's resource line of the
kernels."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
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

HOST = r"""
#include <chrono>
#include <cstdlib>
#include <cstdio>
#include <thread>
#include <vector>
#include "time_measure.hpp"

using namespace optik;

int main(int argc, char **argv) {
    // paths.bin: n, L, P, vmax [n], amax [n], paths [P][L][n]; argv[2]: threads, argv[3]: reps -> seconds per rep
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    double head[3];
    if (std::fread(head, sizeof(double), 3, f) != 3) return 2;
    const int n = (int)head[0], L = (int)head[1], threads = std::atoi(argv[2]), reps = std::atoi(argv[3]);
    const long long P = (long long)head[2];
    std::vector<double> lim(2 * n), paths((size_t)P * L * n), dur(P);
    if (std::fread(lim.data(), sizeof(double), lim.size(), f) != lim.size()) return 2;
    if (std::fread(paths.data(), sizeof(double), paths.size(), f) != paths.size()) return 2;
    std::fclose(f);
    std::vector<double> t((size_t)P * L), qd((size_t)P * L * n), qdd((size_t)P * L * n);
    for (int rep = 0; rep < reps; ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> th;
        for (int k = 0; k < threads; ++k)
            th.emplace_back([&, k] {
                for (long long p = P * k / threads; p < P * (k + 1) / threads; ++p)
                    dur[p] = timing::time_reference(n, &paths[(size_t)p * L * n], n, L, L, lim.data(), lim.data() + n,
                                                    &t[(size_t)p * L], &qd[(size_t)p * L * n], &qdd[(size_t)p * L * n],
                                                    nullptr).duration;
            });
        for (auto &x : th) x.join();
        std::printf("%.9f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    double sum = 0.0;
    for (long long p = 0; p < P; ++p) sum += dur[p] == dur[p] ? dur[p] : 0.0;
    std::printf("# %.17g\n", sum);
    return 0;
}
"""


def host_baseline(workdir, paths, vmax, amax, threads, reps):
    """The seconds of `reps` runs, after one more to warm up, of the serial reference over paths [P, L, n] on `threads`
    host threads, and the sum of the durations it found."""
    exe = os.path.join(workdir, "time_host")
    if not os.path.exists(exe):
        src = os.path.join(workdir, "time_host.cpp")
        with open(src, "w") as fh:
            fh.write(HOST)
        subprocess.run([shutil.which("g++") or "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-I",
                        os.path.join(ROOT, "optik_amd", "csrc"), src, "-o", exe], check=True)
    P, L, n = paths.shape
    fin = os.path.join(workdir, "paths.bin")
    np.concatenate([[n, L, P], vmax, amax, paths.ravel()]).astype(np.float64).tofile(fin)
    out = subprocess.run([exe, fin, str(threads), str(reps + 1)], check=True, capture_output=True,
                         text=True).stdout.split("\n")
    return [float(x) for x in out[1:reps + 1]], float(out[reps + 1][2:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nodes", type=int, default=8192)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--plans", type=int, default=1024)
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--a-max", type=float, default=7.5)
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
    vmax = robot.velocity_limits()
    amax = np.full(hc.n, a.a_max)
    vmax_d, amax_d = torch.from_numpy(vmax).cuda(), torch.from_numpy(amax).cuda()
    work = {}
    for P in (1024, 8192, 65536):
        pick = found[torch.arange(P, device=found.device) % len(found)]
        path, lens = plan["path"][:, pick].contiguous(), plan["len"][pick].contiguous()
        for L in (32, 64):
            work[P, L] = hc.path_resample(path, lens, L)[0]
    timing = {key: hc.path_time(path, None, vmax_d, amax_d) for key, path in work.items()}
    dts = {key: float(r["duration"][r["status"] == 0].max()) / (a.samples - 1) for key, r in timing.items()}
    lib, calls = nat.lib(), {}

    def time_call(path, r):
        L, P = path.shape[0], path.shape[1]
        nat.check(lib.optik_hip_path_time(hc._h, _ptr(path), None, L, P, _ptr(vmax_d), _ptr(amax_d), _ptr(r["t"]),
                                          _ptr(r["qd"]), _ptr(r["qdd"]), _ptr(r["x"]), _ptr(r["duration"]),
                                          _ptr(r["status"]), _stream_ptr()))

    def sample_call(path, r, dt, q, v):
        L, P = path.shape[0], path.shape[1]
        nat.check(lib.optik_hip_trajectory_sample(hc._h, _ptr(path), None, L, P, _ptr(r["t"]), _ptr(r["qd"]),
                                                  _ptr(r["status"]), dt, a.samples, _ptr(q), _ptr(v), _stream_ptr()))
    for key, path in work.items():
        again = {name: torch.empty_like(t) for name, t in timing[key].items()}
        q = torch.empty((a.samples, path.shape[1], hc.n), dtype=torch.float64, device=path.device)
        v = torch.empty_like(q)
        calls[("path_time",) + key] = lambda path=path, again=again: time_call(path, again)
        calls[("trajectory_sample",) + key] = lambda key=key, path=path, q=q, v=v: sample_call(path, timing[key],
                                                                                            dts[key], q, v)
    times = {name: [] for name in calls}
    for rep in range(a.reps + 1):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
    workdir = tempfile.mkdtemp(prefix="time_cost_")
    for (P, L), path in work.items():
        r = timing[P, L]
        rows = np.ascontiguousarray(np.swapaxes(path.cpu().numpy(), 0, 1))
        h1, sum1 = host_baseline(workdir, rows, vmax, amax, 1, a.reps)
        h16, _ = host_baseline(workdir, rows, vmax, amax, 16, a.reps)
        host1, host16 = float(np.median(h1)), float(np.median(h16))
        ok = (r["status"] == 0).cpu().numpy()
        dev_sum = float(np.sum(r["duration"].cpu().numpy()[ok]))
        tt, ts = times["path_time", P, L], times["trajectory_sample", P, L]
        med = float(np.median(tt))
        print(json.dumps({
            "paths": P, "waypoints": L, "reps": a.reps, "plans_found": int(len(found)),
            "status_counts": [int((r["status"] == s).sum()) for s in range(4)],
            "median_duration_s": round(float(np.median(r["duration"].cpu().numpy()[ok])), 4),
            "path_time": {"ms": round(med * 1e3, 3), "min_max_ms": [round(min(tt) * 1e3, 3), round(max(tt) * 1e3, 3)],
                          "paths_per_s": round(P / med)},
            "trajectory_sample": {"samples": a.samples, "ms": round(float(np.median(ts)) * 1e3, 3),
                                  "min_max_ms": [round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)],
                                  "samples_per_s": round(P * a.samples / float(np.median(ts)))},
            "host_1": {"ms": round(host1 * 1e3, 3), "min_max_ms": [round(min(h1) * 1e3, 3), round(max(h1) * 1e3, 3)],
                       "paths_per_s": round(P / host1)},
            "host_16": {"ms": round(host16 * 1e3, 3), "min_max_ms": [round(min(h16) * 1e3, 3), round(max(h16) * 1e3, 3)],
                        "paths_per_s": round(P / host16)},
            "device_over_host_1": round(host1 / med, 2), "device_over_host_16": round(host16 / med, 2),
            "duration_sums_agree": abs(dev_sum - sum1) <= 1e-9 * abs(sum1)}))
    shutil.rmtree(workdir, ignore_errors=True)
    for name, r in sorted(build.kernel_resources().items()):
        if name in ("path_time_kernel", "trajectory_sample_kernel"):
            print("# %s: %d VGPR, %d AGPR, %d B scratch, %d B LDS, %d waves/SIMD"
                  % (name, r["vgpr"], r["agpr"], r["scratch"], r["lds"], r["occupancy"]))


if __name__ == "__main__":
    main()
