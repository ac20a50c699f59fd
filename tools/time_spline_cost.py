#!/usr/bin/env python3
"""Cost of spline retiming beside the timing it follows, on the paths and shapes of
tools/time_cost.py: a Panda's roadmap plans resampled to 32 and to 64 waypoints, P = 1024, 8192 and 65 536 paths, timed
by optik_hip_path_time under the URDF's velocities and 7.5 rad/s^2.  The retiming keeps those two limits and adds the
Panda's published jerk limits (7500, 3750, 5000, 6250, 7500, 10 000, 10 000 rad/s^3).

  path_time            optik_hip_path_time on device tensors, every output written
  path_time_spline     optik_hip_path_time_spline on its result, every output written
  host_1, host_16      the serial reference of csrc/time_spline_measure.hpp compiled with g++ -O2 for the host, over the
                       same paths and times on 1 and on 16 threads

The device calls write into tensors allocated beforehand and run interleaved in one process, --reps rounds after one
warm-up round; the host runs take --reps rounds after one warm-up round too.  Each figure is the median wall time of a
call, synchronised before and after, with [min, max] beside it.  One JSON line per (P, L) -- with the median and the
largest slow-down factor, which limit binds how often, and the count of every status --, and the compiler's resource
line of the two kernels."""
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

PANDA_JERK = [7500.0, 3750.0, 5000.0, 6250.0, 7500.0, 10000.0, 10000.0]  # rad/s^3, the manufacturer's data sheet

HOST = r"""
#include <chrono>
#include <cstdlib>
#include <cstdio>
#include <thread>
#include <vector>
#include "time_spline_measure.hpp"

using namespace optik;

int main(int argc, char **argv) {
    // in.bin: n, L, P, vmax [n], amax [n], jmax [n], paths [P][L][n], times [P][L]; argv[2]: threads, argv[3]: reps
    // -> seconds per rep
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    double head[3];
    if (std::fread(head, sizeof(double), 3, f) != 3) return 2;
    const int n = (int)head[0], L = (int)head[1], threads = std::atoi(argv[2]), reps = std::atoi(argv[3]);
    const long long P = (long long)head[2];
    std::vector<double> lim(3 * n), paths((size_t)P * L * n), tin((size_t)P * L), fac(P);
    if (std::fread(lim.data(), sizeof(double), lim.size(), f) != lim.size()) return 2;
    if (std::fread(paths.data(), sizeof(double), paths.size(), f) != paths.size()) return 2;
    if (std::fread(tin.data(), sizeof(double), tin.size(), f) != tin.size()) return 2;
    std::fclose(f);
    std::vector<double> t((size_t)P * L), qd((size_t)P * L * n), qdd((size_t)P * L * n);
    for (int rep = 0; rep < reps; ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> th;
        for (int k = 0; k < threads; ++k)
            th.emplace_back([&, k] {
                for (long long p = P * k / threads; p < P * (k + 1) / threads; ++p)
                    fac[p] = splinetime::spline_reference(n, &paths[(size_t)p * L * n], n, L, L, &tin[(size_t)p * L], 0,
                                                          lim.data(), lim.data() + n, lim.data() + 2 * n,
                                                          &t[(size_t)p * L], &qd[(size_t)p * L * n],
                                                          &qdd[(size_t)p * L * n]).factor;
            });
        for (auto &x : th) x.join();
        std::printf("%.9f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    double sum = 0.0;
    for (long long p = 0; p < P; ++p) sum += fac[p];
    std::printf("# %.17g\n", sum);
    return 0;
}
"""


def host_baseline(workdir, paths, times, limits, threads, reps):
    """The seconds of `reps` runs, after one more to warm up, of the serial reference over paths [P, L, n] with times
    [P, L] on `threads` host threads, and the sum of the factors it found."""
    exe = os.path.join(workdir, "spline_host")
    if not os.path.exists(exe):
        src = os.path.join(workdir, "spline_host.cpp")
        with open(src, "w") as fh:
            fh.write(HOST)
        subprocess.run([shutil.which("g++") or "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-I",
                        os.path.join(ROOT, "optik_amd", "csrc"), src, "-o", exe], check=True)
    P, L, n = paths.shape
    fin = os.path.join(workdir, "in.bin")
    np.concatenate([[n, L, P], *limits, paths.ravel(), times.ravel()]).astype(np.float64).tofile(fin)
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
    vmax, amax, jmax = robot.velocity_limits(), np.full(hc.n, a.a_max), np.array(PANDA_JERK)
    vmax_d, amax_d, jmax_d = (torch.from_numpy(x).cuda() for x in (vmax, amax, jmax))
    work = {}
    for P in (1024, 8192, 65536):
        pick = found[torch.arange(P, device=found.device) % len(found)]
        path, lens = plan["path"][:, pick].contiguous(), plan["len"][pick].contiguous()
        for L in (32, 64):
            work[P, L] = hc.path_resample(path, lens, L)[0]
    timing = {key: hc.path_time(path, None, vmax_d, amax_d) for key, path in work.items()}
    smooth = {key: hc.path_time_spline(path, timing[key], jmax_d, amax_d, vmax_d) for key, path in work.items()}
    lib, calls = nat.lib(), {}

    def time_call(path, r):
        L, P = path.shape[0], path.shape[1]
        nat.check(lib.optik_hip_path_time(hc._h, _ptr(path), None, L, P, _ptr(vmax_d), _ptr(amax_d), _ptr(r["t"]),
                                          _ptr(r["qd"]), _ptr(r["qdd"]), _ptr(r["x"]), _ptr(r["duration"]),
                                          _ptr(r["status"]), _stream_ptr()))

    def spline_call(path, tm, r):
        L, P = path.shape[0], path.shape[1]
        nat.check(lib.optik_hip_path_time_spline(hc._h, _ptr(path), None, L, P, _ptr(tm["t"]), _ptr(tm["status"]),
                                                 _ptr(vmax_d), _ptr(amax_d), _ptr(jmax_d), _ptr(r["t"]), _ptr(r["qd"]),
                                                 _ptr(r["qdd"]), _ptr(r["duration"]), _ptr(r["factor"]),
                                                 _ptr(r["ratios"]), _ptr(r["status"]), _stream_ptr()))
    for key, path in work.items():
        again_t = {name: torch.empty_like(t) for name, t in timing[key].items()}
        again_s = {name: torch.empty_like(t) for name, t in smooth[key].items()}
        calls[("path_time",) + key] = lambda path=path, again=again_t: time_call(path, again)
        calls[("path_time_spline",) + key] = lambda key=key, path=path, again=again_s: spline_call(path, timing[key], again)
    times = {name: [] for name in calls}
    for rep in range(a.reps + 1):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
    workdir = tempfile.mkdtemp(prefix="time_spline_cost_")
    for (P, L), path in work.items():
        tm, r = timing[P, L], smooth[P, L]
        ok_in = (tm["status"] == 0).cpu().numpy()
        rows = np.ascontiguousarray(np.swapaxes(path.cpu().numpy(), 0, 1))[ok_in]
        trows = np.ascontiguousarray(tm["t"].cpu().numpy().T)[ok_in]
        h1, sum1 = host_baseline(workdir, rows, trows, (vmax, amax, jmax), 1, a.reps)
        h16, _ = host_baseline(workdir, rows, trows, (vmax, amax, jmax), 16, a.reps)
        host1, host16 = float(np.median(h1)), float(np.median(h16))
        status = r["status"].cpu().numpy()
        good = (status == 0) | (status == 4)
        fac, ratios = r["factor"].cpu().numpy(), r["ratios"].cpu().numpy()
        slowed = good & (fac > 1.0)
        tt, ts = times["path_time", P, L], times["path_time_spline", P, L]
        med_t, med_s = float(np.median(tt)), float(np.median(ts))
        print(json.dumps({
            "paths": P, "waypoints": L, "reps": a.reps, "plans_found": int(len(found)),
            "timed_inputs": int(ok_in.sum()),
            "status_counts": [int((status == s).sum()) for s in range(5)],
            "median_factor": round(float(np.median(fac[good])), 4), "max_factor": round(float(fac[good].max()), 4),
            "binding_v_a_j": [int(x) for x in np.bincount(ratios[slowed].argmax(axis=1), minlength=3)],
            "largest_ratio_minus_1": float(ratios[good].max() - 1.0),
            "path_time": {"ms": round(med_t * 1e3, 3), "min_max_ms": [round(min(tt) * 1e3, 3), round(max(tt) * 1e3, 3)],
                          "paths_per_s": round(P / med_t)},
            "path_time_spline": {"ms": round(med_s * 1e3, 3),
                                 "min_max_ms": [round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)],
                                 "paths_per_s": round(P / med_s)},
            "spline_over_path_time": round(med_s / med_t, 2),
            "host_1": {"ms": round(host1 * 1e3, 3), "min_max_ms": [round(min(h1) * 1e3, 3), round(max(h1) * 1e3, 3)],
                       "paths_per_s": round(len(rows) / host1)},
            "host_16": {"ms": round(host16 * 1e3, 3), "min_max_ms": [round(min(h16) * 1e3, 3), round(max(h16) * 1e3, 3)],
                        "paths_per_s": round(len(rows) / host16)},
            "device_over_host_1": round(host1 / len(rows) * P / med_s, 2),
            "device_over_host_16": round(host16 / len(rows) * P / med_s, 2),
            "factor_sums_agree": abs(float(fac[ok_in].sum()) - sum1) <= 1e-9 * abs(sum1)}))
    shutil.rmtree(workdir, ignore_errors=True)
    for name, r in sorted(build.kernel_resources().items()):
        if name in ("path_time_kernel", "path_time_spline_kernel"):
            print("# %s: %d VGPR, %d AGPR, %d SGPR, %d B scratch, %d B static LDS, %d waves/SIMD"
                  % (name, r["vgpr"], r["agpr"], r["sgpr"], r["scratch"], r["lds"], r["occupancy"]))


if __name__ == "__main__":
    main()
