#!/usr/bin/env python3
"""Cost of the tree planner under a pose constraint next to the unconstrained planner in the
same process: a Panda with the sphere model and the wall of section 5.18, upright(home, 0.1) at tol 0.05, iters 256,
step 0.5, max_nodes 256, poll 32, resolution 0.1.  Starts and goals are restart seeds projected onto the constraint
(outside the timing; the ones that did not project or are in collision are replaced by the next that are).

  constrained   HipChain.rrt_plan_constrained, G = 1
  plain         HipChain.rrt_plan_goals on the same starts and goals, G = 1

for Q = 1, 64 and 1024, interleaved, medians of --reps after one warm-up round with [min, max]; the time per iteration
the host loop launched each way (none where every query ended before the first iteration); the shares of projections
that ended PROJECTED; the found counts.  Beside them the roadmap answer to the same queries: seeds + projection +
constrained roadmap build at N = 8192, k = 16, and the plan over it.  No ratio is promised: what is printed is what
was measured, including where the new call loses.  Writes profiles/rrt_constrained_cost.txt."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from optik_amd import PoseConstraint, Robot, build  # noqa: E402
from optik_amd.collision import spheres_along_chain  # noqa: E402

PANDA = (os.path.join(ROOT, "optik_amd", "robots", "panda.urdf"), "panda_link0", "panda_link8")
HOME = [0.0, -0.785398163397, 0.0, -2.35619449019, 0.0, 1.57079632679, 0.785398163397]
WALL = [0.55, 0.0, 0.45, 0.0, 0.0, 0.0, 1.0, 0.2, 0.01, 0.25]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def stats(ts):
    return {"ms": round(float(np.median(ts)) * 1e3, 3), "min_max_ms": [round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)]}


def launched(iters_used, status, iters, poll):
    """The step kernels the host loop launched: it polls at iterations 0, poll, 2 poll, ... and stops at the first poll
    at or after the last query's end, so a batch that rule 0 ends (0 iterations used) costs one launch and nothing
    more; that one launch commits and checks no motion, so such a batch has no time per iteration (None)."""
    used = int(iters_used.max())
    ended = bool((status != 1).all() or used < iters)
    return min(iters, -(-used // poll) * poll + 1) if ended else iters


def per_iteration(seconds, iters_used, n_launched):
    return round(seconds * 1e6 / n_launched, 2) if int(iters_used.max()) > 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--iters", type=int, default=256)
    ap.add_argument("--step", type=float, default=0.5)
    ap.add_argument("--max-nodes", type=int, default=256)
    ap.add_argument("--poll", type=int, default=32)
    ap.add_argument("--resolution", type=float, default=0.1)
    ap.add_argument("--tol", type=float, default=0.05)
    ap.add_argument("--roadmap-nodes", type=int, default=8192)
    ap.add_argument("--roadmap-k", type=int, default=16)
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    frames, centers, radii = spheres_along_chain(robot, 0.05, 2)
    robot.set_collision_model(frames, centers, radii, self_pairs=None)
    robot.set_world(boxes=[np.array(WALL)])
    hc = robot._device_chain()
    c = PoseConstraint.upright(np.array(robot.fk(HOME)), 0.1)
    h = a.resolution
    lines = [f"# tools/rrt_constrained_cost.py -- {torch.cuda.get_device_name(0)}; {build.toolchain_version()}",
             f"# Panda, the wall of section 5.18, upright(home, 0.1), tol {a.tol}; medians of {a.reps} after a warm-up"]
    # the ends: projected seeds that are free
    seeds = hc.seed_batch(1 + 65536, 8 * max(a.queries))
    p = hc.constraint_project_batch(seeds, c)
    good = (p["status"] == 0) & hc.collision_batch(p["x"])[1].bool()
    ends = p["x"][:, good].contiguous()
    for Q in a.queries:
        starts, goals = ends[:, :Q].contiguous(), ends[:, Q:2 * Q].contiguous()
        assert goals.shape[1] == Q, "too few projected seeds"
        args = dict(first=0, max_nodes=a.max_nodes, Lmax=64, poll=a.poll)
        g3 = goals[None].contiguous()
        calls = {"constrained": lambda: hc.rrt_plan_constrained(starts, g3, None, c, a.tol, a.iters, a.step, h, **args),
                 "plain": lambda: hc.rrt_plan_goals(starts, g3, None, a.iters, a.step, h, **args)}
        times, out = {name: [] for name in calls}, {}
        for rep in range(a.reps + 1):
            for name, fn in calls.items():
                out[name], dt = timed(fn)
                if rep:
                    times[name].append(dt)
        res = {"queries": Q, "iters": a.iters, "step": a.step, "max_nodes": a.max_nodes, "poll": a.poll, "resolution": h}
        for name, ts in times.items():
            r = out[name]
            n_it = launched(r["iters"], r["status"], a.iters, a.poll)
            res[name] = dict(stats(ts), iterations_launched=n_it,
                             us_per_iteration=per_iteration(float(np.median(ts)), r["iters"], n_it),
                             status_counts=[int((r["status"] == s).sum()) for s in range(4)])
        per = [res[name]["us_per_iteration"] for name in ("constrained", "plain")]
        res["constrained_over_plain_per_iteration"] = round(per[0] / per[1], 3) if None not in per else None
        pr = out["constrained"]["projected"].sum(dim=1)
        res["projections"] = [int(pr[0]), int(pr[1])]
        res["projected_share"] = round(float(pr[1]) / max(int(pr[0]), 1), 4)
        # the roadmap's answer to the same queries
        sq, gq = starts.t().contiguous().cpu().numpy(), goals.t().contiguous().cpu().numpy()
        ts_b, ts_p = [], []
        for rep in range(a.reps + 1):
            rm, dt_b = timed(lambda: robot.build_constrained_roadmap(c, a.tol, a.roadmap_nodes, a.roadmap_k, h))
            plan, dt_p = timed(lambda: robot.plan_constrained_paths(rm, sq, gq))
            if rep:
                ts_b.append(dt_b)
                ts_p.append(dt_p)
        res["roadmap_build"] = dict(stats(ts_b), nodes=a.roadmap_nodes, k=a.roadmap_k, projected=rm.projected)
        res["roadmap_plan"] = dict(stats(ts_p), status_counts=[int((plan["status"] == s).sum()) for s in range(4)])
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    for name, r in sorted(build.kernel_resources().items()):
        if name.startswith("rrt_"):
            lines.append("# %s: %d VGPR, %d AGPR, %d SGPR, %d B scratch, %d B LDS, %d waves/SIMD"
                         % (name, r["vgpr"], r["agpr"], r["sgpr"], r["scratch"], r["lds"], r["occupancy"]))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "rrt_constrained_cost.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(ln for ln in lines if ln.startswith("#")))


if __name__ == "__main__":
    main()
