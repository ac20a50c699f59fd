#!/usr/bin/env python3
"""Cost of shortcutting under a pose constraint next to the unconstrained shortcut in the same
process: a Panda with the sphere model and the wall of section 5.18, upright(home, 0.3) at tol 0.05, V = 32 vertices,
resolution 0.05.  The paths are P walks of 8 waypoints, every waypoint a restart seed's neighbour projected onto the
constraint (outside the timing).

  constrained   HipChain.path_shortcut_constrained
  plain         HipChain.path_shortcut on the same paths (the code before this section)
  masked        HipChain.constraint_motion_mask on the constrained call's own vertex pairs, the flags being the motion
                check's: a pair the collision check blocks, or does not sample, is skipped
  unmasked      HipChain.constraint_motion_batch over all the pairs: the same verdicts where the flag was set

interleaved, medians of --reps after one warm-up round with [min, max].  No ratio is promised: what is printed is what
was measured.  Writes profiles/shortcut_constrained_cost.txt."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--paths", type=int, default=256)
    ap.add_argument("--waypoints", type=int, default=8)
    ap.add_argument("--vertices", type=int, default=32)
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--tol", type=float, default=0.05)
    ap.add_argument("--span", type=float, default=0.4)
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    frames, centers, radii = spheres_along_chain(robot, 0.05, 2)
    robot.set_collision_model(frames, centers, radii, self_pairs=None)
    robot.set_world(boxes=[np.array(WALL)])
    hc = robot._device_chain()
    c = PoseConstraint.upright(np.array(robot.fk(HOME)), 0.3)
    P, L, V, h = a.paths, a.waypoints, a.vertices, a.resolution
    n = hc.n
    # the paths: walks from the home configuration, every waypoint projected (the ones that do not project stay put)
    rng = np.random.default_rng(1)
    lo, hi = (torch.from_numpy(np.asarray(v, dtype=np.float64)).cuda() for v in robot.joint_limits())
    q = torch.tensor(HOME, dtype=torch.float64, device="cuda")[:, None].repeat(1, P).contiguous()
    way = []
    for _ in range(L):
        step = torch.from_numpy(rng.uniform(-a.span, a.span, (n, P))).cuda()
        cand = torch.minimum(torch.maximum(q + step, lo[:, None]), hi[:, None]).contiguous()
        p = hc.constraint_project_batch(cand, c)
        q = torch.where((p["status"] == 0)[None, :], p["x"], q).contiguous()
        way.append(q.t().contiguous())
    path = torch.stack(way).contiguous()                     # [L, P, n]
    args = dict(resolution=h, vertices=V, hop_penalty=h, max_waypoints=L)
    res0 = hc.path_shortcut_constrained(path, None, c, a.tol, **args)
    # the constrained call's own pairs: shortcut_constrained_measure.hpp's vertices are not returned, so the pairs
    # timed are those of the found routes' inputs -- every pair i < j of each input's waypoints, L (L - 1) / 2 a path
    i, j = np.triu_indices(L, 1)
    qa = path[i].reshape(-1, n).t().contiguous()
    qb = path[j].reshape(-1, n).t().contiguous()
    B = qa.shape[1]
    free = hc.collision_motion_batch(qa, qb, h, clearance=False)[1].to(torch.uint8).contiguous()
    calls = {"constrained": lambda: hc.path_shortcut_constrained(path, None, c, a.tol, **args),
             "plain": lambda: hc.path_shortcut(path, None, h, V, h, L),
             "masked": lambda: hc.constraint_motion_mask(qa, qb, h, c, a.tol, free.clone()),
             "unmasked": lambda: hc.constraint_motion_batch(qa, qb, h, c, a.tol)}
    times, out = {name: [] for name in calls}, {}
    for rep in range(a.reps + 1):
        for name, fn in calls.items():
            out[name], dt = timed(fn)
            if rep:
                times[name].append(dt)
    ok = out["unmasked"][1]
    assert torch.equal(out["masked"].bool(), free.bool() & ok), "the masked verdict is the AND of the two checks"
    res = {"paths": P, "waypoints": L, "vertices": V, "resolution": h, "tol": a.tol, "pairs_timed": B,
           "pairs_free": int(free.sum()), "pairs_ok": int(ok.sum())}
    for name, ts in times.items():
        res[name] = stats(ts)
    res["constrained_over_plain"] = round(res["constrained"]["ms"] / res["plain"]["ms"], 3)
    res["masked_over_unmasked"] = round(res["masked"]["ms"] / res["unmasked"]["ms"], 3)
    res["masked"]["note"] = "includes the clone of the flags"
    for name in ("constrained", "plain"):
        r = out[name]
        res[name]["status_counts"] = [int((r["status"] == s).sum()) for s in range(4)]
        res[name]["mean_len"] = round(float(r["len"].double().mean()), 3)
        res[name]["mean_cost_over_cost_in"] = round(float((r["cost"] / r["cost_in"]).mean()), 4)
    pr = res0["projected"].sum(dim=1)
    res["projections"] = [int(pr[0]), int(pr[1])]
    lines = [f"# tools/shortcut_constrained_cost.py -- {torch.cuda.get_device_name(0)}; {build.toolchain_version()}",
             f"# Panda, the wall of section 5.18, upright(home, 0.3), tol {a.tol}; medians of {a.reps} after a warm-up",
             json.dumps(res)]
    for name, r in sorted(build.kernel_resources().items()):
        if name.startswith("shortcut_c") or name.startswith("shortcut_route") or name.startswith("constraint_motion_mask"):
            lines.append("# %s: %d VGPR, %d AGPR, %d SGPR, %d B scratch, %d B LDS, %d waves/SIMD"
                         % (name, r["vgpr"], r["agpr"], r["sgpr"], r["scratch"], r["lds"], r["occupancy"]))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "shortcut_constrained_cost.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    robot.clear_collision_model()
    robot.set_world()


if __name__ == "__main__":
    main()
