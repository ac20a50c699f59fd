#!/usr/bin/env python3
"""Generates tests/golden/generated/solver_edge_scenarios.json: the inputs that drive the SLSQP restart solver to the
endings a reachable target with O(1) weights never takes ("Solver endings off the reachable path").

Each entry is plain data -- robot (a key of tests/conftest.py:ROBOT_SPECS), target pose [t, quat(i,j,k,w)], caller
seed x0, SolverConfig keywords, optional ee offset, restart range, and whether the -m gpu tests launch it:

  zero_weights    all six weights 0, tol_f = 0: the gradient is 0, five Hessian resets, SLSQP mode 8, zero step -> XTOL
  tiny_weights    weights 1e-160: f and g underflow to 0, the same ending through stopval's far side
  big_weights     weights 1e6: the LDP's dual test fails (LSQ mode 4) -> FAILURE
  stiff_weights / stiffer_weights   weights 1e8 / 1e12: NNLS leaves a zero residual (rnorm <= 0, LSQ mode 4) ->
                  FAILURE; about one restart in a thousand makes the negative LDL' update repair t (t >= 0), hence
                  2048 restarts
  huge_weights    weights 1e150: the LDL' factor degenerates, |E(j,j)| < EPMACH (LSQ mode 5) -> ROUNDOFF_LIMITED
  mixed_weights   (1e4, 1e-4, 1) / (1e-4, 1, 1e4), tol_f = 1e-9: long runs, FAILURE and FTOL mixed
  far             target at 4 x the reach: every restart stalls -> FTOL
  far_tols        the same with tol_f = 0, tol_df = 1e-30, tol_dx = 1e-14: FTOL and XTOL mixed
  corner_lb/_ub/_zero  target = FK(lb) / FK(ub) / FK(0), tol_f = 1e-12: bounds active at the solution
  cap             tol_f = tol_df = 0, tol_dx = -1 on a 6-joint arm: bounded only by the evaluation cap (never
                  launched on the GPU)
  ldl_repair      weights 1e8 again, over a restart range picked so that one of its FIRST 12 restarts makes the
                  negative LDL' update repair t (`if (t >= 0.0) t = EPMACH / sigma`): the ranges in PLAN were found by
                  counting that line's executions restart by restart over restarts 0 .. 8191 of these inputs (one to
                  eight restarts in 8192 take it); the census test checks that they still do.  On the UR10, restart 88
                  toward FK(0) also takes it, twice, on its way to a solution: the corner_zero entry that begins at 80
  nonfinite       weights 1e153: in a few restarts f overflows at a trial point, the line search takes its
                  non-finite branch and never recovers: they run to the evaluation cap (never launched on the GPU)

The restart ranges of the `cap` and `nonfinite` entries are chosen from the oracle: the first window of 12 restarts of
which one to four reach the cap.  The inputs of a gpu entry are drawn again until the oracle's longest restart is within
5000 evaluations (mixed_weights has tails beyond that).
Deterministic: numpy's default_rng with a fixed seed per (robot, class); floats written with repr (bit-exact).

Usage: python tools/gen_solver_edge_scenarios.py          (rewrites the file)
"""
from __future__ import annotations

import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from conftest import ROBOT_SPECS  # noqa: E402
from oracle import binding as ob  # noqa: E402
from oracle import urdf_chain  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "generated", "solver_edge_scenarios.json")

W = lambda v: dict(linear_weight=(v, v, v), angular_weight=(v, v, v))  # noqa: E731
CLASS_CONFIG = {
    "zero_weights": dict(tol_f=0.0, **W(0.0)),
    "tiny_weights": dict(**W(1e-160)),
    "big_weights": dict(**W(1e6)),
    "stiff_weights": dict(**W(1e8)),
    "stiffer_weights": dict(**W(1e12)),
    "huge_weights": dict(**W(1e150)),
    "mixed_weights": dict(tol_f=1e-9, linear_weight=(1e4, 1e-4, 1.0), angular_weight=(1e-4, 1.0, 1e4)),
    "far": dict(),
    "far_tols": dict(tol_f=0.0, tol_df=1e-30, tol_dx=1e-14),
    "corner_lb": dict(tol_f=1e-12),
    "corner_ub": dict(tol_f=1e-12),
    "corner_zero": dict(tol_f=1e-12),
    "cap": dict(tol_f=0.0, tol_df=0.0, tol_dx=-1.0),
    "nonfinite": dict(**W(1e153)),
    "ldl_repair": dict(**W(1e8)),
}

# (robot, class, solution mode, restart range, ee offset?, launched on the GPU?)  Three joint-count groups, each
# with every class: n <= 7, n = 8, n >= 9.
PLAN = [
    # ---- n <= 7
    ("panda", "zero_weights", "speed", (0, 256), False, True),
    ("ur10", "tiny_weights", "quality", (0, 256), False, True),
    ("ur3e", "big_weights", "speed", (0, 256), False, True),
    ("panda_hand", "big_weights", "quality", (4097, 4097 + 256), False, True),
    ("panda", "stiff_weights", "speed", (0, 2048), False, True),
    ("ur10", "stiffer_weights", "quality", (0, 2048), False, True),
    ("ur10", "huge_weights", "speed", (0, 256), False, True),
    ("panda", "huge_weights", "quality", (0, 256), True, True),
    ("panda", "mixed_weights", "speed", (0, 256), False, True),
    ("ur3e", "mixed_weights", "quality", (0, 256), False, True),
    ("panda3", "far", "speed", (0, 256), False, True),
    ("ur10", "far", "quality", (2**33 + 5, 2**33 + 5 + 256), False, True),
    ("panda_hand", "far_tols", "speed", (0, 256), False, True),
    ("ur3e", "far_tols", "quality", (0, 256), False, True),
    ("panda", "corner_lb", "quality", (0, 512), False, True),
    ("ur10", "corner_ub", "speed", (0, 256), False, True),
    ("panda_hand", "corner_zero", "speed", (0, 256), False, True),
    ("panda3", "corner_ub", "quality", (0, 256), False, True),
    ("ur10", "ldl_repair", "speed", (6046, 6046 + 256), False, True),       # restart 6051 repairs t
    ("panda", "ldl_repair", "quality", (7255, 7255 + 256), False, True),    # restart 7260
    ("ur10", "corner_zero", "quality", (80, 80 + 256), False, True),        # restart 88 (twice, and succeeds)
    ("ur10", "cap", "speed", None, False, False),
    ("ur3e", "nonfinite", "speed", None, False, False),
    # ---- n = 8
    ("arm8", "zero_weights", "quality", (0, 256), False, True),
    ("arm8", "tiny_weights", "speed", (0, 256), False, True),
    ("arm8", "big_weights", "speed", (1, 257), False, True),
    ("arm8", "stiff_weights", "quality", (0, 2048), False, True),
    ("arm8", "stiffer_weights", "speed", (0, 2048), False, True),
    ("arm8", "huge_weights", "quality", (0, 256), True, True),
    ("arm8", "mixed_weights", "speed", (0, 256), False, True),
    ("arm8", "far", "speed", (0, 256), False, True),
    ("arm8", "far_tols", "quality", (0, 256), False, True),
    ("arm8", "corner_lb", "speed", (0, 256), False, True),
    ("arm8", "corner_ub", "quality", (0, 256), False, True),
    ("arm8", "corner_zero", "speed", (0, 256), False, True),
    ("arm8", "ldl_repair", "speed", (3998, 3998 + 256), False, True),       # restarts 4003, 4056
    ("arm8", "nonfinite", "speed", None, False, False),
    # ---- n >= 9
    ("arm9", "zero_weights", "speed", (0, 256), False, True),
    ("arm10", "tiny_weights", "quality", (0, 256), False, True),
    ("arm10", "big_weights", "speed", (0, 256), False, True),
    ("arm16", "big_weights", "quality", (0, 256), False, True),
    ("arm10", "stiff_weights", "speed", (0, 2048), False, True),
    ("arm9", "stiffer_weights", "quality", (0, 2048), False, True),
    ("arm9", "huge_weights", "quality", (0, 256), True, True),
    ("arm10", "huge_weights", "speed", (4097, 4097 + 256), False, True),
    ("arm10", "mixed_weights", "speed", (0, 256), False, True),
    ("arm9", "mixed_weights", "quality", (0, 256), False, True),
    ("arm16", "far", "speed", (0, 256), False, True),
    ("arm10", "far_tols", "quality", (0, 256), False, True),
    ("arm9", "corner_lb", "speed", (0, 256), False, True),
    ("arm10", "corner_ub", "quality", (0, 256), False, True),
    ("arm16", "corner_zero", "speed", (0, 256), False, True),
    ("arm10", "ldl_repair", "quality", (1504, 1504 + 256), False, True),    # restart 1509
    ("arm16", "ldl_repair", "speed", (260, 260 + 256), False, True),        # restart 265
    ("arm10", "nonfinite", "speed", None, False, False),
]

CAP_WINDOW = 12      # restarts in a cap / nonfinite entry
CAP_MAX_CAPPED = 4   # ... of which at most this many reach the evaluation cap (and at least one does)
GPU_MAX_EVALS = 5000  # the bound on a gpu entry's longest restart (tests/test_oracle_solver_edge_census.py)


def group_of(n):
    return "n<=7" if n <= 7 else ("n=8" if n == 8 else "n>=9")


def load(name):
    path, base, ee = ROBOT_SPECS[name]
    with open(path) as fh:
        d = urdf_chain.chain_from_urdf(fh.read(), base, ee)
    return d, ob.make_chain(**d)


def make_inputs(d, ch, cls, rng, ee_pose):
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    x0 = rng.uniform(lb, ub)
    q = rng.uniform(lb, ub)
    if cls == "corner_lb":
        q = lb.copy()
    elif cls == "corner_ub":
        q = ub.copy()
    elif cls == "corner_zero":
        q = np.zeros_like(lb)
    _, tgt = ob.fk(ch, q, ee_offset=ee_pose)
    if cls in ("far", "far_tols"):
        reach = max(np.linalg.norm(ob.fk(ch, rng.uniform(lb, ub), ee_offset=ee_pose)[1][:3]) for _ in range(64))
        t = tgt[:3] / np.linalg.norm(tgt[:3])
        tgt = np.concatenate([4.0 * reach * t, tgt[3:]])
    return tgt, x0


def pick_cap_window(ch, cfg_kw, tgt, x0):
    """The first window of CAP_WINDOW restarts with 1 .. CAP_MAX_CAPPED of them at the evaluation cap."""
    R = 256
    ref = ob.ik(ch, ob.make_config(**cfg_kw), tgt, x0, 0, R, n_threads=os.cpu_count() or 4, early_exit=False,
                per_restart=True)
    capped = ref["status"] == ob.RES_ITER_CAP
    for b in range(0, R - CAP_WINDOW + 1):
        if 1 <= int(capped[b:b + CAP_WINDOW].sum()) <= CAP_MAX_CAPPED:
            return b, b + CAP_WINDOW
    return None


def build_scenarios():
    ob.build()
    robots, out = {}, []
    for robot, cls, mode, rng_range, with_ee, gpu in PLAN:
        if robot not in robots:
            robots[robot] = load(robot)
        d, ch = robots[robot]
        rng = np.random.default_rng(zlib.crc32(f"{robot}/{cls}/{mode}".encode()))
        ee7 = None
        if with_ee:
            q = rng.normal(size=4)
            ee7 = np.concatenate([rng.uniform(-0.1, 0.1, 3), q / np.linalg.norm(q)])
        ee_pose = ob.Pose.make(ee7[:3], ee7[3:]) if ee7 is not None else None
        kw = dict(solution_mode=mode, **CLASS_CONFIG[cls])
        while True:
            tgt, x0 = make_inputs(d, ch, cls, rng, ee_pose)
            if not gpu:
                rng_range = pick_cap_window(ch, kw, tgt, x0)  # (none among 256 restarts: draw again)
                if rng_range is not None:
                    break
                continue
            # a gpu entry is bounded by the ORACLE's count: draw again (same stream) until its longest restart fits
            ref = ob.ik(ch, ob.make_config(**kw), tgt, x0, rng_range[0], rng_range[1], n_threads=os.cpu_count() or 4,
                        early_exit=False, per_restart=True, ee_offset=ee_pose)
            if int(ref["evals"].max()) <= GPU_MAX_EVALS:
                break
        out.append(dict(
            name=f"{robot}-{cls}-{mode}", robot=robot, n=len(d["lb"]), group=group_of(len(d["lb"])), cls=cls,
            target=[float(v) for v in tgt], x0=[float(v) for v in x0],
            config={k: ([float(x) for x in v] if isinstance(v, tuple) else v) for k, v in kw.items()},
            ee_offset=[float(v) for v in ee7] if ee7 is not None else None,
            restart_begin=int(rng_range[0]), restart_end=int(rng_range[1]), gpu=bool(gpu)))
    return out


def main():
    doc = dict(
        generated_by="tools/gen_solver_edge_scenarios.py (inputs only; every expected value is computed by the oracle "
                     "when a test runs)",
        scenarios=build_scenarios())
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=0, separators=(",", ":"))
        fh.write("\n")
    print("wrote", OUT, len(doc["scenarios"]), "scenarios")


if __name__ == "__main__":
    main()
