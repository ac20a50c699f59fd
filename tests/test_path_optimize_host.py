"""CPU-only: the path optimiser's arithmetic (optik_amd/csrc/path_optimize.hpp, built with g++ as plain C++) on frames
from a numpy forward kinematics: the hinge and the metric's inverse against their formulas, the gradient of the cost
against central differences, the optimiser itself on a blocked scene, and the new symbols of the two C headers."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from avoid_util import Scene, load_tables, make_test_world, numpy_frames
from conftest import ROBOT_SPECS, ROOT
from path_optimize_util import H, REACH, Params, blocked_scene, build_path_optimize, line_path, near_a_kink

NAMES = ["panda", "arm8"]


@pytest.fixture(scope="module")
def po(tmp_path_factory):
    return build_path_optimize(str(tmp_path_factory.mktemp("pathopt_host")))


def test_hinge_values_and_slope(po):
    e = 0.15
    d = np.array([-0.1, 0.0, e / 2, e, 2 * e, math.inf, math.nan])
    c, cp = po.hinge(d, 0.0, e)  # (safety 0: d = dist - safety is dist itself, so the joins are hit exactly)
    dd = d
    assert c[0] == (-dd[0]) + 0.5 * e and cp[0] == -1.0
    for k in (1, 2, 3):
        assert c[k] == ((dd[k] - e) * (dd[k] - e)) / (2.0 * e) and cp[k] == (dd[k] - e) / e
    assert abs(c[1] - 0.5 * e) < 1e-15 and abs(cp[1] + 1.0) < 1e-15  # the two branches meet at d = 0 ...
    assert abs(c[3]) < 1e-30 and abs(cp[3]) < 1e-15                   # ... and the hinge reaches zero at d = e
    assert c[4] == 0.0 and cp[4] == 0.0 and c[5] == 0.0 and cp[5] == 0.0
    assert math.isnan(c[6]) and math.isnan(cp[6])
    # c' is the central difference of c away from the joins: c is linear (exact up to round-off, 1e-16 / 1e-6) or
    # quadratic (the central difference of a quadratic is exact) on each side
    x = np.array([-0.2, -0.05, 0.02, 0.07, 0.13, 0.2, 0.5])
    h, safety = 1e-6, 0.05
    cm, cc, cq = po.hinge(x - h + safety, safety, e)[0], po.hinge(x + safety, safety, e)[1], \
        po.hinge(x + h + safety, safety, e)[0]
    assert np.abs((cq - cm) / (2 * h) - cc).max() <= 1e-9


@pytest.mark.parametrize("M", [1, 2, 7, 62])
def test_ainv_is_the_inverse_of_the_first_difference_metric(po, M):
    A = 2.0 * np.eye(M) - np.eye(M, k=1) - np.eye(M, k=-1)
    Ainv = po.ainv(M)
    assert np.abs(A @ Ainv - np.eye(M)).max() <= 1e-12
    assert np.array_equal(Ainv, Ainv.T)


def _scene(name):
    from optik_amd import Robot
    from optik_amd.collision import auto_pairs, spheres_along_chain
    robot = Robot.from_urdf_file(*ROBOT_SPECS[name])
    tables = load_tables(*ROBOT_SPECS[name])
    n = robot.num_positions()
    frames, centers, radii = spheres_along_chain(robot, 0.05, 2)
    spheres, boxes, grid = make_test_world()
    scene = Scene(tables["axes"][:n], frames, centers, radii, auto_pairs(frames), spheres, boxes, grid)
    return robot, tables, scene


GRAD_SEEDS = {"panda": 21, "arm8": 22}  # (chosen on the CPU so that the exclusions stay under the cap)


@pytest.mark.parametrize("name", NAMES)
def test_gradient_of_the_cost_is_the_central_difference(po, name):
    """U at q -+ H e_(t,j) against g_(t,j) at 1e-6, as tests/test_collision_gradient_host.py checks the rows: the
    smoothness part is quadratic (exact), the obstacle part is a C1 hinge of the rows' distances.  A waypoint where a
    row's witness changes within the step, or whose witness point is within a step's motion of a kink of the min,
    has no derivative there: its components are left out (at most 10 % of the checked components)."""
    robot, tables, scene = _scene(name)
    n = robot.num_positions()
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(GRAD_SEEDS[name])
    L, B = 5, 6
    lo, hi = np.maximum(lb, -2.8), np.minimum(ub, 2.8)
    ends = rng.uniform(lo, hi, size=(B, 2, n))
    paths = np.array([line_path(a, b, L) for a, b in ends]) + rng.normal(size=(B, L, n)) * 0.05
    paths = np.clip(paths, lo, hi)
    prm = Params(0.05, 1.0, 1.0, scene.influence, scene.safety)
    moves = [(t, j, s) for t in range(1, L - 1) for j in range(n) for s in (H, -H)]
    batch = np.repeat(paths[:, None], 1 + len(moves), axis=1)  # [B, 1 + moves, L, n]
    for k, (t, j, s) in enumerate(moves):
        batch[:, 1 + k, t, j] += s
    flat = batch.reshape(-1, L, n)
    cache = {}

    def fk(x):
        key = x.tobytes()
        if key not in cache:
            cache[key] = numpy_frames(tables, x)
        return cache[key]
    frames = np.array([[fk(x) for x in p] for p in flat])
    res = po.step(scene, prm, lb, ub, flat, frames)
    U = res["cost"][:, 0].reshape(B, 1 + len(moves))
    g = res["g"].reshape(B, 1 + len(moves), L, n)[:, 0]
    wit = res["witness"].reshape(B, 1 + len(moves), L, n + 2, 3)
    frames = frames.reshape(B, 1 + len(moves), L, n + 2, 7)
    checked = compared = 0
    worst = 0.0
    for b in range(B):
        for t in range(1, L - 1):
            checked += n
            ks = [1 + k for k, m in enumerate(moves) if m[0] == t]
            changed = (wit[b, ks, t] != wit[b, 0, t]).any()
            kink = any(near_a_kink(scene, frames[b, 0, t], f, wit[b, 0, t, f], REACH * H) for f in range(n + 2))
            if changed or kink:
                continue
            for j in range(n):
                kp, km = 1 + moves.index((t, j, H)), 1 + moves.index((t, j, -H))
                fd = (U[b, kp] - U[b, km]) / (2 * H)
                err = abs(fd - g[b, t, j])
                worst = max(worst, err)
                compared += 1
                assert err <= 1e-6, (name, b, t, j, fd, g[b, t, j])
    print(f"{name}: {compared} of {checked} components compared, worst error {worst:.3g}")
    assert (g[:, 0] == 0.0).all() and (g[:, -1] == 0.0).all()
    assert (res["cost"][:, 2].reshape(B, -1)[:, 0] > 0.0).any()  # (the obstacle term is in play)
    assert checked >= 100 and checked - compared <= 0.10 * checked, (checked, compared)


def _blocked():
    from optik_amd import _native as nat
    sc = blocked_scene()
    tables = load_tables(*ROBOT_SPECS["panda"])
    scene = Scene(tables["axes"][:7], sc["frames"], sc["centers"], sc["radii"], None, sc["spheres"], None, None,
                  sc["influence"], sc["safety"])
    prm = Params(nat.PATH_OPTIMIZE_STEP, nat.PATH_OPTIMIZE_W_SMOOTH, nat.PATH_OPTIMIZE_W_OBS, sc["influence"],
                 sc["safety"])
    return sc, tables, scene, prm, nat.PATH_OPTIMIZE_ITERS


def test_host_optimiser_clears_the_blocked_scene(po):
    sc, tables, scene, prm, iters = _blocked()
    lb, ub = (np.array(v) for v in sc["robot"].joint_limits())
    path = line_path(sc["qa"], sc["qb"], sc["L"])
    q, first, last = po.optimize(scene, prm, lb, ub, path, iters, lambda x: numpy_frames(tables, x))
    print("clearance", first["wp_clearance"][0].min(), "->", last["wp_clearance"][0].min(), "F_obs",
          first["cost"][0, 2], "->", last["cost"][0, 2])
    assert first["wp_clearance"][0].min() < sc["safety"]  # blocked: a waypoint inside the safety distance
    assert first["wp_clearance"][0][[0, -1]].min() >= sc["influence"]  # (the two ends are well clear)
    assert (last["wp_clearance"][0] >= sc["safety"]).all()
    assert last["cost"][0, 2] < first["cost"][0, 2]
    assert np.array_equal(q[[0, -1]].view(np.uint64), path[[0, -1]].view(np.uint64))
    assert last["clearance"][0] == last["wp_clearance"][0].min()


def test_one_unit_step_without_obstacles_is_the_straight_line(po):
    tables = load_tables(*ROBOT_SPECS["panda"])
    scene = Scene(tables["axes"][:7], [], np.zeros((0, 3)), np.zeros(0))
    rng = np.random.default_rng(4)
    for L in (3, 8, 33, 64):
        q = rng.uniform(-1.0, 1.0, size=(1, L, 7))
        frames = np.array([[numpy_frames(tables, x) for x in q[0]]])
        for step, ws in ((1.0, 1.0), (0.25, 4.0)):
            res = po.step(scene, Params(step, ws, 0.0, 0.2, 0.05), np.full(7, -10.0), np.full(7, 10.0), q, frames)
            assert np.abs(res["q"][0] - line_path(q[0, 0], q[0, -1], L)).max() <= 1e-12
            assert res["cost"][0, 2] == 0.0 and res["clearance"][0] == math.inf


def test_new_symbols_are_declared_and_exported():
    from optik_amd import _native as nat
    with open(os.path.join(ROOT, "include", "optik_hip.h")) as fh:
        hip_h = fh.read()
    with open(os.path.join(ROOT, "include", "optik.h")) as fh:
        host_h = fh.read()
    assert re.search(r"\bint optik_hip_path_optimize\(", hip_h) and "OPTIK_HIP_PATH_OPTIMIZE_MAX_WAYPOINTS 64" in hip_h
    assert re.search(r"\bint optik_robot_path_optimize\(", host_h)
    lib = nat.lib()
    assert hasattr(lib, "optik_hip_path_optimize") and hasattr(lib, "optik_robot_path_optimize")
    nm = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    names = {ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip()}
    assert {"optik_hip_path_optimize", "optik_robot_path_optimize"} <= names
