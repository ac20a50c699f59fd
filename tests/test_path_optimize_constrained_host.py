"""CPU-only: path optimisation under a pose constraint as the composed reference runs it
(tests/path_optimize_constrained_util.py: path_optimize.hpp's update, constraint_measure.hpp's projection, the fallback)
on frames from a numpy forward kinematics: the scene the -m gpu test relies on, the fallback, the free box, and the new
symbols of the two C headers."""
import os
import re
import subprocess

import numpy as np
import pytest

import path_optimize_constrained_util as pcu
from avoid_util import Scene, load_tables, numpy_frames
from conftest import ROBOT_SPECS, ROOT
from constraint_util import free_constraint, pinned_constraint


@pytest.fixture(scope="module")
def co(tmp_path_factory):
    return pcu.build_composed(str(tmp_path_factory.mktemp("pathopt_con_host")),
                              str(tmp_path_factory.mktemp("constraint_con_host")))


@pytest.fixture(scope="module")
def blocked(oracle):
    from optik_amd import _native as nat
    sc = pcu.blocked_scene()
    tables = load_tables(*ROBOT_SPECS["panda"])
    scene = Scene(tables["axes"][:7], sc["frames"], sc["centers"], sc["radii"], None, sc["spheres"], None, None,
                  sc["influence"], sc["safety"])
    prm = pcu.Params(nat.PATH_OPTIMIZE_STEP, nat.PATH_OPTIMIZE_W_SMOOTH, nat.PATH_OPTIMIZE_W_OBS, sc["influence"],
                     sc["safety"])
    ref7 = np.asarray(oracle.fk(oracle.make_chain(**tables), sc["qa"])[1])
    return dict(sc=sc, tables=tables, scene=scene, prm=prm, iters=nat.PATH_OPTIMIZE_ITERS, ref7=ref7,
                path=pcu.line_path(sc["qa"], sc["qb"], sc["L"]), frames_of=lambda x: numpy_frames(tables, x))


def test_the_scene_needs_the_constraint_and_the_constrained_optimiser_keeps_it(co, blocked):
    """What tests/test_gpu_path_optimize_constrained.py relies on, shown with the reference alone: (1) the straight
    line satisfies upright(FK(qa)); (2) the unconstrained optimiser's result does not, at UPRIGHT_TOL; (3) the
    constrained one clears the sphere with every waypoint within PTOL and every projection ended projected."""
    b = blocked
    sc, tables, path = b["sc"], b["tables"], b["path"]
    c = pcu.upright_constraint(b["ref7"], pcu.UPRIGHT_TILT)
    lb, ub = np.asarray(tables["lb"]), np.asarray(tables["ub"])
    v_in = co.cref.measure(tables, c, path)["v"]
    assert v_in.max() <= pcu.PTOL                                                     # (1)
    qu, _, last_u = co.po.optimize(b["scene"], b["prm"], lb, ub, path, b["iters"], b["frames_of"])
    v_un = co.cref.measure(tables, c, qu)["v"]
    assert (last_u["wp_clearance"][0] >= sc["safety"]).all() and v_un.max() > pcu.UPRIGHT_TOL  # (2)
    q, first, last, projected, violation = co.optimize(b["scene"], b["prm"], tables, c, path[None], b["iters"],
                                                       b["frames_of"], pcu.PTOL, **pcu.PROJECT)
    v_out = co.cref.measure(tables, c, q[0])["v"]
    print(f"violation: input {v_in.max():.3g}, unconstrained {v_un.max():.3g}, constrained {v_out.max():.3g}; F_obs "
          f"{first['cost'][0, 2]:.4g} -> {last['cost'][0, 2]:.4g} (unconstrained {last_u['cost'][0, 2]:.4g}); clearance "
          f"{first['clearance'][0]:.4g} -> {last['clearance'][0]:.4g}; projected {projected.tolist()}")
    assert v_out.max() <= pcu.PTOL and violation[0] == v_out.max()                   # (3)
    assert last["cost"][0, 2] < first["cost"][0, 2]
    assert projected[0, 0] == projected[0, 1] == b["iters"] * (sc["L"] - 2) > 0
    assert (last["wp_clearance"][0] >= sc["safety"]).all()
    assert np.array_equal(q[0, [0, -1]].view(np.uint64), path[[0, -1]].view(np.uint64))
    # the segments between the waypoints are straight in joint space and only checked: here they pass at UPRIGHT_TOL
    assert co.cref.motion(tables, c, q[0, :-1], q[0, 1:], 0.05, pcu.UPRIGHT_TOL)["ok"].all()


def test_a_projection_that_does_not_end_keeps_the_old_waypoint(co, blocked):
    """A pinned box and a budget of one iteration: the waypoints the first update moves cannot be brought back, and
    keep the bits of the input; with the budget of the defaults they are projected."""
    b = blocked
    tables, path = b["tables"], b["path"]
    c = pinned_constraint(b["ref7"])
    frames = np.array([[b["frames_of"](x) for x in path]])
    short = co.step(b["scene"], b["prm"], tables, c, path[None], frames, pcu.PTOL, 1, 1e-6, 0.5)
    assert 0 <= short["projected"][0, 1] < short["projected"][0, 0] == len(path) - 2
    kept = short["kept"][0]
    assert kept.any() and not kept[[0, -1]].any()
    assert np.array_equal(short["q"][0][kept].view(np.uint64), path[kept].view(np.uint64))
    plain = co.po.step(b["scene"], b["prm"], tables["lb"], tables["ub"], path[None], frames)
    assert not np.array_equal(plain["q"][0][kept], path[kept]), "the step had moved them"
    for key in ("cost", "clearance"):  # steps 1 - 5 are the unconstrained ones
        assert np.array_equal(short[key], plain[key])


def test_a_free_box_is_the_unconstrained_update(co, blocked):
    b = blocked
    tables, path = b["tables"], b["path"]
    frames = np.array([[b["frames_of"](x) for x in path]])
    got = co.step(b["scene"], b["prm"], tables, free_constraint(b["ref7"]), path[None], frames, 0.0, 0, 1e-6, 0.5)
    want = co.po.step(b["scene"], b["prm"], tables["lb"], tables["ub"], path[None], frames)
    assert np.array_equal(got["q"].view(np.uint64), want["q"].view(np.uint64))
    assert got["projected"].tolist() == [[0, 0]]
    assert co.violation(tables, free_constraint(b["ref7"]), got["q"]).tolist() == [0.0]


def test_the_violation_takes_a_nan_and_keeps_it():
    v = np.array([[0.1, np.nan, 0.3], [0.2, 0.5, 0.1], [0.0, 0.0, 0.0]])
    out = pcu.fold_violation(v)
    assert np.isnan(out[0]) and out[1] == 0.5 and out[2] == 0.0


def test_new_symbols_are_declared_and_exported():
    from optik_amd import _native as nat
    with open(os.path.join(ROOT, "include", "optik_hip.h")) as fh:
        hip_h = fh.read()
    with open(os.path.join(ROOT, "include", "optik.h")) as fh:
        host_h = fh.read()
    assert re.search(r"\bint optik_hip_path_optimize_constrained\(", hip_h)
    assert re.search(r"\bint optik_robot_path_optimize_constrained\(", host_h)
    nm = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    names = {ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip()}
    assert {"optik_hip_path_optimize_constrained", "optik_robot_path_optimize_constrained"} <= names
