"""CPU-only: collision repair as the host build of optik_amd/csrc/repair_measure.hpp runs it (tests/repair_util.py:
the header alone under g++, repair_reference over constraint_measure.hpp's forward kinematics and projection and
collision_gradient.hpp's witness rows): a planar two-joint arm whose clearance has a closed form, and the Panda with a
sphere model in the world of avoid_util.make_test_world."""
import os
import re
import subprocess

import numpy as np
import pytest

import repair_util as ru
from avoid_util import Scene, load_tables, make_test_world
from conftest import ROBOT_SPECS, ROOT
from constraint_util import Constraint, free_constraint, pinned_constraint

PRM = ru.Params(0.2, 0.05, 0.05, 64)     # the planar arm
PPRM = ru.Params(0.1, 0.02, 0.05, 256)   # the Panda: its self pairs sit 5 cm apart in every configuration


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ru.build_repair(str(tmp_path_factory.mktemp("repair_host")))


@pytest.fixture(scope="module")
def planar():
    """The planar arm, its scene, and rows: 0 free, 1 - 3 colliding (the tool sphere overlaps the world sphere)."""
    chain, scene = ru.planar_chain(), ru.planar_scene()
    q = np.array([[0.3, 0.6], [0.15, 1.0], [0.1, 1.0], [0.2, 0.95]])
    clr = ru.planar_clearance(q)
    assert clr[0] >= PRM.safety and (clr[1:] < 0.0).all(), clr
    return chain, scene, q


@pytest.fixture(scope="module")
def panda(oracle):
    """The Panda with spheres along its links in make_test_world()'s spheres and boxes, 64 random configurations of
    which some collide, and the pose of the first colliding one."""
    from optik_amd import Robot
    from optik_amd.collision import auto_pairs, spheres_along_chain
    robot = Robot.from_urdf_file(*ROBOT_SPECS["panda"])
    tables = load_tables(*ROBOT_SPECS["panda"])
    frames, centers, radii = spheres_along_chain(robot, 0.05, 2)
    spheres, boxes, _ = make_test_world()
    scene = Scene(tables["axes"][:7], frames, centers, radii, auto_pairs(frames), spheres, boxes, None, PPRM.influence,
                  PPRM.safety)
    lb, ub = np.asarray(tables["lb"]), np.asarray(tables["ub"])
    q = np.random.default_rng(11).uniform(np.maximum(lb, -2.5), np.minimum(ub, 2.5), (64, 7))
    ch = oracle.make_chain(**tables)
    return dict(tables=tables, scene=scene, q=q, lb=lb, ub=ub, pose=lambda x: np.asarray(oracle.fk(ch, np.asarray(x))[1]),
                spheres=len(np.ravel(radii)) if np.ndim(radii) else len(frames))


def _clearance(ref, chain, scene, x):
    return ref.witness(chain, scene, x)[0].min(axis=1)


def test_the_header_compiles_alone_and_checks_its_parameters(ref):
    assert ref.params_ok(PRM) and ref.params_ok(ru.Params(0.2, 0.0, 1e-3, 0, 0.0)) and ref.params_ok(
        ru.Params(0.2, 0.05, 0.05, 4096))
    for bad in (ru.Params(0.05, 0.05, 0.05, 8), ru.Params(0.2, -0.01, 0.05, 8), ru.Params(np.inf, 0.05, 0.05, 8),
                ru.Params(0.2, 0.05, 0.0, 8), ru.Params(0.2, 0.05, np.inf, 8), ru.Params(0.2, np.nan, 0.05, 8),
                ru.Params(0.2, 0.05, 0.05, -1), ru.Params(0.2, 0.05, 0.05, 4097), ru.Params(0.2, 0.05, 0.05, 8, -1.0),
                ru.Params(0.2, 0.05, 0.05, 8, np.nan)):
        assert not ref.params_ok(bad), bad.array()


def test_planar_free_input_comes_back_bit_for_bit_and_colliding_ones_are_pushed_free(ref, planar):
    chain, scene, q = planar
    r = ref.repair(chain, scene, PRM, q)
    print({k: r[k].tolist() for k in ru.KEYS})
    assert r["status"].tolist() == [ru.FREE] * 4
    assert r["iterations"][0] == 0 and r["moved"][0] == 0.0 and np.array_equal(ru.bits(r["x"][0]), ru.bits(q[0]))
    assert (r["iterations"][1:] > 0).all() and (r["moved"][1:] > 0.0).all()
    closed = ru.planar_clearance(r["x"])
    assert (closed >= PRM.safety - 1e-12).all() and np.allclose(closed, r["clearance"], rtol=0, atol=1e-12)
    assert (r["x"] >= chain["lb"]).all() and (r["x"] <= chain["ub"]).all()
    assert np.array_equal(r["moved"], np.abs(r["x"] - q).max(axis=1)) and (r["violation"] == 0.0).all()
    # the same input gives the same bits twice
    again = ref.repair(chain, scene, PRM, q)
    for k in ru.KEYS:
        assert again[k].tobytes() == r[k].tobytes(), k


def test_planar_a_joint_on_its_limit_stays_clamped(ref, planar):
    """Limits that end at the colliding row's own joint values on the side the gradient pushes to: that joint stays,
    the other does the work (or the row ends without moving past the limit)."""
    _, scene, q = planar
    free = ref.repair(ru.planar_chain(), scene, PRM, q[1:2])
    d = free["x"][0] - q[1]
    assert d[0] != 0.0 and d[1] != 0.0
    chain = ru.planar_chain()
    j = 0
    (chain["lb"] if d[j] < 0 else chain["ub"])[j] = q[1, j]
    r = ref.repair(chain, scene, PRM, q[1:2])
    print(d, {k: r[k].tolist() for k in ru.KEYS})
    assert r["x"][0, j] == q[1, j] and r["x"][0, 1] != q[1, 1]
    assert (r["x"] >= chain["lb"]).all() and (r["x"] <= chain["ub"]).all()
    assert r["status"][0] == ru.FREE and ru.planar_clearance(r["x"])[0] >= PRM.safety - 1e-12


def test_planar_no_iterations_nan_and_max_move(ref, planar):
    chain, scene, q = planar
    r = ref.repair(chain, scene, ru.Params(0.2, 0.05, 0.05, 0), q)
    assert r["status"].tolist() == [ru.FREE, ru.LIMIT, ru.LIMIT, ru.LIMIT] and (r["iterations"] == 0).all()
    assert np.array_equal(ru.bits(r["x"]), ru.bits(q)) and (r["moved"] == 0.0).all()
    assert np.allclose(r["clearance"], ru.planar_clearance(q), rtol=0, atol=1e-12)
    bad = q.copy()
    bad[1, 0], bad[2, 1] = np.nan, np.inf
    r = ref.repair(chain, scene, PRM, bad)
    assert r["status"].tolist() == [ru.FREE, ru.NAN, ru.NAN, ru.FREE]
    assert np.isnan(r["clearance"][1:3]).all() and (r["iterations"][1:3] == 0).all()
    assert np.array_equal(ru.bits(r["x"][:3]), ru.bits(bad[:3])) and r["iterations"][3] > 0
    # max_move below what the repair needs: stuck at the last accepted iterate, which is within max_move
    full = ref.repair(chain, scene, PRM, q)
    cap = 0.5 * float(full["moved"][1])
    r = ref.repair(chain, scene, ru.Params(0.2, 0.05, 0.05, 64, cap), q[1:2])
    assert r["status"][0] == ru.STUCK and r["moved"][0] <= cap and 0 < r["iterations"][0] < full["iterations"][1]
    assert np.array_equal(r["moved"], np.abs(r["x"] - q[1:2]).max(axis=1))
    assert r["clearance"][0] < PRM.safety
    assert ref.repair(chain, scene, ru.Params(0.2, 0.05, 0.05, 64, 0.0), q[1:2])["iterations"][0] == 0


def test_planar_a_vanishing_gradient_is_stuck(ref):
    """The colliding sphere sits on the base frame, which no joint moves: every gobs_j is 0."""
    chain = ru.planar_chain()
    scene = Scene([[0.0, 0, 1], [0.0, 0, 1]], [0], [[0.0, 0, 0]], [0.1], None, [[0.1, 0.0, 0.0, 0.1]], None, None, 0.2, 0.05)
    r = ref.repair(chain, scene, PRM, [[0.3, 0.6]])
    assert r["status"][0] == ru.STUCK and r["iterations"][0] == 0 and r["clearance"][0] < 0.0
    assert np.array_equal(ru.bits(r["x"]), ru.bits(np.array([[0.3, 0.6]])))


def test_panda_colliding_rows_are_repaired_inside_the_limits(ref, panda):
    p = panda
    before = _clearance(ref, p["tables"], p["scene"], p["q"])
    hit = before < PPRM.safety
    r = ref.repair(p["tables"], p["scene"], PPRM, p["q"])
    print(f"{p['spheres']} spheres; {int(hit.sum())} of {len(hit)} rows below the safety distance; status "
          f"{np.bincount(r['status'], minlength=4).tolist()}; iterations up to {int(r['iterations'].max())}")
    assert 8 <= hit.sum() <= len(hit) - 8
    assert (r["status"][~hit] == ru.FREE).all() and (r["iterations"][~hit] == 0).all()
    assert np.array_equal(ru.bits(r["x"][~hit]), ru.bits(p["q"][~hit]))
    ok = r["status"] == ru.FREE
    assert (ok & hit).sum() >= hit.sum() // 2, "most colliding rows are repaired with the default step and budget"
    after = _clearance(ref, p["tables"], p["scene"], r["x"])
    assert np.array_equal(ru.bits(after), ru.bits(r["clearance"])), "the clearance is the returned x's"
    assert (after[ok] >= PPRM.safety).all()
    assert (r["x"] >= p["lb"]).all() and (r["x"] <= p["ub"]).all()
    assert (r["iterations"][r["status"] == ru.LIMIT] == PPRM.iters).all()


def test_panda_a_free_box_equals_no_box_bit_for_bit(ref, panda):
    p = panda
    plain = ref.repair(p["tables"], p["scene"], PPRM, p["q"][:24])
    boxed = ref.repair(p["tables"], p["scene"], PPRM, p["q"][:24], free_constraint(p["pose"](p["q"][0])), **ru.PROJECT)
    for k in ru.KEYS:
        assert boxed[k].tobytes() == plain[k].tobytes(), k


def test_panda_position_only_keeps_the_tool_in_place(ref, panda, tmp_path_factory):
    """Every colliding row under its own position-only box of 1 mm: a status-0 row has violation <= ptol, measured
    again with the constraint driver."""
    from constraint_util import build_constraint
    cref = build_constraint(str(tmp_path_factory.mktemp("repair_constraint")))
    p = panda
    hit = np.nonzero(_clearance(ref, p["tables"], p["scene"], p["q"]) < PPRM.safety)[0][:12]
    inf, done = np.inf, 0
    for b in hit:
        c = Constraint(p["pose"](p["q"][b]), [-1e-3] * 3 + [-inf] * 3, [1e-3] * 3 + [inf] * 3)
        r = ref.repair(p["tables"], p["scene"], PPRM, p["q"][b:b + 1], c, **ru.PROJECT)
        v = cref.measure(p["tables"], c, r["x"])["v"]
        assert np.array_equal(ru.bits(v), ru.bits(r["violation"]))
        if r["status"][0] == ru.FREE:
            done += 1
            assert r["iterations"][0] > 0 and v[0] <= ru.PROJECT["ptol"] and r["clearance"][0] >= PPRM.safety
            assert (r["x"] >= p["lb"]).all() and (r["x"] <= p["ub"]).all()
    print(f"{done} of {len(hit)} colliding rows slid free with the tool within 1 mm")
    assert done == 8, "the count of the host build, which is deterministic: a change in how often the projection succeeds"


def test_panda_a_region_the_projection_cannot_reach_is_stuck_at_the_input(ref, panda):
    """A pose pinned two metres away: the first projection spends its budget, nothing is accepted."""
    p = panda
    hit = np.nonzero(_clearance(ref, p["tables"], p["scene"], p["q"]) < PPRM.safety)[0][:4]
    far = p["pose"](p["q"][hit[0]]).copy()
    far[:3] += 2.0
    r = ref.repair(p["tables"], p["scene"], PPRM, p["q"][hit], pinned_constraint(far), ptol=1e-6, piters=8, damping=1e-6,
                   max_step=0.5)
    assert (r["status"] == ru.STUCK).all() and (r["iterations"] == 0).all() and (r["moved"] == 0.0).all()
    assert np.array_equal(ru.bits(r["x"]), ru.bits(p["q"][hit])) and (r["violation"] > 1.0).all()


def test_the_defaults_clear_the_scene_of_the_example_and_nothing_more(ref, oracle):
    """optik_amd._native.REPAIR_STEP and REPAIR_ITERS on the scene of examples/ik_repair.py: the start state inside
    the table is pushed free, the goal is free as it is, at least 85 % of the cell's colliding configurations are freed
    -- and a quarter of the budget frees fewer than half of them (the defaults are not generous)."""
    import importlib.util
    from optik_amd import Robot
    from optik_amd import _native as nat
    from optik_amd.collision import auto_pairs
    spec = importlib.util.spec_from_file_location("ik_repair_example", os.path.join(ROOT, "examples", "ik_repair.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    robot = Robot.from_urdf_file(*ROBOT_SPECS["panda"])
    tables = load_tables(*ROBOT_SPECS["panda"])
    frames, centers, radii = ex.model(robot)
    scene = Scene(tables["axes"][:7], frames, centers, radii, auto_pairs(frames), None, [ex.TABLE], None, ex.INFLUENCE,
                  ex.SAFETY)
    prm = ru.Params(ex.INFLUENCE, ex.SAFETY, nat.REPAIR_STEP, nat.REPAIR_ITERS)
    ends = np.array([ex.START, ex.GOAL])
    before = _clearance(ref, tables, scene, ends)
    r = ref.repair(tables, scene, prm, ends)
    print({k: r[k].tolist() for k in ru.KEYS})
    assert -0.01 < before[0] < 0.0 and before[1] >= ex.SAFETY
    assert r["status"].tolist() == [ru.FREE, ru.FREE] and r["iterations"][0] > 0 and r["iterations"][1] == 0
    assert r["moved"][0] < 0.1
    lb, ub = np.asarray(tables["lb"]), np.asarray(tables["ub"])
    cell = np.random.default_rng(ex.SEED).uniform(np.maximum(lb, -2.5), np.minimum(ub, 2.5), (ex.CELL, 7))
    hit = _clearance(ref, tables, scene, cell) < ex.SAFETY
    full = ref.repair(tables, scene, prm, cell[hit])
    quarter = ref.repair(tables, scene, ru.Params(ex.INFLUENCE, ex.SAFETY, nat.REPAIR_STEP, nat.REPAIR_ITERS // 4),
                         cell[hit])
    done, less = int((full["status"] == ru.FREE).sum()), int((quarter["status"] == ru.FREE).sum())
    print(f"{int(hit.sum())} colliding of {ex.CELL}: {done} freed with the defaults, {less} with a quarter of the budget")
    assert hit.sum() >= 32 and done >= 0.85 * hit.sum() and less < 0.5 * hit.sum()
    # the tool held where it is ("what it does not do"): within 2 cm the start slides free in 24
    # steps; within 1 mm the default budget ends LIMIT a few millimetres inside, and four times the budget does too
    ref7 = np.asarray(oracle.fk(oracle.make_chain(**tables), np.array(ex.START))[1])
    inf = np.inf

    def held(tol, iters):
        c = Constraint(ref7, [-tol] * 3 + [-inf] * 3, [tol] * 3 + [inf] * 3)
        return ref.repair(tables, scene, ru.Params(ex.INFLUENCE, ex.SAFETY, nat.REPAIR_STEP, iters), [ex.START], c,
                          **ru.PROJECT)
    wide, tight, long = held(2e-2, nat.REPAIR_ITERS), held(1e-3, nat.REPAIR_ITERS), held(1e-3, 4 * nat.REPAIR_ITERS)
    print("2 cm:", wide["status"][0], wide["iterations"][0], "1 mm:", tight["status"][0], tight["clearance"][0],
          "1 mm, 4 x budget:", long["status"][0], long["clearance"][0])
    assert wide["status"][0] == ru.FREE and wide["iterations"][0] == 24 and wide["violation"][0] <= 1e-6
    assert tight["status"][0] == ru.LIMIT and tight["iterations"][0] == nat.REPAIR_ITERS
    assert -0.003 < tight["clearance"][0] < -0.002 and tight["violation"][0] <= 1e-6
    assert long["status"][0] == ru.LIMIT and -0.001 < long["clearance"][0] < 0.0


def test_new_symbols_are_declared_and_exported():
    from optik_amd import _native as nat
    with open(os.path.join(ROOT, "include", "optik_hip.h")) as fh:
        hip_h = fh.read()
    with open(os.path.join(ROOT, "include", "optik.h")) as fh:
        host_h = fh.read()
    assert re.search(r"\bint optik_hip_collision_repair_batch\(", hip_h)
    assert re.search(r"\bint optik_robot_collision_repair_batch\(", host_h)
    nm = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    names = {ln.split()[-1] for ln in nm.stdout.splitlines() if ln.strip()}
    assert {"optik_hip_collision_repair_batch", "optik_robot_collision_repair_batch"} <= names
