"""-m gpu: the repair hook of ik_region (HipChain.ik_region / optik_hip_ik_region_repair, Robot.ik_region_batch_arrays /
optik_robot_ik_region_repair) on the scene of examples/ik_repair.py: a Panda, 9 spheres along its links, a table.

The reference is tests/repair_util.region_repair_reference: the host build of region_measure.hpp for the restarts, then
the host build of repair_measure.hpp for every column whose key is finite, on the host's own forward kinematics.

The discriminating scene the issue asks for, chosen on the CPU with the two host builds: the tool at (0.7, 0, 0.12) -- 10
cm below the table's top, under its far edge region -- within a position box of 2 cm, any orientation, restarts 23 ..
38.  Host-side counts: 13 of the 16 restarts project, NONE of them is free, 8 take a repaired x.  So the unrepaired call
returns count == 0 and the repaired one count >= 1 (DISCRIMINATING below; asserted on the reference and on the device).
With restarts 0 .. 15 the same scene's targets always have free restarts; the two of TARGETS are those with the most
repaired ones there: per target 10 restarts project, 4 and 5 are free as they are, 6 and 4 take a repaired x."""
import importlib.util
import os

import numpy as np
import pytest

import region_util as gu
import repair_util as ru
from avoid_util import Scene
from conftest import ROBOT_SPECS, ROOT
from gpu_util import assert_bit_equal

pytestmark = pytest.mark.gpu

R, K, MIN_DIST, TOL = 16, 8, 0.1, 1e-6
PROJECT = dict(iters=256, damping=1e-6, max_step=0.5)
TARGETS = [([0.7, 0.0, 0.15, 1.0, 0.0, 0.0, 0.0], 0.02), ([0.55, 0.0, 0.15, 1.0, 0.0, 0.0, 0.0], 0.02)]
HOST_REPAIRED = [6, 4]   # (the reference's counts, found on the CPU)
DISCRIMINATING = dict(target=([0.7, 0.0, 0.12, 1.0, 0.0, 0.0, 0.0], 0.02), begin=23, projected=13, free=0, repaired=8)


def _example():
    spec = importlib.util.spec_from_file_location("ik_repair_example", os.path.join(ROOT, "examples", "ik_repair.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


@pytest.fixture(scope="module")
def cell(tmp_path_factory):
    from optik_amd import Robot
    from optik_amd.collision import auto_pairs
    ex = _example()
    robot = Robot.from_urdf_file(*ROBOT_SPECS["panda"])
    frames, centers, radii = ex.model(robot)
    for obj in (robot, robot.hip_chain()):
        obj.set_collision_model(frames, centers, radii, self_pairs="auto", margin=0.0)
        obj.set_world(boxes=[ex.TABLE])
    tables = robot.chain_tables()
    scene = Scene(tables["axes"][:7], frames, centers, radii, auto_pairs(frames), None, [ex.TABLE], None, ex.INFLUENCE,
                  ex.SAFETY)
    inf = np.inf
    regions = np.array([np.concatenate([ref7, [-p] * 3 + [-inf] * 3, [p] * 3 + [inf] * 3]) for ref7, p in TARGETS])
    x0 = np.array([ex.GOAL, ex.GOAL])
    repair = dict(influence=ex.INFLUENCE, safety=ex.SAFETY, step=0.05, iters=256, max_move=np.inf)
    ref = ru.build_repair(str(tmp_path_factory.mktemp("region_repair")))
    rref = gu.build_region(str(tmp_path_factory.mktemp("region_repair_rows")))
    prm = ru.Params(ex.INFLUENCE, ex.SAFETY, 0.05, 256)
    want = ru.region_repair_reference(ref, rref, tables, scene, prm, regions, x0, 0, R, TOL, PROJECT["iters"],
                                      PROJECT["damping"], PROJECT["max_step"], gu.MODE_QUALITY)
    d7, dp = DISCRIMINATING["target"]
    dreg = np.concatenate([d7, [-dp] * 3 + [-inf] * 3, [dp] * 3 + [inf] * 3])[None]
    dargs = (tables, dreg, x0[:1], DISCRIMINATING["begin"], R, TOL, PROJECT["iters"], PROJECT["damping"],
             PROJECT["max_step"], gu.MODE_QUALITY)
    dbase = rref.restarts(*dargs)
    dwant = ru.region_repair_reference(ref, rref, tables, scene, prm, *dargs[1:])
    fin = dbase["key"] < np.inf
    dfree = int((ref.witness(tables, scene, dbase["x"][fin])[0].min(axis=1) >= 0.0).sum())
    return dict(robot=robot, regions=regions, x0=x0, repair=repair, want=want, safety=ex.SAFETY, dreg=dreg, dwant=dwant,
                dprojected=int(fin.sum()), dfree=dfree)


def _call(hc, cell, **kw):
    import torch
    reg = torch.tensor(cell["regions"], device="cuda:0")
    x0 = torch.tensor(cell["x0"], device="cuda:0")
    res = hc.ik_region(reg, x0, 0, R, K, MIN_DIST, tol=TOL, mode="quality", per_restart=True, **PROJECT, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _raw_old_entry(hc, cell):
    """optik_hip_ik_region itself, called through the library with buffers of its own: the entry the parent commit has."""
    import ctypes as C
    import torch
    from optik_amd import _native as nat
    reg = torch.tensor(cell["regions"], device="cuda:0")
    x0 = torch.tensor(cell["x0"], device="cuda:0")
    T, n, cols = len(cell["regions"]), 7, len(cell["regions"]) * R
    f64, dev = torch.float64, "cuda:0"
    res = dict(count=torch.empty(T, dtype=torch.int32, device=dev), x=torch.empty((T, K, n), dtype=f64, device=dev),
               violation=torch.empty((T, K), dtype=f64, device=dev), idx=torch.empty((T, K), dtype=torch.int64, device=dev),
               key=torch.empty((T, K), dtype=f64, device=dev), restart_x=torch.empty((n, cols), dtype=f64, device=dev),
               restart_violation=torch.empty(cols, dtype=f64, device=dev),
               restart_status=torch.empty(cols, dtype=torch.int32, device=dev),
               restart_iterations=torch.empty(cols, dtype=torch.int32, device=dev),
               restart_key=torch.empty(cols, dtype=f64, device=dev))
    o = nat.IkRegionOutputs()
    o.d_x, o.d_violation = res["restart_x"].data_ptr(), res["restart_violation"].data_ptr()
    o.d_status, o.d_iterations = res["restart_status"].data_ptr(), res["restart_iterations"].data_ptr()
    o.d_key, o.d_count, o.d_sol_x = res["restart_key"].data_ptr(), res["count"].data_ptr(), res["x"].data_ptr()
    o.d_sol_violation, o.d_sol_idx, o.d_sol_key = res["violation"].data_ptr(), res["idx"].data_ptr(), res["key"].data_ptr()
    rc = nat.lib().optik_hip_ik_region(hc._h, None, reg.data_ptr(), x0.data_ptr(), T, 0, R, TOL, PROJECT["iters"],
                                       PROJECT["damping"], PROJECT["max_step"], gu.MODE_QUALITY, None, None, None, 0.0, K,
                                       MIN_DIST, C.byref(o), None)
    assert rc == 0
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def test_repair_none_is_the_call_without_the_argument_byte_for_byte(cell):
    """Three ways to the same bytes: optik_hip_ik_region called raw (the old entry itself, which now goes through the
    shared body), HipChain.ik_region without the argument, and with repair=None.  Without repair the device form's
    dict has no "repaired" (it launches nothing more); the host-row form has zeros."""
    hc = cell["robot"].hip_chain()
    raw, plain, none = _raw_old_entry(hc, cell), _call(hc, cell), _call(hc, cell, repair=None)
    assert sorted(raw) == sorted(plain) == sorted(none) and "repaired" not in none
    for k in raw:
        assert raw[k].tobytes() == plain[k].tobytes() == none[k].tobytes(), k
    r = cell["robot"]
    from optik_amd import SolverConfig
    cfg = SolverConfig("quality", max_time=0.0, max_restarts=R)
    a = r.ik_region_batch_arrays(cfg, _constraints(cell), cell["x0"], k=K, min_dist=MIN_DIST, restarts=R, tol=TOL)
    b = r.ik_region_batch_arrays(cfg, _constraints(cell), cell["x0"], k=K, min_dist=MIN_DIST, restarts=R, tol=TOL,
                                 repair=None)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (b["repaired"] == 0).all()
    for k in ("count", "x", "violation", "key"):   # the host rows are the device's selection
        assert a[k].tobytes() == raw[k].tobytes(), k


def _constraints(cell):
    from optik_amd import PoseConstraint
    out = []
    for reg in cell["regions"]:
        t, q = reg[:3], reg[3:7]
        i, j, k, w = q
        m = np.eye(4)
        m[:3, :3] = [[1 - 2 * (j * j + k * k), 2 * (i * j - k * w), 2 * (i * k + j * w)],
                     [2 * (i * j + k * w), 1 - 2 * (i * i + k * k), 2 * (j * k - i * w)],
                     [2 * (i * k - j * w), 2 * (j * k + i * w), 1 - 2 * (i * i + j * j)]]
        m[:3, 3] = t
        out.append(PoseConstraint(m, reg[7:13], reg[13:19]))
    return out


def test_the_repaired_columns_are_the_references_and_the_rows_returned_hold_their_promises(cell):
    robot, want = cell["robot"], cell["want"]
    hc = robot.hip_chain()
    print("host: repaired per target", want["repaired"].tolist())
    assert want["repaired"].tolist() == HOST_REPAIRED
    plain, got = _call(hc, cell), _call(hc, cell, repair=cell["repair"])
    assert got["repaired"].tolist() == want["repaired"].tolist()
    assert_bit_equal(got["restart_x"].T, want["x"], "per-restart x after the repair pass")
    assert_bit_equal(got["restart_violation"], want["v"], "per-restart violation after the repair pass")
    # every column the reference does not mark is the unrepaired call's, bit for bit
    keep = ~want["mark"]
    assert got["restart_x"].T[keep].tobytes() == plain["restart_x"].T[keep].tobytes()
    assert got["restart_violation"][keep].tobytes() == plain["restart_violation"][keep].tobytes()
    assert got["restart_status"].tobytes() == plain["restart_status"].tobytes()
    # the marked columns: the key by the region kernel's rule, finite because they are free now
    mk = want["mark"]
    assert_bit_equal(got["restart_key"][mk], want["key"][mk], "the recomputed keys")
    print("count without repair", plain["count"].tolist(), "with", got["count"].tolist())
    assert (got["count"] >= plain["count"]).all() and (got["count"] >= 1).all()
    lb, ub = (np.array(v) for v in robot.joint_limits())
    cons = _constraints(cell)
    for t in range(len(cons)):
        rows = got["x"][t, :got["count"][t]]
        assert (robot.collision_clearance_batch_arrays(rows)[0] >= 0.0).all(), "free under the model's margin"
        assert (robot.constraint_batch_arrays(rows, cons[t])[1] <= TOL).all()
        assert (rows >= lb).all() and (rows <= ub).all()
        for i in range(len(rows)):
            for j in range(i):
                assert np.abs(rows[i] - rows[j]).max() > MIN_DIST
    # the host-row form: the same selection
    from optik_amd import SolverConfig
    out = robot.ik_region_batch_arrays(SolverConfig("quality", max_time=0.0, max_restarts=R), cons, cell["x0"], k=K,
                                       min_dist=MIN_DIST, restarts=R, tol=TOL, repair=cell["repair"])
    assert out["repaired"].tolist() == want["repaired"].tolist() and out["count"].tolist() == got["count"].tolist()
    assert_bit_equal(out["x"], got["x"], "host rows")


def test_the_discriminating_scene_no_row_without_repair_and_rows_with_it(cell):
    import torch
    d, robot = DISCRIMINATING, cell["robot"]
    print("host:", cell["dprojected"], "projected,", cell["dfree"], "free,", int(cell["dwant"]["repaired"][0]), "repaired")
    assert (cell["dprojected"], cell["dfree"], int(cell["dwant"]["repaired"][0])) == (d["projected"], d["free"],
                                                                                     d["repaired"])
    hc = robot.hip_chain()
    reg = torch.tensor(cell["dreg"], device="cuda:0")
    x0 = torch.tensor(cell["x0"][:1], device="cuda:0")
    args = (reg, x0, d["begin"], d["begin"] + R, K, MIN_DIST)
    plain = hc.ik_region(*args, tol=TOL, **PROJECT)
    fixed = hc.ik_region(*args, tol=TOL, repair=cell["repair"], **PROJECT)
    count = int(fixed["count"][0])
    print("count without repair", int(plain["count"][0]), "with", count)
    assert int(plain["count"][0]) == 0 and count >= 1 and int(fixed["repaired"][0]) == d["repaired"]
    rows = fixed["x"][0, :count].cpu().numpy()
    assert (robot.collision_clearance_batch_arrays(rows)[0] >= 0.0).all()
    from constraint_util import Constraint
    c = Constraint(cell["dreg"][0, :7], cell["dreg"][0, 7:13], cell["dreg"][0, 13:19])
    assert (robot.constraint_batch_arrays(rows, c)[1] <= TOL).all()
    lb, ub = (np.array(v) for v in robot.joint_limits())
    assert (rows >= lb).all() and (rows <= ub).all()


def test_keep_is_measured_again_on_a_repaired_column(cell):
    """keep = the first region itself at a tolerance every repaired column passes (they satisfy it at TOL), then a
    keep box no column passes: count 0 and the repaired columns' keys +inf."""
    from constraint_util import Constraint
    hc = cell["robot"].hip_chain()
    reg = cell["regions"][0]
    same = (Constraint(reg[:7], reg[7:13], reg[13:19]), 1e-5)
    got = _call(hc, cell, repair=cell["repair"], keep=same)
    assert got["repaired"][0] == cell["want"]["repaired"][0] and got["count"][0] >= 1
    far = reg[:7].copy()
    far[0] += 1.0
    none = _call(hc, cell, repair=cell["repair"], keep=(Constraint(far, [-1e-3] * 6, [1e-3] * 6), 1e-6))
    assert (none["count"] == 0).all() and np.isinf(none["restart_key"]).all()


def test_refusals_of_the_repair_argument():
    import torch
    from optik_amd import Robot
    from optik_amd import _native as nat
    bare = Robot.from_urdf_file(*ROBOT_SPECS["panda"]).hip_chain()
    reg = torch.zeros((0, 19), dtype=torch.float64, device="cuda:0")
    x0 = torch.zeros((0, 7), dtype=torch.float64, device="cuda:0")
    with pytest.raises(nat.OptikHipError, match="no collision model"):   # at T = 0 too
        bare.ik_region(reg, x0, 0, R, K, MIN_DIST, repair=dict(influence=0.1, safety=0.02))
    for bad in (dict(influence=0.02, safety=0.02), dict(influence=0.1, safety=0.02, iters=5000),
                dict(influence=0.1, safety=0.02, step=0.0), dict(influence=0.1), dict(influence=0.1, safety=0.02, x=1)):
        with pytest.raises(ValueError):
            bare.ik_region(reg, x0, 0, R, K, MIN_DIST, repair=bad)
    wide = Robot.from_urdf_file(*ROBOT_SPECS["arm9"]).hip_chain()
    with pytest.raises(nat.OptikHipError, match="not supported"):
        wide.ik_region(reg, torch.zeros((0, 9), dtype=torch.float64, device="cuda:0"), 0, R, K, MIN_DIST,
                       repair=dict(influence=0.1, safety=0.02))
