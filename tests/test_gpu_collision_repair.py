"""-m gpu: collision repair on the device (HipChain.collision_repair_batch / optik_hip_collision_repair_batch,
Robot.repair_configurations / optik_robot_collision_repair_batch) against repair_reference of
optik_amd/csrc/repair_measure.hpp as tests/repair_util.py builds it for the host.

Which of the two comparisons was done: the reference runs on the HOST's forward kinematics (constraint::fk under the
lane emulation, the operation sequence of ik_eval.hpp's forward pass) and its own witness rows, not on rows read back
from the device -- so all six outputs are compared bit for bit over the whole loop, forward kinematics, witness pass,
hinge, step, projection and the violation included.

Also: the wave borders and the capped grid, chains of 1, 2, 6, 7 and 8 joints with and without a tip frame, the three
world kinds, the mixed batch, the properties of status-0 rows by the public checks, the host-row form, the refusals."""
import ctypes as C

import numpy as np
import pytest

import repair_util as ru
from avoid_util import Scene, make_test_world
from conftest import ROBOT_SPECS
from constraint_util import Constraint, free_constraint
from gpu_util import _out, _sentinels_left, assert_bit_equal

pytestmark = pytest.mark.gpu

# 1 and 2 joints without a tip frame, 6 and 7 with one, 7 with another tip, 8 with one
NAMES = ["panda1", "panda2", "ur10", "panda", "panda_hand", "arm8"]
SIZES = [1, 63, 64, 65, 130]   # the wave borders
# (a budget that bounds the time the host reference takes; rows that end FREE at once, FREE after steps and LIMIT all
# occur and all are compared; STUCK and NAN rows are the mixed batch's)
PRM = ru.Params(0.1, 0.02, 0.05, 24)
PROJ = dict(ptol=1e-6, piters=24, damping=1e-6, max_step=0.5)
SHORT_CENTRE = [[0.35, 0.0, 0.05]]   # in the last frame of the 1- and 2-joint chains
_SETUPS = {}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ru.build_repair(str(tmp_path_factory.mktemp("repair_gpu")))


def _small_grid():
    """8^3 nodes of 0.25 m over [-1, 0.75]^2 x [0, 1.75]: a tilted ceiling near z = 0.8."""
    i, j, k = np.meshgrid(*(np.arange(8),) * 3, indexing="ij")
    values = (0.8 - 0.25 * k + 0.02 * i - 0.01 * j).astype(np.float32)
    return np.array([-1.0, -1.0, 0.0]), 0.25, values


def _setup(name, world="all"):
    """Robot and HipChain with a sphere model with self pairs and the world asked for, the scene as the host driver
    reads it and the chain tables the device reads."""
    key = (name, world)
    if key not in _SETUPS:
        from optik_amd import Robot
        from optik_amd.collision import auto_pairs, spheres_along_chain
        robot = Robot.from_urdf_file(*ROBOT_SPECS[name])
        n = robot.num_positions()
        frames, centers, radii = spheres_along_chain(robot, 0.05, 2)
        frames = np.asarray(frames, dtype=np.int32).ravel()
        if n <= 2:  # (the Panda's first links stand on the base's axis: a sphere held out on an arm of 35 cm instead)
            frames, centers, radii = np.array([n + 1], dtype=np.int32), np.array(SHORT_CENTRE), np.array([0.08])
        radii = np.broadcast_to(np.asarray(radii, dtype=np.float64), (len(frames),)).copy()
        spheres, boxes, grid = make_test_world()
        if world == "spheres":
            boxes, grid = None, None
        elif world == "boxes":
            spheres, grid = None, None
        elif world == "grid":
            spheres, boxes, grid = None, None, _small_grid()
        for obj in (robot, robot.hip_chain()):
            obj.set_collision_model(frames, centers, radii, self_pairs="auto", margin=0.0)
            obj.set_world(spheres=spheres, boxes=boxes)
            if grid is not None:
                obj.set_world_grid(*grid)
        tables = robot.chain_tables()
        scene = Scene(tables["axes"][:n], frames, centers, radii, auto_pairs(frames), spheres, boxes, grid,
                      PRM.influence, PRM.safety)
        _SETUPS[key] = (robot, scene, tables)
    return _SETUPS[key]


def _rows(robot, seed, B):
    lb, ub = (np.array(v) for v in robot.joint_limits())
    return np.random.default_rng(seed).uniform(np.maximum(lb, -2.8), np.minimum(ub, 2.8), (B, len(lb)))


def _device(hc, x, prm=PRM, c=None, proj=PROJ):
    """One call into sentinel-filled outputs; host arrays, x as [B, n]."""
    import torch
    B, n = x.shape
    q = torch.tensor(np.ascontiguousarray(x.T), device="cuda:0")
    res = dict(x=_out((n, B), torch.float64), clearance=_out((B,), torch.float64), violation=_out((B,), torch.float64),
               moved=_out((B,), torch.float64), status=_out((B,), torch.int32), iterations=_out((B,), torch.int32))
    box = (None, None, None)
    if c is not None:
        dp = C.POINTER(C.c_double)
        keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (c.ref7, c.lo, c.hi)]
        box = tuple(a.ctypes.data_as(dp) for a in keep)
    hc.collision_repair_into(q, prm.influence, prm.safety, prm.step, prm.iters, prm.max_move, box, proj["ptol"],
                             proj["piters"], proj["damping"], proj["max_step"], None, res)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in res.items()}
    for k, v in out.items():
        assert _sentinels_left(v) == 0, f"{k}: elements were not written"
    out["x"] = np.ascontiguousarray(out["x"].T)
    return out


def _agree(got, want, what):
    for k in ("x", "clearance", "violation", "moved"):
        assert_bit_equal(got[k], want[k], f"{what} {k}")
    for k in ("status", "iterations"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k].tolist(), want[k].tolist())


def _take(res, B):
    return {k: v[:B] for k, v in res.items()}


def _ref7(oracle, tables, q):
    return np.asarray(oracle.fk(oracle.make_chain(**tables), np.asarray(q))[1])


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_host_reference_bit_for_bit(ref, oracle, name):
    """All six outputs, without a box and under one, at every batch size of SIZES and under a capped grid."""
    from optik_amd import _native as nat
    robot, scene, tables = _setup(name)
    hc = robot.hip_chain()
    x = _rows(robot, 10 + NAMES.index(name), max(SIZES))
    want = ref.repair(tables, scene, PRM, x)
    print(f"{name}: status {np.bincount(want['status'], minlength=4).tolist()}, iterations up to "
          f"{int(want['iterations'].max())}")
    assert (want["iterations"] > 0).sum() >= 8, "rows that move are part of the comparison"
    for B in SIZES:
        _agree(_device(hc, x[:B]), _take(want, B), f"{name} B={B}")
    x3 = np.concatenate([x, x, x])[:300]   # under the capped grid one block of 256 lanes: rows 256 .. 299 on a second trip
    with nat.options(grid_cap=1):
        got3 = _device(hc, x3)
    _agree(_take(got3, 130), want, f"{name} capped grid, first trip")
    _agree({k: v[260:300] for k, v in got3.items()}, _take(want, 40), f"{name} capped grid, second trip")
    # under a box: the rows near row 0, the tool within 15 cm of row 0's and free to turn
    lb, ub = (np.array(v) for v in robot.joint_limits())
    near = np.clip(x[0] + 0.3 * np.random.default_rng(5).normal(size=(65, len(lb))), lb, ub)
    inf = np.inf
    c = Constraint(_ref7(oracle, tables, x[0]), [-0.15] * 3 + [-inf] * 3, [0.15] * 3 + [inf] * 3)
    wantc = ref.repair(tables, scene, PRM, near, c, **PROJ)
    print(f"{name} boxed: status {np.bincount(wantc['status'], minlength=4).tolist()}")
    _agree(_device(hc, near, c=c), wantc, f"{name} boxed")
    # a box free on every axis is no box
    _agree(_device(hc, x[:65], c=free_constraint(c.ref7)), _take(want, 65), f"{name} free box")


@pytest.mark.parametrize("world", ["spheres", "boxes", "grid"])
def test_world_kinds(ref, world):
    robot, scene, tables = _setup("panda", world)
    x = _rows(robot, 21, 65)
    want = ref.repair(tables, scene, PRM, x)
    print(f"{world}: status {np.bincount(want['status'], minlength=4).tolist()}")
    assert (want["iterations"] > 0).any()
    _agree(_device(robot.hip_chain(), x), want, world)


def test_the_mixed_batch_and_the_public_checks(ref, oracle):
    """Free, colliding, NaN, infinite, on-the-limit and stuck rows in one call; the free rows come back byte for byte;
    every status-0 row is free by collision_clearance_batch_arrays at the safety distance and, under the box, within
    ptol by constraint_batch_arrays; the host-row form gives the same bits."""
    robot, scene, tables = _setup("panda")
    hc = robot.hip_chain()
    lb, ub = (np.array(v) for v in robot.joint_limits())
    x = _rows(robot, 33, 96)
    x[5, 2], x[6, 0] = np.nan, np.inf
    x[7] = np.where(np.arange(7) % 2 == 0, ub, lb)
    prm = ru.Params(0.1, 0.02, 0.05, 48, 0.15)   # (max_move 0.15: some rows get stuck on it)
    want = ref.repair(tables, scene, prm, x)
    got = _device(hc, x, prm)
    _agree(got, want, "mixed")
    counts = np.bincount(got["status"], minlength=4)
    print("mixed:", counts.tolist())
    assert counts[ru.FREE] > 0 and counts[ru.STUCK] > 0 and counts[ru.NAN] == 2
    untouched = got["iterations"] == 0
    assert untouched.sum() >= 8 and got["x"][untouched].tobytes() == x[untouched].tobytes()
    ok = got["status"] == ru.FREE
    clr = robot.collision_clearance_batch_arrays(got["x"][ok])[0]
    assert_bit_equal(clr, got["clearance"][ok], "the public clearance of the status-0 rows")
    assert (clr >= prm.safety).all()
    moved = ok & (got["iterations"] > 0)
    assert moved.any() and (got["x"][moved] >= lb).all() and (got["x"][moved] <= ub).all()
    assert (got["moved"] <= prm.max_move).all()
    # under a box
    near = np.clip(x[0] + 0.3 * np.random.default_rng(6).normal(size=(64, 7)), lb, ub)
    inf = np.inf
    from optik_amd import PoseConstraint
    region = PoseConstraint(np.array(robot.fk(list(x[0]))), [-0.15] * 3 + [-inf] * 3, [0.15] * 3 + [inf] * 3)
    out = robot.repair_configurations(near, PRM.influence, PRM.safety, PRM.step, PRM.iters, region=region,
                                      tol=PROJ["ptol"], iters_project=PROJ["piters"], damping=PROJ["damping"],
                                      max_step=PROJ["max_step"])
    assert sorted(out) == sorted(ru.KEYS)
    wantc = ref.repair(tables, scene, PRM, near, Constraint(region.ref7, region.lo, region.hi), **PROJ)
    _agree(out, wantc, "host rows, boxed")
    okc = (out["status"] == ru.FREE) & (out["iterations"] > 0)
    assert okc.any()
    v = robot.constraint_batch_arrays(out["x"][okc], region)[1]
    assert (v <= PROJ["ptol"]).all()
    assert (robot.collision_clearance_batch_arrays(out["x"][okc])[0] >= PRM.safety).all()
    # in place, and twice the same bits
    import torch
    q = torch.tensor(np.ascontiguousarray(x.T), device="cuda:0")
    res = hc.collision_repair_batch(q, prm.influence, prm.safety, prm.step, prm.iters, max_move=prm.max_move, out=q)
    assert res["x"] is q
    assert_bit_equal(q.cpu().numpy().T, got["x"], "in place")
    assert np.array_equal(res["status"].cpu().numpy(), got["status"])


def test_refusals_before_any_device_work(oracle):
    import torch
    from optik_amd import Robot
    from optik_amd import _native as nat
    robot, _, tables = _setup("panda")
    hc = robot.hip_chain()
    dp = C.POINTER(C.c_double)
    good = dict(influence=0.1, safety=0.02, step=0.05, iters=8, max_move=np.inf, ref=[0.0, 0, 0, 0, 0, 0, 1],
                lo=[-1.0] * 6, hi=[1.0] * 6, ptol=1e-6, piters=8, damping=1e-6, pstep=0.5)

    def raw(chain, a, B, box=True):
        keep = [np.ascontiguousarray(a[k], dtype=np.float64) for k in ("ref", "lo", "hi")]
        ptrs = [k.ctypes.data_as(dp) for k in keep] if box else [None, None, None]
        q = torch.zeros((7, max(B, 1)), dtype=torch.float64, device="cuda:0")
        o = nat.RepairOutputs(q.data_ptr(), None, None, None, None, None)
        return nat.lib().optik_hip_collision_repair_batch(
            chain._h, None, q.data_ptr() if B else None, B, a["influence"], a["safety"], a["step"], a["iters"],
            a["max_move"], *ptrs, a["ptol"], a["piters"], a["damping"], a["pstep"], C.byref(o), None)

    assert raw(hc, good, 3) == 0 and raw(hc, good, 0) == 0 and raw(hc, good, 3, box=False) == 0
    bad = [dict(influence=0.02), dict(safety=-0.01), dict(step=0.0), dict(step=np.inf), dict(influence=np.nan),
           dict(iters=-1), dict(iters=4097), dict(max_move=-1.0), dict(max_move=np.nan),
           dict(ref=[0.0, 0, 0, 0, 0, 0, 2]), dict(lo=[2.0] * 6), dict(ptol=-1.0), dict(piters=4097),
           dict(damping=-1.0), dict(pstep=0.0)]
    for change in bad:
        a = dict(good, **change)
        assert raw(hc, a, 3) == -1, change   # OPTIK_HIP_EINVAL
        assert raw(hc, a, 0) == -1, ("also when B = 0", change)
    # (without a box its projection's arguments are not looked at)
    assert raw(hc, dict(good, ptol=-1.0), 3, box=False) == 0
    assert raw(hc, good, -1) == -1
    q = torch.zeros((7, 2), dtype=torch.float64, device="cuda:0")
    for kw in (dict(influence=0.02, safety=0.02), dict(influence=0.1, safety=0.02, step=-1.0),
               dict(influence=0.1, safety=0.02, iters=5000), dict(influence=0.1, safety=0.02, max_move=-0.5)):
        with pytest.raises(ValueError):
            hc.collision_repair_batch(q, **kw)
        with pytest.raises(ValueError):
            robot.repair_configurations(np.zeros((2, 7)), **kw)
    # no model
    bare = Robot.from_urdf_file(*ROBOT_SPECS["panda"])
    for B in (0, 3):
        assert raw(bare.hip_chain(), good, B) == -1
        assert b"no collision model" in nat.lib().optik_hip_last_error()
        with pytest.raises(RuntimeError, match="no collision model"):
            bare.repair_configurations(np.zeros((B, 7)), 0.1, 0.02)
    # B = 0 with a model is a no-op
    out = robot.repair_configurations(np.zeros((0, 7)), 0.1, 0.02)
    assert out["x"].shape == (0, 7) and out["status"].shape == (0,)


@pytest.mark.parametrize("name", ["arm9", "gantry"])
def test_unsupported_chains_are_refused_also_without_rows(name):
    import torch
    from optik_amd import Robot
    from optik_amd import _native as nat
    robot = Robot.from_urdf_file(*ROBOT_SPECS[name])
    n = robot.num_positions()
    hc = robot.hip_chain()
    for B in (0, 3):
        q = torch.zeros((n, B), dtype=torch.float64, device="cuda:0")
        with pytest.raises(nat.OptikHipError, match="not supported"):
            hc.collision_repair_batch(q, 0.1, 0.02)
        with pytest.raises(RuntimeError, match="not supported"):
            robot.repair_configurations(np.zeros((B, n)), 0.1, 0.02)
