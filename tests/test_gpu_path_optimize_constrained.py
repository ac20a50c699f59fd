"""-m gpu: path optimisation under a pose constraint on the device (HipChain.path_optimize_constrained /
optik_hip_path_optimize_constrained, Robot.optimize_paths_constrained / optik_robot_path_optimize_constrained) against
the reference composed in tests/path_optimize_constrained_util.py from the two host drivers, applied to
link_frames_batch's frames: bit for bit; the fallback; the free box against path_optimize; the launch shape; the
invariant; the scene of the host test; a NaN waypoint; the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import path_optimize_constrained_util as pcu
from avoid_util import Scene, make_test_world
from conftest import ROBOT_SPECS
from constraint_util import Constraint, free_constraint, pinned_constraint, upright_constraint
from gpu_util import assert_bit_equal
from path_optimize_util import Params, line_path

pytestmark = pytest.mark.gpu

NAMES = ["panda", "ur3e", "arm8"]
LENGTHS = [3, 5, 64]   # one interior lane, a few, a full wave
COUNTS = [1, 5, 130]   # one path, a partial block of 4 waves, more than one block
PRM = Params(0.05, 1.0, 2.0, 0.25, 0.03)
TILT = 0.1
# the projection: the defaults but for the budget, which bounds the time the host reference takes on waypoints that
# start far from the constraint (both outcomes occur, and both are compared)
PROJ = dict(ptol=1e-6, piters=24, damping=1e-6, max_step=0.5)
KEYS = ("q", "cost_first", "cost_last", "clearance", "violation")
_SETUPS = {}


@pytest.fixture(scope="module")
def co(tmp_path_factory):
    return pcu.build_composed(str(tmp_path_factory.mktemp("pathopt_con_gpu")),
                              str(tmp_path_factory.mktemp("constraint_con_gpu")))


def _setup(name):
    """Robot and HipChain with a model with self pairs and the spheres, boxes and grid of make_test_world(), and the
    chain tables the device reads."""
    if name not in _SETUPS:
        from optik_amd import Robot
        from optik_amd.collision import auto_pairs, spheres_along_chain
        robot = Robot.from_urdf_file(*ROBOT_SPECS[name])
        n = robot.num_positions()
        frames, centers, radii = spheres_along_chain(robot, 0.05, 2)
        spheres, boxes, grid = make_test_world()
        for obj in (robot, robot.hip_chain()):
            obj.set_collision_model(frames, centers, radii, self_pairs="auto", margin=0.0)
            obj.set_world(spheres=spheres, boxes=boxes)
            obj.set_world_grid(*grid)
        tables = robot.chain_tables()
        scene = Scene(tables["axes"][:n], frames, centers, radii, auto_pairs(frames), spheres, boxes, grid,
                      PRM.influence, PRM.safety)
        _SETUPS[name] = (robot, scene, tables)
    return _SETUPS[name]


def _paths(robot, seed, P, L, noise=0.03):
    """P noisy lines between random configurations inside the limits, [P, L, n]."""
    n = robot.num_positions()
    lb, ub = (np.array(v) for v in robot.joint_limits())
    lo, hi = np.maximum(lb, -2.8), np.minimum(ub, 2.8)
    rng = np.random.default_rng(seed)
    ends = rng.uniform(lo, hi, size=(P, 2, n))
    paths = np.array([line_path(a, b, L) for a, b in ends]) + rng.normal(size=(P, L, n)) * noise
    return np.clip(paths, lo, hi)


def _ref7(oracle, tables, q):
    return np.asarray(oracle.fk(oracle.make_chain(**tables), np.asarray(q))[1])


def _dev(paths):
    """[P, L, n] host -> [L, P, n] device."""
    import torch
    return torch.tensor(np.ascontiguousarray(paths.transpose(1, 0, 2)), device="cuda:0")


def _host(t):
    """[L, P, n] device -> [P, L, n] host."""
    return np.ascontiguousarray(t.cpu().numpy().transpose(1, 0, 2))


def _out(res):
    out = {k: res[k].cpu().numpy() for k in ("cost_first", "cost_last", "clearance", "status", "violation")}
    out["q"] = _host(res["q"])
    out["projected"] = np.ascontiguousarray(res["projected"].cpu().numpy().T)
    return out


def _run(hc, paths, c, iters, prm=PRM, proj=PROJ, **kw):
    return _out(hc.path_optimize_constrained(_dev(paths), c, iters, prm.step, prm.w_smooth, prm.w_obs, prm.influence,
                                             prm.safety, **proj, **kw))


def _frames(hc, paths):
    P, L, n = paths.shape
    q = _dev(paths).reshape(L * P, n).T.contiguous()
    return hc.link_frames_batch(q).cpu().numpy().reshape(L, P, n + 2, 7).transpose(1, 0, 2, 3)


def _reference(co, hc, scene, tables, c, paths, prm=PRM, proj=PROJ, update=True):
    """The composed reference on the device's own frames of the waypoints: one evaluation and one constrained update."""
    return co.step(scene, prm, tables, c, paths, _frames(hc, paths), proj["ptol"], proj["piters"], proj["damping"],
                   proj["max_step"], update=update)


def _agree(got, ref, ref2, violation, what):
    """got: the device after one update; ref: the reference's update of the input; ref2: its evaluation of ref's q."""
    assert_bit_equal(got["q"], ref["q"], what + " waypoints after one update")
    assert_bit_equal(got["cost_first"], ref["cost"], what + " cost_first")
    assert_bit_equal(got["cost_last"], ref2["cost"], what + " cost_last")
    assert_bit_equal(got["clearance"], ref2["clearance"], what + " clearance")
    assert_bit_equal(got["violation"], violation, what + " violation")
    assert np.array_equal(got["projected"], ref["projected"]), (what, got["projected"], ref["projected"])


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("name", NAMES)
def test_one_update_equals_the_composed_reference_bit_for_bit(co, oracle, name, L):
    robot, scene, tables = _setup(name)
    hc = robot.hip_chain()
    paths = _paths(robot, 100 * NAMES.index(name) + L, max(COUNTS), L)
    c = upright_constraint(_ref7(oracle, tables, paths[0, 0]), TILT)
    ref = _reference(co, hc, scene, tables, c, paths)
    ref2 = _reference(co, hc, scene, tables, c, ref["q"], update=False)
    violation = co.violation(tables, c, ref["q"])
    total = ref["projected"].sum(axis=0)
    print(f"{name} L={L}: {total[0]} projections, {total[1]} ended projected, iterations "
          f"{np.bincount(ref['iterations']).tolist()}")
    assert total[0] == max(COUNTS) * (L - 2) > 0 and total[1] > 0
    assert (ref["cost"][:, 2] > 0.0).sum() >= len(paths) // 4  # (the obstacle term is in play)
    for P in COUNTS:
        got = _run(hc, paths[:P], c, 1)
        assert (got["status"] == 0).all()
        _agree(got, {k: v[:P] for k, v in ref.items() if k != "iterations"}, {k: v[:P] for k, v in ref2.items()
                                                                            if k != "iterations"},
               violation[:P], f"{name} L={L} P={P}")
    # the host form: the same bits, row-major
    out = robot.optimize_paths_constrained(paths[:5], c, 1, PRM.step, PRM.w_smooth, PRM.w_obs, PRM.influence, PRM.safety,
                                           ptol=PROJ["ptol"], iters_project=PROJ["piters"], damping=PROJ["damping"],
                                           max_step=PROJ["max_step"])
    assert sorted(out) == ["clearance", "cost_first", "cost_last", "paths", "projected", "status", "violation"]
    assert_bit_equal(out["paths"], ref["q"][:5], f"{name} L={L} host form waypoints")
    assert_bit_equal(out["cost_first"], ref["cost"][:5], f"{name} L={L} host form cost_first")
    assert_bit_equal(out["cost_last"], ref2["cost"][:5], f"{name} L={L} host form cost_last")
    assert_bit_equal(out["clearance"], ref2["clearance"][:5], f"{name} L={L} host form clearance")
    assert_bit_equal(out["violation"], violation[:5], f"{name} L={L} host form violation")
    assert np.array_equal(out["projected"], ref["projected"][:5]) and (out["status"] == 0).all()


# (seed and scales chosen on the CPU with the composed reference alone: both outcomes occur in numbers)
FALLBACK_SEED, FALLBACK_PTOL = 17, 1e-5


def _fallback_paths(robot, P, L):
    """Short noisy lines about one configuration, the noise growing with the path's index from 1e-4 to 3e-2 rad: after
    the update one Gauss-Newton iteration brings some waypoints of the quiet paths back onto a pinned pose at
    FALLBACK_PTOL and none of the noisy ones (43 of 240 on the frames of a numpy forward kinematics)."""
    n = robot.num_positions()
    lb, ub = (np.array(v) for v in robot.joint_limits())
    q0 = np.clip(0.5 * (lb + ub) + 0.3, lb + 0.3, ub - 0.3)
    rng = np.random.default_rng(FALLBACK_SEED)
    scale = np.geomspace(1e-4, 3e-2, P)[:, None, None]
    paths = q0 + rng.normal(size=(P, L, n)) * scale
    return q0, np.clip(paths, lb, ub)


def test_the_fallback_is_taken(co, oracle):
    robot, scene, tables = _setup("panda")
    hc = robot.hip_chain()
    q0, paths = _fallback_paths(robot, 24, 12)
    c = pinned_constraint(_ref7(oracle, tables, q0))
    proj = dict(PROJ, ptol=FALLBACK_PTOL, piters=1)
    ref = _reference(co, hc, scene, tables, c, paths, proj=proj)
    total = ref["projected"].sum(axis=0)
    print("pinned box, one iteration:", total.tolist(), "per path", ref["projected"][:, 1].tolist())
    assert 0 < total[1] < total[0]
    ref2 = _reference(co, hc, scene, tables, c, ref["q"], proj=proj, update=False)
    got = _run(hc, paths, c, 1, proj=proj)
    kept = ref["kept"]
    assert kept.sum() == total[0] - total[1] and not kept[:, [0, -1]].any()
    assert np.array_equal(got["q"][kept].view(np.uint64), paths[kept].view(np.uint64)), "a kept waypoint is the input's"
    _agree(got, ref, ref2, co.violation(tables, c, ref["q"]), "pinned box")
    assert (got["violation"] > FALLBACK_PTOL).any(), "a kept waypoint is reported, not hidden"


def test_no_update_copies_the_input_and_reports_it(co, oracle):
    robot, scene, tables = _setup("panda")
    hc = robot.hip_chain()
    paths = _paths(robot, 5, 9, 12)
    c = upright_constraint(_ref7(oracle, tables, paths[0, 0]), TILT)
    ref = _reference(co, hc, scene, tables, c, paths, update=False)
    got = _run(hc, paths, c, 0)
    assert np.array_equal(got["q"].view(np.uint64), paths.view(np.uint64))
    assert_bit_equal(got["cost_first"], ref["cost"], "cost_first")
    assert_bit_equal(got["cost_last"], ref["cost"], "cost_last")
    assert_bit_equal(got["clearance"], ref["clearance"], "clearance")
    assert_bit_equal(got["violation"], co.violation(tables, c, paths), "the input's violation")
    assert (got["violation"] > 0.0).any() and (got["projected"] == 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_a_free_box_is_path_optimize(name):
    robot, _, _ = _setup(name)
    hc = robot.hip_chain()
    paths = _paths(robot, 31, 9, 20)
    c = free_constraint([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    got = _run(hc, paths, c, 3, proj=dict(ptol=0.0, piters=0, damping=1e-6, max_step=0.5))
    want = hc.path_optimize(_dev(paths), 3, PRM.step, PRM.w_smooth, PRM.w_obs, PRM.influence, PRM.safety)
    assert_bit_equal(got["q"], _host(want["q"]), "waypoints")
    for key in ("cost_first", "cost_last", "clearance"):
        assert_bit_equal(got[key], want[key].cpu().numpy(), key)
    assert np.array_equal(got["status"], want["status"].cpu().numpy())
    assert (got["violation"] == 0.0).all() and (got["projected"] == 0).all()
    assert not np.array_equal(got["q"], paths)


def test_launch_shape_does_not_matter(oracle):
    """K = 5 updates in one launch are 5 chained in-place launches of one update (the counters add up); 130 paths in
    one launch are the same paths one per launch; and a grid capped at one block, whose waves take several paths
    each (tests/test_gpu_grid_stride.py), gives the same bits."""
    from optik_amd import _native as nat
    robot, _, tables = _setup("panda")
    hc = robot.hip_chain()
    K, L, P = 5, 20, 130
    paths = _paths(robot, 7, P, L)
    c = upright_constraint(_ref7(oracle, tables, paths[0, 0]), TILT)
    fused = _run(hc, paths, c, K)
    assert fused["projected"][:, 0].tolist() == [K * (L - 2)] * P and 0 < fused["projected"][:, 1].sum()
    q = _dev(paths)
    first, counts = None, np.zeros((P, 2), dtype=np.int64)
    for k in range(K):
        res = hc.path_optimize_constrained(q, c, 1, PRM.step, PRM.w_smooth, PRM.w_obs, PRM.influence, PRM.safety, **PROJ,
                                           out=q)
        assert res["q"] is q
        if k == 0:
            first = res["cost_first"].cpu().numpy()
        counts += res["projected"].cpu().numpy().T
    last = _out(res)
    assert_bit_equal(fused["q"], _host(q), "5 updates in one launch vs 5 launches")
    assert_bit_equal(fused["cost_first"], first, "cost_first")
    for key in ("cost_last", "clearance", "violation"):
        assert_bit_equal(fused[key], last[key], key)
    assert np.array_equal(fused["projected"], counts)
    assert not np.array_equal(fused["q"], paths)
    for p in range(P):
        single = _run(hc, paths[p:p + 1], c, K)
        for key in KEYS:
            assert_bit_equal(single[key], fused[key][p:p + 1], f"path {p} alone: {key}")
        assert np.array_equal(single["projected"], fused["projected"][p:p + 1]), p
    with nat.options(grid_cap=1):
        assert nat.get_option("grid_cap") == 1
        capped = _run(hc, paths, c, K)
    for key in KEYS:
        assert_bit_equal(capped[key], fused[key], f"grid_cap = 1: {key}")
    assert np.array_equal(capped["projected"], fused["projected"]) and np.array_equal(capped["status"], fused["status"])


def test_waypoints_on_the_constraint_stay_on_it(oracle):
    """From resample_paths_constrained's output, every waypoint within ptol, K updates leave every path's violation
    within ptol -- whether or not every projection ended -- and the violation is what constraint_batch_arrays says."""
    from optik_amd import PoseConstraint
    robot, _, _ = _setup("panda")
    n, ptol, K = robot.num_positions(), 1e-6, 10
    rough = _paths(robot, 23, 24, 6)
    c = PoseConstraint.upright(np.array(robot.fk(list(rough[0, 0]))), 0.3)
    ends = robot.constraint_project_batch_arrays(rough[:, [0, -1]].reshape(-1, n), c, ptol)
    good = (ends["status"].reshape(-1, 2) == 0).all(axis=1)
    lines = np.array([line_path(a, b, 6) for a, b in ends["x"].reshape(-1, 2, n)[good]])
    dense, st, _ = robot.resample_paths_constrained(lines, None, c, 16, ptol=ptol)
    dense = dense[st == 0]
    P = len(dense)
    assert P >= 8
    v_in = robot.constraint_batch_arrays(dense.reshape(-1, n), c)[1].reshape(P, 16)
    assert (v_in <= ptol).all()
    res = robot.optimize_paths_constrained(dense, c, K, PRM.step / 4, PRM.w_smooth, PRM.w_obs, PRM.influence, PRM.safety,
                                           ptol=ptol, iters_project=8)
    print("invariant: projected", res["projected"].sum(axis=0).tolist(), "violation max", res["violation"].max())
    assert (res["projected"][:, 0] == K * 14).all() and res["projected"][:, 1].sum() > 0
    assert (res["violation"] <= ptol).all() and (res["status"] == 0).all()
    v_out = robot.constraint_batch_arrays(res["paths"].reshape(-1, n), c)[1].reshape(P, 16)
    assert_bit_equal(res["violation"], v_out.max(axis=1), "violation vs constraint_batch_arrays")
    assert not np.array_equal(res["paths"], dense)
    assert np.array_equal(res["paths"][:, [0, -1]].view(np.uint64), dense[:, [0, -1]].view(np.uint64))


def test_blocked_scene_comes_out_free_and_upright():
    """The scene of tests/test_path_optimize_constrained_host.py on the device: optimize_paths clears the sphere and
    tips the tool over; optimize_paths_constrained clears it with the tool upright."""
    from optik_amd import PoseConstraint
    sc = pcu.blocked_scene()
    robot = sc["robot"]
    robot.set_collision_model(sc["frames"], sc["centers"], sc["radii"], self_pairs=None, margin=0.0)
    robot.set_world(spheres=sc["spheres"])
    path = line_path(sc["qa"], sc["qb"], sc["L"])
    c = PoseConstraint.upright(np.array(robot.fk(list(sc["qa"]))), pcu.UPRIGHT_TILT)
    resolution, tol = 0.05, pcu.UPRIGHT_TOL
    assert not robot.collision_motion_batch_arrays(path[:-1], path[1:], resolution)[1].all()  # blocked
    assert robot.check_paths_constraint(path[None], None, c, tol, resolution)["ok"][0]        # and upright
    plain = robot.optimize_paths(path[None], influence=sc["influence"], safety=sc["safety"], resolution=resolution)
    assert plain[5][0] and not robot.check_paths_constraint(plain[0], None, c, tol, resolution)["ok"][0]
    res = robot.optimize_paths_constrained(path[None], c, influence=sc["influence"], safety=sc["safety"],
                                           resolution=resolution, tol=tol)
    print("clearance", res["clearance"], "F_obs", res["cost_first"][0, 2], "->", res["cost_last"][0, 2], "violation",
          res["violation"], "projected", res["projected"].tolist())
    assert res["free"].shape == res["keeps"].shape == (1,) and res["free"][0] and res["keeps"][0]
    assert res["status"][0] == 0 and res["violation"][0] <= pcu.PTOL
    assert res["cost_last"][0, 2] < res["cost_first"][0, 2] and res["clearance"][0] >= sc["safety"]
    assert res["projected"][0, 0] == res["projected"][0, 1] > 0
    assert np.array_equal(res["paths"][0, [0, -1]].view(np.uint64), path[[0, -1]].view(np.uint64))
    # without a resolution nothing is checked; tol alone is refused
    assert "free" not in robot.optimize_paths_constrained(path[None], c, 1)
    with pytest.raises(ValueError):
        robot.optimize_paths_constrained(path[None], c, 1, tol=tol)


def test_a_nan_waypoint_spoils_its_own_path_only(oracle):
    robot, _, tables = _setup("panda")
    hc = robot.hip_chain()
    paths = _paths(robot, 11, 5, 12)
    c = upright_constraint(_ref7(oracle, tables, paths[0, 0]), TILT)
    want = _run(hc, paths, c, 4)
    bad = paths.copy()
    bad[2, 6, 3] = math.nan
    got = _run(hc, bad, c, 4)
    assert got["status"].tolist() == [0, 0, 1, 0, 0]
    assert np.isnan(got["cost_first"][2]).all() and np.isnan(got["cost_last"][2]).all()
    assert np.isnan(got["clearance"][2]) and np.isnan(got["violation"][2])
    ok = [0, 1, 3, 4]
    for key in KEYS:
        assert_bit_equal(got[key][ok], want[key][ok], f"the other four paths: {key}")
    assert np.array_equal(got["projected"][ok], want["projected"][ok])
    # (the ends of the spoilt path do not move either, and nothing of it ends projected: every step is NaN)
    assert np.array_equal(got["q"][2, [0, -1]].view(np.uint64), paths[2, [0, -1]].view(np.uint64))
    assert got["projected"][2].tolist() == [4 * 10, 0]


def test_bad_arguments_are_einval(oracle):
    import torch
    from optik_amd import _native as nat
    robot, _, tables = _setup("panda")
    hc = robot.hip_chain()
    dp = C.POINTER(C.c_double)
    ref7 = _ref7(oracle, tables, np.zeros(7))
    box = upright_constraint(ref7, TILT)
    flipped = Constraint(ref7, box.lo, box.hi)
    flipped.lo = box.lo.copy()
    flipped.lo[4] = box.hi[4] + 1.0
    nan_ref = Constraint(np.where(np.arange(7) == 1, math.nan, ref7), box.lo, box.hi)
    good = dict(L=8, iters=1, step=0.05, w_smooth=1.0, w_obs=1.0, influence=0.2, safety=0.05, c=box, ptol=1e-6,
                piters=4, damping=1e-6, max_step=0.5)
    bad = [dict(L=2), dict(L=65), dict(influence=0.05), dict(influence=0.04), dict(step=0.0), dict(iters=-1),
           dict(step=math.inf), dict(w_smooth=-1.0), dict(w_obs=math.nan), dict(safety=-0.01), dict(influence=math.inf),
           dict(c=flipped), dict(c=nan_ref), dict(ptol=-1.0), dict(piters=nat.CONSTRAINT_MAX_ITERS + 1),
           dict(damping=math.inf), dict(damping=math.nan), dict(max_step=0.0), dict(max_step=-1.0)]

    def raw(a, chain, q, P):
        arr = lambda v: np.ascontiguousarray(v, dtype=np.float64).ctypes.data_as(dp)  # noqa: E731
        ptr = q.data_ptr() if q is not None else None
        return nat.lib().optik_hip_path_optimize_constrained(
            chain._h, None, ptr, a["L"], P, a["iters"], a["step"], a["w_smooth"], a["w_obs"], a["influence"],
            a["safety"], arr(a["c"].ref7), arr(a["c"].lo), arr(a["c"].hi), a["ptol"], a["piters"], a["damping"],
            a["max_step"], ptr, None, None, None, None, None, None, None)

    for change in bad:
        a = dict(good, **change)
        q = torch.zeros((a["L"], 2, 7), dtype=torch.float64, device="cuda:0")
        assert raw(a, hc, q, 2) == -1, change  # OPTIK_HIP_EINVAL
        assert raw(a, hc, None, 0) == -1, ("also when P = 0", change)
        with pytest.raises(ValueError):
            hc.path_optimize_constrained(q, a["c"], a["iters"], a["step"], a["w_smooth"], a["w_obs"], a["influence"],
                                         a["safety"], a["ptol"], a["piters"], a["damping"], a["max_step"])
        with pytest.raises(ValueError):
            robot.optimize_paths_constrained(np.zeros((2, a["L"], 7)), a["c"], a["iters"], a["step"], a["w_smooth"],
                                             a["w_obs"], a["influence"], a["safety"], ptol=a["ptol"],
                                             iters_project=a["piters"], damping=a["damping"], max_step=a["max_step"])
    q = torch.zeros((8, 2, 7), dtype=torch.float64, device="cuda:0")
    assert raw(good, hc, q, -1) == -1
    # P = 0 is a no-op
    assert raw(good, hc, None, 0) == 0
    out = robot.optimize_paths_constrained(np.zeros((0, 8, 7)), box, 1)
    assert out["paths"].shape == (0, 8, 7) and out["violation"].shape == (0,) and out["projected"].shape == (0, 2)
    res = hc.path_optimize_constrained(torch.zeros((8, 0, 7), dtype=torch.float64, device="cuda:0"), box, 1, 0.05, 1.0,
                                       1.0, 0.2, 0.05)
    assert res["q"].shape == (8, 0, 7) and res["projected"].shape == (2, 0)


@pytest.mark.parametrize("name", ["arm9", "gantry"])
def test_unsupported_chains_are_refused_also_without_paths(name):
    import torch
    from optik_amd import Robot
    from optik_amd import _native as nat
    robot = Robot.from_urdf_file(*ROBOT_SPECS[name])
    n = robot.num_positions()
    hc = robot.hip_chain()
    c = upright_constraint([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], TILT)
    for P in (0, 3):
        q = torch.zeros((8, P, n), dtype=torch.float64, device="cuda:0")
        with pytest.raises(nat.OptikHipError, match="not supported"):
            hc.path_optimize_constrained(q, c, 1, 0.05, 1.0, 1.0, 0.2, 0.05)
        with pytest.raises(RuntimeError, match="not supported"):
            robot.optimize_paths_constrained(np.zeros((P, 8, n)), c, 1)
