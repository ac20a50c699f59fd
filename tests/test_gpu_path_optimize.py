"""-m gpu: the path optimiser on the device (HipChain.path_optimize / optik_hip_path_optimize, Robot.optimize_paths /
optik_robot_path_optimize) against optik_amd/csrc/path_optimize.hpp built with g++ and applied to link_frames_batch's
frames: bit for bit; the launch shape does not matter; the blocked scene of the host test comes out free."""
import math

import numpy as np
import pytest

from avoid_util import Scene, make_test_world
from conftest import ROBOT_SPECS
from gpu_util import assert_bit_equal
from path_optimize_util import Params, blocked_scene, build_path_optimize, line_path

pytestmark = pytest.mark.gpu

NAMES = ["panda", "ur3e", "arm8"]
LENGTHS = [3, 5, 33, 64]
COUNTS = [1, 5, 130]  # one path, a partial block of 4 waves, more than one block
PRM = Params(0.05, 1.0, 2.0, 0.25, 0.03)
_SETUPS = {}


@pytest.fixture(scope="module")
def po(tmp_path_factory):
    return build_path_optimize(str(tmp_path_factory.mktemp("pathopt_gpu")))


def _setup(name):
    """Robot and HipChain with a model with self pairs and the spheres, boxes and grid of make_test_world()."""
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
        scene = Scene(robot.chain_tables()["axes"][:n], frames, centers, radii, auto_pairs(frames), spheres, boxes,
                      grid, PRM.influence, PRM.safety)
        _SETUPS[name] = (robot, scene)
    return _SETUPS[name]


def _paths(robot, seed, P, L):
    """P noisy lines between random configurations inside the limits, [P, L, n]."""
    n = robot.num_positions()
    lb, ub = (np.array(v) for v in robot.joint_limits())
    lo, hi = np.maximum(lb, -2.8), np.minimum(ub, 2.8)
    rng = np.random.default_rng(seed)
    ends = rng.uniform(lo, hi, size=(P, 2, n))
    paths = np.array([line_path(a, b, L) for a, b in ends]) + rng.normal(size=(P, L, n)) * 0.03
    return np.clip(paths, lo, hi)


def _dev(paths):
    """[P, L, n] host -> [L, P, n] device."""
    import torch
    return torch.tensor(np.ascontiguousarray(paths.transpose(1, 0, 2)), device="cuda:0")


def _host(t):
    """[L, P, n] device -> [P, L, n] host."""
    return np.ascontiguousarray(t.cpu().numpy().transpose(1, 0, 2))


def _run(hc, paths, iters, prm=PRM, **kw):
    res = hc.path_optimize(_dev(paths), iters, prm.step, prm.w_smooth, prm.w_obs, prm.influence, prm.safety, **kw)
    return dict(q=_host(res["q"]), cost_first=res["cost_first"].cpu().numpy(), cost_last=res["cost_last"].cpu().numpy(),
                clearance=res["clearance"].cpu().numpy(), status=res["status"].cpu().numpy())


def _reference(po, robot, scene, paths, prm=PRM):
    """The host driver on the device's own frames of the waypoints: one evaluation and one update of every path."""
    hc = robot.hip_chain()
    P, L, n = paths.shape
    q = _dev(paths).reshape(L * P, n).T.contiguous()
    frames = hc.link_frames_batch(q).cpu().numpy().reshape(L, P, n + 2, 7).transpose(1, 0, 2, 3)
    clr = hc.collision_batch(q)[0].cpu().numpy().reshape(L, P).min(axis=0)
    return po.step(scene, prm, hc.lb, hc.ub, paths, frames), clr


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("name", NAMES)
def test_one_update_equals_the_host_header_bit_for_bit(po, name, L):
    robot, scene = _setup(name)
    hc = robot.hip_chain()
    paths = _paths(robot, 100 * NAMES.index(name) + L, max(COUNTS), L)
    ref, clr = _reference(po, robot, scene, paths)
    assert (ref["cost"][:, 2] > 0.0).sum() >= len(paths) // 2  # (the obstacle term is in play)
    for P in COUNTS:
        what = f"{name} L={L} P={P}"
        one = _run(hc, paths[:P], 1)
        assert_bit_equal(one["q"], ref["q"][:P], what + " waypoints after one update")
        assert_bit_equal(one["cost_first"], ref["cost"][:P], what + " cost_first")
        assert (one["status"] == 0).all()
        # the input's clearance: the evaluation alone
        zero = _run(hc, paths[:P], 0)
        assert_bit_equal(zero["clearance"], ref["clearance"][:P], what + " clearance of the input")
        assert_bit_equal(zero["clearance"], clr[:P], what + " clearance vs collision_batch's minimum")
        assert_bit_equal(zero["cost_first"], ref["cost"][:P], what + " iters = 0 cost_first")
        assert_bit_equal(zero["cost_last"], ref["cost"][:P], what + " iters = 0 cost_last")
        assert np.array_equal(zero["q"].view(np.uint64), paths[:P].view(np.uint64)), what + ": iters = 0 copies"
    # what follows the update: the last evaluation is the first one of the updated path
    ref2, clr2 = _reference(po, robot, scene, one["q"])
    assert_bit_equal(one["cost_last"], ref2["cost"], f"{name} L={L} cost_last")
    assert_bit_equal(one["clearance"], ref2["clearance"], f"{name} L={L} clearance after the update")
    assert_bit_equal(one["clearance"], clr2, f"{name} L={L} clearance after the update vs collision_batch")
    # the host form: the same bits, row-major
    out = robot.optimize_paths(paths[:5], 1, PRM.step, PRM.w_smooth, PRM.w_obs, PRM.influence, PRM.safety)
    assert_bit_equal(out[0], ref["q"][:5], f"{name} L={L} host form waypoints")
    assert_bit_equal(out[1], ref["cost"][:5], f"{name} L={L} host form cost_first")
    assert_bit_equal(out[2], ref2["cost"][:5], f"{name} L={L} host form cost_last")
    assert_bit_equal(out[3], ref2["clearance"][:5], f"{name} L={L} host form clearance")
    assert (out[4] == 0).all()


def test_launch_shape_does_not_matter():
    """K = 7 updates in one launch are 7 chained launches of one update, and 130 paths in one launch are the same
    paths one per launch: bit for bit."""
    robot, _ = _setup("panda")
    hc = robot.hip_chain()
    K, L, P = 7, 33, 130
    paths = _paths(robot, 7, P, L)
    fused = _run(hc, paths, K)
    q = _dev(paths)
    first = None
    for k in range(K):
        res = hc.path_optimize(q, 1, PRM.step, PRM.w_smooth, PRM.w_obs, PRM.influence, PRM.safety, out=q)
        if k == 0:
            first = res["cost_first"].cpu().numpy()
    assert_bit_equal(fused["q"], _host(q), "7 updates in one launch vs 7 launches")
    assert_bit_equal(fused["cost_first"], first, "cost_first")
    assert_bit_equal(fused["cost_last"], res["cost_last"].cpu().numpy(), "cost_last")
    assert_bit_equal(fused["clearance"], res["clearance"].cpu().numpy(), "clearance")
    assert not np.array_equal(fused["q"], paths)
    for p in range(P):
        single = _run(hc, paths[p:p + 1], K)
        for key in ("q", "cost_first", "cost_last", "clearance"):
            assert_bit_equal(single[key], fused[key][p:p + 1], f"path {p} alone: {key}")


def test_blocked_scene_comes_out_free():
    from optik_amd import _native as nat
    sc = blocked_scene()
    robot = sc["robot"]
    robot.set_collision_model(sc["frames"], sc["centers"], sc["radii"], self_pairs=None, margin=0.0)
    robot.set_world(spheres=sc["spheres"])
    path = line_path(sc["qa"], sc["qb"], sc["L"])
    resolution = 0.05
    before = robot.collision_motion_batch_arrays(path[:-1], path[1:], resolution)[1]
    assert not before.all()  # free = 0 for the input
    out, first, last, clearance, status, free = robot.optimize_paths(
        path[None], influence=sc["influence"], safety=sc["safety"], resolution=resolution)
    print("clearance", clearance, "F_obs", first[0, 2], "->", last[0, 2])
    assert free.shape == (1,) and free[0] and status[0] == 0
    assert last[0, 2] < first[0, 2]
    assert clearance[0] >= sc["safety"]
    assert np.array_equal(out[0, [0, -1]].view(np.uint64), path[[0, -1]].view(np.uint64))
    # the defaults are the documented ones
    again = robot.optimize_paths(path[None], nat.PATH_OPTIMIZE_ITERS, nat.PATH_OPTIMIZE_STEP,
                                 nat.PATH_OPTIMIZE_W_SMOOTH, nat.PATH_OPTIMIZE_W_OBS, sc["influence"], sc["safety"])
    assert_bit_equal(again[0], out, "defaults")


def test_in_place_equals_out_of_place():
    robot, _ = _setup("panda")
    hc = robot.hip_chain()
    paths = _paths(robot, 3, 9, 20)
    want = _run(hc, paths, 3)
    q = _dev(paths)
    res = hc.path_optimize(q, 3, PRM.step, PRM.w_smooth, PRM.w_obs, PRM.influence, PRM.safety, out=q)
    assert res["q"] is q
    assert_bit_equal(_host(q), want["q"], "in place")
    assert_bit_equal(res["cost_last"].cpu().numpy(), want["cost_last"], "in place cost_last")


def test_without_a_model_one_unit_step_is_the_straight_line():
    from optik_amd import Robot
    robot = Robot.from_urdf_file(*ROBOT_SPECS["panda"])
    hc = robot.hip_chain()
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(5)
    for L in (3, 16, 64):
        paths = rng.uniform(np.maximum(lb, -1.0), np.minimum(ub, 1.0), size=(6, L, 7))
        for step, ws in ((1.0, 1.0), (0.25, 4.0)):
            res = _run(hc, paths, 1, Params(step, ws, 3.0, 0.2, 0.05))
            lines = np.array([line_path(p[0], p[-1], L) for p in paths])
            assert np.abs(res["q"] - lines).max() <= 1e-12
            assert (res["cost_first"][:, 2] == 0.0).all() and (res["cost_last"][:, 2] == 0.0).all()
            assert np.isposinf(res["clearance"]).all() and (res["status"] == 0).all()
            assert (res["cost_last"][:, 1] <= res["cost_first"][:, 1]).all()


def test_a_nan_waypoint_spoils_its_own_path_only():
    robot, _ = _setup("panda")
    hc = robot.hip_chain()
    paths = _paths(robot, 11, 5, 12)
    want = _run(hc, paths, 4)
    bad = paths.copy()
    bad[2, 6, 3] = math.nan
    got = _run(hc, bad, 4)
    assert got["status"].tolist() == [0, 0, 1, 0, 0]
    assert np.isnan(got["cost_first"][2]).all() and np.isnan(got["cost_last"][2]).all()
    assert np.isnan(got["clearance"][2])
    ok = [0, 1, 3, 4]
    for key in ("q", "cost_first", "cost_last", "clearance"):
        assert_bit_equal(got[key][ok], want[key][ok], f"the other four paths: {key}")
    # (the ends of the spoilt path do not move either)
    assert np.array_equal(got["q"][2, [0, -1]].view(np.uint64), paths[2, [0, -1]].view(np.uint64))


def test_a_waypoint_outside_the_limits_comes_back_clamped():
    robot, _ = _setup("panda")
    hc = robot.hip_chain()
    paths = _paths(robot, 12, 3, 8)
    paths[1, 3, 0] = hc.ub[0] + 1.0
    paths[2, 5, 6] = hc.lb[6] - 0.5
    res = _run(hc, paths, 1, Params(1e-3, 0.0, 0.0, 0.2, 0.05))  # (no force: the update is the clamp alone)
    want = paths.copy()
    want[1, 3, 0], want[2, 5, 6] = hc.ub[0], hc.lb[6]
    assert np.array_equal(res["q"], want)
    res = _run(hc, paths, 3)
    assert (res["q"][:, 1:-1] <= hc.ub).all() and (res["q"][:, 1:-1] >= hc.lb).all()


def test_bad_arguments_are_einval():
    import torch
    from optik_amd import _native as nat
    robot, _ = _setup("panda")
    hc = robot.hip_chain()
    good = dict(L=8, iters=1, step=0.05, w_smooth=1.0, w_obs=1.0, influence=0.2, safety=0.05)
    bad = [dict(L=2), dict(L=65), dict(influence=0.05), dict(influence=0.04), dict(step=0.0), dict(iters=-1),
           dict(step=math.inf), dict(w_smooth=-1.0), dict(w_obs=math.nan), dict(safety=-0.01), dict(influence=math.inf)]
    for change in bad:
        a = dict(good, **change)
        q = torch.zeros((a["L"], 2, 7), dtype=torch.float64, device="cuda:0")
        rc = nat.lib().optik_hip_path_optimize(hc._h, None, q.data_ptr(), a["L"], 2, a["iters"], a["step"],
                                               a["w_smooth"], a["w_obs"], a["influence"], a["safety"], q.data_ptr(),
                                               None, None, None, None, None)
        assert rc == -1, (change, rc)  # OPTIK_HIP_EINVAL
        with pytest.raises(ValueError):
            hc.path_optimize(q, a["iters"], a["step"], a["w_smooth"], a["w_obs"], a["influence"], a["safety"])
        with pytest.raises(ValueError):
            robot.optimize_paths(np.zeros((2, a["L"], 7)), a["iters"], a["step"], a["w_smooth"], a["w_obs"],
                                 a["influence"], a["safety"])
    q = torch.zeros((8, 2, 7), dtype=torch.float64, device="cuda:0")
    assert nat.lib().optik_hip_path_optimize(hc._h, None, q.data_ptr(), 8, -1, 1, 0.05, 1.0, 1.0, 0.2, 0.05,
                                             q.data_ptr(), None, None, None, None, None) == -1
    # P = 0 is a no-op
    assert nat.lib().optik_hip_path_optimize(hc._h, None, None, 8, 0, 1, 0.05, 1.0, 1.0, 0.2, 0.05, None, None, None,
                                             None, None, None) == 0
    out = robot.optimize_paths(np.zeros((0, 8, 7)), 1)
    assert out[0].shape == (0, 8, 7) and out[4].shape == (0,)


@pytest.mark.parametrize("name", ["arm9", "gantry"])
def test_unsupported_chains_are_refused_also_without_paths(name):
    import torch
    from optik_amd import Robot
    from optik_amd import _native as nat
    robot = Robot.from_urdf_file(*ROBOT_SPECS[name])
    n = robot.num_positions()
    hc = robot.hip_chain()
    for P in (0, 3):
        q = torch.zeros((8, P, n), dtype=torch.float64, device="cuda:0")
        with pytest.raises(nat.OptikHipError, match="not supported"):
            hc.path_optimize(q, 1, 0.05, 1.0, 1.0, 0.2, 0.05)
        with pytest.raises(RuntimeError, match="not supported"):
            robot.optimize_paths(np.zeros((P, 8, n)), 1)
