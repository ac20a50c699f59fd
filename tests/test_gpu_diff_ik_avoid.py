"""-m gpu: collision-avoiding diff_ik (Robot.diff_ik_avoid / diff_ik_avoid_batch_arrays, HipChain.diff_ik_avoid_batch
/ optik_hip_diff_ik_avoid_batch).  A batch row is the single call bit for bit, and both are the g++ chain: the frames
of link_frames_batch, the witness rows of collision_gradient.hpp, the damped LP of diff_ik_lp.hpp."""
import os
import subprocess
import sys

import numpy as np
import pytest

from avoid_util import Scene, build_avoid, make_test_world
from conftest import ROBOT_SPECS, ROBOTS, ROOT
from gpu_util import assert_bit_equal

pytestmark = pytest.mark.gpu

NAMES = ["panda", "ur10", "arm8"]
B = 300
INFLUENCE, SAFETY, GAIN = 0.25, 0.03, 1.0


@pytest.fixture(scope="module")
def avoid(tmp_path_factory):
    return build_avoid(str(tmp_path_factory.mktemp("avoid_gpu_diff_ik")))


def _robot(name):
    from optik_amd import Robot
    return Robot.from_urdf_file(*ROBOT_SPECS[name])


def _setup(name, far=False):
    from optik_amd.collision import auto_pairs, spheres_along_chain
    robot = _robot(name)
    n = robot.num_positions()
    frames, centers, radii = spheres_along_chain(robot, 0.05, 2)
    spheres, boxes, grid = make_test_world()
    if far:  # every obstacle far beyond the influence distance, no self pairs, no grid
        spheres, boxes, grid = spheres + [50.0, 0.0, 0.0, 0.0], boxes + np.array([50.0] + [0.0] * 9), None
        pairs = None
    else:
        pairs = auto_pairs(frames)
    # (Robot.hip_chain() is a chain of its own: the device form gets the same model and world)
    for obj in (robot, robot.hip_chain()):
        obj.set_collision_model(frames, centers, radii, self_pairs=pairs, margin=0.0)
        obj.set_world(spheres=spheres, boxes=boxes)
        if grid is not None:
            obj.set_world_grid(*grid)
    scene = Scene(robot.chain_tables()["axes"][:n], frames, centers, radii, pairs, spheres, boxes, grid,
                  INFLUENCE, SAFETY, GAIN)
    rng = np.random.default_rng(70 + NAMES.index(name))
    lb, ub = (np.array(v) for v in robot.joint_limits())
    x = rng.uniform(np.maximum(lb, -2.8), np.minimum(ub, 2.8), size=(B, n))
    V = rng.normal(size=(B, 6)) * rng.choice([0.05, 0.5, 3.0], size=B)[:, None]
    vm = rng.uniform(0.3, 2.0, size=(B, n))
    x[23, 0] = np.nan
    vm[31, 1] = -1.0
    return robot, scene, x, V, vm


def _rot(quat):
    i, j, k, w = quat
    return np.array([[w * w + i * i - j * j - k * k, 2 * (i * j - w * k), 2 * (w * j + i * k)],
                     [2 * (w * k + i * j), w * w - i * i + j * j - k * k, 2 * (j * k - w * i)],
                     [2 * (i * k - w * j), 2 * (w * i + j * k), w * w - i * i - j * j + k * k]])


@pytest.mark.parametrize("name", NAMES)
def test_batch_rows_are_the_single_call_and_the_host_chain(avoid, name):
    import torch
    robot, scene, x, V, vm = _setup(name)
    n = robot.num_positions()
    alpha, v, found = robot.diff_ik_avoid_batch_arrays(x, V, vm, INFLUENCE, SAFETY, GAIN)
    # the single call, row by row
    for b in range(B):
        out = robot.diff_ik_avoid(x[b], V[b], vm[b], INFLUENCE, SAFETY, GAIN) if not np.isnan(x[b]).any() else None
        assert (out is not None) == bool(found[b]), (name, b)
        if out is not None:
            assert np.array_equal(np.array([out[0]] + out[1]).view(np.uint64),
                                  np.concatenate([[alpha[b]], v[b]]).view(np.uint64)), (name, b)
    assert not found[23] and not found[31] and (v[~found] == 0.0).all() and (alpha[~found] == 0.0).all()
    # the g++ chain on the device's frames and Jacobians
    hc = robot.hip_chain()
    q = torch.tensor(x.T.copy(), device="cuda:0")
    frames = hc.link_frames_batch(q).cpu().numpy()
    jac = hc.fk_batch(q, jacobian=True)[1].cpu().numpy().T
    ref = avoid.avoid(scene, frames, jac, V, vm)
    assert np.array_equal(ref["status"] == 0, found), (name, np.flatnonzero((ref["status"] == 0) != found)[:10])
    assert_bit_equal(alpha, ref["alpha"], f"{name} alpha vs the host chain")
    assert_bit_equal(v, ref["v"], f"{name} v vs the host chain")
    assert (ref["m"] > 0).sum() >= B // 10, np.bincount(ref["m"])  # (the scene does put rows inside the influence)
    # the device form
    da, dv, ds = hc.diff_ik_avoid_batch(q, torch.tensor(V.T.copy(), device="cuda:0"),
                                        torch.tensor(vm.T.copy(), device="cuda:0"), INFLUENCE, SAFETY, GAIN)
    assert_bit_equal(da.cpu().numpy(), alpha, "device form alpha")
    assert_bit_equal(dv.cpu().numpy().T, v, "device form v")
    assert np.array_equal(ds.cpu().numpy() == 0, found)
    # on every solved row: the damper rows hold, the twist is realised, alpha is at most plain diff_ik's
    pa, pv, pf = robot.diff_ik_batch_arrays(x, V, vm)
    solved = np.flatnonzero(found)
    assert len(solved) >= B // 10
    for b in solved:
        m = ref["m"][b]
        assert np.all(ref["G"][b, :m] @ v[b] >= ref["h"][b, :m] - 1e-9), (name, b)
        R = _rot(frames[b, n + 1, 3:])
        J = jac[b].reshape(n, 6).T
        JW = np.vstack([R @ J[:3], R @ J[3:]])
        assert np.allclose(JW @ v[b], alpha[b] * V[b], rtol=0, atol=1e-8), (name, b)
        assert pf[b] and alpha[b] <= pa[b] + 1e-12, (name, b, alpha[b], pa[b])


@pytest.mark.parametrize("name", NAMES)
def test_nothing_within_influence_gives_the_bits_of_diff_ik_batch(name):
    robot, scene, x, V, vm = _setup(name, far=True)
    want = robot.diff_ik_batch_arrays(x, V, vm)
    got = robot.diff_ik_avoid_batch_arrays(x, V, vm, INFLUENCE, SAFETY, GAIN)
    # (row 23 has NaN frames: with a model its rows are NaN, which is no solution and zeros)
    ok = np.arange(B) != 23
    assert not got[2][23] and got[0][23] == 0.0 and (got[1][23] == 0.0).all()
    assert_bit_equal(got[0][ok], want[0][ok], f"{name} alpha, obstacles far away")
    assert_bit_equal(got[1][ok], want[1][ok], f"{name} v, obstacles far away")
    assert np.array_equal(got[2][ok], want[2][ok])
    robot.clear_collision_model()
    got = robot.diff_ik_avoid_batch_arrays(x, V, vm, INFLUENCE, SAFETY, GAIN)
    assert_bit_equal(got[0], want[0], f"{name} alpha, no model")
    assert_bit_equal(got[1], want[1], f"{name} v, no model")
    assert np.array_equal(got[2], want[2])


def _wall_scene(gap):
    """A Panda with a sphere on its end effector and a wall (a box) `gap` metres in front of that sphere along +x."""
    robot = _robot("panda")
    x = np.array([0.0, 0.3, 0.0, -1.8, 0.0, 2.1, 0.7])
    robot.set_collision_model([8], [[0.0, 0.0, 0.0]], [0.05], self_pairs=None)
    tip = np.array(robot.fk(x.tolist()))[:3, 3]
    robot.set_world(boxes=[[tip[0] + 0.05 + gap + 0.1, tip[1], tip[2], 0.0, 0.0, 0.0, 1.0, 0.1, 2.0, 2.0]])
    return robot, x


def test_a_wall_two_centimetres_away():
    robot, x = _wall_scene(0.02)
    V, vm = np.array([0.5, 0.0, 0.0, 0.0, 0.0, 0.0]), np.ones(7)
    influence, safety = 0.1, 0.01
    dist, grad, wit = robot.collision_witness_batch_arrays(x[None])
    assert abs(dist[0, 8] - 0.02) < 1e-12 and tuple(wit[0, 8]) == (0, 1, 0)
    h = -1.0 * (dist[0, 8] - safety) / (influence - safety)
    plain = robot.diff_ik(x, V, vm)
    damped = robot.diff_ik_avoid(x, V, vm, influence, safety)
    assert plain is not None and damped is not None
    assert grad[0, 8] @ np.array(plain[1]) < h - 1e-3   # straight into the wall: the damper row is violated
    assert grad[0, 8] @ np.array(damped[1]) >= h - 1e-9
    assert 0.0 < damped[0] < plain[0]


def test_inside_safety_with_no_way_out_reports_no_solution():
    """A 6-joint arm whose forearm sphere is 10 cm inside an obstacle: the damper asks for a separation speed of
    gain * 0.15 / 0.15 = 100 m/s, which |v| <= 1 rad/s cannot give."""
    robot = _robot("ur10")
    x = np.array([0.3, -1.0, 1.2, 0.2, 0.5, 0.0])
    robot.set_collision_model([3], [[0.0, 0.0, 0.0]], [0.05], self_pairs=None)
    p = np.array(robot.link_frames_batch_arrays(x[None]))[0, 3, :3, 3]
    robot.set_world(spheres=[[p[0] + 0.05, p[1], p[2], 0.1]])
    dist = robot.collision_witness_batch_arrays(x[None])[0]
    assert abs(dist[0, 3] + 0.1) < 1e-12
    alpha, v, found = robot.diff_ik_avoid_batch_arrays(x[None], [0.1, 0, 0, 0, 0, 0], np.ones(6), 0.2, 0.05, 100.0)
    assert not found[0] and alpha[0] == 0.0 and (v[0] == 0.0).all()
    assert robot.diff_ik_avoid(x, [0.1, 0, 0, 0, 0, 0], np.ones(6), 0.2, 0.05, 100.0) is None


def test_bad_damper_parameters_are_einval():
    import torch
    from optik_amd import _native as nat
    robot = _robot("panda")
    hc = robot.hip_chain()
    q = torch.zeros((7, 2), dtype=torch.float64, device="cuda:0")
    V = torch.zeros(6, dtype=torch.float64, device="cuda:0")
    vm = torch.ones(7, dtype=torch.float64, device="cuda:0")
    for infl, safe, gain in [(0.1, 0.1, 1.0), (0.05, 0.1, 1.0), (0.1, -0.01, 1.0), (0.1, 0.01, 0.0), (0.1, 0.01, -1.0),
                             (np.inf, 0.01, 1.0), (0.1, np.nan, 1.0), (0.1, 0.01, np.inf)]:
        rc = nat.lib().optik_hip_diff_ik_avoid_batch(hc._h, None, q.data_ptr(), V.data_ptr(), 0, vm.data_ptr(), 0, 2,
                                                     infl, safe, gain, None, None, None, None)
        assert rc == -1, (infl, safe, gain, rc)  # OPTIK_HIP_EINVAL
        with pytest.raises(ValueError):
            robot.diff_ik_avoid(np.zeros(7), np.zeros(6), np.ones(7), infl, safe, gain)
    with pytest.raises(nat.OptikHipError, match="not supported"):
        _robot("arm9").hip_chain().diff_ik_avoid_batch(torch.zeros((9, 2), dtype=torch.float64, device="cuda:0"), V,
                                                       torch.ones(9, dtype=torch.float64, device="cuda:0"), 0.1, 0.01)


def test_servo_loop_never_goes_below_safety():
    """50 steps of dt = 0.01 s at |v_i| <= 1 rad/s into a wall.  The damper bounds the linearised approach; one step's
    linearisation error is at most 1/2 |d^2 dist / dq^2| |v dt|^2 <= 1/2 * 1.5 m * 7 * (0.01)^2 = 5.3e-4 m (the second
    derivative of a point's position on a revolute chain is bounded by its lever arm, < 1.5 m here, and the distance to
    a plane is linear in the position), and a step is only taken from a clearance >= safety minus the previous step's
    error, where the row forbids approaching: 1e-3 covers it."""
    robot, x = _wall_scene(0.12)
    V, vm = np.array([0.5, 0.0, 0.0, 0.0, 0.0, 0.0]), np.ones(7)
    influence, safety, dt = 0.1, 0.03, 0.01
    clr = []
    for _ in range(50):
        out = robot.diff_ik_avoid(x, V, vm, influence, safety)
        assert out is not None
        x = x + dt * np.array(out[1])
        clr.append(robot.collision_clearance_batch_arrays(x[None])[0][0])
    assert min(clr) >= safety - 1e-3, min(clr)
    assert clr[-1] < influence  # it did approach: the wall was 12 cm away


def test_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT)
    panda = [os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"]
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "diff_ik_avoid.py"), *panda, "150"], env=env,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    with_avoid = float(res.stdout.split("steps: ")[1].split(" m")[0])
    plain = float(res.stdout.split("), ")[1].split(" m")[0])
    assert with_avoid >= 0.02 - 1e-3 > plain, res.stdout  # (safety 0.02 m: held with the dampers, not without)
