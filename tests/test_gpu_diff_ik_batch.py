"""-m gpu: batched diff_ik (Robot.diff_ik_batch_arrays / optik_robot_diff_ik_batch, HipChain.diff_ik_batch /
optik_hip_diff_ik_batch).  Row b of a batch is what Robot.diff_ik(x0[b], V[b], v_max[b], ee_offset) returns, bit
for bit: the same FK / Jacobian device code and the same LP source (optik_amd/csrc/diff_ik_lp.hpp) on the device."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROBOT_SPECS, ROBOTS, ROOT
from gpu_util import assert_bit_equal

pytestmark = pytest.mark.gpu

NAMES = ["ur3e", "panda", "arm8", "panda1", "panda2", "panda3", "panda4", "panda5", "panda_hand"]


def _robot(name):
    from optik_amd import Robot
    return Robot.from_urdf_file(*ROBOT_SPECS[name])


def _ee_offset():
    c, s = np.cos(0.3), np.sin(0.3)
    off = np.array([[c, -s, 0.0, 0.05], [s, c, 0.0, -0.02], [0.0, 0.0, 1.0, 0.1], [0.0, 0.0, 0.0, 1.0]])
    return off


def _rows(robot, rng, B):
    """Random configurations within limits with singular ones mixed in (q = 0: aligned axes on the Panda), twists
    from zero through tiny (alpha = 1) to large (alpha < 1), limits with zero, negative and NaN entries."""
    n = robot.num_positions()
    lb, ub = (np.array(v) for v in robot.joint_limits())
    x = rng.uniform(lb, ub, size=(B, n))
    x[::20] = 0.0
    x[7::40, : min(n, 3)] = 0.0
    scale = rng.choice([0.0, 1e-3, 0.05, 1.0, 10.0], p=[0.1, 0.2, 0.2, 0.4, 0.1], size=B)
    V = rng.normal(size=(B, 6)) * scale[:, None]
    vm = rng.uniform(0.2, 2.0, size=(B, n))
    vm[3::10, rng.integers(n)] = 0.0
    vm[5::50, rng.integers(n)] = -0.5
    vm[11::100, rng.integers(n)] = np.nan
    return x, V, vm


def _single(robot, x, V, vm, ee=None):
    B, n = x.shape
    alpha, v, found = np.zeros(B), np.zeros((B, n)), np.zeros(B, dtype=bool)
    for b in range(B):
        out = robot.diff_ik(x[b], V[b], vm[b], ee)
        if out is not None:
            found[b] = True
            alpha[b], v[b] = out[0], out[1]
    return alpha, v, found


@pytest.mark.parametrize("name", NAMES)
def test_batch_rows_equal_single_calls_bit_for_bit(name):
    robot = _robot(name)
    rng = np.random.default_rng(1000 + NAMES.index(name))
    x, V, vm = _rows(robot, rng, 2000)
    for ee in (None, _ee_offset().tolist()):
        alpha, v, found = robot.diff_ik_batch_arrays(x, V, vm, ee)
        ra, rv, rf = _single(robot, x, V, vm, ee)
        assert np.array_equal(found, rf), (name, np.flatnonzero(found != rf)[:10])
        assert 0 < found.sum() < len(found)
        assert_bit_equal(alpha, ra, f"{name} alpha (ee_offset {ee is not None})")
        assert_bit_equal(v, rv, f"{name} v (ee_offset {ee is not None})")
        assert np.all(alpha[~found] == 0.0) and np.all(v[~found] == 0.0)
        # the list form: what B calls of diff_ik return
        lst = robot.diff_ik_batch(x[:50], V[:50], vm[:50], ee)
        for b in range(50):
            assert lst[b] == robot.diff_ik(x[b], V[b], vm[b], ee)


def test_broadcast_forms_equal_repeated_rows():
    import torch
    robot = _robot("panda")
    n = robot.num_positions()
    rng = np.random.default_rng(3)
    lb, ub = (np.array(v) for v in robot.joint_limits())
    B = 777
    x = rng.uniform(lb, ub, size=(B, n))
    V1 = rng.normal(size=6) * 0.3
    vm1 = rng.uniform(0.2, 2.0, size=n)
    Vr, vmr = np.tile(V1, (B, 1)), np.tile(vm1, (B, 1))
    # host form
    a0, v0, f0 = robot.diff_ik_batch_arrays(x, Vr, vmr)
    for Vx, vmx in ((V1, vm1), (Vr, vm1), (V1, vmr)):
        a1, v1, f1 = robot.diff_ik_batch_arrays(x, Vx, vmx)
        assert np.array_equal(f0, f1)
        assert_bit_equal(a1, a0, "host broadcast alpha")
        assert_bit_equal(v1, v0, "host broadcast v")
    # device form: ld = 0 reads the one vector for every row
    hc = robot.hip_chain()
    q_d = torch.tensor(x.T.copy(), device="cuda:0")
    ref = hc.diff_ik_batch(q_d, torch.tensor(Vr.T.copy(), device="cuda:0"), torch.tensor(vmr.T.copy(), device="cuda:0"))
    got = hc.diff_ik_batch(q_d, torch.tensor(V1, device="cuda:0"), torch.tensor(vm1, device="cuda:0"))
    torch.cuda.synchronize()
    for g, r, what in zip(got, ref, ("alpha", "v", "status")):
        assert np.array_equal(g.cpu().numpy(), r.cpu().numpy()), f"device broadcast {what}"
    assert_bit_equal(ref[0].cpu().numpy(), a0, "device alpha vs host form")
    assert_bit_equal(ref[1].cpu().numpy().T, v0, "device v vs host form")


@pytest.mark.parametrize("B", [0, 1, 1000])
def test_device_form_on_a_side_stream(B):
    import torch
    robot = _robot("panda")
    hc = robot.hip_chain()
    rng = np.random.default_rng(B)
    x, V, vm = _rows(robot, rng, max(B, 1))
    x, V, vm = x[:B], V[:B], vm[:B]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        q_d = torch.tensor(x.T.copy(), device="cuda:0").reshape(robot.num_positions(), B)
        V_d = torch.tensor(V.T.copy(), device="cuda:0").reshape(6, B)
        vm_d = torch.tensor(vm.T.copy(), device="cuda:0").reshape(robot.num_positions(), B)
        alpha, v, status = hc.diff_ik_batch(q_d, V_d, vm_d)
    s.synchronize()
    assert alpha.shape == (B,) and v.shape == (robot.num_positions(), B) and status.shape == (B,)
    if B == 0:
        return
    a0, v0, f0 = robot.diff_ik_batch_arrays(x, V, vm)
    assert np.array_equal(status.cpu().numpy() == 0, f0)
    assert_bit_equal(alpha.cpu().numpy(), a0, "alpha")
    assert_bit_equal(v.cpu().numpy().T, v0, "v")


def test_device_form_past_two_to_the_twenty():
    import torch
    robot = _robot("panda")
    hc = robot.hip_chain()
    n = robot.num_positions()
    B = (1 << 20) + 3
    g = torch.Generator(device="cuda:0").manual_seed(5)
    lb = torch.tensor(robot.joint_limits()[0], device="cuda:0")[:, None]
    ub = torch.tensor(robot.joint_limits()[1], device="cuda:0")[:, None]
    q = (lb + (ub - lb) * torch.rand((n, B), generator=g, device="cuda:0", dtype=torch.float64)).contiguous()
    V = torch.randn((6, B), generator=g, device="cuda:0", dtype=torch.float64)
    vm = 0.2 + 1.8 * torch.rand((n, B), generator=g, device="cuda:0", dtype=torch.float64)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        alpha, v, status = hc.diff_ik_batch(q, V, vm)
    s.synchronize()
    rows = np.unique(np.concatenate([np.random.default_rng(6).integers(0, B, size=2000), np.arange(B - 300, B)]))
    idx = torch.tensor(rows, device="cuda:0")
    x = q[:, idx].T.cpu().numpy()
    a0, v0, f0 = robot.diff_ik_batch_arrays(x, V[:, idx].T.cpu().numpy(), vm[:, idx].T.cpu().numpy())
    assert np.array_equal(status[idx].cpu().numpy() == 0, f0)
    assert_bit_equal(alpha[idx].cpu().numpy(), a0, "alpha")
    assert_bit_equal(v[:, idx].T.cpu().numpy(), v0, "v")


@pytest.mark.parametrize("name", ["arm9", "gantry"])
def test_refusals_are_the_single_calls(name):
    from optik_amd import _native as nat
    robot = _robot(name)
    n = robot.num_positions()
    with pytest.raises(RuntimeError) as single:
        robot.diff_ik([0.0] * n, [0.1, 0, 0, 0, 0, 0], [1.0] * n)
    with pytest.raises(RuntimeError) as batch:
        robot.diff_ik_batch_arrays(np.zeros((4, n)), [0.1, 0, 0, 0, 0, 0], np.ones(n))
    assert str(batch.value) == str(single.value)
    import torch
    hc = robot.hip_chain()
    with pytest.raises(nat.OptikHipError):
        hc.diff_ik_batch(torch.zeros((n, 4), dtype=torch.float64, device="cuda:0"),
                         torch.zeros(6, dtype=torch.float64, device="cuda:0"),
                         torch.ones(n, dtype=torch.float64, device="cuda:0"))


def test_invalid_ee_offset_is_refused():
    robot = _robot("ur3e")
    bad = _ee_offset() * 2.0
    with pytest.raises(ValueError, match="invalid target transform specified"):
        robot.diff_ik([0.0] * 6, [0.1, 0, 0, 0, 0, 0], [1.0] * 6, bad.tolist())
    with pytest.raises(ValueError, match="invalid target transform specified"):
        robot.diff_ik_batch_arrays(np.zeros((3, 6)), [0.1, 0, 0, 0, 0, 0], np.ones(6), bad.tolist())


def test_batched_rate_is_far_above_single_calls():
    """Panda at B = 2^16 through the host form (host arrays in and out, like the single call): at least 100x the
    configurations/s of a loop of single diff_ik calls."""
    robot = _robot("panda")
    rng = np.random.default_rng(9)
    x, V, vm = _rows(robot, rng, 1 << 16)
    robot.diff_ik_batch_arrays(x, V, vm)  # warm-up: workspace, code objects
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        robot.diff_ik_batch_arrays(x, V, vm)
        ts.append(time.perf_counter() - t0)
    batch_rate = len(x) / min(ts)
    for b in range(20):
        robot.diff_ik(x[b], V[b], vm[b])
    t0 = time.perf_counter()
    for b in range(300):
        robot.diff_ik(x[b], V[b], vm[b])
    single_rate = 300 / (time.perf_counter() - t0)
    assert batch_rate >= 100 * single_rate, (batch_rate, single_rate)


def test_many_diff_ik_example():
    env = dict(os.environ, PYTHONPATH=ROOT)
    panda = [os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"]
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "many_diff_ik.py"), *panda, "4096", "3"],
                         env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    assert res.stdout.startswith("4096 of 4096 configurations solved"), res.stdout
    assert "configurations/s" in res.stdout
