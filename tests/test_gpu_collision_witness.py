"""-m gpu: the clearance witnesses and gradients on the device (HipChain.collision_witness_batch /
optik_hip_collision_witness_batch, Robot.collision_witness_batch_arrays) against optik_amd/csrc/collision_gradient.hpp
built with g++ and applied to link_frames_batch's frames: bit for bit."""
import numpy as np
import pytest

from avoid_util import Scene, build_avoid, make_test_world
from conftest import ROBOT_SPECS
from gpu_util import assert_bit_equal

pytestmark = pytest.mark.gpu

NAMES = ["panda", "ur10", "arm8"]
B = 300  # more than one block of 256, and a partial wave


@pytest.fixture(scope="module")
def avoid(tmp_path_factory):
    return build_avoid(str(tmp_path_factory.mktemp("avoid_gpu_witness")))


def _setup(name, world=True):
    from optik_amd import Robot
    from optik_amd.collision import auto_pairs, spheres_along_chain
    robot = Robot.from_urdf_file(*ROBOT_SPECS[name])
    n = robot.num_positions()
    frames, centers, radii = spheres_along_chain(robot, 0.05, 2)
    spheres, boxes, grid = make_test_world()
    # (Robot.hip_chain() is a chain of its own: the device form gets the same model and world)
    for obj in (robot, robot.hip_chain()):
        obj.set_collision_model(frames, centers, radii, self_pairs="auto", margin=0.0)
        if world:
            obj.set_world(spheres=spheres, boxes=boxes)
            obj.set_world_grid(*grid)
    axes = robot.chain_tables()["axes"][:n]
    scene = Scene(axes, frames, centers, radii, auto_pairs(frames), spheres if world else None,
                  boxes if world else None, grid if world else None)
    rng = np.random.default_rng(40 + NAMES.index(name))
    lb, ub = (np.array(v) for v in robot.joint_limits())
    x = rng.uniform(np.maximum(lb, -2.8), np.minimum(ub, 2.8), size=(B, n))
    x[17, n // 2] = np.nan  # every frame after that joint is NaN
    return robot, scene, x


def _device_rows(robot, x):
    import torch
    hc = robot.hip_chain()
    q = torch.tensor(x.T.copy(), device="cuda:0")
    dist, grad, wit = hc.collision_witness_batch(q)
    frames = hc.link_frames_batch(q)
    clr = hc.collision_batch(q)[0]
    torch.cuda.synchronize()
    n = x.shape[1]
    return (dist.cpu().numpy().T, grad.cpu().numpy().transpose(2, 0, 1), wit.cpu().numpy().transpose(2, 0, 1),
            frames.cpu().numpy().reshape(len(x), n + 2, 7), clr.cpu().numpy())


@pytest.mark.parametrize("world", [True, False], ids=["world", "model_only"])
@pytest.mark.parametrize("name", NAMES)
def test_rows_equal_the_host_header_bit_for_bit(avoid, name, world):
    robot, scene, x = _setup(name, world)
    dist, grad, wit, frames, clr = _device_rows(robot, x)
    rd, rw, rg = avoid.witness(scene, frames)
    assert_bit_equal(dist, rd, f"{name} dist")
    assert np.array_equal(wit, rw), (name, np.argwhere(wit != rw)[:5])
    assert_bit_equal(grad, rg, f"{name} grad")
    assert_bit_equal(dist.min(axis=1), clr, f"{name} min over rows vs collision_batch")
    assert np.isnan(dist[17]).all() and np.isnan(grad[17]).all() and (wit[17] == -1).all()
    ok = np.arange(B) != 17
    assert np.isfinite(dist[ok]).any() and (wit[ok][:, :, 1].max() == 3)
    if world:
        assert set(np.unique(wit[ok][:, :, 1])) >= {0, 1, 2, 3}
    # the host form: the same rows, row-major
    hd, hg, hw = robot.collision_witness_batch_arrays(x)
    assert_bit_equal(hd, dist, f"{name} host form dist")
    assert_bit_equal(hg, grad, f"{name} host form grad")
    assert np.array_equal(hw, wit)


def test_without_a_model_every_row_is_empty():
    from optik_amd import Robot
    robot = Robot.from_urdf_file(*ROBOT_SPECS["panda"])
    x = np.zeros((5, 7))
    dist, grad, wit = robot.collision_witness_batch_arrays(x)
    assert np.isposinf(dist).all() and (grad == 0.0).all() and (wit == -1).all()


def test_nine_joints_are_unsupported():
    import torch
    from optik_amd import Robot
    from optik_amd import _native as nat
    robot = Robot.from_urdf_file(*ROBOT_SPECS["arm9"])
    with pytest.raises(nat.OptikHipError) as e:
        robot.hip_chain().collision_witness_batch(torch.zeros((9, 4), dtype=torch.float64, device="cuda:0"))
    assert "not supported" in str(e.value)
    with pytest.raises(RuntimeError, match="not supported"):
        robot.collision_witness_batch_arrays(np.zeros((2, 9)))
