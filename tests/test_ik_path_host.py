"""CPU checks of ik_path: the entry points are exported, and every argument error -- an empty, unlimited or too large
restart range, a NaN or negative max_step, shapes, a start configuration outside the joint limits, an invalid
transform -- is refused on the host before any device call (these run on a machine without a GPU)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import REF_GOLDEN


@pytest.fixture(scope="module")
def built():
    from optik_amd import build
    build.build()
    from optik_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def ur3e(built):
    from optik_amd import Robot
    return Robot.from_urdf_file(os.path.join(REF_GOLDEN, "ur3e.urdf"), "ur_base_link", "ur_ee_link")


def test_path_symbols_are_exported(built):
    for s in ("optik_hip_ik_path", "optik_robot_ik_path"):
        assert hasattr(built, s), f"{s} is not exported by liboptik_amd.so"


def _inputs(robot, P=3, L=4):
    lb, ub = (np.array(v) for v in robot.joint_limits())
    return np.tile(np.eye(4), (P, L, 1, 1)), np.tile((lb + ub) / 2, (P, 1))


def test_arguments_are_validated_before_any_device_call(ur3e):
    from optik_amd import SolverConfig
    tg, x0 = _inputs(ur3e)
    cfg = SolverConfig("speed", max_time=0.0, max_restarts=64)
    for unlimited in (SolverConfig("quality"), SolverConfig("speed", max_time=0.5, max_restarts=0)):
        with pytest.raises(ValueError, match="max_restarts"):
            ur3e.ik_paths_arrays(unlimited, tg, x0)
        with pytest.raises(ValueError, match="max_restarts"):
            ur3e.ik_path(unlimited, tg[0], x0[0])
    with pytest.raises(ValueError, match="max_restarts"):
        ur3e.ik_paths_arrays(SolverConfig("speed", max_time=0.0, max_restarts=4097), tg, x0)
    for ms in (-1.0, float("nan"), -1e-300, float("-inf")):
        with pytest.raises(ValueError, match="max_step"):
            ur3e.ik_paths_arrays(cfg, tg, x0, max_step=ms)
        with pytest.raises(ValueError, match="max_step"):
            ur3e.ik_path(cfg, tg[0], x0[0], max_step=ms)
    for bad_tg in (tg[0], tg[:, :, :3], tg[:, :0], tg[:0]):
        with pytest.raises(ValueError, match="targets"):
            ur3e.ik_paths_arrays(cfg, bad_tg, x0)
    with pytest.raises(ValueError, match="targets"):
        ur3e.ik_path(cfg, tg[0, 0], x0[0])
    with pytest.raises(ValueError, match="x0s"):
        ur3e.ik_paths_arrays(cfg, tg, x0[:2])
    with pytest.raises(ValueError, match="x0s"):
        ur3e.ik_paths_arrays(cfg, tg, x0[:, :5])
    with pytest.raises(ValueError):
        ur3e.ik_path(cfg, tg[0], x0[0][:5])
    bad = tg.copy()
    bad[1, 2, 3, 0] = 1e-9
    with pytest.raises(ValueError, match="invalid target transform"):
        ur3e.ik_paths_arrays(cfg, bad, x0)
    with pytest.raises(ValueError, match="invalid target transform"):
        ur3e.ik_path(cfg, bad[1], x0[1])
    _, ub = ur3e.joint_limits()
    out = x0.copy()
    out[2, 1] = ub[1] + 0.5
    with pytest.raises(ValueError, match="joint limits"):
        ur3e.ik_paths_arrays(cfg, tg, out)
    with pytest.raises(ValueError, match="joint limits"):
        ur3e.ik_path(cfg, tg[2], out[2])


def test_c_abi_refuses_before_any_device_call(built, ur3e):
    """optik_robot_ik_path itself: -1 with a message for max_restarts and max_step; -2 for a start configuration
    outside the limits; -3 for an invalid transform (with OPTIK_BATCH_VALIDATE_POSES)."""
    from optik_amd import _native as nat
    from optik_amd import robot as rb
    L = built
    P, W = 3, 4
    tg, x0 = _inputs(ur3e, P, W)
    tg16 = np.ascontiguousarray(tg.reshape(P * W, 16))
    x0 = np.ascontiguousarray(x0)
    dp = C.POINTER(C.c_double)

    def call(max_step=float("inf"), restarts=64, x=x0, t=tg16, flags=rb.BATCH_ROW_MAJOR | rb.BATCH_VALIDATE_POSES,
             p=P, w=W):
        cfg = nat.make_config("speed", 0.0, restarts)
        return L.optik_robot_ik_path(ur3e._h, C.byref(cfg), p, w, t.ctypes.data_as(dp), flags, x.ctypes.data_as(dp),
                                     None, max_step, None, None, None, None, None)

    def err():
        return L.optik_robot_last_error().decode()

    for kw, words in (({"restarts": 0}, "max_restarts"), ({"restarts": 4097}, "max_restarts"),
                      ({"max_step": -0.5}, "max_step"), ({"max_step": float("nan")}, "max_step"),
                      ({"p": 0}, "bad argument"), ({"w": 0}, "bad argument")):
        assert call(**kw) == -1, kw
        assert words in err(), (kw, err())
    x_bad = x0.copy()
    x_bad[1, 0] = 1e3
    assert call(x=x_bad) == -2 and "joint limits" in err()
    t_bad = tg16.copy()
    t_bad[P * W - 1, 0] = 2.0  # the last waypoint of the last path
    assert call(t=t_bad) == -3 and "invalid target transform" in err()
