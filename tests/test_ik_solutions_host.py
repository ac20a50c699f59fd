"""CPU checks of ik_solutions: the entry points are exported, and every argument error -- k, min_dist, an unlimited
or too large max_restarts, shapes, a seed outside the joint limits -- is refused on the host before any device call
(these run on a machine without a GPU)."""
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


def test_solutions_symbols_are_exported(built):
    for s in ("optik_hip_ik_solutions", "optik_robot_ik_solutions"):
        assert hasattr(built, s), f"{s} is not exported by liboptik_amd.so"


def _inputs(robot, T=3):
    lb, ub = (np.array(v) for v in robot.joint_limits())
    return np.tile(np.eye(4), (T, 1, 1)), np.tile((lb + ub) / 2, (T, 1))


def test_arguments_are_validated_before_any_device_call(ur3e):
    from optik_amd import SolverConfig
    tg, x0 = _inputs(ur3e)
    cfg = SolverConfig("quality", max_time=0.0, max_restarts=256)
    for k in (0, 257, -1, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            ur3e.ik_solutions_batch_arrays(cfg, tg, x0, k=k)
        with pytest.raises(ValueError, match="k must be"):
            ur3e.ik_solutions(cfg, tg[0], x0[0], k=k)
    for md in (-1.0, float("nan"), float("inf"), -1e-300):
        with pytest.raises(ValueError, match="min_dist"):
            ur3e.ik_solutions_batch_arrays(cfg, tg, x0, min_dist=md)
    for unlimited in (SolverConfig("quality"), SolverConfig("speed", max_time=0.5, max_restarts=0)):
        with pytest.raises(ValueError, match="max_restarts"):
            ur3e.ik_solutions_batch_arrays(unlimited, tg, x0)
    with pytest.raises(ValueError, match="max_restarts"):
        ur3e.ik_solutions(SolverConfig("quality", max_time=0.0, max_restarts=(1 << 22) + 1), tg[0], x0[0])
    with pytest.raises(ValueError, match="targets"):
        ur3e.ik_solutions_batch_arrays(cfg, tg[:, :3], x0)
    with pytest.raises(ValueError, match="x0s"):
        ur3e.ik_solutions_batch_arrays(cfg, tg, x0[:2])
    with pytest.raises(ValueError, match="x0s"):
        ur3e.ik_solutions_batch_arrays(cfg, tg, x0[:, :5])
    with pytest.raises(ValueError):
        ur3e.ik_solutions(cfg, tg[0], x0[0][:5])
    bad = tg.copy()
    bad[1, 3, 0] = 1e-9
    with pytest.raises(ValueError, match="invalid target transform"):
        ur3e.ik_solutions_batch_arrays(cfg, bad, x0)
    _, ub = ur3e.joint_limits()
    out = x0.copy()
    out[2, 1] = ub[1] + 0.5
    with pytest.raises(RuntimeError, match="joint limits"):
        ur3e.ik_solutions_batch_arrays(cfg, tg, out)


def test_c_abi_refuses_before_any_device_call(built, ur3e):
    """optik_robot_ik_solutions itself: -1 with a message for k, min_dist and max_restarts; -2 for a seed outside the
    limits; -3 for an invalid transform (with OPTIK_BATCH_VALIDATE_POSES)."""
    from optik_amd import _native as nat
    from optik_amd import robot as rb
    L = built
    tg, x0 = _inputs(ur3e)
    tg16 = np.ascontiguousarray(tg.reshape(3, 16))
    x0 = np.ascontiguousarray(x0)
    dp = C.POINTER(C.c_double)

    def call(K=4, min_dist=0.1, restarts=256, x=x0, t=tg16, flags=rb.BATCH_ROW_MAJOR | rb.BATCH_VALIDATE_POSES):
        cfg = nat.make_config("quality", 0.0, restarts)
        return L.optik_robot_ik_solutions(ur3e._h, C.byref(cfg), 3, t.ctypes.data_as(dp), flags, x.ctypes.data_as(dp),
                                          None, K, min_dist, None, None, None, None)

    def err():
        return L.optik_robot_last_error().decode()

    for kw, words in (({"K": 0}, "K must be"), ({"K": 257}, "K must be"), ({"min_dist": -0.5}, "min_dist"),
                      ({"min_dist": float("nan")}, "min_dist"), ({"restarts": 0}, "max_restarts"),
                      ({"restarts": (1 << 22) + 1}, "max_restarts")):
        assert call(**kw) == -1, kw
        assert words in err(), (kw, err())
    x_bad = x0.copy()
    x_bad[0, 0] = 1e3
    assert call(x=x_bad) == -2 and "joint limits" in err()
    t_bad = tg16.copy()
    t_bad[1, 0] = 2.0
    assert call(t=t_bad) == -3 and "invalid target transform" in err()
