"""-m gpu: path timing and trajectory sampling on the device against the host.  HipChain.path_time and
trajectory_sample against the serial reference of csrc/time_measure.hpp (g++), every output bit for bit, over the
shapes at which the kernel takes another path: n = 1 (4 pairs, fewer than a wave), 7 and 16 (289 pairs, more than one
per lane), L = 3 (the shortest), 4 and 64 (a full wave), P = 1 and 65, mixed lengths and statuses in one launch; a
path's independence of the batch; Robot.time_paths / sample_trajectories through the C ABI rows; the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import time_util as tu
from conftest import ROBOT_SPECS

pytestmark = pytest.mark.gpu

CHAINS = {1: "panda1", 7: "panda", 16: "arm16"}
DT, T = 0.05, 40


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def robots():
    from optik_amd import Robot
    made = {}

    def get(name):
        if name not in made:
            made[name] = Robot.from_urdf_file(*ROBOT_SPECS[name])
        return made[name]
    return get


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return tu.build_time_ref(str(tmp_path_factory.mktemp("time_measure")))


def _t(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all((tu.bits(got) == tu.bits(want)) | (np.isnan(got) & np.isnan(want))))


def _limits(n):
    v = np.linspace(1.5, 2.5, n)
    if n > 2:
        v[2] = math.inf
    return v, np.linspace(4.0, 9.0, n)


def _inputs(n, L, P):
    """P paths [P, L, n]: gentle ones, unbiased walks, and one each of: len 3, an invalid len 2, a NaN, a repeated
    start, three equal waypoints (where L has room)."""
    rng = np.random.default_rng(1000 * n + 10 * L + P)
    paths = tu.random_walks(rng, P, L, n)
    paths[::2] = tu.gentle_paths(rng, len(paths[::2]), L, n)
    lens = np.full(P, L, dtype=np.int32)
    if P > 8:
        lens[1], lens[3] = 3, 2
        paths[5, L // 2, n - 1] = math.nan
        paths[6, 1] = paths[6, 0]
        lens[7] = max(3, L - 1)
        if L >= 8:
            paths[8, 3:6] = paths[8, 3]
        paths[9, 0, 0] = math.inf
    return paths, lens


def _device(torch, hc, paths, lens, vmax, amax):
    path_d = _t(torch, tu.to_device_layout(paths))
    lens_d = None if lens is None else _t(torch, np.asarray(lens, dtype=np.int32))
    res = hc.path_time(path_d, lens_d, _t(torch, vmax), _t(torch, amax))
    q, v = hc.trajectory_sample(path_d, res, DT, T, lens_d)
    torch.cuda.synchronize()
    sw = lambda a: np.ascontiguousarray(np.swapaxes(a.cpu().numpy(), 0, 1))  # noqa: E731
    return dict(times=sw(res["t"]), velocities=sw(res["qd"]), accelerations=sw(res["qdd"]), x=sw(res["x"]),
                duration=res["duration"].cpu().numpy(), status=res["status"].cpu().numpy(), q=sw(q), v=sw(v))


def _agree(got, want, what):
    for key in ("status", "duration", "times", "x", "velocities", "accelerations", "q", "v"):
        assert _same(got[key], want[key]), (what, key)


@pytest.fixture(scope="module")
def cases(ref):
    """The serial reference of every shape, computed once."""
    out = {}
    for n in CHAINS:
        vmax, amax = _limits(n)
        for L in (3, 4, 64):
            paths, lens = _inputs(n, L, 65)
            want = ref.time(paths, lens, vmax, amax)
            want["q"], want["v"] = ref.sample(paths, lens, want, DT, T)
            out[n, L] = (paths, lens, want)
    return out


@pytest.mark.parametrize("L", [3, 4, 64])
@pytest.mark.parametrize("n", [1, 7, 16])
def test_device_matches_the_reference(torch_dev, robots, cases, n, L):
    hc = robots(CHAINS[n]).hip_chain()
    assert hc.n == n
    vmax, amax = _limits(n)
    paths, lens, want = cases[n, L]
    got = _device(torch_dev, hc, paths, lens, vmax, amax)
    _agree(got, want, (n, L))
    st = want["status"]
    assert st[3] == tu.BAD_LENGTH and st[5] == tu.PATH_NAN and st[6] == tu.BAD_LENGTH and st[9] == tu.PATH_NAN
    assert st[1] in (tu.TIMED, tu.STALLED) and np.sum(st == tu.TIMED) >= 20, st
    # one path alone: the same bits as inside the launch of 65
    for p in (0, 1, 3, 5, 6, 64):
        one = _device(torch_dev, hc, paths[p:p + 1], lens[p:p + 1], vmax, amax)
        _agree(one, {k: v[p:p + 1] for k, v in want.items()}, (n, L, p))
    if L == 64:  # lens None: L each
        full = np.flatnonzero(lens == L)[:5]
        got = _device(torch_dev, hc, paths[full], None, vmax, amax)
        _agree(got, {k: v[full] for k, v in want.items()}, (n, L, "no lens"))


@pytest.mark.parametrize("n", [1, 7, 16])
def test_rows_match_the_device(torch_dev, robots, cases, n):
    robot = robots(CHAINS[n])
    vmax, amax = _limits(n)
    paths, lens, want = cases[n, 64]
    out = robot.time_paths(paths, lens, a_max=amax, v_max=vmax)
    for key in ("status", "duration", "times", "velocities", "accelerations"):
        assert _same(out[key], want[key]), key
    half = robot.time_paths(paths, lens, a_max=2.0 * amax, v_max=2.0 * vmax, scale=0.5)
    assert _same(half["times"], want["times"])
    ok = want["status"] == tu.TIMED
    dt = float(np.max(want["duration"][ok])) / 29.5
    q, v = robot.sample_trajectories(paths, out, dt, lens)
    Tn = q.shape[1]
    assert Tn == int(np.ceil(want["duration"][ok] / dt).max()) + 1
    import torch
    hc = robot.hip_chain()
    path_d, lens_d = _t(torch, tu.to_device_layout(paths)), _t(torch, lens)
    res = hc.path_time(path_d, lens_d, _t(torch, vmax), _t(torch, amax))
    qd_, vd_ = hc.trajectory_sample(path_d, res, dt, Tn, lens_d)
    assert _same(q, np.swapaxes(qd_.cpu().numpy(), 0, 1)) and _same(v, np.swapaxes(vd_.cpu().numpy(), 0, 1))
    assert _same(q[ok, -1], np.stack([paths[p, lens[p] - 1] for p in np.flatnonzero(ok)]))
    assert _same(q[~ok], np.broadcast_to(paths[~ok, :1], q[~ok].shape))
    if n == 7:
        v_urdf = robot.velocity_limits()
        assert _same(robot.time_paths(paths, lens, a_max=5.0)["times"],
                     robot.time_paths(paths, lens, a_max=5.0, v_max=v_urdf)["times"])
        q2, v2, free = robot.sample_trajectories(paths[:4], {k: a[:4] for k, a in out.items()}, dt, lens[:4],
                                                 resolution=0.05)
        assert _same(q2, q[:4, :q2.shape[1]]) and free.shape == (4,) and free.dtype == bool and free.all()


def test_refusals(torch_dev, robots):
    from optik_amd import _native as nat
    robot = robots("panda")
    paths = tu.gentle_paths(np.random.default_rng(0), 2, 8, 7)
    for kw in (dict(a_max=0.0), dict(a_max=math.inf), dict(a_max=math.nan), dict(a_max=5.0, v_max=0.0),
               dict(a_max=5.0, v_max=math.nan), dict(a_max=5.0, v_max=[1.0, 2.0]), dict(a_max=5.0, scale=0.0), dict()):
        with pytest.raises(ValueError):
            robot.time_paths(paths, **kw)
    for bad in (np.zeros((2, 2, 7)), np.zeros((2, 65, 7)), np.zeros((2, 8, 6))):
        with pytest.raises(ValueError):
            robot.time_paths(bad, a_max=5.0)
    timing = robot.time_paths(paths, a_max=5.0)
    assert list(timing["status"]) == [0, 0]
    for dt in (0.0, -1.0, math.nan, float(timing["duration"].max()) / 70000.0):
        with pytest.raises(ValueError):
            robot.sample_trajectories(paths, timing, dt)
    with pytest.raises(ValueError):
        robot.sample_trajectories(paths[:1], timing, 0.01)
    # the kernel layer itself: OPTIK_HIP_EINVAL (-1) before any device work
    lib, hc = nat.lib(), robot.hip_chain()
    null = C.c_void_p(None)

    def time(L=8, P=4, chain=hc):
        return lib.optik_hip_path_time(chain._h, null, null, L, P, null, null, null, null, null, null, null, null, null)

    def sample(L=8, P=0, dt=0.01, Tout=10, chain=hc):
        return lib.optik_hip_trajectory_sample(chain._h, null, null, L, P, null, null, null, dt, Tout, null, null, null)
    for kw in (dict(L=2), dict(L=65), dict(P=-1), dict(P=(1 << 30) + 1)):
        assert time(**kw) == -1, kw
        assert sample(**kw) == -1, kw
    for kw in (dict(dt=0.0), dict(dt=-0.01), dict(dt=math.nan), dict(dt=math.inf), dict(Tout=0), dict(Tout=65537)):
        assert sample(**kw) == -1, kw
    assert time() == 0 and time(P=0) == 0 and sample() == 0, "nothing to write: a no-op"
    assert sample(Tout=65536) == 0
    gantry = robots("gantry").hip_chain()
    EUNSUPPORTED = -2
    assert time(chain=gantry) == EUNSUPPORTED and time(P=0, chain=gantry) == EUNSUPPORTED
    assert sample(chain=gantry) == EUNSUPPORTED
    with pytest.raises(RuntimeError):
        robots("gantry").time_paths(np.zeros((1, 8, robots("gantry").num_positions())), a_max=1.0)
