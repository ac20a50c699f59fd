"""-m gpu: path timing with tool limits on the device against the host.  HipChain.path_time_tool against the serial
reference of csrc/time_tool_measure.hpp, every output bit for bit, over the shapes at which the kernel takes another
path: n = 1 (9 pairs, fewer than a wave), 7 and 16 (324 pairs, six a lane, and the seventeenth member of the forward
pass), L = 3 (the shortest), 4 and 64 (a full wave), P = 1 and 65, mixed lengths and statuses in one launch, with and
without an ee_offset, each limit alone and all together; the identity with optik_hip_path_time; a path's independence of
the batch; NULL outputs, P = 0 and the refusals; Robot.time_paths_tool through the C ABI rows."""
import ctypes as C
import math

import numpy as np
import pytest

import time_tool_util as ttu
import time_util as tu
from conftest import ROBOT_SPECS
from gpu_util import _out, _sentinels_left

pytestmark = pytest.mark.gpu

CHAINS = {1: "panda1", 7: "panda", 16: "arm16"}
TOOL = ttu.limits4(0.5, 1.5, 1.0, 2.0)
EE7 = np.array([0.05, -0.02, 0.1, 0.0, math.sin(0.3), 0.0, math.cos(0.3)])
KEYS = ("status", "duration", "times", "x", "velocities", "accelerations", "tool_speed", "tool_accel", "tool_wspeed")
# (limits, ee_offset): all together with and without the offset, each limit alone
CASES = [(TOOL, None), (TOOL, EE7), (ttu.limits4(tool_v_max=0.25), EE7), (ttu.limits4(tool_a_tangential=0.8), None),
         (ttu.limits4(tool_a_normal=0.5), EE7), (ttu.limits4(tool_w_max=1.0), None)]


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
    return ttu.build_time_tool_ref(str(tmp_path_factory.mktemp("time_tool_measure")))


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
    start, three equal waypoints (where L has room), an infinity."""
    rng = np.random.default_rng(2000 * n + 10 * L + P)
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


def _sw(a):
    return np.ascontiguousarray(np.swapaxes(a.cpu().numpy(), 0, 1))


def _host_layout(res):
    return dict(times=_sw(res["t"]), velocities=_sw(res["qd"]), accelerations=_sw(res["qdd"]), x=_sw(res["x"]),
                duration=res["duration"].cpu().numpy(), status=res["status"].cpu().numpy(),
                tool_speed=_sw(res["tool_speed"]), tool_accel=_sw(res["tool_accel"]), tool_wspeed=_sw(res["tool_wspeed"]))


def _device(torch, hc, paths, lens, vmax, amax, lim, ee7):
    path_d = _t(torch, tu.to_device_layout(paths))
    lens_d = None if lens is None else _t(torch, np.asarray(lens, dtype=np.int32))
    res = hc.path_time_tool(path_d, lens_d, _t(torch, vmax), _t(torch, amax), *lim, ee_offset7=ee7)
    torch.cuda.synchronize()
    return _host_layout(res)


def _agree(got, want, what):
    for key in KEYS:
        assert _same(got[key], want[key]), (what, key)


@pytest.mark.parametrize("L", [3, 4, 64])
@pytest.mark.parametrize("n", [1, 7, 16])
def test_device_matches_the_reference(torch_dev, robots, ref, n, L):
    robot = robots(CHAINS[n])
    hc, chain = robot.hip_chain(), robot.chain_tables()
    assert hc.n == n
    vmax, amax = _limits(n)
    paths, lens = _inputs(n, L, 65)
    for k, (lim, ee7) in enumerate(CASES):
        want = ref.time(chain, paths, lens, vmax, amax, lim, ee7)
        got = _device(torch_dev, hc, paths, lens, vmax, amax, lim, ee7)
        _agree(got, want, (n, L, k))
        st = want["status"]
        assert st[3] == tu.BAD_LENGTH and st[5] == tu.PATH_NAN and st[6] == tu.BAD_LENGTH and st[9] == tu.PATH_NAN
        assert st[1] in (tu.TIMED, tu.STALLED) and np.sum(st == tu.TIMED) >= 20, st
        if k > 1:
            continue
        # one path alone: the same bits as inside the launch of 65
        for p in (0, 1, 3, 5, 6, 64):
            one = _device(torch_dev, hc, paths[p:p + 1], lens[p:p + 1], vmax, amax, lim, ee7)
            _agree(one, {key: v[p:p + 1] for key, v in want.items()}, (n, L, k, p))
        if L == 64:  # lens None: L each
            full = np.flatnonzero(lens == L)[:5]
            got = _device(torch_dev, hc, paths[full], None, vmax, amax, lim, ee7)
            _agree(got, {key: v[full] for key, v in want.items()}, (n, L, k, "no lens"))
        # the tool's rows bind somewhere in the launch: the limits are not idle.  (n = 1: the joint's own velocity
        # limit is the angular speed's, and without the offset the tool sits on the joint's axis and only turns)
        ok = st == tu.TIMED
        if n > 1 and L == 64:
            assert want["tool_wspeed"][ok].max() >= TOOL[3] * (1 - 1e-9)
            assert want["tool_speed"][ok].max() >= TOOL[0] * (1 - 1e-9)
        elif n == 1 and ee7 is None:
            assert np.all(want["tool_speed"] == 0.0) and want["tool_wspeed"][ok].max() > 0.0


@pytest.mark.parametrize("n", [1, 7, 16])
def test_no_limit_is_path_time_on_the_device(torch_dev, robots, n):
    hc = robots(CHAINS[n]).hip_chain()
    vmax, amax = _limits(n)
    paths, lens = _inputs(n, 64, 65)
    path_d, lens_d = _t(torch_dev, tu.to_device_layout(paths)), _t(torch_dev, lens)
    vmax_d, amax_d = _t(torch_dev, vmax), _t(torch_dev, amax)
    base = hc.path_time(path_d, lens_d, vmax_d, amax_d)
    for ee7 in (None, EE7):
        tool = hc.path_time_tool(path_d, lens_d, vmax_d, amax_d, ee_offset7=ee7)
        torch_dev.cuda.synchronize()
        for key in ("t", "qd", "qdd", "x", "duration", "status"):
            assert _same(tool[key].cpu().numpy(), base[key].cpu().numpy()), (n, key)
    assert int((base["status"] == 0).sum()) >= 20


def test_a_path_does_not_depend_on_the_batch(torch_dev, robots):
    hc = robots("arm16").hip_chain()
    vmax, amax = _limits(16)
    paths, lens = _inputs(16, 64, 65)
    many = _device(torch_dev, hc, paths, lens, vmax, amax, TOOL, EE7)
    one = _device(torch_dev, hc, paths[:1], lens[:1], vmax, amax, TOOL, EE7)
    assert many["status"][0] == tu.TIMED
    _agree(one, {key: v[:1] for key, v in many.items()}, "P = 1 against path 0 of P = 65")


def test_null_outputs_sentinels_and_refusals(torch_dev, robots):
    import torch
    from optik_amd import _native as nat
    from optik_amd.device import _ptr
    robot = robots("panda")
    lib, hc = nat.lib(), robot.hip_chain()
    n, L, P = 7, 16, 5
    vmax, amax = _limits(n)
    paths = tu.gentle_paths(np.random.default_rng(4), P, L, n)
    path_d, vmax_d, amax_d = _t(torch, tu.to_device_layout(paths)), _t(torch, vmax), _t(torch, amax)
    lim = (C.c_double * 4)(*TOOL)
    null, nolim = C.c_void_p(None), C.POINTER(C.c_double)()
    shapes = dict(t=(L, P), qd=(L, P, n), qdd=(L, P, n), x=(L, P), duration=(P,), status=(P,), tool_speed=(L, P),
                  tool_accel=(L, P, 2), tool_wspeed=(L, P))

    def buffers():
        return {k: _out(s, torch.int32 if k == "status" else torch.float64) for k, s in shapes.items()}

    def call(bufs, skip=(), L=L, P=P, limits=lim, chain=hc):
        ptr = {k: (null if k in skip else _ptr(b)) for k, b in bufs.items()}
        return lib.optik_hip_path_time_tool(chain._h, _ptr(path_d), null, L, P, _ptr(vmax_d), _ptr(amax_d), limits,
                                            None, ptr["t"], ptr["qd"], ptr["qdd"], ptr["x"], ptr["duration"],
                                            ptr["status"], ptr["tool_speed"], ptr["tool_accel"], ptr["tool_wspeed"],
                                            null)

    def untouched(bufs):
        torch.cuda.synchronize()
        return all(_sentinels_left(b.cpu().numpy()) == b.numel() for b in bufs.values())

    full = buffers()
    assert call(full) == 0
    torch.cuda.synchronize()
    assert all(_sentinels_left(b.cpu().numpy()) == 0 for b in full.values())
    assert list(full["status"].cpu().numpy()) == [0] * P
    # NULL outputs are skipped: the others have the full call's bits
    for skip in (("t", "qd", "qdd", "x", "duration", "status"), ("tool_speed", "tool_accel", "tool_wspeed"),
                 ("qd", "tool_accel")):
        part = buffers()
        assert call(part, skip) == 0
        torch.cuda.synchronize()
        for k, b in part.items():
            if k in skip:
                assert _sentinels_left(b.cpu().numpy()) == b.numel(), k
            else:
                assert torch.equal(b.view(torch.uint8), full[k].view(torch.uint8)), (skip, k)
    # nothing to do: P = 0, or every output NULL
    idle = buffers()
    assert call(idle, P=0) == 0 and call(idle, skip=tuple(shapes)) == 0 and untouched(idle)
    # OPTIK_HIP_EINVAL (-1) and OPTIK_HIP_EUNSUPPORTED (-2), before any device work
    for kw in (dict(L=2), dict(L=65), dict(P=-1), dict(P=(1 << 30) + 1), dict(limits=nolim)):
        assert call(idle, **kw) == -1, kw
    for i in range(4):
        for bad in (0.0, -1.0, math.nan, -math.inf):
            v = list(TOOL)
            v[i] = bad
            assert call(idle, limits=(C.c_double * 4)(*v)) == -1, (i, bad)
            assert call(idle, limits=(C.c_double * 4)(*v), P=0) == -1, (i, bad)
    assert call(idle, limits=(C.c_double * 4)(*([math.inf] * 4)), P=0) == 0
    gantry = robots("gantry").hip_chain()
    assert call(idle, chain=gantry) == -2 and call(idle, chain=gantry, P=0) == -2
    assert untouched(idle)
    # the Python layers refuse the same on the host
    for kw in (dict(tool_v_max=0.0), dict(tool_a_tangential=math.nan), dict(tool_a_normal=-1.0), dict(tool_w_max=0.0),
               dict(scale=0.0), dict(a_max=None)):
        with pytest.raises(ValueError):
            robot.time_paths_tool(paths, **{"a_max": 5.0, **kw})
    with pytest.raises(ValueError):
        hc.path_time_tool(path_d, None, vmax_d, amax_d, tool_v_max=-0.25)
    with pytest.raises(RuntimeError):
        robots("gantry").time_paths_tool(np.zeros((1, 8, robots("gantry").num_positions())), a_max=1.0)


def test_time_paths_tool(torch_dev, robots, ref):
    robot = robots("panda")
    chain = robot.chain_tables()
    vmax, amax = _limits(7)
    paths = tu.gentle_paths(np.random.default_rng(8), 8, 32, 7)
    lens = np.full(8, 32, dtype=np.int32)
    lens[2] = 9
    kw = dict(zip(ttu.LIMIT_KEYS, TOOL))
    want = ref.time(chain, paths, lens, vmax, amax, TOOL)
    out = robot.time_paths_tool(paths, lens, a_max=amax, v_max=vmax, **kw)
    assert set(out) == set(KEYS) - {"x"}
    for key in out:
        assert _same(out[key], want[key]), key
    assert np.all(want["status"] == tu.TIMED) and want["tool_speed"].max() >= 0.5 * (1 - 1e-9)
    # scale: the speeds with v_max, the accelerations with a_max
    half = robot.time_paths_tool(paths, lens, a_max=2.0 * amax, v_max=2.0 * vmax, scale=0.5,
                                 **{k: 2.0 * v for k, v in kw.items()})
    for key in out:
        assert _same(half[key], want[key]), key
    # an ee_offset [4, 4]: a translation
    off = np.eye(4)
    off[:3, 3] = [0.05, -0.02, 0.1]
    want_off = ref.time(chain, paths, lens, vmax, amax, TOOL, [0.05, -0.02, 0.1, 0.0, 0.0, 0.0, 1.0])
    got_off = robot.time_paths_tool(paths, lens, a_max=amax, v_max=vmax, ee_offset=off, **kw)
    for key in got_off:
        assert _same(got_off[key], want_off[key]), key
    # without a tool limit: time_paths
    plain = robot.time_paths(paths, lens, a_max=amax, v_max=vmax)
    free = robot.time_paths_tool(paths, lens, a_max=amax, v_max=vmax)
    for key in plain:
        assert _same(free[key], plain[key]), key
    # the dict goes into sample_trajectories as it is
    dt = float(want["duration"].max()) / 24.5
    q, v = robot.sample_trajectories(paths, out, dt, lens)
    assert q.shape == (8, 26, 7) and _same(q[:, 0], paths[:, 0])
    assert _same(q[:, -1], np.stack([paths[p, lens[p] - 1] for p in range(8)])) and np.all(v[:, -1] == 0.0)
