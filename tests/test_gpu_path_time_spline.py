"""-m gpu: spline retiming on the device against the host.  HipChain.path_time_spline against the serial reference of
csrc/time_spline_measure.hpp, every output bit for bit, over the shapes at which the kernel takes another path: n = 1
(one lane in the recurrences), 7 and 16 (the widest rotation of the LDS rows), L = 3 (one row of the system), 4 and 64
(a full wave), P = 1 and 65, with lengths, binding limits and the statuses 0 to 3 mixed in one launch; a path's
independence of the batch, its neighbours and the stream; the later trips of the wave's loop over the paths under a
capped grid; NULL outputs, P = 0 and the refusals; Robot.smooth_timing through the C ABI rows and on into
sample_trajectories; a path that rounding leaves at status 4, in the sampler and through a second pass."""
import ctypes as C
import math

import numpy as np
import pytest

import time_spline_util as su
import time_util as tu
from conftest import ROBOT_SPECS
from gpu_util import _out, _sentinels_left

pytestmark = pytest.mark.gpu

CHAINS = {1: "panda1", 7: "panda", 16: "arm16"}
KEYS = ("status", "duration", "factor", "ratios", "times", "velocities", "accelerations")
# rad/s^3: beside the timing's own v_max and a_max, some paths of a 64-waypoint launch bind the acceleration, the others
# the jerk; at 4 waypoints the velocity binds too
J_MAX = 150.0


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
def refs(tmp_path_factory):
    return (tu.build_time_ref(str(tmp_path_factory.mktemp("spline_gpu_time"))),
            su.build_spline_ref(str(tmp_path_factory.mktemp("spline_gpu"))))


_CASES = {}


@pytest.fixture(scope="module")
def case(refs):
    """(n, L, P) -> the mixed batch of time_spline_util, its limits and the reference's result, computed once."""
    def get(n, L, P):
        if (n, L, P) not in _CASES:
            paths, lens, times, status, v, a = su.mixed_batch(refs[0], np.random.default_rng(3000 * n + 10 * L + P), P, L, n)
            if n > 2:
                v[2] = math.inf
            j = np.full(n, J_MAX)
            want = refs[1].retime(paths, lens, times, status, v, a, j)
            _CASES[(n, L, P)] = dict(paths=paths, lens=lens, times=times, status=status, v=v, a=a, j=j, want=want)
        return _CASES[(n, L, P)]
    return get


def _t(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all((tu.bits(got) == tu.bits(want)) | (np.isnan(got) & np.isnan(want))))


def _sw(a):
    return np.ascontiguousarray(np.swapaxes(a.cpu().numpy(), 0, 1))


def _host_layout(res):
    return dict(times=_sw(res["t"]), velocities=_sw(res["qd"]), accelerations=_sw(res["qdd"]),
                duration=res["duration"].cpu().numpy(), factor=res["factor"].cpu().numpy(),
                ratios=res["ratios"].cpu().numpy(), status=res["status"].cpu().numpy())


def _device(torch, hc, c, rows=None, lens=True):
    """The rows `rows` of case c (None: all) through HipChain.path_time_spline, in the host's layout."""
    rows = np.arange(len(c["paths"])) if rows is None else np.asarray(rows)
    timing = dict(t=_t(torch, tu.to_device_layout(c["times"][rows])), status=_t(torch, c["status"][rows]))
    res = hc.path_time_spline(_t(torch, tu.to_device_layout(c["paths"][rows])), timing, _t(torch, c["j"]),
                              _t(torch, c["a"]), _t(torch, c["v"]), _t(torch, c["lens"][rows]) if lens else None)
    torch.cuda.synchronize()
    return _host_layout(res)


def _agree(got, want, what, rows=None):
    for key in KEYS:
        assert _same(got[key], want[key] if rows is None else want[key][rows]), (what, key)


@pytest.mark.parametrize("L", [3, 4, 64])
@pytest.mark.parametrize("n", [1, 7, 16])
def test_device_matches_the_reference(torch_dev, robots, case, n, L):
    hc = robots(CHAINS[n]).hip_chain()
    assert hc.n == n
    c = case(n, L, 65)
    want = c["want"]
    _agree(_device(torch_dev, hc, c), want, (n, L, 65))
    st = want["status"]
    # (a 4 may turn up in any batch whose jerk binds -- rounding --, and parity holds for it as for the rest; what becomes
    # of one in the sampler and in a second pass: test_over_limit_is_held_by_the_sampler_and_cleared_by_a_second_pass)
    assert {su.SMOOTH, su.BAD_TIMES, su.BAD_LENGTH, su.NOT_FINITE} <= set(st.tolist()) <= {0, 1, 2, 3, 4}, st
    assert st[7] == su.BAD_TIMES and c["status"][7] == tu.STALLED and np.sum(st == su.SMOOTH) >= 30
    ok = st == su.SMOOTH
    assert (want["ratios"][ok] <= 1.0).all()
    slowed = ok & (want["factor"] > 1.0)
    binding = np.bincount(want["ratios"][slowed].argmax(axis=1), minlength=3)
    print(f"n = {n}, L = {L}: {ok.sum()} smooth, {slowed.sum()} slowed; velocity, acceleration, jerk bind in {binding}")
    if L == 64:
        assert (binding > 0).sum() >= 2
    if L == 3:  # (one interior knot: the spline is gentler than the timing's trapezoid, and nothing is slowed)
        assert slowed.sum() < ok.sum()
    # P = 1
    one = case(n, L, 1)
    assert one["want"]["status"][0] == su.SMOOTH
    _agree(_device(torch_dev, hc, one), one["want"], (n, L, 1))
    if L == 64:  # lens None: L each
        full = np.flatnonzero(c["lens"] == L)[:6]
        _agree(_device(torch_dev, hc, c, full, lens=False), want, (n, L, "no lens"), full)


def test_a_path_does_not_depend_on_the_batch_its_neighbours_or_the_stream(torch_dev, robots, case):
    hc = robots("arm16").hip_chain()
    c = case(16, 64, 65)
    want = c["want"]
    for p in (0, 1, 3, 7, 26, 64):
        _agree(_device(torch_dev, hc, c, [p]), want, ("alone", p), [p])
    back = np.arange(65)[::-1]
    _agree(_device(torch_dev, hc, c, back), want, "reversed neighbours", back)
    side = torch_dev.cuda.Stream()
    with torch_dev.cuda.stream(side):
        got = _device(torch_dev, hc, c)
    side.synchronize()
    _agree(got, want, "side stream")


@pytest.mark.parametrize("n", [7, 16])
def test_later_trips_under_a_capped_grid(torch_dev, robots, case, n):
    """The option grid_cap (tests/test_gpu_grid_stride.py) puts 1 or 3 blocks in the device's place: one wave then
    walks all 65 paths through the same LDS, a smooth path behind a refused one and the other way round, or three waves
    a ragged third each.  Sentinel-filled outputs: a path that is skipped shows."""
    import torch
    from optik_amd import _native as nat
    from optik_amd.device import _ptr
    hc = robots(CHAINS[n]).hip_chain()
    L, P = 64, 65
    c = case(n, L, P)
    ins = [_t(torch, a) for a in (tu.to_device_layout(c["paths"]), c["lens"], tu.to_device_layout(c["times"]), c["status"],
                                  c["v"], c["a"], c["j"])]
    shapes = dict(t=(L, P), qd=(L, P, n), qdd=(L, P, n), duration=(P,), factor=(P,), ratios=(P, 3), status=(P,))
    got = {}
    for cap in (0, 1, 3):
        outs = {k: _out(s, torch.int32 if k == "status" else torch.float64) for k, s in shapes.items()}
        with nat.options(grid_cap=cap):
            assert nat.get_option("grid_cap") == cap
            nat.check(nat.lib().optik_hip_path_time_spline(
                hc._h, _ptr(ins[0]), _ptr(ins[1]), L, P, _ptr(ins[2]), _ptr(ins[3]), _ptr(ins[4]), _ptr(ins[5]),
                _ptr(ins[6]), *[_ptr(outs[k]) for k in shapes], C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
        for k, b in outs.items():
            left = _sentinels_left(b.cpu().numpy())
            # (NaN times and durations of refused paths are the kernel's own NaN, not the sentinel's payload)
            assert left == 0, f"cap {cap}: {left} values of {k} not written"
        got[cap] = _host_layout(outs)
        _agree(got[cap], c["want"], ("cap", cap))
    assert nat.get_option("grid_cap") == 0


def test_null_outputs_and_refusals(torch_dev, robots, case):
    import torch
    from optik_amd import _native as nat
    from optik_amd.device import _ptr
    robot = robots("panda")
    lib, hc = nat.lib(), robot.hip_chain()
    n, L, P = 7, 4, 65
    c = case(n, L, P)
    ins = [_t(torch, a) for a in (tu.to_device_layout(c["paths"]), c["lens"], tu.to_device_layout(c["times"]), c["status"],
                                  c["v"], c["a"], c["j"])]
    null = C.c_void_p(None)
    shapes = dict(t=(L, P), qd=(L, P, n), qdd=(L, P, n), duration=(P,), factor=(P,), ratios=(P, 3), status=(P,))

    def buffers():
        return {k: _out(s, torch.int32 if k == "status" else torch.float64) for k, s in shapes.items()}

    def call(bufs, skip=(), L=L, P=P, chain=hc, status_in=True):
        ptr = [null if k in skip else _ptr(bufs[k]) for k in shapes]
        return lib.optik_hip_path_time_spline(chain._h, _ptr(ins[0]), _ptr(ins[1]), L, P, _ptr(ins[2]),
                                              _ptr(ins[3]) if status_in else null, _ptr(ins[4]), _ptr(ins[5]),
                                              _ptr(ins[6]), *ptr, null)

    def untouched(bufs):
        torch.cuda.synchronize()
        return all(_sentinels_left(b.cpu().numpy()) == b.numel() for b in bufs.values())

    full = buffers()
    assert call(full) == 0
    torch.cuda.synchronize()
    _agree(_host_layout(full), c["want"], "the C ABI")
    for skip in (("t", "qd", "qdd"), ("duration", "factor", "ratios", "status"), ("qd",), ("qdd", "ratios")):
        part = buffers()
        assert call(part, skip) == 0
        torch.cuda.synchronize()
        for k, b in part.items():
            if k in skip:
                assert _sentinels_left(b.cpu().numpy()) == b.numel(), k
            else:
                assert torch.equal(b.view(torch.uint8), full[k].view(torch.uint8)), (skip, k)
    # d_status_in NULL: every input status is 0 -- the stalled inputs' NaN times are then read, and are not finite
    free = buffers()
    assert call(free, status_in=False) == 0
    torch.cuda.synchronize()
    st = free["status"].cpu().numpy()
    stalled = c["status"] != 0
    assert stalled.sum() >= 4 and (st[stalled] == su.NOT_FINITE).all() and np.array_equal(st[~stalled], c["want"]["status"][~stalled])
    # nothing to do: P = 0, or every output NULL
    idle = buffers()
    assert call(idle, P=0) == 0 and call(idle, skip=tuple(shapes)) == 0 and untouched(idle)
    # OPTIK_HIP_EINVAL (-1) and OPTIK_HIP_EUNSUPPORTED (-2), before any device work
    for kw in (dict(L=2), dict(L=65), dict(P=-1), dict(P=(1 << 30) + 1)):
        assert call(idle, **kw) == -1, kw
    gantry = robots("gantry").hip_chain()
    assert call(idle, chain=gantry) == -2 and call(idle, chain=gantry, P=0) == -2
    assert untouched(idle)
    # the Python layers refuse on the host
    paths = c["paths"]
    timing = dict(times=c["times"], status=c["status"])
    for kw in (dict(j_max=0.0), dict(a_max=math.nan), dict(v_max=-1.0), dict(j_max=[1.0, 2.0]), dict(a_max=-math.inf)):
        with pytest.raises(ValueError):
            robot.smooth_timing(paths, timing, **{"j_max": 40.0, "a_max": 5.0, **kw})
    with pytest.raises(ValueError):
        robot.smooth_timing(paths, dict(times=c["times"][:, :3], status=c["status"]), 40.0, 5.0)
    with pytest.raises(ValueError):
        hc.path_time_spline(ins[0], dict(t=ins[2], status=ins[3]), ins[6], ins[5], ins[4][:3])
    g = robots("gantry")
    with pytest.raises(RuntimeError):
        g.smooth_timing(np.zeros((1, 8, g.num_positions())), dict(times=np.zeros((1, 8)), status=np.zeros(1)), 1.0, 1.0)


def test_smooth_timing_agrees_with_the_chain_and_feeds_the_sampler(torch_dev, robots, refs, case):
    robot = robots("panda")
    hc = robot.hip_chain()
    c = case(7, 64, 65)
    out = robot.smooth_timing(c["paths"], dict(times=c["times"], status=c["status"]), c["j"], c["a"], c["v"], c["lens"])
    assert set(out) == set(KEYS)
    _agree(out, _device(torch_dev, hc, c), "Robot against HipChain")
    _agree(out, c["want"], "Robot against the reference")
    # time_paths -> smooth_timing -> sample_trajectories; v_max None: the URDF's limits
    paths = tu.gentle_paths(np.random.default_rng(9), 2, 8, 7)
    timed = robot.time_paths(paths, a_max=6.0)
    # (12 D / T^3 is the least peak jerk of a rest-to-rest motion with free end accelerations: with D >= 0.95 rad,
    # 2 rad/s^3 binds below 1.78 s)
    assert (timed["status"] == 0).all() and (timed["duration"] < 1.7).all()
    smooth = robot.smooth_timing(paths, timed, j_max=2.0, a_max=6.0)
    explicit = robot.smooth_timing(paths, timed, 2.0, 6.0, robot.velocity_limits())
    for key in KEYS:
        assert _same(smooth[key], explicit[key]), key
    assert (smooth["status"] == 0).all() and (smooth["factor"] > 1.0).all() and (smooth["ratios"] <= 1.0).all()
    assert _same(smooth["times"], smooth["factor"][:, None] * timed["times"])
    # a sample at k * dt with dt = t'_i, k = 1 sits on waypoint i: the sampler copies the knot and its velocity
    for p in range(2):
        for i in range(1, 8):
            dt = float(smooth["times"][p, i])
            q, v = robot.sample_trajectories(paths[p:p + 1], {k: a[p:p + 1] for k, a in smooth.items()}, dt)
            assert _same(q[0, 1], paths[p, i]) and _same(v[0, 1], smooth["velocities"][p, i]), (p, i)
    # and the sampled curve is the reference's on the same knots
    dt = float(smooth["duration"].max()) / 24.5
    q, v = robot.sample_trajectories(paths, smooth, dt)
    wq, wv = refs[0].sample(paths, None, smooth, dt, q.shape[1])
    assert q.shape == (2, 26, 7) and _same(q, wq) and _same(v, wv)


def test_over_limit_is_held_by_the_sampler_and_cleared_by_a_second_pass(torch_dev, robots, refs):
    """The single-joint batch in which rounding leaves one path at a jerk ratio of 1 + 3e-12, status 4: the device
    agrees with the reference on it; sample_trajectories holds it at its start, as every status other than 0; passed in
    again -- its status 4 counts as timed -- it is scaled by 1 + 2e-12, ends at 0 and is then sampled to its goal, while
    the paths that were 0 come back bit for bit."""
    robot = robots("panda1")
    hc = robot.hip_chain()
    paths, lens, times, status, v, a = su.over_limit_batch(refs[0])
    j = np.full(1, su.OVER_LIMIT_J)
    c = dict(paths=paths, lens=lens, times=times, status=status, v=v, a=a, j=j)
    want = refs[1].retime(paths, lens, times, status, v, a, j)
    over, good = np.flatnonzero(want["status"] == su.OVER_LIMIT), np.flatnonzero(want["status"] == su.SMOOTH)
    assert len(over) >= 1 and len(good) >= 30
    first = _device(torch_dev, hc, c)
    _agree(first, want, "first pass, HipChain")
    out = robot.smooth_timing(paths, dict(times=times, status=status), j, a, v, lens)
    _agree(out, want, "first pass, Robot")
    p = int(over[0])
    dt = float(out["duration"][p]) / 20.0
    q, qd = robot.sample_trajectories(paths[p:p + 1], {k: x[p:p + 1] for k, x in out.items()}, dt, lens[p:p + 1])
    assert q.shape[1] == 1 and _same(q[0, 0], paths[p, 0]) and not qd.any()
    want2 = refs[1].retime(paths, lens, want["times"], want["status"], v, a, j)
    assert (want2["status"][over] == su.SMOOTH).all() and (want2["ratios"][over] <= 1.0).all()
    assert (want2["factor"][over] > 1.0).all() and (want2["factor"][over] <= 1.0 + 1e-11).all()
    assert (want2["factor"][good] == 1.0).all()
    for key in KEYS:
        if key != "factor":  # (1 now, the first pass's k then)
            assert _same(want2[key][good], want[key][good]), key
    _agree(_device(torch_dev, hc, dict(c, times=first["times"], status=first["status"])), want2, "second pass, HipChain")
    again = robot.smooth_timing(paths, out, j, a, v, lens)
    _agree(again, want2, "second pass, Robot")
    q, qd = robot.sample_trajectories(paths[p:p + 1], {k: x[p:p + 1] for k, x in again.items()}, dt, lens[p:p + 1])
    assert q.shape[1] >= 21 and _same(q[0, -1], paths[p, lens[p] - 1]) and qd[0, 1:-1].any()
