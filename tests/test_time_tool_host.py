"""CPU-only: the arithmetic of path timing with tool limits (optik_amd/csrc/time_tool_measure.hpp, compiled for the host
as tests/constraint_util.py compiles its header).  With no tool limit it is time_measure.hpp bit for bit; its
forward kinematics is constraint::fk bit for bit; the four tool rows and the joint rows hold on gentle paths and on
random walks, recomputed in numpy from the test's own forward kinematics; a speed cap binds; the profile against scipy's
HiGHS on the same rows where every slope is >= 0; a tool that does not move; the statuses; the argument rules."""
import math
import os

import numpy as np
import pytest

import time_tool_util as ttu
import time_util as tu
from conftest import ROBOT_SPECS, ROBOTS

CHAINS = {1: "panda1", 7: "panda", 16: "arm16"}
VMAX, AMAX = 2.0, 5.0
TOOL = ttu.limits4(0.5, 1.5, 1.0, 2.0)  # m/s, m/s^2, m/s^2, rad/s: each binds on the gentle Panda paths below
EE7 = np.array([0.05, -0.02, 0.1, 0.0, math.sin(0.3), 0.0, math.cos(0.3)])


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ttu.build_time_tool_ref(str(tmp_path_factory.mktemp("time_tool_measure")))


@pytest.fixture(scope="module")
def joint_ref(tmp_path_factory):
    return tu.build_time_ref(str(tmp_path_factory.mktemp("time_measure")))


@pytest.fixture(scope="module")
def chain_of():
    from optik_amd import Robot
    made = {}

    def get(name):
        if name not in made:
            made[name] = Robot.from_urdf_file(*ROBOT_SPECS[name]).chain_tables()
        return made[name]
    return get


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all((tu.bits(got) == tu.bits(want)) | (np.isnan(got) & np.isnan(want))))


SHARED = ("status", "duration", "times", "x", "velocities", "accelerations")


# ---- identity ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 7, 16])
def test_no_tool_limit_is_time_reference(ref, joint_ref, chain_of, n):
    rng = np.random.default_rng(40 + n)
    L = 24
    paths = np.concatenate([tu.random_walks(rng, 12, L, n), tu.gentle_paths(rng, 12, L, n)])
    lens = np.full(24, L)
    lens[3], lens[15], lens[16] = 3, 4, 17
    vmax = np.linspace(1.5, 2.5, n)
    want = joint_ref.time(paths, lens, vmax, AMAX)
    assert np.sum(want["status"] == tu.TIMED) >= 12
    for ee7 in (None, EE7):
        got = ref.time(chain_of(CHAINS[n]), paths, lens, vmax, AMAX, ttu.NO_LIMITS, ee7)
        for key in SHARED:
            assert _same(got[key], want[key]), (n, key)
        # the forward kinematics without the joint frames is constraint::fk
        assert np.array_equal(tu.bits(got["ee"]), tu.bits(got["ee_constraint"]))
        pos, quat = ttu.np_fk(chain_of(CHAINS[n]), paths[0], ee7)
        assert np.max(np.abs(pos - got["ee"][0, :, :3])) <= 1e-13 and np.max(np.abs(quat - got["ee"][0, :, 3:])) <= 1e-13


# ---- feasibility ---------------------------------------------------------------------------------------------------

def _check_rows(chain, paths, lens, out, lim, ee7=None):
    """The four tool rows and the joint rows of every profile that was written, from the test's own FK."""
    worst = np.zeros(6)
    for p in range(len(paths)):
        if out["status"][p] not in (tu.TIMED, tu.STALLED):
            continue
        ln = int(lens[p])
        path, x = paths[p, :ln], out["x"][p, :ln]
        assert x[0] == 0.0 and x[-1] == 0.0 and np.all(x >= 0.0), (p, x)
        pos, quat = ttu.np_fk(chain, path, ee7)
        excess = ttu.tool_excess(pos, quat, x, lim) + tu.constraint_excess(path, x, VMAX, AMAX)
        print(f"path {p}: len {ln} status {out['status'][p]} speed {excess[0]:.15g} tangential {excess[1]:.15g} "
              f"normal {excess[2]:.15g} angular {excess[3]:.15g} joint velocity {excess[4]:.15g} "
              f"acceleration {excess[5]:.15g} of the limit")
        assert max(excess) <= 1.0 + 1e-9, (p, excess)
        worst = np.maximum(worst, excess)
        # the new outputs are the rows' left sides
        g, ct, cn, w = ttu.tool_terms(pos, quat)
        r, u = np.sqrt(x), np.concatenate([(x[1:] - x[:-1]) / 2.0, [0.0]])
        tang = g * u + ct * x
        tang[-1] = 0.0
        for got, want in ((out["tool_speed"][p, :ln], g * r), (out["tool_accel"][p, :ln, 0], tang),
                          (out["tool_accel"][p, :ln, 1], cn * x), (out["tool_wspeed"][p, :ln], w * r)):
            assert np.max(np.abs(got - want)) <= 1e-9 * max(1.0, np.max(np.abs(want))), (p, got, want)
        assert np.all(out["tool_speed"][p, ln:] == 0.0) and np.all(out["tool_accel"][p, ln:] == 0.0)
        assert np.all(out["tool_wspeed"][p, ln:] == 0.0)
    return worst


@pytest.mark.parametrize("n", [7, 16])
def test_every_row_holds(ref, chain_of, n):
    rng = np.random.default_rng(60 + n)
    L = 32
    paths = np.concatenate([tu.gentle_paths(rng, 8, L, n), tu.random_walks(rng, 8, L, n)])
    lens = np.full(16, L)
    lens[2], lens[10] = 3, 9
    chain = chain_of(CHAINS[n])
    for lim, ee7 in ((TOOL, None), (TOOL, EE7), (ttu.limits4(tool_v_max=0.25), None),
                     (ttu.limits4(tool_a_tangential=0.8, tool_w_max=1.0), None), (ttu.limits4(tool_a_normal=0.5), EE7)):
        out = ref.time(chain, paths, lens, VMAX, AMAX, lim, ee7)
        assert np.all(out["status"][:8] == tu.TIMED), out["status"]
        assert np.all((out["status"] == tu.TIMED) | (out["status"] == tu.STALLED)), out["status"]
        worst = _check_rows(chain, paths, lens, out, lim, ee7)
        # every finite limit is reached by some path (the limits are not idle in this test)
        assert np.all(worst[:4][np.isfinite(lim)] >= 1.0 - 1e-9), (worst, lim)


# ---- a limit that binds --------------------------------------------------------------------------------------------

def test_a_speed_cap_binds(ref, chain_of):
    rng = np.random.default_rng(7)
    chain, P, L = chain_of("panda"), 8, 32
    paths = tu.gentle_paths(rng, P, L, 7)
    free = ref.time(chain, paths, None, VMAX, AMAX)
    assert np.all(free["status"] == tu.TIMED)
    # one cap for the call: half the peak of the path whose unlimited peak is the lowest, so at most half of every peak
    cap = 0.5 * float(free["tool_speed"].max(axis=1).min())
    out = ref.time(chain, paths, None, VMAX, AMAX, ttu.limits4(tool_v_max=cap))
    assert np.all(out["status"] == tu.TIMED), out["status"]
    peak = out["tool_speed"].max(axis=1)
    print("cap", cap, "peaks", peak, "durations", out["duration"], "unlimited", free["duration"])
    assert np.all(peak <= cap * (1.0 + 1e-9)) and np.all(np.abs(peak - cap) <= 1e-9 * cap), (peak, cap)
    assert np.all(out["duration"] > free["duration"])


# ---- against an LP -------------------------------------------------------------------------------------------------

def _lp_profile(path, pos, quat, lim):
    """max sum x over the joints' rows of time_measure.hpp and the tool's four rows: variables x_0 .. x_(m-1)."""
    from scipy.optimize import linprog
    m, n = path.shape
    d, c = tu.derivatives(path)
    g, ct, cn, w = ttu.tool_terms(pos, quat)
    A, b = [], []

    def cap(i, coeff, bound):
        row = np.zeros(m)
        row[i] = coeff
        A.append(row)
        b.append(bound)

    def two_sided(i, dd, cc, bound):
        row = np.zeros(m)
        row[i + 1] += dd / 2.0
        row[i] += cc - dd / 2.0
        A.extend([row, -row])
        b.extend([bound, bound])

    for i in range(m - 1):
        for j in range(n):
            cap(i, d[i, j] ** 2, VMAX ** 2)
            two_sided(i, d[i, j], c[i, j], AMAX)
        cap(i, g[i] ** 2, lim[0] ** 2)
        two_sided(i, g[i], ct[i], lim[1])
        cap(i, cn[i], lim[2])
        cap(i, w[i] ** 2, lim[3] ** 2)
    bounds = [(0.0, 0.0)] + [(0.0, None)] * (m - 2) + [(0.0, 0.0)]
    res = linprog(-np.ones(m), A_ub=np.array(A), b_ub=np.array(b), bounds=bounds, method="highs")
    assert res.status == 0, res.message
    return res.x


@pytest.mark.parametrize("L", [16, 64])
def test_gentle_paths_match_the_lp(ref, chain_of, L):
    pytest.importorskip("scipy", reason="scipy (HiGHS) is not installed")
    rng = np.random.default_rng(L)
    chain = chain_of("panda")
    paths = tu.gentle_paths(rng, 4, L, 7)
    out = ref.time(chain, paths, None, VMAX, AMAX, TOOL)
    free = ref.time(chain, paths, None, VMAX, AMAX)
    for p in range(4):
        pos, quat = ttu.np_fk(chain, paths[p])
        # the method claims optimality only where every slope, the tool row's included, is >= 0
        assert np.nanmin(tu.slopes(paths[p])) >= 0.0 and np.nanmin(ttu.tool_slopes(pos)) >= 0.0
        assert out["status"][p] == tu.TIMED and out["duration"][p] > free["duration"][p]
        x_lp = _lp_profile(paths[p], pos, quat, TOOL)
        err = np.max(np.abs(out["x"][p] - x_lp))
        print(f"L {L} path {p}: |x - x_LP| = {err:.3g} of max x = {x_lp.max():.6g}")
        assert err <= 1e-6 * x_lp.max()


# ---- degenerate stages ---------------------------------------------------------------------------------------------

def test_a_tool_that_does_not_move(ref, joint_ref, chain_of):
    from optik_amd import Robot
    # the tool on the axis of the only joint that moves: link 7's origin, turned by joint 7 (no trailing fixed joint,
    # so the position never meets the angle)
    chain = Robot.from_urdf_file(os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link7").chain_tables()
    rng = np.random.default_rng(11)
    L = 12
    base = tu.gentle_paths(rng, 1, L, 7)[0]
    spin = np.tile(base[0], (L, 1))
    spin[:, 6] = base[:, 6]                 # only joint 7 moves: g = 0 at every waypoint
    held = base.copy()
    held[4:7, :6] = held[4, :6]             # joints 1 - 6 rest over waypoints 4, 5, 6: g_5 = 0, C_5 = 0
    paths = np.stack([spin, held])
    lim = ttu.limits4(0.1, 0.5, 0.5)        # no angular limit: nothing of the tool bounds a stage with g = 0
    out = ref.time(chain, paths, None, VMAX, AMAX, lim)
    want = joint_ref.time(paths, None, VMAX, AMAX)
    assert list(want["status"]) == [tu.TIMED, tu.TIMED]
    for key in SHARED:                      # the joint rows alone decide path 0, bit for bit
        assert _same(out[key][0], want[key][0]), key
    assert np.all(out["tool_speed"][0] == 0.0) and np.all(out["tool_accel"][0] == 0.0)
    assert np.all(out["tool_wspeed"][0, 1:-1] > 0.0)
    assert out["status"][1] == want["status"][1] and out["tool_speed"][1, 5] == 0.0 and out["x"][1, 5] > 0.0
    assert np.all(out["tool_accel"][1, 5] == 0.0) and out["tool_speed"][1, 3] > 0.0
    # with an angular limit the stage is bounded by it
    slow = ref.time(chain, paths, None, VMAX, AMAX, ttu.limits4(tool_w_max=0.5))
    assert slow["status"][0] == tu.TIMED and slow["duration"][0] > want["duration"][0]
    assert slow["tool_wspeed"][0].max() <= 0.5 * (1 + 1e-9)
    # a one-joint chain whose end effector lies on the joint's axis, the tool turned by an ee_offset without translation
    one = chain_of("panda1")
    p1 = tu.gentle_paths(rng, 2, L, 1)
    turn = np.array([0.0, 0.0, 0.0, math.sin(0.4), 0.0, 0.0, math.cos(0.4)])
    got = ref.time(one, p1, None, VMAX, AMAX, ttu.limits4(0.1, 0.5, 0.5), turn)
    want = joint_ref.time(p1, None, VMAX, AMAX)
    for key in SHARED:
        assert _same(got[key], want[key]), key
    assert np.all(got["tool_speed"] == 0.0)


def test_statuses_are_time_paths(ref, joint_ref, chain_of):
    rng = np.random.default_rng(3)
    n, L = 7, 8
    paths = tu.gentle_paths(rng, 7, L, n)
    lens = [2, L + 1, L, L, L, 3, L]
    paths[2, 1] = paths[2, 0]           # d_0 = c_0 = 0: stage 0 bounds nothing, the tool's rows included
    paths[3, 5, 2] = math.nan
    paths[4, 3:6] = paths[4, 3]         # three equal waypoints inside
    paths[6, 0, 0] = math.inf
    out = ref.time(chain_of("panda"), paths, lens, VMAX, AMAX, TOOL)
    want = joint_ref.time(paths, lens, VMAX, AMAX)
    assert list(out["status"]) == list(want["status"])
    assert list(out["status"]) == [tu.BAD_LENGTH, tu.BAD_LENGTH, tu.BAD_LENGTH, tu.PATH_NAN, tu.BAD_LENGTH, tu.TIMED,
                                   tu.PATH_NAN]
    bad = out["status"] != tu.TIMED
    assert np.all(np.isnan(out["times"][bad])) and np.all(np.isnan(out["duration"][bad]))
    for key in ("x", "velocities", "accelerations", "tool_speed", "tool_accel", "tool_wspeed"):
        assert np.all(out[key][bad] == 0.0), key
    assert np.all(out["times"][5, 3:] == out["duration"][5]) and np.all(out["tool_speed"][5, 3:] == 0.0)
    # a repeated start bounds nothing, whatever the pose: the rotation between equal quaternions is 0, not the 1e-17
    # their product would leave, so a finite angular limit does not make a stage of it
    for n in (7, 16):
        walks = tu.random_walks(rng, 20, 3, n)
        walks[:, 1] = walks[:, 0]
        for ee7 in (None, EE7):
            again = ref.time(chain_of(CHAINS[n]), walks, None, VMAX, AMAX, TOOL, ee7)
            assert np.all(again["status"] == tu.BAD_LENGTH), again["status"]


def test_check_time_tool_args():
    from optik_amd import _native as nat
    lim = nat.check_time_tool_args(0.25, 2.0, math.inf, 1.0, 0.5)
    assert list(lim) == [0.125, 1.0, math.inf, 0.5] and lim.dtype == np.float64
    assert list(nat.check_time_tool_args()) == [math.inf] * 4
    for kw in (dict(tool_v_max=0.0), dict(tool_v_max=-1.0), dict(tool_a_tangential=math.nan), dict(tool_a_normal=0.0),
               dict(tool_w_max=-math.inf), dict(tool_w_max="fast"), dict(tool_v_max=[0.1, 0.2]), dict(scale=0.0),
               dict(scale=1.5), dict(scale=math.nan)):
        with pytest.raises(ValueError):
            nat.check_time_tool_args(**kw)
