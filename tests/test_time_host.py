"""CPU-only: the arithmetic of path timing and trajectory sampling (optik_amd/csrc/time_measure.hpp, built with g++).
The profile of a straight line against the closed-form trapezoid; the constraints on random walks; the profile against
scipy's HiGHS on the same constraints; the statuses; the sampler at the waypoints, past the end and on a line; the
URDF's velocity limits; the host-side argument rules.

The random walks: the header states that the greedy forward pass is made for paths whose slopes s_j are >= 0, that is
|c| <= |d| / 2.  A walk whose steps keep their sign per joint and vary within [0.6, 1] of a scale has
|c| <= 0.4 and |d| >= 0.6 of it inside and is in that domain; every assertion is made of each such path.  An
unbiased walk (steps uniform in [-1, 1] of the scale) reverses joints from one waypoint to the next, so a third of
them reach a stage whose only admissible successor is x = 0 next to the x = 0 of the goal: the header's own status 1,
whose times are NaN by definition.  Of those walks the constraints are asserted of every path -- status 1 still writes
its profile -- and the times of the paths whose status is 0."""
import math
import os

import numpy as np
import pytest

import time_util as tu
from conftest import ROBOT_SPECS, TEST_ROBOTS


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return tu.build_time_ref(str(tmp_path_factory.mktemp("time_measure")))


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all(tu.bits(got) == tu.bits(want)))


# ---- the straight line ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale,binds", [(1.0, False), (8.0, True)])
def test_straight_line_is_the_trapezoid(ref, scale, binds):
    L, D = 16, np.array([0.1, -0.05, 0.02]) * scale
    amax, vmax = np.array([2.0, 3.0, 4.0]), np.array([2.0, 2.0, 2.0])
    path = (np.arange(L)[:, None] * D)[None]
    out = ref.time(path, None, vmax, amax)
    assert out["status"][0] == tu.TIMED
    k, xcap = np.min(amax / np.abs(D)), np.min((vmax / np.abs(D)) ** 2)
    i = np.arange(L)
    want = np.minimum(np.minimum(2 * k * i, xcap), 2 * k * (L - 1 - i))
    assert bool(np.any(want == xcap)) == binds
    x = out["x"][0]
    assert np.all(np.abs(x - want) <= 1e-12 * want), (x, want)
    r = np.sqrt(want)
    duration = np.sum(2.0 / (r[:-1] + r[1:]))
    assert abs(out["duration"][0] - duration) <= 1e-12 * duration
    assert out["times"][0, 0] == 0.0 and out["times"][0, -1] == out["duration"][0]


# ---- feasibility ---------------------------------------------------------------------------------------------------

def _drift_walks(rng, P, L, n, scale=0.3):
    step = rng.uniform(0.6, 1.0, (P, L, n)) * scale * rng.choice([-1.0, 1.0], (P, 1, n))
    return np.cumsum(step, axis=1)


def _check_profile(paths, out, p, ln, vmax, amax, timed):
    path, x = paths[p, :ln], out["x"][p, :ln]
    assert x[0] == 0.0 and x[-1] == 0.0 and np.all(x >= 0.0), (p, x)
    vel, acc = tu.constraint_excess(path, x, vmax, amax)
    print(f"path {p}: len {ln} status {out['status'][p]} velocity {vel:.17g} acceleration {acc:.17g} of the limit")
    assert vel <= 1.0 + 1e-9 and acc <= 1.0 + 1e-9, (p, vel, acc)
    d, c = tu.derivatives(path)
    u = (x[1:] - x[:-1]) / 2.0
    assert _same(out["velocities"][p, :ln], d * np.sqrt(x)[:, None])
    qdd = np.zeros_like(path)
    qdd[:-1] = d[:-1] * u[:, None] + c[:-1] * x[:-1, None]
    assert _same(out["accelerations"][p, :ln], qdd)
    if timed:
        t = out["times"][p, :ln]
        assert t[0] == 0.0 and np.all(np.diff(t) > 0.0) and t[-1] == out["duration"][p], (p, t)
        r = np.sqrt(x)
        want = np.concatenate([[0.0], np.cumsum(2.0 / (r[:-1] + r[1:]))])
        assert _same(t, want), (p, t, want)


SHAPES = [(n, ln) for n in (1, 4, 7, 16) for ln in (3, 4, 12, 64)]


def test_random_walks_are_feasible(ref):
    rng = np.random.default_rng(20)
    vmax, amax = 2.0, 5.0
    count = 0
    for k, (n, ln) in enumerate(SHAPES):
        P = 13 if k < 8 else 12
        paths = _drift_walks(rng, P, ln, n)
        assert np.nanmin(tu.slopes(paths[0])) >= 0.0
        out = ref.time(paths, None, vmax, amax)
        assert np.all(out["status"] == tu.TIMED), (n, ln, out["status"])
        for p in range(P):
            _check_profile(paths, out, p, ln, vmax, amax, True)
        count += P
    assert count == 200


def test_unbiased_walks_keep_the_limits(ref):
    rng = np.random.default_rng(21)
    vmax, amax = 2.0, 5.0
    timed = 0
    for n, ln in SHAPES:
        P = 6
        paths = tu.random_walks(rng, P, ln, n)
        out = ref.time(paths, None, vmax, amax)
        assert np.all((out["status"] == tu.TIMED) | (out["status"] == tu.STALLED)), out["status"]
        for p in range(P):
            ok = out["status"][p] == tu.TIMED
            _check_profile(paths, out, p, ln, vmax, amax, ok)
            assert ok or (np.all(np.isnan(out["times"][p])) and math.isnan(out["duration"][p]))
            timed += int(ok)
    assert timed > 0


# ---- against an LP -------------------------------------------------------------------------------------------------

def _lp_profile(path, vmax, amax):
    """max sum x over the header's constraints: variables x_0 .. x_(m-1), u_i = (x_(i+1) - x_i) / 2 eliminated."""
    from scipy.optimize import linprog
    m, n = path.shape
    d, c = tu.derivatives(path)
    A, b = [], []
    for i in range(m - 1):
        for j in range(n):
            row = np.zeros(m)
            row[i] = d[i, j] ** 2
            A.append(row)
            b.append(vmax ** 2)
            row = np.zeros(m)
            row[i + 1] += d[i, j] / 2.0
            row[i] += c[i, j] - d[i, j] / 2.0
            A.append(row)
            b.append(amax)
            A.append(-row)
            b.append(amax)
    bounds = [(0.0, 0.0)] + [(0.0, None)] * (m - 2) + [(0.0, 0.0)]
    res = linprog(-np.ones(m), A_ub=np.array(A), b_ub=np.array(b), bounds=bounds, method="highs")
    assert res.status == 0, res.message
    return res.x


@pytest.mark.parametrize("L", [16, 64])
def test_gentle_paths_match_the_lp(ref, L):
    pytest.importorskip("scipy", reason="scipy (HiGHS) is not installed")
    rng = np.random.default_rng(L)
    n, vmax, amax = 7, 2.0, 5.0
    paths = tu.gentle_paths(rng, 4, L, n)
    out = ref.time(paths, None, vmax, amax)
    for p in range(4):
        assert np.nanmin(tu.slopes(paths[p])) >= 0.0
        assert out["status"][p] == tu.TIMED
        x_lp = _lp_profile(paths[p], vmax, amax)
        err = np.max(np.abs(out["x"][p] - x_lp))
        print(f"L {L} path {p}: |x - x_LP| = {err:.3g} of max x = {x_lp.max():.6g}")
        assert err <= 1e-6 * x_lp.max()


def test_random_walks_stay_below_the_lp(ref):
    pytest.importorskip("scipy", reason="scipy (HiGHS) is not installed")
    rng = np.random.default_rng(5)
    n, L, vmax, amax = 7, 16, 2.0, 5.0
    paths = tu.random_walks(rng, 50, L, n)
    assert min(np.nanmin(tu.slopes(p)) for p in paths) < 0.0
    out = ref.time(paths, None, vmax, amax)
    for p in range(50):
        x_lp = _lp_profile(paths[p], vmax, amax)
        assert np.sum(out["x"][p]) <= np.sum(x_lp) * (1.0 + 1e-6), p


# ---- statuses ------------------------------------------------------------------------------------------------------

def test_statuses(ref):
    rng = np.random.default_rng(3)
    n, L = 4, 8
    paths = _drift_walks(rng, 6, L, n)
    lens = [2, L + 1, L, L, L, 3]
    paths[2, 1] = paths[2, 0]           # d_0 = c_0 = 0: stage 0 bounds nothing
    paths[3, 5, 2] = math.nan
    paths[4, 3:6] = paths[4, 3]         # three equal waypoints inside
    out = ref.time(paths, lens, 2.0, 5.0)
    assert list(out["status"]) == [tu.BAD_LENGTH, tu.BAD_LENGTH, tu.BAD_LENGTH, tu.PATH_NAN, tu.BAD_LENGTH, tu.TIMED]
    bad = out["status"] != tu.TIMED
    assert np.all(np.isnan(out["times"][bad])) and np.all(np.isnan(out["duration"][bad]))
    assert np.all(out["velocities"][bad] == 0.0) and np.all(out["x"][bad] == 0.0)
    # behind the path's own waypoints: the duration, at rest
    assert np.all(out["times"][5, 3:] == out["duration"][5]) and np.all(out["velocities"][5, 3:] == 0.0)
    # a waypoint repeated once inside is a path like any other
    once = _drift_walks(rng, 1, L, n)
    once[0, 4] = once[0, 3]
    assert ref.time(once, None, 2.0, 5.0)["status"][0] in (tu.TIMED, tu.STALLED)
    # no velocity limit at all: the acceleration members still bound x
    free = ref.time(paths[5:6], [L], math.inf, 5.0)
    assert free["status"][0] == tu.TIMED and math.isfinite(free["duration"][0])
    assert free["duration"][0] <= ref.time(paths[5:6], [L], 2.0, 5.0)["duration"][0]


def test_check_time_args():
    from optik_amd import _native as nat
    v, a = nat.check_time_args(3, 16, 5.0, [1.0, math.inf, 2.0], 0.5)
    assert list(v) == [0.5, math.inf, 1.0] and list(a) == [2.5, 2.5, 2.5]
    for kw in (dict(a_max=0.0), dict(a_max=-1.0), dict(a_max=math.inf), dict(a_max=math.nan), dict(a_max=[1.0, 2.0]),
               dict(v_max=0.0), dict(v_max=-2.0), dict(v_max=math.nan), dict(v_max=[1.0, 1.0, 1.0, 1.0]),
               dict(L=2), dict(L=65), dict(L=3.5), dict(scale=0.0), dict(scale=1.5), dict(scale=math.nan)):
        with pytest.raises(ValueError):
            nat.check_time_args(3, **kw)
    assert nat.check_sample_args(0.001, 65536) == 0.001
    for dt, T in ((0.0, 1), (-1.0, 1), (math.nan, 1), (math.inf, 1), (0.01, 0), (0.01, 65537)):
        with pytest.raises(ValueError):
            nat.check_sample_args(dt, T)


# ---- sampling ------------------------------------------------------------------------------------------------------

def test_samples_on_a_straight_line(ref):
    L, D = 12, np.array([0.2, -0.1, 0.05])
    path = (np.arange(L)[:, None] * D + np.array([0.3, 0.1, -0.2]))[None]
    timing = ref.time(path, None, 2.0, 5.0)
    T = int(math.ceil(timing["duration"][0] / 0.01)) + 3
    q, v = ref.sample(path, None, timing, 0.01, T)
    rel = (q[0] - path[0, 0]) / D
    assert np.max(np.abs(rel - rel[:, :1])) <= 1e-12 * (L - 1)
    assert np.all(np.diff(rel[:, 0]) >= 0.0) and rel[0, 0] == 0.0
    assert _same(q[0, -1], path[0, -1]) and np.all(v[0, -2:] == 0.0)
    assert np.all(np.abs(v[0]) <= 2.0 * (1 + 1e-9))


def test_samples_at_the_waypoints_and_past_the_end(ref):
    rng = np.random.default_rng(9)
    n, L = 7, 16
    paths = tu.gentle_paths(rng, 3, L, n)
    paths[2, 4, 1] = math.nan
    timing = ref.time(paths, None, 2.0, 5.0)
    assert list(timing["status"]) == [0, 0, 3]
    for p in range(2):
        for i in range(1, L - 1):
            # dt = t_i and k = 1: tau = t_i exactly
            one = {k: v[p:p + 1] for k, v in timing.items()}
            q, v = ref.sample(paths[p:p + 1], None, one, timing["times"][p, i], 2)
            assert _same(q[0, 1], paths[p, i]) and _same(v[0, 1], timing["velocities"][p, i]), (p, i)
            assert _same(q[0, 0], paths[p, 0])
    q, v = ref.sample(paths, None, timing, float(np.nanmax(timing["duration"])), 3)
    assert _same(q[:2, 1], paths[:2, -1]) and _same(q[:2, 2], paths[:2, -1]) and np.all(v[:2, 1:] == 0.0)
    assert np.all(tu.bits(q[2]) == tu.bits(np.broadcast_to(paths[2, 0], (3, n)))) and np.all(v[2] == 0.0)


# ---- the URDF's velocity limits ------------------------------------------------------------------------------------

def test_velocity_limits_of_the_urdf(tmp_path):
    import re
    from optik_amd import Robot
    for name in ("panda", "ur10"):
        path, base, ee = ROBOT_SPECS[name]
        robot = Robot.from_urdf_file(path, base, ee)
        text = open(path).read()
        want = []
        for jm in re.finditer(r"<joint\b[^>]*type=\"revolute\".*?</joint>", text, re.S):
            want.append(float(re.search(r"velocity=\"([^\"]+)\"", jm.group(0)).group(1)))
        got = robot.velocity_limits()
        assert len(got) == robot.num_positions() and list(got) == want[:len(got)], (name, got, want)
    assert Robot.from_urdf_file(*ROBOT_SPECS["panda"]).velocity_limits()[0] == 2.175
    assert Robot.from_urdf_file(*ROBOT_SPECS["ur10"]).velocity_limits()[0] == 2.16
    text = open(os.path.join(TEST_ROBOTS, "arm8.urdf")).read()
    bare = tmp_path / "bare.urdf"
    bare.write_text(re.sub(r"\s+velocity=\"[^\"]*\"", "", text))
    robot = Robot.from_urdf_file(str(bare), "l0", "l9")
    assert np.all(np.isinf(robot.velocity_limits())) and len(robot.velocity_limits()) == 8
    zero = tmp_path / "zero.urdf"
    zero.write_text(re.sub(r"velocity=\"[^\"]*\"", "velocity=\"0\"", text))
    assert np.all(np.isinf(Robot.from_urdf_file(str(zero), "l0", "l9").velocity_limits()))
