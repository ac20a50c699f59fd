"""CPU-only: the arithmetic of IK into pose regions (optik_amd/csrc/region_measure.hpp, built for the host) against the
host build of constraint_measure.hpp applied to [x0 | oracle seeds], the key rule in numpy, the precondition of the GPU
tests' regions, the PoseConstraint constructors for regions and the Python validation."""
import math

import numpy as np
import pytest

import constraint_util as cu
import region_util as gu
from constraint_util import PROJECTED, bits
from selection_util import solutions_ref


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return gu.build_region(str(tmp_path_factory.mktemp("region_measure")))


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return cu.build_constraint(str(tmp_path_factory.mktemp("region_constraint")))


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))


def _scene(oracle, chains, name):
    d, oc = chains[name]
    ref7 = np.asarray(oracle.fk(oc, gu.mid_config(d))[1])
    return d, oc, gu.make_regions(ref7), gu.x0_rows(d)


@pytest.fixture(scope="module")
def host_rows(ref, oracle, chains):
    """name -> (scene, {(begin, mode): rows}) computed once and left unchanged."""
    out = {}
    for name in gu.ROBOTS:
        d, oc, regs, x0 = _scene(oracle, chains, name)
        rows = {(b, m): ref.restarts(d, [gu.region_row(c) for c in regs], x0, b, gu.R, gu.TOL, mode=m, **gu.PROJECT)
                for b in (0, 5) for m in (gu.MODE_QUALITY, gu.MODE_SPEED)}
        out[name] = ((d, oc, regs, x0), rows)
    return out


@pytest.mark.parametrize("name", gu.ROBOTS)
@pytest.mark.parametrize("begin", (0, 5))
def test_rows_equal_the_projection_of_x0_and_the_oracle_seeds(cref, oracle, host_rows, name, begin):
    (d, oc, regs, x0), rows = host_rows[name]
    got = rows[(begin, gu.MODE_QUALITY)]
    for t, c in enumerate(regs):
        starts = np.array([x0[t] if i == 0 else oracle.restart_seed(oc, i) for i in range(begin, begin + gu.R)])
        want = cref.project(d, c, starts, gu.TOL, **gu.PROJECT)
        sl = slice(t * gu.R, (t + 1) * gu.R)
        assert _same(got["x"][sl], want["x"]) and _same(got["v"][sl], want["v"]), (name, t)
        assert np.array_equal(got["status"][sl], want["status"]), (name, t)
        assert np.array_equal(got["iterations"][sl], want["iterations"]), (name, t)


@pytest.mark.parametrize("name", gu.ROBOTS)
def test_keys_equal_the_numpy_restatement(host_rows, name):
    (d, _, _, x0), rows = host_rows[name]
    for (begin, mode), got in rows.items():
        index = np.tile(np.arange(begin, begin + gu.R), gu.T)
        want = gu.np_keys(got["x"], np.repeat(x0, gu.R, axis=0), got["status"], index, mode)
        assert _same(got["key"], want), (name, begin, mode)
        # x, violation, status and iterations do not depend on the mode
        other = rows[(begin, gu.MODE_QUALITY)]
        assert _same(got["x"], other["x"]) and np.array_equal(got["status"], other["status"])


@pytest.mark.parametrize("name", gu.ROBOTS)
def test_keep_sets_the_key_to_inf_where_the_measured_violation_exceeds_its_tol(ref, cref, host_rows, name):
    (d, _, regs, x0), rows = host_rows[name]
    base = rows[(0, gu.MODE_QUALITY)]
    keep, ktol = cu.upright_constraint(regs[0].ref7, 0.3), 0.05
    got = ref.restarts(d, [gu.region_row(c) for c in regs], x0, 0, gu.R, gu.TOL, mode=gu.MODE_QUALITY,
                       keep=(keep, ktol), **gu.PROJECT)
    v = cref.measure(d, keep, base["x"])["v"]
    want = np.where(v <= ktol, base["key"], np.inf)
    assert _same(got["key"], want), name
    assert _same(got["x"], base["x"]) and np.array_equal(got["status"], base["status"])
    dropped = np.isfinite(base["key"]) & ~np.isfinite(got["key"])
    assert dropped.any() and np.isfinite(got["key"]).any(), name  # (the case does both)


@pytest.mark.parametrize("name", gu.ROBOTS)
def test_the_gpu_tests_regions_have_enough_projected_and_distinct_rows(host_rows, name):
    """The precondition of tests/test_gpu_ik_region.py, on the reference alone."""
    _, rows = host_rows[name]
    for begin in (0, 5):
        got = rows[(begin, gu.MODE_QUALITY)]
        for t in range(gu.T):
            sl = slice(t * gu.R, (t + 1) * gu.R)
            assert int((got["status"][sl] == PROJECTED).sum()) >= 4, (name, begin, t)
            assert len(solutions_ref(got["key"][sl], got["x"][sl].T, begin, gu.K, gu.MIN_DIST)) >= 2, (name, begin, t)


def test_a_nan_region_gives_failed_rows_and_a_free_box_zero_iterations(ref, oracle, chains):
    d, oc, regs, x0 = _scene(oracle, chains, "panda")
    bad = gu.region_row(regs[0])
    bad[1] = math.nan
    free = gu.region_row(cu.free_constraint(regs[0].ref7))
    got = ref.restarts(d, [bad, free], x0[:2], 0, 9, gu.TOL, mode=gu.MODE_SPEED, **gu.PROJECT)
    assert (got["status"][:9] == cu.FAILED).all() and np.isinf(got["key"][:9]).all()
    assert (got["status"][9:] == PROJECTED).all() and (got["iterations"][9:] == 0).all()
    assert np.array_equal(got["key"][9:], np.arange(9.0))
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    starts = np.array([x0[1]] + [oracle.restart_seed(oc, i) for i in range(1, 9)])
    assert _same(got["x"][9:], np.clip(starts, lb, ub))


def test_constructors_give_the_stated_boxes():
    from optik_amd import PoseConstraint
    pose = np.eye(4)
    pose[:3, 3] = [0.4, 0.1, 0.5]
    inf = math.inf
    c = PoseConstraint.position_only(pose)
    assert np.array_equal(c.lo, [0, 0, 0, -inf, -inf, -inf]) and np.array_equal(c.hi, [0, 0, 0, inf, inf, inf])
    c = PoseConstraint.position_only(pose, 0.02)
    assert np.array_equal(c.lo, [-0.02] * 3 + [-inf] * 3) and np.array_equal(c.hi, [0.02] * 3 + [inf] * 3)
    for k, axis in enumerate("xyz"):
        c = PoseConstraint.axis_free(pose, axis)
        lo, hi = np.zeros(6), np.zeros(6)
        lo[3 + k], hi[3 + k] = -inf, inf
        assert np.array_equal(c.lo, lo) and np.array_equal(c.hi, hi), axis
    c = PoseConstraint.axis_free(pose, pos_tol=0.01, rot_tol=0.1)
    assert np.array_equal(c.lo, [-0.01] * 3 + [-0.1, -0.1, -inf]) and np.array_equal(c.hi, [0.01] * 3 + [0.1, 0.1, inf])
    c = PoseConstraint.around(pose, 0.01, 0.2)
    assert np.array_equal(c.lo, [-0.01] * 3 + [-0.2] * 3) and np.array_equal(c.hi, [0.01] * 3 + [0.2] * 3)
    assert np.array_equal(c.ref7, [0.4, 0.1, 0.5, 0, 0, 0, 1])
    for bad in (lambda: PoseConstraint.axis_free(pose, "w"), lambda: PoseConstraint.position_only(pose, -1.0),
                lambda: PoseConstraint.around(pose, 0.1, math.nan), lambda: PoseConstraint.axis_free(pose, rot_tol=inf)):
        with pytest.raises(ValueError):
            bad()


def test_python_validation_raises_before_any_device_work():
    """region_rows, keep_arrays and the argument checks of Robot.ik_region_batch_arrays, none of which needs a GPU."""
    import types
    from optik_amd import PoseConstraint
    from optik_amd import _native as nat
    from optik_amd.constraint import keep_arrays, region_rows
    good = PoseConstraint.position_only(np.eye(4), 0.02)
    rows = region_rows(good, 3)
    assert rows.shape == (3, 19) and np.array_equal(rows[2], np.concatenate([good.ref7, good.lo, good.hi]))
    assert region_rows([good, good], 2).shape == (2, 19)
    with pytest.raises(ValueError, match="sequence of T = 3"):
        region_rows([good, good], 3)
    nan_ref = types.SimpleNamespace(ref7=np.array([0, 0, math.nan, 0, 0, 0, 1.0]), lo=good.lo, hi=good.hi)
    with pytest.raises(ValueError, match="region 1: .*finite"):
        region_rows([good, nan_ref], 2)
    not_unit = types.SimpleNamespace(ref7=np.array([0, 0, 0, 0, 0, 0, 1.1]), lo=good.lo, hi=good.hi)
    with pytest.raises(ValueError, match="region 0: .*unit norm"):
        region_rows(not_unit, 1)
    crossed = types.SimpleNamespace(ref7=good.ref7, lo=np.ones(6), hi=np.zeros(6))
    with pytest.raises(ValueError, match="region 0: .*lo <= hi"):
        region_rows([crossed], 1)
    assert keep_arrays(None) is None and keep_arrays((good, 0.05))[3] == 0.05
    for bad in (good, (good,), (good, -1.0), (good, math.nan), (1.0, 0.1), (crossed, 0.1)):
        with pytest.raises(ValueError):
            keep_arrays(bad)
    for bad in (0, nat.MAX_SOLUTION_RESTARTS + 1, 2.5, True):
        with pytest.raises(ValueError):
            nat.check_region_restarts(bad)
    assert nat.check_region_restarts(256) == 256
    for bad_k in (0, 257):
        with pytest.raises(ValueError):
            nat.check_solutions_args(bad_k, 0.1)
