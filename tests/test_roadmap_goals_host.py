"""CPU-only: the rules of goal-set planning (optik_amd/csrc/roadmap_goals_measure.hpp, built with g++).  The serial
reference against roadmap_measure.hpp's plan_reference goal by goal, as the theorem of DESIGN.md section 5.25 says, on
random graphs; G = 1 against the single-goal reference in every output; the prescribed ties, NaN and Lmax cases
against hand-written expectations; the exported symbols and the host-side refusals."""
import ctypes as C

import numpy as np
import pytest

import roadmap_goals_util as gu
import roadmap_util as ru


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ru.build_roadmap_ref(str(tmp_path_factory.mktemp("roadmap_measure")))


@pytest.fixture(scope="module")
def goals(tmp_path_factory):
    return gu.build_goals_ref(str(tmp_path_factory.mktemp("roadmap_goals_measure")))


def _per_goal(ref, g, q, L):
    """The single-goal plans to the goals that at least one query counts."""
    return {j: ref.query(g, gu.single(q, j), L) for j in range(int(q["gcount"].max()))}


def test_theorem_on_random_graphs(ref, goals):
    rng = np.random.default_rng(2525)
    L = 16
    finite = unique = 0
    seen = set()
    for N, k, Q in ((64, 4, 48), (200, 6, 48), (1100, 8, 24)):
        g = ru.random_graph(rng, N, k)
        for G in (1, 3, 8, 16):
            for kg in (1, 4):
                q = gu.random_goal_queries(rng, g, Q, 3, kg, G)
                assert q["gcount"].min() == 0 and q["gcount"].max() == G
                res = goals.query(g, q, L)
                f, u = gu.assert_theorem((N, G, kg), res, _per_goal(ref, g, q, L), q)
                finite, unique = finite + f, unique + u
                seen |= set(res["status"].tolist())
    # the theorem's third part speaks of a unique cheapest goal: the draws must not make it vacuous -- at least half
    # of the 8 * (48 + 48 + 24) = 960 queries have a route, and at least 90 % of those a unique cheapest goal
    assert 2 * finite >= 960 and 10 * unique >= 9 * finite, (finite, unique)
    assert {ru.FOUND, ru.NO_ROUTE, ru.TOO_LONG} <= seen


def test_theorem_where_routes_are_rare(ref, goals):
    rng = np.random.default_rng(2526)
    g = ru.random_graph(rng, 200, 6, p_blocked=0.7)
    q = gu.random_goal_queries(rng, g, 64, 3, 4, 4, p_direct=0.0, p_inf=0.7)
    res = goals.query(g, q, 16)
    gu.assert_theorem("rare", res, _per_goal(ref, g, q, 16), q)
    counted = q["gcount"] > 0
    assert (res["status"][counted] == ru.NO_ROUTE).any() and (res["status"][counted] == ru.FOUND).any()


def test_one_goal_equals_the_single_goal_reference(ref, goals):
    rng = np.random.default_rng(2527)
    for N, k in ((64, 4), (200, 6), (1100, 8)):
        g = ru.random_graph(rng, N, k)
        for kg in (1, 4):
            single = ru.queries_for(rng, g, 32, 3, kg)
            res, one = goals.query(g, gu.stack_goals([single]), 16), ref.query(g, single, 16)
            for key in ("status", "len"):
                assert np.array_equal(res[key], one[key]), (N, kg, key)
            for key in ("cost", "path", "d"):
                assert np.array_equal(gu.bits(res[key]), gu.bits(one[key])), (N, kg, key)
            assert np.array_equal(res["which"], np.where(one["status"] == ru.FOUND, 0, -1)), (N, kg)
    # ... and on roadmap_util's own synthetic cases, NaN queries and Lmax = 2 among them
    for name, g, single, L in ru.synthetic_cases():
        res, one = goals.query(g, gu.stack_goals([single]), L), ref.query(g, single, L)
        for key in ("status", "len"):
            assert np.array_equal(res[key], one[key]), (name, key)
        for key in ("cost", "path", "d"):
            assert np.array_equal(gu.bits(res[key]), gu.bits(one[key])), (name, key)


def test_prescribed_cases(goals):
    names = set()
    for name, g, q, L, expect in gu.prescribed_cases():
        gu.assert_prescribed(name, goals.query(g, q, L), g, q, L, expect)
        names.add(name)
    assert len(names) == len(gu.prescribed_cases())


def test_uncounted_goals_are_not_read(goals):
    """Whatever stands past gcount -- NaN, or other numbers -- the plan is the same."""
    rng = np.random.default_rng(2528)
    g = ru.random_graph(rng, 64, 4)
    q = gu.random_goal_queries(rng, g, 32, 3, 4, 8)
    other = {k: v.copy() for k, v in q.items()}
    for j in range(8):
        gone = q["gcount"] <= j
        other["goals"][j][:, gone] = 0.5
        other["gw"][j][:, gone] = 0.0
        other["gidx"][j][:, gone] = 1
        other["direct"][j][gone] = 0.0
    a, b = goals.query(g, q, 16), goals.query(g, other, 16)
    for key in a:
        assert np.array_equal(gu.bits(a[key]) if a[key].dtype == np.float64 else a[key],
                              gu.bits(b[key]) if b[key].dtype == np.float64 else b[key]), key
    # a count outside 0 .. G is clamped
    wide = {k: v.copy() for k, v in q.items()}
    full = q["gcount"] == 8
    wide["gcount"][full] = 99
    wide["gcount"][q["gcount"] == 0] = -3
    c = goals.query(g, wide, 16)
    assert np.array_equal(c["status"], a["status"]) and np.array_equal(gu.bits(c["cost"]), gu.bits(a["cost"]))


@pytest.fixture(scope="module")
def lib():
    from optik_amd import build
    build.build()
    from optik_amd import _native
    return _native.lib()


def test_symbols_and_argument_rules_on_the_host(lib):
    from optik_amd import _native as nat
    assert hasattr(lib, "optik_hip_roadmap_query_goals")
    assert nat.ROADMAP_MAX_GOALS == gu.MAX_GOALS
    assert nat.check_roadmap_goals(1) == 1 and nat.check_roadmap_goals(16) == 16
    for bad in (0, 17, -1, 2.5, True):
        with pytest.raises(ValueError):
            nat.check_roadmap_goals(bad)
    # the kernel layer refuses a missing chain before any device work
    assert lib.optik_hip_roadmap_query_goals(None, None, 4, None, None, 4, None, None, None, 2, 0, None, None, 4, None,
                                             None, 4, None, 8, None, None, None, None, None, None, None, None) != 0
    robot = ru.wall_scene()["robot"]
    assert hasattr(robot._L, "optik_robot_roadmap_plan_goals")
    n = robot.num_positions()
    starts, goals3 = np.zeros((2, n)), np.zeros((2, 3, n))
    # the host API refuses a null argument and G out of range before it asks for a device
    assert robot._L.optik_robot_roadmap_plan_goals(None, None, None, None, 3, 2, 8, None, None, None, None, None) == -1
    dp = starts.ctypes.data_as(C.POINTER(C.c_double))
    gp = goals3.ctypes.data_as(C.POINTER(C.c_double))
    for G in (0, 17):
        assert robot._L.optik_robot_roadmap_plan_goals(robot._h, dp, gp, None, G, 2, 8, None, None, None, None,
                                                       None) == -1
    assert robot._L.optik_robot_roadmap_plan_goals(robot._h, dp, None, None, 3, 2, 8, None, None, None, None,
                                                   None) == -1
    # the Robot layer: shapes, G, max_waypoints, and the lazy roadmap
    with pytest.raises(ValueError):
        robot.plan_to_goals(starts, np.zeros((2, 17, n)))
    with pytest.raises(ValueError):
        robot.plan_to_goals(starts, np.zeros((2, 0, n)))
    with pytest.raises(ValueError):
        robot.plan_to_goals(starts, np.zeros((3, 3, n)))
    with pytest.raises(ValueError):
        robot.plan_to_goals(starts, goals3, counts=[1, 2, 3])
    with pytest.raises(ValueError):
        robot.plan_to_goals(starts, goals3, max_waypoints=65)
    robot._roadmap_lazy = True  # (what build_roadmap(lazy=True) records)
    for call in (lambda: robot.plan_to_goals(starts, goals3),
                 lambda: robot.plan_to_poses(None, starts, np.zeros((2, 4, 4)), k=3)):
        with pytest.raises(RuntimeError, match="lazy") as err:
            call()
        assert "plan_paths" in str(err.value)
