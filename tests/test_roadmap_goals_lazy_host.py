"""CPU-only: the rules of goal-set planning on lazy roadmaps (optik_amd/csrc/roadmap_goals_lazy_measure.hpp, built with
g++).  The serial reference against roadmap_goals_measure.hpp's plan over the eager graph, as the theorem of DESIGN.md
section 5.34 says; against roadmap_lazy_measure.hpp's loop for G = 1; with the freezing rule applied against without,
on draws that are asserted to exercise it; the prescribed graphs; the exported symbols and the host-side refusals."""
import math

import numpy as np
import pytest

import roadmap_goals_lazy_util as glu
import roadmap_goals_util as gu
import roadmap_lazy_util as lu
import roadmap_util as ru


@pytest.fixture(scope="module")
def goals(tmp_path_factory):
    return gu.build_goals_ref(str(tmp_path_factory.mktemp("roadmap_goals_measure")))


@pytest.fixture(scope="module")
def lazy(tmp_path_factory):
    return lu.build_lazy_ref(str(tmp_path_factory.mktemp("roadmap_lazy_measure")))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return glu.build_goals_lazy_ref(str(tmp_path_factory.mktemp("roadmap_goals_lazy_measure")))


@pytest.fixture(scope="module")
def random_runs(ref):
    """[(name, graph, truth, queries, Lmax, the specification's run at 4096 rounds)]: computed once."""
    return [(name, g, t, q, L, ref.plan(g, t, q, L, glu.MAX_ROUNDS)) for name, g, t, q, L in glu.random_cases()]


def test_lazy_goal_plan_equals_the_eager_plan(goals, random_runs):
    seen = set()
    for name, g, truth, q, L, res in random_runs:
        eager = goals.query(glu.eager_graph(g, truth), q, L)
        glu.assert_theorem(name, res, eager)
        seen |= set(res["status"].tolist())
        # the final lazy graph contains the eager graph
        assert np.all(res["w"] <= lu.eager_weights(g, truth)), name
        assert res["rounds"] <= res["checked"], name
    assert {ru.FOUND, ru.NO_ROUTE} <= seen and glu.UNSETTLED not in seen


def test_the_draws_exercise_the_loop(random_runs):
    traces = {}
    for name, g, truth, q, L, res in random_runs:
        traces.setdefault(g["nodes"].shape[1], []).append(glu.trace_of(res))
        print(name, "passes", res["rounds"] + 1, "checked", res["checked"], "trace", glu.trace_of(res))
    assert set(traces) == {N for N, _ in glu.RANDOM_SIZES}
    glu.assert_draws_exercise_the_loop(traces)


def test_freezing_changes_nothing(ref, random_runs):
    """The freezing rule applied (what the device does with skip_settled) against every query in every pass: every
    output, the state and both counters, on the same draws; and a query is frozen once and for all."""
    for name, g, truth, q, L, res in random_runs:
        frozen = ref.plan(g, truth, q, L, glu.MAX_ROUNDS, freeze=True)
        glu.assert_same_plan(name, frozen, res)
        assert np.array_equal(frozen["frozen_after"], res["frozen_after"]), name
        for rounds in (0, 1, 2):
            glu.assert_same_plan((name, rounds), ref.plan(g, truth, q, L, rounds, freeze=True),
                                 ref.plan(g, truth, q, L, rounds))
    for name, (g, truth, q, L) in glu.prescribed_cases().items():
        for rounds in (0, 1, 8):
            glu.assert_same_plan((name, rounds), ref.plan(g, truth, q, L, rounds, freeze=True),
                                 ref.plan(g, truth, q, L, rounds))


def test_one_goal_is_the_single_goal_loop(ref, lazy):
    for name, g, truth, q, L, random in lu.lazy_cases():
        Q = q["start"].shape[1]
        one = gu.stack_goals([q])
        for rounds in (1, glu.MAX_ROUNDS):
            a, b = ref.plan(g, truth, one, L, rounds), lazy.plan(g, truth, q, L, rounds)
            for key in ("status", "len", "cost", "path", "w", "verdict"):
                assert glu.same_or_nan(a[key], b[key]), (name, rounds, key)
            assert (a["rounds"], a["checked"]) == (b["rounds"], b["checked"]), (name, rounds)
            assert np.array_equal(a["which"], np.where(a["status"] == ru.FOUND, 0, -1)), (name, rounds, Q)


def _expect(res, j, status, length, cost, which):
    assert (res["status"][j], res["len"][j], res["which"][j]) == (status, length, which), (
        res["status"], res["len"], res["which"])
    assert res["cost"][j] == cost or (math.isnan(cost) and math.isnan(res["cost"][j])), res["cost"]


def _rows(*rows):
    return np.stack([np.asarray(r, dtype=np.float64) for r in rows])


def test_detour_moves_the_answer_to_the_other_goal(ref, goals):
    g, truth, q, L = glu.prescribed_cases()["detour_two_goals"]
    start, goal0, goal1 = q["start"][:, 0], q["goals"][0, :, 0], q["goals"][1, :, 0]
    # no check: the route by node 2 to goal 0, 0.25 + 1.0 + 0.25, unchecked -- status 4, goal 0 behind the start
    r0 = ref.plan(g, truth, q, L, 0)
    _expect(r0, 0, glu.UNSETTLED, 2, 1.5, -1)
    assert (r0["rounds"], r0["checked"]) == (0, 0) and np.all(r0["verdict"][g["nbr"] >= 0] == lu.UNKNOWN)
    assert np.array_equal(r0["path"][:, 0], _rows(start, *[goal0] * (L - 1)))
    # one check: 3 -> 2 is blocked; the route by node 1 to goal 1, 0.25 + 1.5 + 0.25, still unchecked
    r1 = ref.plan(g, truth, q, L, 1)
    _expect(r1, 0, glu.UNSETTLED, 2, 2.0, -1)
    assert (r1["rounds"], r1["checked"]) == (1, 1) and r1["verdict"][0, 3] == lu.BLOCKED and r1["w"][0, 3] == math.inf
    assert np.array_equal(r1["path"][:, 0], _rows(start, *[goal0] * (L - 1)))
    for rounds in (2, 3, glu.MAX_ROUNDS):
        r = ref.plan(g, truth, q, L, rounds)
        _expect(r, 0, ru.FOUND, 4, 2.0, 1)
        assert (r["rounds"], r["checked"]) == (2, 2) and r["verdict"][1, 3] == lu.FREE
        assert np.array_equal(r["path"][:, 0], _rows(start, g["nodes"][:, 3], g["nodes"][:, 1], *[goal1] * (L - 3)))
        assert r["frozen_after"][0] == 3
        glu.assert_theorem("detour", r, goals.query(glu.eager_graph(g, truth), q, L))
    # the verdicts are kept: the same plan again checks nothing
    again = ref.plan(g, truth, q, L, 0, state=(r["w"], r["verdict"]))
    _expect(again, 0, ru.FOUND, 4, 2.0, 1)
    assert again["checked"] == 0


def test_twin_slots_take_the_lowest(ref):
    cases = glu.prescribed_cases()
    g, truth, q, L = cases["twin_slots"]
    r = ref.plan(g, truth, q, L, 8)
    # 2 -> 1 by slot 1: slot 0 costs more, slot 2 is the same motion in a later slot
    _expect(r, 0, ru.FOUND, 5, 2.0, 0)
    assert r["checked"] == 2 and r["verdict"][:, 2].tolist() == [lu.UNKNOWN, lu.FREE, lu.UNKNOWN]
    g, truth, q, L = cases["twin_slots_blocked"]
    r = ref.plan(g, truth, q, L, 8)
    _expect(r, 0, ru.FOUND, 5, 2.0, 0)
    assert (r["rounds"], r["checked"]) == (2, 3) and r["verdict"][:, 2].tolist() == [lu.UNKNOWN, lu.BLOCKED, lu.FREE]


def test_a_too_long_query_stays_live(ref, goals):
    """Query 0's cheap route needs 6 waypoints at Lmax 5: TOO_LONG, cost 2.0, nothing of it walked.  Query 1's route
    holds 1 -> 0, which is blocked: after that check query 0's cheapest route is the long jump 3 -> 0, 4 waypoints,
    and it is FOUND -- had pass 1 frozen it, it would have stayed TOO_LONG."""
    g, truth, q, L = glu.prescribed_cases()["too_long_then_found"]
    r0 = ref.plan(g, truth, q, L, 0)
    _expect(r0, 0, ru.TOO_LONG, 2, 2.0, -1)
    _expect(r0, 1, glu.UNSETTLED, 2, 1.5, -1)
    for freeze in (False, True):
        r = ref.plan(g, truth, q, L, 8, freeze=freeze)
        _expect(r, 0, ru.FOUND, 4, 5.5, 0)
        _expect(r, 1, ru.NO_ROUTE, 2, math.inf, -1)
        assert (r["rounds"], r["checked"]) == (2, 3)
        assert r["verdict"][0, 1] == lu.BLOCKED and r["verdict"][0, 2] == lu.FREE and r["verdict"][1, 3] == lu.FREE
        assert r["verdict"][0, 3] == lu.UNKNOWN
        assert r["frozen_after"].tolist() == [3, 2]
    glu.assert_theorem("too_long_then_found", r, goals.query(glu.eager_graph(g, truth), q, L))


def test_counts_nan_and_short_lmax(ref):
    cases = glu.prescribed_cases()
    g, truth, q, L = cases["no_goals"]
    r = ref.plan(g, truth, q, L, 8)
    _expect(r, 0, ru.NO_ROUTE, 2, math.inf, -1)
    assert r["checked"] == 0 and np.array_equal(r["path"][:, 0], _rows(*[q["start"][:, 0]] * L))
    assert r["frozen_after"][0] == 1
    g, truth, q, L = cases["nan_counted"]
    r = ref.plan(g, truth, q, L, 8)
    _expect(r, 0, ru.QUERY_NAN, 2, math.nan, -1)
    assert r["checked"] == 0 and r["frozen_after"][0] == 1
    # the same NaN past the count is not read: the detour's answer with goal 0 alone -- behind the blocked 3 -> 2
    # no route is left
    g, truth, q, L = cases["nan_uncounted"]
    r = ref.plan(g, truth, q, L, 8)
    _expect(r, 0, ru.NO_ROUTE, 2, math.inf, -1)
    assert (r["rounds"], r["checked"]) == (1, 1)
    # Lmax 2: only a direct motion fits, and only if it is the cheapest way (1.0 against 1.5 by the graph)
    g, truth, q, L = cases["lmax2_direct"]
    _expect(ref.plan(g, truth, q, L, 8), 0, ru.FOUND, 2, 1.0, 1)
    g, truth, q, L = cases["lmax2_none"]
    r = ref.plan(g, truth, q, L, 8)
    _expect(r, 0, ru.TOO_LONG, 2, 1.5, -1)
    assert r["checked"] == 0
    # Lmax 3: start, one node, goal -- node 1 has a start link (1.0) and goal 1's link (0.25); no graph hop, no check
    g, truth, q, L = cases["lmax3_one_node"]
    r = ref.plan(g, truth, q, L, 8)
    _expect(r, 0, ru.FOUND, 3, 1.25, 1)
    assert r["checked"] == 0 and np.all(r["verdict"][g["nbr"] >= 0] == lu.UNKNOWN)
    assert np.array_equal(r["path"][:, 0], _rows(q["start"][:, 0], g["nodes"][:, 1], q["goals"][1, :, 0]))


def test_reset_forgets_the_verdicts(ref):
    g, truth, q, L = glu.prescribed_cases()["detour_two_goals"]
    first = ref.plan(g, truth, q, L, 8)
    assert first["cost"][0] == 2.0 and first["which"][0] == 1
    free = lu.all_free(g)
    kept = ref.plan(g, free, q, L, 8, state=(first["w"], first["verdict"]))
    assert kept["cost"][0] == 2.0 and kept["checked"] == 0          # without a reset the old verdict stands
    fresh = ref.plan(g, free, q, L, 8)
    _expect(fresh, 0, ru.FOUND, 4, 1.5, 0)
    assert fresh["checked"] == 1 and fresh["verdict"][0, 3] == lu.FREE


# ---- the library: symbols and the refusals that need no device -----------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from optik_amd import build
    build.build()
    from optik_amd import _native
    return _native.lib()


def test_symbols_are_exported(lib):
    for name in ("optik_hip_roadmap_lazy_plan_goals", "optik_hip_roadmap_lazy_plan_goals_from_flags",
                 "optik_robot_roadmap_plan_goals_lazy"):
        assert hasattr(lib, name), name
    from optik_amd.device import HipChain
    from optik_amd.robot import Robot
    for name in ("roadmap_plan_goals_lazy", "roadmap_plan_goals_lazy_from_flags", "roadmap_plan_poses_lazy",
                 "roadmap_plan_region_lazy"):
        assert hasattr(HipChain, name), name
    for name in ("plan_to_goals_lazy", "plan_to_poses_lazy", "plan_to_region_lazy"):
        assert hasattr(Robot, name), name
    assert "lazy" in Robot._LAZY_GOALS_MSG and "plan_paths" in Robot._LAZY_GOALS_MSG
    assert "plan_to_goals_lazy" in Robot._LAZY_GOALS_MSG


def test_argument_rules_on_the_host(lib):
    # the kernel layer refuses a missing chain before any device work
    assert lib.optik_hip_roadmap_lazy_plan_goals(None, None, None, 4, None, None, None, 4, 0.1, None, None, None, 2, 0,
                                                 None, None, 4, None, None, 4, None, 8, 1, 1, None, None, None, None,
                                                 None, None, None, None) != 0
    assert lib.optik_hip_roadmap_lazy_plan_goals_from_flags(None, None, 4, None, None, None, None, 4, None, None, None,
                                                            None, None, 2, 0, None, None, 4, None, None, 4, None, 8, 1,
                                                            1, None, None, None, None, None, None, None, None) != 0
    # ... and the host layer a missing robot
    assert lib.optik_robot_roadmap_plan_goals_lazy(None, None, None, None, 2, 0, 8, 1, None, None, None, None, None,
                                                   None, None) != 0


def test_robot_refuses_an_eager_roadmap_and_names_the_eager_call():
    """Robot.plan_to_goals_lazy looks at the kind of roadmap the robot holds before it touches the device."""
    from optik_amd.robot import Robot
    robot = Robot.__new__(Robot)
    robot._roadmap_lazy = False
    with pytest.raises(RuntimeError, match="plan_to_goals"):
        robot.plan_to_goals_lazy(np.zeros((1, 7)), np.zeros((1, 2, 7)))
