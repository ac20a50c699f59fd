"""CPU-only: the rules of the tree planner with a goal set (optik_amd/csrc/rrt_goals_measure.hpp, built with g++).  The
serial reference plan_goals_reference against the closed-form obstacles of rrt_util in a 2-joint space: G = 1 against
plan_reference in every field and both trees; goal sets with unreachable members; rule 0 case by case and its tie;
what lies past the count; the caps; the exported symbols and the host-side refusals."""
import math

import numpy as np
import pytest

import roadmap_util as ru
import rrt_goals_util as gu
import rrt_util as tu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return gu.build_rrt_goals_ref(str(tmp_path_factory.mktemp("rrt_goals_measure")))


@pytest.fixture(scope="module")
def ref1(tmp_path_factory):
    return tu.build_rrt_ref(str(tmp_path_factory.mktemp("rrt_measure")))


def plan(ref, free, start, goals, count=None, I=400, step=0.3, M=256, Lmax=64, seed=5):
    orc = tu.Oracle2(free)
    lo, hi = tu.LIMITS2
    goals = np.asarray(goals, dtype=np.float64)
    res = ref.plan(lo, hi, np.asarray(start, dtype=np.float64), goals, len(goals) if count is None else count,
                   tu.samples2(I, seed), step, M, Lmax, orc.config_free, orc.motions_free)
    return res, orc


def same_bits(a, b, keys):
    for key in keys:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        if x.dtype == np.float64:
            assert np.array_equal(ru.bits(x), ru.bits(y)), key
        else:
            assert np.array_equal(x, y), key


def wall_and_disc(q):
    """rrt_util's wall without a gap, and its disc moved to (-1, 0): a goal between the two is hidden from a start
    left of the disc, a goal right of the wall is out of reach."""
    return tu.wall(q) and tu.disc(np.asarray(q) + np.array([1.0, 0.0]))


FIELDS = ("status", "len", "iters", "nodes", "junction", "cost", "path", "conf", "parent")


@pytest.mark.parametrize("free, start, goal, kw", [
    (tu.disc, [-1.5, 0.0], [1.5, 0.1], {}),                      # found through the trees
    (tu.wall_with_gap, [-1.5, -1.0], [1.5, -1.2], {}),
    (tu.wall_with_gap, [-1.5, -1.0], [1.5, -1.2], dict(Lmax=2)),  # status 2
    (tu.disc, [-1.5, 1.0], [1.5, 1.2], {}),                      # direct
    (tu.disc, [0.1, 0.1], [1.5, 1.2], {}),                       # the start blocked
    (tu.disc, [-1.5, 0.0], [0.1, 0.1], {}),                      # the goal blocked
    (tu.disc, [-1.5, 0.0], [1.5, math.nan], {}),                 # status 3
    (tu.disc, [math.inf, 0.0], [1.5, 0.0], {}),
    (tu.wall, [-1.5, -1.0], [1.5, -1.2], dict(I=300, M=40)),     # status 1 after all the iterations, a full tree
    (tu.wall_with_gap, [-1.5, -1.0], [1.5, -1.2], dict(M=2))])
def test_one_goal_is_plan_reference_bit_for_bit(ref, ref1, free, start, goal, kw):
    got, _ = plan(ref, free, start, [goal], **kw)
    orc = tu.Oracle2(free)
    lo, hi = tu.LIMITS2
    a = dict(I=400, step=0.3, M=256, Lmax=64, seed=5)
    a.update(kw)
    want = ref1.plan(lo, hi, np.array(start, dtype=np.float64), np.array(goal, dtype=np.float64),
                     tu.samples2(a["I"], a["seed"]), a["step"], a["M"], a["Lmax"], orc.config_free, orc.motions_free)
    same_bits(got, want, FIELDS)
    assert got["which"] == (0 if want["status"] == tu.FOUND else -1)


def test_the_route_ends_in_a_reachable_goal(ref):
    start = np.array([-1.8, 0.0])
    goals = np.array([[1.0, 0.5], [1.5, -1.0], [-0.25, 0.0], [0.0, 0.0]])   # two behind the wall, one hidden, one in it
    res, orc = plan(ref, wall_and_disc, start, goals)
    assert res["status"] == tu.FOUND and res["which"] == 2 and res["len"] > 2 and 1 <= res["iters"] <= 400
    path, L = res["path"], res["len"]
    assert np.array_equal(ru.bits(path[0]), ru.bits(start))
    assert np.array_equal(ru.bits(path[L - 1]), ru.bits(goals[res["which"]]))
    assert np.array_equal(path[L:], np.broadcast_to(goals[2], path[L:].shape))     # padded with goal `which`
    for t in range(L - 1):
        assert (path[t].tobytes(), path[t + 1].tobytes()) in orc.approved, t      # in travel direction
    assert res["cost"] == tu.forward_cost(path, L)
    gu.check_forest(res, start, goals, free=[0, 1, 2])
    # the junction's branch of tree 1 ends in the root of goal `which`; the goals behind the wall grew subtrees that
    # stayed behind it
    assert res["root_goal"][gu.root_of(res, int(res["junction"][1]))] == 2
    for j in range(int(res["nodes"][1])):
        side = res["conf"][1, j, 0]
        assert (side >= 0.1) == (gu.root_of(res, j) in (0, 1)), j
    lo, hi = tu.LIMITS2
    assert (path >= lo).all() and (path <= hi).all()


def test_two_far_side_goals_through_the_gap(ref):
    start = np.array([-1.5, -1.0])
    goals = np.array([[0.0, 0.0], [1.5, -1.2], [1.2, 0.4]])                       # goal 0 inside the wall
    res, orc = plan(ref, tu.wall_with_gap, start, goals)
    assert res["status"] == tu.FOUND and res["which"] in (1, 2) and res["len"] > 2
    path, L = res["path"], res["len"]
    assert np.array_equal(ru.bits(path[L - 1]), ru.bits(goals[res["which"]]))
    for t in range(L - 1):
        assert (path[t].tobytes(), path[t + 1].tobytes()) in orc.approved, t
    assert res["cost"] == tu.forward_cost(path, L)
    gu.check_forest(res, start, goals, free=[1, 2])
    assert res["root_goal"][gu.root_of(res, int(res["junction"][1]))] == res["which"]


def test_rule_0_case_by_case(ref):
    start, far = np.array([-1.5, 0.0]), np.array([1.5, 0.1])
    # no goals: status 1, the start repeated, nothing asked
    res, orc = plan(ref, tu.disc, start, [far, far], count=0)
    assert (res["status"], res["len"], res["iters"], res["which"]) == (tu.NO_ROUTE, 2, 0, -1) and res["cost"] == math.inf
    assert np.array_equal(res["path"], np.tile(start, (64, 1))) and orc.asked == 0 and list(res["nodes"]) == [0, 0]
    res, _ = plan(ref, tu.disc, start, [far, far], count=-3)                       # (clamped)
    assert res["status"] == tu.NO_ROUTE and np.array_equal(res["path"], np.tile(start, (64, 1)))
    # every goal blocked
    inside = [[0.1, 0.1], [0.0, -0.2]]
    res, orc = plan(ref, tu.disc, start, inside)
    assert (res["status"], res["len"], res["iters"], res["which"], res["roots"]) == (tu.NO_ROUTE, 2, 0, -1, 0)
    assert res["cost"] == math.inf and orc.asked == 0 and list(res["nodes"]) == [0, 0]
    assert np.array_equal(res["path"][0], start) and np.array_equal(res["path"][1:], np.tile(inside[0], (63, 1)))
    # the start blocked
    res, orc = plan(ref, tu.disc, [0.1, 0.1], [far, [1.5, 1.2]])
    assert (res["status"], res["iters"], res["which"]) == (tu.NO_ROUTE, 0, -1) and orc.asked == 0
    assert np.array_equal(res["path"][1:], np.tile(far, (63, 1)))
    # a NaN in a counted goal is status 3 -- before anything else, also with a blocked start --, in one past the count
    # nothing
    for s in (start, [0.1, 0.1]):
        res, orc = plan(ref, tu.disc, s, [far, [math.nan, 0.0]], count=2)
        assert (res["status"], res["len"], res["iters"], res["which"]) == (tu.QUERY_NAN, 2, 0, -1)
        assert math.isnan(res["cost"]) and orc.asked == 0
        assert np.array_equal(res["path"][0], s) and np.array_equal(res["path"][1:], np.tile(far, (63, 1)))
    res, _ = plan(ref, tu.disc, start, [far, [math.inf, 0.0]], count=2)
    assert res["status"] == tu.QUERY_NAN
    with_nan, _ = plan(ref, tu.disc, start, [far, [math.nan, 0.0]], count=1)
    alone, _ = plan(ref, tu.disc, start, [far])
    assert with_nan["status"] == tu.FOUND and with_nan["which"] == 0
    same_bits(with_nan, alone, FIELDS + ("which", "roots"))
    # a count above G is clamped to G
    res, _ = plan(ref, tu.disc, start, [far], count=9)
    same_bits(res, alone, FIELDS + ("which", "roots"))


def test_rule_0_direct_goals(ref):
    start = np.array([-1.5, 1.0])
    # the nearest of the visible goals, whatever its slot; the hidden one (behind the disc) is nearer than none of them
    res, orc = plan(ref, tu.disc, start, [[1.5, 1.2], [0.0, 1.5], [-1.0, -1.0], [-1.5, 1.4]])
    assert (res["status"], res["len"], res["iters"], res["which"]) == (tu.FOUND, 2, 0, 3) and res["cost"] == 1.4 - 1.0
    assert orc.asked == 4 and list(res["nodes"]) == [0, 0]
    assert np.array_equal(res["path"][1:], np.tile([-1.5, 1.4], (63, 1)))
    # two direct goals at equal distance: the lower g, in either order
    a, b = [-1.0, 1.0], [-1.5, 1.5]
    for goals in ([a, b], [b, a]):
        res, _ = plan(ref, tu.disc, start, [[0.0, 0.0]] + goals)
        assert (res["status"], res["which"], res["cost"]) == (tu.FOUND, 1, 0.5)
        assert np.array_equal(res["path"][1], goals[0])
    # a direct goal wins over a nearer goal that is hidden: rule 0 looks at free direct motions only
    res, _ = plan(ref, wall_and_disc, [-1.8, 0.0], [[-0.25, 0.0], [-1.8, 1.9]])
    assert (res["status"], res["which"], res["len"]) == (tu.FOUND, 1, 2)


def test_nothing_past_the_count_is_read(ref):
    start = np.array([-1.8, 0.0])
    goals = np.array([[1.0, 0.5], [-0.25, 0.0], [0.0, 0.0], [0.0, 0.0]])
    base, orc = plan(ref, wall_and_disc, start, goals[:2])
    assert base["status"] == tu.FOUND and base["which"] == 1 and base["len"] > 2
    for fill in (math.nan, 0.0, -1.0):       # NaN rows, rows in the wall, rows in the disc
        g = goals.copy()
        g[2:] = [fill, 0.0]
        res, o = plan(ref, wall_and_disc, start, g, count=2)
        same_bits(res, base, ("status", "len", "iters", "nodes", "junction", "cost", "path", "conf", "parent", "which"))
        assert res["roots"] == 2 and res["root_goal"].tolist() == [0, 1, -1, -1] and o.asked == orc.asked
    # a free row past the count is no root either (it would be directly visible)
    g = goals.copy()
    g[2:] = [-1.8, 0.5]
    res, _ = plan(ref, wall_and_disc, start, g, count=2)
    same_bits(res, base, ("status", "len", "iters", "nodes", "cost", "path", "which"))


def test_caps(ref):
    assert ref.caps(1) == (gu.MAX_GOALS, 2) and ref.caps(2)[1] == 2 and ref.caps(3)[1] == 3 and ref.caps(16)[1] == 16
    start = np.array([-1.8, 0.0])
    goals = np.array([[1.0, 0.5], [1.5, -1.0], [-0.25, 0.0]])
    # max_nodes == G: tree 1 is full of roots and never grows; tree 0 still extends and may join a root
    res, _ = plan(ref, wall_and_disc, start, goals, M=3)
    assert res["nodes"][1] == 3 and res["nodes"][0] <= 3 and res["status"] in (tu.FOUND, tu.NO_ROUTE)
    gu.check_forest(res, start, goals, free=[0, 1, 2])
    if res["status"] == tu.NO_ROUTE:
        assert res["iters"] == 400 and res["which"] == -1 and res["cost"] == math.inf
    # Lmax = 2: status 2 keeps the cost, which is -1 and the path is the start and goal 0
    full, _ = plan(ref, wall_and_disc, start, goals)
    res, _ = plan(ref, wall_and_disc, start, goals, Lmax=2)
    assert full["status"] == tu.FOUND and full["len"] > 2
    assert (res["status"], res["len"], res["which"]) == (tu.TOO_LONG, 2, -1) and res["cost"] == full["cost"]
    assert res["iters"] == full["iters"] and np.array_equal(res["nodes"], full["nodes"])
    assert np.array_equal(res["path"], np.stack([start, goals[0]]))
    # the same arguments, the same bits
    again, _ = plan(ref, wall_and_disc, start, goals)
    same_bits(again, full, FIELDS + ("which", "roots", "root_goal"))


# ---- the library: symbols and the refusals that need no device -----------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from optik_amd import build
    build.build()
    from optik_amd import _native
    return _native.lib()


def test_symbols_are_exported(lib):
    for name in ("optik_hip_rrt_plan_goals", "optik_robot_rrt_plan_goals"):
        assert hasattr(lib, name), name


def test_argument_rules_on_the_host():
    from optik_amd import _native as nat
    assert nat.RRT_MAX_GOALS == gu.MAX_GOALS == nat.ROADMAP_MAX_GOALS
    assert nat.check_rrt_goals(1, 2) == 1 and nat.check_rrt_goals(16, 16) == 16 and nat.check_rrt_goals(8, 256) == 8
    for G, M in ((0, 256), (17, 256), (2.5, 256), (True, 256), (3, 2), (16, 15)):
        with pytest.raises(ValueError):
            nat.check_rrt_goals(G, M)


def test_the_header_states_the_cap():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "optik_hip.h")).read()
    assert re.search(rf"#define OPTIK_HIP_RRT_MAX_GOALS {gu.MAX_GOALS}\b", text)
    assert "optik_hip_rrt_plan_goals" in text
    assert "optik_robot_rrt_plan_goals" in open(os.path.join(root, "include", "optik.h")).read()
