"""CPU-only: the rules of the bidirectional tree planner (optik_amd/csrc/rrt_measure.hpp, built with g++).  The serial
reference against closed-form obstacles in a 2-joint space -- every segment of a found path approved in the direction
of travel, the ends, the cost, the trees, the caps --; the nearest and steer rules on their own; the wall scene of the
-m gpu test, chosen here with the host motion check; the exported symbols and the host-side refusals."""
import math

import numpy as np
import pytest

import roadmap_util as ru
import rrt_util as tu
from motion_util import build_motion


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return tu.build_rrt_ref(str(tmp_path_factory.mktemp("rrt_measure")))


def plan2(ref, free, start, goal, I=400, step=0.3, M=256, Lmax=64, seed=5):
    orc = tu.Oracle2(free)
    lo, hi = tu.LIMITS2
    res = ref.plan(lo, hi, start, goal, tu.samples2(I, seed), step, M, Lmax, orc.config_free, orc.motions_free)
    return res, orc


@pytest.mark.parametrize("free, start, goal", [(tu.disc, [-1.5, 0.0], [1.5, 0.1]),
                                               (tu.wall_with_gap, [-1.5, -1.0], [1.5, -1.2])])
def test_found_path_is_approved_in_travel_direction(ref, free, start, goal):
    start, goal = np.array(start), np.array(goal)
    res, orc = plan2(ref, free, start, goal)
    assert res["status"] == tu.FOUND and 3 <= res["len"] <= 64 and 1 <= res["iters"] <= 400
    path, L = res["path"], res["len"]
    assert np.array_equal(path[0], start) and np.array_equal(path[L - 1], goal)
    assert np.array_equal(path[L:], np.broadcast_to(goal, path[L:].shape))   # padded with the goal
    for t in range(L - 1):
        assert (path[t].tobytes(), path[t + 1].tobytes()) in orc.approved, t
    assert res["cost"] == tu.forward_cost(path, L)
    tu.check_trees(res, start, goal)
    assert (res["nodes"] <= 256).all() and (res["nodes"] >= 1).all()
    # the junction joins the two branches: tree 0's node is waypoint d0 - 1, tree 1's the next
    j0, j1 = res["junction"]
    d0 = 0
    v = j0
    while v >= 0:
        d0 += 1
        v = res["parent"][0, v]
    assert np.array_equal(path[d0 - 1], res["conf"][0, j0]) and np.array_equal(path[d0], res["conf"][1, j1])
    lo, hi = tu.LIMITS2
    assert (path >= lo).all() and (path <= hi).all()


def test_direct_case(ref):
    res, orc = plan2(ref, tu.disc, np.array([-1.5, 1.0]), np.array([1.5, 1.2]))
    assert res["status"] == tu.FOUND and res["len"] == 2 and res["iters"] == 0 and orc.asked == 1
    assert res["cost"] == 3.0 and list(res["nodes"]) == [0, 0]


def test_ends_that_end_the_query_before_iteration_0(ref):
    res, orc = plan2(ref, tu.disc, np.array([0.1, 0.1]), np.array([1.5, 1.2]))       # the start inside the disc
    assert res["status"] == tu.NO_ROUTE and res["cost"] == math.inf and res["iters"] == 0 and orc.asked == 0
    assert np.array_equal(res["path"][0], [0.1, 0.1]) and np.array_equal(res["path"][1:], np.tile([1.5, 1.2], (63, 1)))
    for bad in (math.nan, math.inf):
        res, orc = plan2(ref, tu.disc, np.array([-1.5, 0.0]), np.array([1.5, bad]))
        assert res["status"] == tu.QUERY_NAN and math.isnan(res["cost"]) and res["iters"] == 0 and res["len"] == 2
        assert orc.asked == 0


def test_wall_without_a_gap_ends_in_no_route(ref):
    start, goal = np.array([-1.5, -1.0]), np.array([1.5, -1.2])
    res, _ = plan2(ref, tu.wall, start, goal, I=300, M=40)
    assert res["status"] == tu.NO_ROUTE and res["cost"] == math.inf and res["iters"] == 300 and res["len"] == 2
    assert (res["nodes"] <= 40).all() and res["nodes"].max() == 40      # a tree fills up and the planner goes on
    tu.check_trees(res, start, goal)
    # no node has crossed the wall
    assert (res["conf"][0, :res["nodes"][0], 0] <= -0.1).all() and (res["conf"][1, :res["nodes"][1], 0] >= 0.1).all()


def test_max_nodes_2_terminates(ref):
    res, _ = plan2(ref, tu.wall_with_gap, np.array([-1.5, -1.0]), np.array([1.5, -1.2]), M=2)
    assert res["status"] == tu.NO_ROUTE and res["iters"] == 400 and (res["nodes"] <= 2).all()


def test_lmax_2_keeps_the_cost(ref):
    start, goal = np.array([-1.5, -1.0]), np.array([1.5, -1.2])
    full, _ = plan2(ref, tu.wall_with_gap, start, goal)
    res, _ = plan2(ref, tu.wall_with_gap, start, goal, Lmax=2)
    assert full["status"] == tu.FOUND and full["len"] > 2
    assert res["status"] == tu.TOO_LONG and res["len"] == 2 and res["cost"] == full["cost"]
    assert res["iters"] == full["iters"] and np.array_equal(res["nodes"], full["nodes"])
    assert np.array_equal(res["path"], np.stack([start, goal]))


def test_same_arguments_same_bits(ref):
    a, _ = plan2(ref, tu.wall_with_gap, np.array([-1.5, -1.0]), np.array([1.5, -1.2]))
    b, _ = plan2(ref, tu.wall_with_gap, np.array([-1.5, -1.0]), np.array([1.5, -1.2]))
    for key in ("path", "conf", "parent", "nodes", "junction"):
        assert np.array_equal(ru.bits(a[key]) if a[key].dtype == np.float64 else a[key],
                              ru.bits(b[key]) if b[key].dtype == np.float64 else b[key]), key
    assert (a["status"], a["len"], a["iters"], a["cost"]) == (b["status"], b["len"], b["iters"], b["cost"])


def test_nearest_order(ref):
    conf = np.array([[1.0, 0.0], [0.0, 0.5], [0.0, -0.5], [0.5, 0.5]])
    assert ref.nearest(conf, np.array([0.0, 0.0])) == (1, 0.5)          # nodes 1, 2 and 3 tie: the lowest index
    assert ref.nearest(conf[::-1].copy(), np.array([0.0, 0.0])) == (0, 0.5)
    assert ref.nearest(conf, np.array([1.0, 0.0])) == (0, 0.0)
    nan = np.array([[math.nan, 0.0], [5.0, 5.0]])
    assert ref.nearest(nan, np.array([0.0, 0.0])) == (1, 5.0)           # a number before a NaN
    j, d = ref.nearest(nan[:1], np.array([0.0, 0.0]))
    assert j == 0 and math.isnan(d)


def test_steer_rule(ref):
    lo, hi = tu.LIMITS2
    p = np.array([0.0, 0.0])
    assert np.array_equal(ref.steer(p, np.array([0.25, -0.3]), 0.3, lo, hi), [0.25, -0.3])   # d <= step: copied
    x = np.array([1.0, -0.7])
    s = 0.3 / 1.0
    assert np.array_equal(ref.steer(p, x, 0.3, lo, hi), [0.0 + s * (1.0 - 0.0), 0.0 + s * (-0.7 - 0.0)])
    assert ref.steer(p, p, 0.3, lo, hi) is None                         # d = 0
    assert ref.steer(p, np.array([math.nan, 0.0]), 0.3, lo, hi) is None
    assert ref.steer(p, np.array([math.inf, 0.0]), 0.3, lo, hi) is None
    # the clamp: a parent outside the limits (a start may be), and a copied sample outside them
    c = ref.steer(np.array([2.5, 0.0]), np.array([2.6, 1.0]), 0.3, lo, hi)
    assert c[0] == 2.0 and -2.0 <= c[1] <= 2.0
    assert np.array_equal(ref.steer(p, np.array([0.1, -0.2]), 0.3, np.array([0.15, -0.1]), hi), [0.15, -0.1])


def test_wall_scene_is_blocked_and_the_reference_finds_a_route(ref, oracle, chains, tmp_path):
    """The expectation of tests/test_gpu_rrt.py's wall-scene tests, from the host alone: the straight move is not
    free, and the serial reference joins the trees well within the constants the GPU test uses."""
    sc = ru.wall_scene()
    motion = build_motion(str(tmp_path))
    d, ch = chains["panda"]
    lo, hi = np.array(d["lb"]), np.array(d["ub"])
    samples = np.array([oracle.restart_seed(ch, tu.WALL_FIRST + i) for i in range(tu.WALL_ITERS)])
    assert (samples >= lo).all() and (samples <= hi).all()

    def config_free(q):
        return bool(np.isfinite(ru.host_checked_weights(sc, motion, q[None], q[None]))[0])

    def motions_free(qa, qb):
        return np.isfinite(ru.host_checked_weights(sc, motion, qa, qb))

    assert not motions_free(sc["start"][None], sc["goal"][None])[0]
    for s, g in ((sc["start"], sc["goal"]), (sc["goal"], sc["start"])):
        res = ref.plan(lo, hi, s, g, samples, tu.WALL_STEP, tu.WALL_NODES, 64, config_free, motions_free)
        assert res["status"] == tu.FOUND and 3 <= res["len"] <= 64 and res["iters"] <= tu.WALL_ITERS // 2
        assert (res["nodes"] < tu.WALL_NODES).all() and res["cost"] == tu.forward_cost(res["path"], res["len"])
        full = ref.plan(lo, hi, s, g, samples, tu.WALL_STEP, tu.WALL_NODES, 2, config_free, motions_free)
        assert full["status"] == tu.TOO_LONG and full["cost"] == res["cost"]


# ---- the library: symbols and the refusals that need no device -----------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from optik_amd import build
    build.build()
    from optik_amd import _native
    return _native.lib()


def test_rrt_symbols_are_exported(lib):
    for name in ("optik_hip_rrt_plan", "optik_hip_rrt_chunk", "optik_robot_rrt_plan",
                 "optik_hip_rrt_nearest_from_nodes"):
        assert hasattr(lib, name), name


def test_argument_rules_on_the_host():
    from optik_amd import _native as nat
    assert (nat.RRT_MAX_ITERS, nat.RRT_MIN_NODES, nat.RRT_MAX_NODES, nat.RRT_MAX_POLL) == (
        tu.MAX_ITERS, tu.MIN_NODES, tu.MAX_NODES, tu.MAX_POLL)
    assert nat.check_rrt_args(65536, 0.1, 4096, 64, 65536, 7) == (65536, 0.1, 4096, 65536, 7)
    assert nat.check_rrt_args(None, None, None, 2, None) == (nat.RRT_ITERS, nat.RRT_STEP, nat.RRT_NODES, nat.RRT_POLL, 0)
    for kw in (dict(iters=0), dict(iters=65537), dict(iters=2.5), dict(iters=True), dict(step=0.0), dict(step=-1.0),
               dict(step=math.nan), dict(step=math.inf), dict(max_nodes=1), dict(max_nodes=4097),
               dict(max_waypoints=1), dict(max_waypoints=65), dict(poll=0), dict(poll=65537), dict(first=-1)):
        with pytest.raises(ValueError):
            nat.check_rrt_args(**kw)


def test_the_header_states_the_caps():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "optik_hip.h")).read()
    for name, value in (("MAX_ITERS", tu.MAX_ITERS), ("MAX_NODES", tu.MAX_NODES), ("MAX_POLL", tu.MAX_POLL)):
        assert re.search(rf"#define OPTIK_HIP_RRT_{name} {value}\b", text), name
