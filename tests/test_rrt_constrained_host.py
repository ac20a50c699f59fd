"""The rules of the tree planner under a pose constraint (csrc/rrt_constrained_measure.hpp) on the host: the serial
reference with g++, the constraint with constraint_measure.hpp on the host (rrt_constrained_util), the collision
verdicts from the host motion check (roadmap_util.host_checked_weights).  No GPU."""
import math

import numpy as np
import pytest

import constraint_util as cu
import roadmap_util as ru
import rrt_constrained_util as xu
import rrt_goals_util as gu
import rrt_util as tu
from motion_util import build_motion

SHARED = ("status", "len", "iters", "which", "roots")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return xu.build_rrt_constrained_ref(str(tmp_path_factory.mktemp("rrt_constrained_measure")))


@pytest.fixture(scope="module")
def gref(tmp_path_factory):
    return gu.build_rrt_goals_ref(str(tmp_path_factory.mktemp("rrt_goals_measure")))


@pytest.fixture(scope="module")
def cmlib(tmp_path_factory):
    return xu.build_host_constraint_lib(str(tmp_path_factory.mktemp("constraint_host")))


@pytest.fixture(scope="module")
def panda(oracle, chains, tmp_path_factory):
    """The wall scene of DESIGN.md section 5.18 with the host motion check, and the samples of the planner."""
    sc = ru.wall_scene()
    motion = build_motion(str(tmp_path_factory.mktemp("motion")))
    d, ch = chains["panda"]
    samples = np.array([oracle.restart_seed(ch, xu.FIRST + i) for i in range(xu.ITERS)])
    free = lambda qa, qb: np.isfinite(ru.host_checked_weights(sc, motion, qa, qb))  # noqa: E731
    return dict(sc=sc, d=d, lo=np.array(d["lb"]), hi=np.array(d["ub"]), samples=samples, free=free,
                config_free=lambda q: bool(free(q[None], q[None])[0]),
                ref7=np.asarray(oracle.fk(ch, sc["start"])[1]))


def _callbacks(panda, hc, tol=xu.TOL, ptol=xu.PTOL, piters=xu.PITERS):
    h = panda["sc"]["h"]
    return (lambda q: panda["config_free"](q) and hc.violation(q) <= tol,
            lambda qa, qb: panda["free"](qa, qb) & hc.motion_ok(qa, qb, h, tol),
            lambda x: hc.project(x, ptol, piters, xu.DAMPING, xu.MAX_STEP))


def _same_bits(a, b, what):
    assert np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64),
                          np.ascontiguousarray(b, dtype=np.float64).view(np.uint64)), what


def _assert_shared_equal(got, want, what):
    for key in SHARED:
        assert got[key] == want[key], (what, key, got[key], want[key])
    for key in ("nodes", "junction", "root_goal", "parent"):
        assert np.array_equal(got[key], want[key]), (what, key)
    for key in ("cost", "path", "conf"):
        _same_bits(got[key], want[key], (what, key))


# ---- a free box is the unconstrained planner, bit for bit ------------------------------------------------------------

@pytest.mark.parametrize("free, start, goal", [
    (tu.wall_with_gap, [-1.0, 0.0], [1.0, 0.0]), (tu.disc, [-1.0, 0.1], [1.0, -0.1]), (tu.wall, [-1.0, 0.0], [1.0, 0.0])])
def test_free_box_on_the_2_joint_scenes(ref, gref, free, start, goal):
    """A free box as the reference sees it: every projection returns its input after 0 iterations, every constraint
    verdict is ok where the motion is sampled -- the callbacks are the obstacle's alone."""
    lo, hi = tu.LIMITS2
    samples = tu.samples2(400, 5)
    start, goal = np.array(start), np.array(goal)
    o1, o2 = tu.Oracle2(free), tu.Oracle2(free)
    want = gref.plan(lo, hi, start, goal[None], 1, samples, 0.3, 256, 64, o1.config_free, o1.motions_free)
    got = ref.plan(lo, hi, start, goal[None], 1, samples, 0.3, 256, 64, o2.config_free, o2.motions_free,
                   lambda x: (x, xu.PROJECTED, 0))
    _assert_shared_equal(got, want, free.__name__)
    assert got["projected"][0] == got["projected"][1] == len(got["projections"])
    assert (got["projected"][0] > 0) == (got["iters"] > 0)


def test_free_box_on_the_panda(ref, gref, cmlib, panda):
    """The same with constraint_measure.hpp itself: its projection of a clamped candidate onto a free box runs 0
    iterations and changes nothing, its motion verdict is ok wherever the motion is sampled."""
    hc = xu.HostConstraint(cmlib, panda["d"], cu.free_constraint(panda["ref7"]))
    config_ok, motions_ok, project = _callbacks(panda, hc, tol=0.0, ptol=0.0, piters=0)
    sc = panda["sc"]
    for s, g in ((sc["start"], sc["goal"]), (sc["goal"], sc["start"])):
        want = gref.plan(panda["lo"], panda["hi"], s, g[None], 1, panda["samples"], 0.3, xu.NODES, 64,
                         panda["config_free"], panda["free"])
        got = ref.plan(panda["lo"], panda["hi"], s, g[None], 1, panda["samples"], 0.3, xu.NODES, 64, config_ok,
                       motions_ok, project)
        assert want["status"] == tu.FOUND and want["len"] > 2
        _assert_shared_equal(got, want, "panda")
        assert all(p == (xu.PROJECTED, 0) for p in got["projections"])


# ---- the Panda carrying its end effector upright past the wall ------------------------------------------------------
# Chosen here with the host build: upright(fk(start), TILT = 0.3) -- the wall pair differs in joint 1 only and its end
# effector points straight down, so both ends satisfy the constraint exactly -- tol 0.05, ptol 1e-6, piters 16, step
# 0.5, first 1, max_nodes 64.  The serial reference joins the trees after 51 iterations with 20 and 15 nodes and 10
# waypoints (95 projections, all PROJECTED), and after 107 iterations with 33 and 41 nodes and 13 waypoints for the pair
# reversed (186 projections, 185 PROJECTED).

@pytest.fixture(scope="module")
def upright(ref, cmlib, panda):
    hc = xu.HostConstraint(cmlib, panda["d"], cu.upright_constraint(panda["ref7"], xu.TILT))
    sc = panda["sc"]
    cb = _callbacks(panda, hc)
    plan = lambda s, g, **kw: ref.plan(panda["lo"], panda["hi"], s, np.atleast_2d(g), kw.pop("count", 1),  # noqa: E731
                                       panda["samples"], xu.STEP, xu.NODES, 64, *cb)
    return dict(hc=hc, cb=cb, plan=plan, fwd=plan(sc["start"], sc["goal"]), back=plan(sc["goal"], sc["start"]))


def test_upright_pair_is_found_where_the_host_build_says(upright):
    f, b = upright["fwd"], upright["back"]
    print("pair:", f["status"], f["iters"], f["nodes"], f["len"], f["projected"], "reversed:", b["status"], b["iters"],
          b["nodes"], b["len"], b["projected"])
    assert (f["status"], f["iters"], f["nodes"].tolist(), f["len"], f["projected"].tolist()) == (
        tu.FOUND, 51, [20, 15], 10, [95, 95])
    assert (b["status"], b["iters"], b["nodes"].tolist(), b["len"], b["projected"].tolist()) == (
        tu.FOUND, 107, [33, 41], 13, [186, 185])


def test_upright_nodes_and_segments(upright, panda):
    hc, sc = upright["hc"], panda["sc"]
    config_ok, motions_ok, _ = upright["cb"]
    for res, (s, g) in ((upright["fwd"], (sc["start"], sc["goal"])), (upright["back"], (sc["goal"], sc["start"]))):
        for t in (0, 1):
            for j in range(1, res["nodes"][t]):    # (node 0 is the root: it satisfies the constraint at tol)
                q = res["conf"][t, j]
                assert hc.violation(q) <= xu.PTOL and (q >= panda["lo"]).all() and (q <= panda["hi"]).all(), (t, j)
        L, p = res["len"], res["path"]
        _same_bits(p[0], s, "start")
        _same_bits(p[L - 1:], np.tile(g, (64 - L + 1, 1)), "goal and padding")
        assert motions_ok(p[:L - 1], p[1:L]).all()                       # both host checks, in path order
        assert res["cost"] == tu.forward_cost(p, L) and res["which"] == 0


def test_upright_same_arguments_same_bits(upright, panda):
    again = upright["plan"](panda["sc"]["start"], panda["sc"]["goal"])
    _assert_shared_equal(again, upright["fwd"], "second run")
    assert np.array_equal(again["projected"], upright["fwd"]["projected"])
    assert again["projections"] == upright["fwd"]["projections"]


def test_the_unconstrained_path_tips_the_glass_over(gref, upright, panda):
    """The reason the feature exists: plan_goals_reference's path for the same pair has a segment that fails the
    constraint check."""
    sc, hc = panda["sc"], upright["hc"]
    u = gref.plan(panda["lo"], panda["hi"], sc["start"], sc["goal"][None], 1, panda["samples"], xu.STEP, xu.NODES, 64,
                  panda["config_free"], panda["free"])
    assert u["status"] == tu.FOUND and u["len"] > 2
    p = u["path"][:u["len"]]
    assert panda["free"](p[:-1], p[1:]).all() and not hc.motion_ok(p[:-1], p[1:], sc["h"], xu.TOL).all()


def test_the_timing_reference_takes_the_paths_slowly(upright, panda, tmp_path):
    """What the example and the device test time the paths with, chosen here with time_measure.hpp's serial reference.
    A tree's path has a corner at every waypoint.  At the URDF's velocity limits the pair's path stalls (status 1: the
    profile stops at its last two waypoints) with 5 rad/s^2 and with the Panda's own acceleration limits alike.  At 0.5
    rad/s and 5 rad/s^2 both paths are timed and never stop on the way: every corner is taken at the velocity limit, so
    half the speed takes exactly twice as long -- a margin of a factor of two in the speed."""
    import time_util
    tref = time_util.build_time_ref(str(tmp_path))
    urdf = np.asarray(panda["sc"]["robot"].velocity_limits())
    for res, seconds in ((upright["fwd"], 9.295), (upright["back"], 10.786)):
        L, p = res["len"], res["path"][None]
        slow = tref.time(p, [L], np.full(7, 0.5), np.full(7, 5.0))
        print("at 0.5 rad/s:", slow["status"][0], slow["duration"][0], "x", slow["x"][0, :L])
        assert slow["status"][0] == time_util.TIMED and abs(slow["duration"][0] - seconds) < 5e-4
        assert (slow["x"][0, 1:L - 1] > 0.0).all()
        slower = tref.time(p, [L], np.full(7, 0.25), np.full(7, 5.0))
        assert slower["status"][0] == time_util.TIMED
        assert abs(slower["duration"][0] - 2.0 * slow["duration"][0]) < 1e-9 * slow["duration"][0]
    fwd = upright["fwd"]
    for a_max in (np.full(7, 5.0), np.array([15.0, 7.5, 10.0, 12.5, 15.0, 20.0, 20.0])):
        assert tref.time(fwd["path"][None], [fwd["len"]], urdf, a_max)["status"][0] == time_util.STALLED


def test_the_table_behind_the_default_piters(ref, panda, upright):
    """DESIGN.md section 5.30 reads the default piters from one table: the serial reference on the example's scene, the
    pair and the pair reversed, with a projection budget of 4096, the iteration count of every projection it attempts,
    and the share that ends PROJECTED within 1, 2, 4, ... iterations.  This recomputes the table and the choice: the
    smallest power of two after which a doubling gains at most one point."""
    sc = panda["sc"]
    cb = _callbacks(panda, upright["hc"], piters=4096)
    runs = [ref.plan(panda["lo"], panda["hi"], s, g[None], 1, panda["samples"], xu.STEP, xu.NODES, 64, *cb)
            for s, g in ((sc["start"], sc["goal"]), (sc["goal"], sc["start"]))]
    # (with the budget of 4096 the trees are those of piters = 16 but for the one projection of the pair reversed that
    # 16 leave unfinished: it ends after 20, and the iteration, node and waypoint counts stay what they are with 16)
    assert [(r["status"], r["iters"], r["nodes"].tolist(), r["len"], r["projected"].tolist()) for r in runs] == [
        (tu.FOUND, 51, [20, 15], 10, [95, 95]), (tu.FOUND, 107, [33, 41], 13, [186, 186])]
    status = np.array([s for r in runs for s, _ in r["projections"]])
    its = np.array([i for r in runs for _, i in r["projections"]])
    assert len(its) == 281 and (status == xu.PROJECTED).all() and its.max() == 20
    within = (0, 1, 2, 4, 8, 16, 32)
    share = [round(100.0 * float((its <= k).mean()), 2) for k in within]
    print("share PROJECTED within", within, "iterations:", share)
    assert share == [37.72, 51.25, 78.29, 91.81, 95.02, 99.64, 100.0]
    gains = {k: share[within.index(2 * k)] - share[within.index(k)] for k in (1, 2, 4, 8, 16)}
    assert min(k for k, g in gains.items() if g <= 1.0) == xu.PITERS == 16


# ---- cases that end before the iterations -------------------------------------------------------------------------

def test_a_start_that_violates_gives_status_1(upright, panda):
    sc = panda["sc"]
    tipped = sc["start"].copy()
    tipped[5] -= 1.0                                                     # (the wrist tilts the end effector by 1 rad)
    assert panda["config_free"](tipped) and upright["hc"].violation(tipped) > xu.TOL
    res = upright["plan"](tipped, sc["goal"])
    assert (res["status"], res["iters"], res["nodes"].tolist(), res["projected"].tolist(), res["which"]) == (
        tu.NO_ROUTE, 0, [0, 0], [0, 0], -1)
    assert res["cost"] == math.inf and np.array_equal(res["path"][1:], np.tile(sc["goal"], (63, 1)))


def test_a_goal_that_violates_is_not_a_root(upright, panda):
    sc = panda["sc"]
    tipped = sc["goal"].copy()
    tipped[5] -= 1.0
    goals = np.stack([tipped, sc["goal"], np.full(7, math.nan)])
    res = upright["plan"](sc["start"], goals, count=2)
    assert res["roots"] == 1 and res["root_goal"].tolist() == [1, -1, -1]
    assert res["status"] == tu.FOUND and res["which"] == 1
    _same_bits(res["path"][res["len"] - 1], sc["goal"], "the path ends in goal 1")
    # (with goal 1 the only root the trees are the single-goal query's)
    assert res["iters"] == upright["fwd"]["iters"] and np.array_equal(res["nodes"], upright["fwd"]["nodes"])


def test_a_nan_counted_goal_gives_status_3(upright, panda):
    sc = panda["sc"]
    bad = sc["goal"].copy()
    bad[3] = math.nan
    res = upright["plan"](sc["start"], np.stack([sc["goal"], bad]), count=2)
    assert res["status"] == tu.QUERY_NAN and math.isnan(res["cost"]) and res["iters"] == 0
    assert res["nodes"].tolist() == [0, 0] and res["projected"].tolist() == [0, 0]


# ---- the projection's verdicts ------------------------------------------------------------------------------------

def test_piters_0_with_a_pinned_axis_accepts_no_candidate(ref, cmlib, panda):
    """Pinned at the start's own height (lo = hi = 0 on linear z): the start and the goal, which differ in joint 1 only,
    satisfy it; a steered candidate does not, and with no iteration allowed no projection ends PROJECTED."""
    inf = math.inf
    c = cu.Constraint(panda["ref7"], [-inf, -inf, 0.0, -inf, -inf, -inf], [inf, inf, 0.0, inf, inf, inf])
    hc = xu.HostConstraint(cmlib, panda["d"], c)
    sc = panda["sc"]
    assert hc.violation(sc["start"]) <= 1e-9 and hc.violation(sc["goal"]) <= 1e-9
    config_ok, motions_ok, project = _callbacks(panda, hc, tol=1e-9, ptol=1e-12, piters=0)
    res = ref.plan(panda["lo"], panda["hi"], sc["start"], sc["goal"][None], 1, panda["samples"][:32], xu.STEP, xu.NODES,
                   64, config_ok, motions_ok, project)
    assert res["status"] == tu.NO_ROUTE and res["iters"] == 32 and res["nodes"].tolist() == [1, 1]
    assert res["projected"][0] == 32 and res["projected"][1] == 0
    assert all(p == (xu.BUDGET_SPENT, 0) for p in res["projections"])


def test_takes_rule(ref):
    P, B, F = xu.PROJECTED, xu.BUDGET_SPENT, xu.FAILED
    assert ref.takes(P, 0, False) and ref.takes(P, 0, True) and ref.takes(P, 3, False)
    assert not ref.takes(P, 1, True) and not ref.takes(P, 7, True)
    for same in (False, True):
        assert not ref.takes(B, 16, same) and not ref.takes(F, 0, same) and not ref.takes(F, 2, same)


def _plan2(ref, project, I=8, M=16):
    """Two joints, no obstacle at all, start and goal three steps apart: what the projection callback says is all
    that can stop a tree."""
    lo, hi = tu.LIMITS2
    samples = np.tile(np.array([[1.5, 1.5], [-1.5, -1.5]]), (I // 2, 1))
    ok = lambda qa, qb: [bool(np.max(np.abs(a - b)) > 0.0 and np.max(np.abs(a - b)) <= 0.45) for a, b in zip(qa, qb)]  # noqa: E731
    return ref.plan(lo, hi, np.array([-1.0, -1.0]), np.array([[1.0, 1.0]]), 1, samples, 0.3, M, 64, lambda q: True, ok,
                    project)


def test_a_projection_back_onto_its_parent_is_not_a_node(ref):
    """The constructed candidate: a projection that runs one iteration and lands on the node it was steered from is
    counted as PROJECTED and not taken; after 0 iterations the same coordinates would be (and a motion of length 0
    is not sampled, so nothing is appended either way)."""
    start = np.array([-1.0, -1.0])
    res = _plan2(ref, lambda x: (start.copy(), xu.PROJECTED, 1), I=4)
    assert res["nodes"].tolist() == [1, 1] and res["status"] == tu.NO_ROUTE
    # iterations 0 and 2 steer from the start and land on it: not taken; 1 and 3 steer from the goal, land on the start,
    # which is not their parent: taken, but the nearest node of tree 0 is the start itself at distance 0 -- no
    # back-extension, and neither motion (goal - start is 2.0 long for this test's verdicts, start - start is 0) passes
    assert res["projected"].tolist() == [4, 4]
    res = _plan2(ref, lambda x: (x, xu.PROJECTED, 1))
    assert res["status"] == tu.FOUND and res["projected"][0] == res["projected"][1]


def test_every_status_path_of_an_iteration(ref):
    """Candidate refused (one projection counted), candidate taken and back-extension refused (two counted, tree b
    does not grow), both taken."""
    calls = []

    def refuse_every_second(x):
        calls.append(x.copy())
        return (x, xu.PROJECTED, 0) if len(calls) % 2 == 1 else (x, xu.BUDGET_SPENT, 16)

    res = _plan2(ref, refuse_every_second, I=4)
    # every iteration: the candidate (odd call) is taken, the back-extension (even call) is refused; the trees walk
    # towards each other along the diagonal 0.3 at a time, from 2.0 apart
    assert res["projected"].tolist() == [8, 4] and res["iters"] == 4 and res["status"] == tu.NO_ROUTE
    assert res["nodes"].tolist() == [3, 3]                                   # (two candidates each, no e)
    calls.clear()
    res = _plan2(ref, refuse_every_second, I=6)
    # iteration 5's candidate is 0.2 from the other tree: no back-extension is asked for, and the connection passes
    assert res["projected"].tolist() == [11, 6] and res["iters"] == 6 and res["status"] == tu.FOUND
    assert res["nodes"].tolist() == [4, 4] and res["len"] == 8
    res = _plan2(ref, lambda x: (x, xu.FAILED, 0), I=6)
    assert res["projected"].tolist() == [6, 0] and res["nodes"].tolist() == [1, 1]
    res = _plan2(ref, lambda x: (x, xu.PROJECTED, 2), I=6)
    assert res["status"] == tu.FOUND and res["projected"][0] == res["projected"][1] >= 2


# ---- the library: symbols and the rules that need no device ---------------------------------------------------------

def test_symbols_and_defaults():
    import os
    import re
    from optik_amd import build
    build.build()
    from optik_amd import _native as nat
    from optik_amd import robot as _robot  # noqa: F401  (declares the optik_robot_* signatures)
    for name in ("optik_hip_rrt_plan_constrained", "optik_robot_rrt_plan_constrained"):
        assert hasattr(nat.lib(), name), name
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "optik_hip.h")).read()
    assert re.search(rf"#define OPTIK_HIP_RRT_PROJECT_ITERS {nat.RRT_PROJECT_ITERS}\b", text)
    assert nat.RRT_PROJECT_ITERS == xu.PITERS
