"""CPU-only: the rules of lazy roadmaps (optik_amd/csrc/roadmap_lazy_measure.hpp, built with g++).  The serial lazy
reference against roadmap_measure.hpp's plan_reference over the eager graph, as the theorem of DESIGN.md section 5.24
says, on the synthetic graphs and on random graphs with random truth tables; the rounds bound and status 4; the
prescribed graphs (a shared edge, twin slots, a route of exactly Lmax waypoints); the reset; the wall scene of the -m
gpu end-to-end test with the host motion check; the exported symbols and the host-side refusals."""
import math

import numpy as np
import pytest

import roadmap_lazy_util as lu
import roadmap_util as ru
from motion_util import build_motion


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ru.build_roadmap_ref(str(tmp_path_factory.mktemp("roadmap_measure")))


@pytest.fixture(scope="module")
def lazy(tmp_path_factory):
    return lu.build_lazy_ref(str(tmp_path_factory.mktemp("roadmap_lazy_measure")))


def _eager(ref, g, truth, q, L):
    return ref.query(dict(nodes=g["nodes"], nbr=g["nbr"], w=lu.eager_weights(g, truth)), q, L)


def test_lazy_reference_equals_the_eager_plan(ref, lazy):
    seen, found, total = set(), 0, 0
    for name, g, truth, q, L, random in lu.lazy_cases():
        res = lazy.plan(g, truth, q, L, lu.MAX_ROUNDS)
        eager = _eager(ref, g, truth, q, L)
        lu.assert_theorem(name, res, eager)
        seen |= set(res["status"].tolist())
        if random:
            found += int((res["status"] == ru.FOUND).sum())
            total += len(res["status"])
        # the final lazy graph contains the eager graph, and what it blocked beyond the reset it checked
        assert np.all(res["w"] <= lu.eager_weights(g, truth)), name
        assert res["checked"] == int(((res["verdict"] == lu.FREE) | (
            (res["verdict"] == lu.BLOCKED) & (lazy.plan(g, truth, q, L, 0)["verdict"] == lu.UNKNOWN))).sum()), name
        assert res["rounds"] <= res["checked"], name
    assert seen == {ru.FOUND, ru.NO_ROUTE, ru.TOO_LONG, ru.QUERY_NAN}
    assert total == 5 * len(lu.RANDOM_SIZES) and 2 * found >= total, (found, total)


def test_rounds_bound_gives_the_lower_bound_and_status_4(ref, lazy):
    g, truth, q, L = lu.prescribed_cases()["detour_blocked"]
    r0 = lazy.plan(g, truth, q, L, 0)
    assert r0["status"][0] == lu.UNSETTLED and r0["len"][0] == 2 and r0["rounds"] == 0 and r0["checked"] == 0
    assert r0["cost"][0] == 2.0                                   # 0.25 + 1.0 + 0.5 + 0.25 through node 2, unchecked
    assert np.array_equal(r0["path"][0, 0], q["start"][:, 0]) and np.all(r0["path"][1:, 0] == q["goal"][:, 0])
    assert np.all(r0["verdict"][g["nbr"] >= 0] == lu.UNKNOWN)
    r1 = lazy.plan(g, truth, q, L, 1)
    assert r1["status"][0] == lu.UNSETTLED and r1["rounds"] == 1 and r1["checked"] == 2
    assert r1["cost"][0] == 2.5 and r1["verdict"][0, 3] == lu.BLOCKED and r1["verdict"][0, 2] == lu.FREE
    assert r1["w"][0, 3] == math.inf and r1["verdict"][1, 3] == lu.UNKNOWN
    for rounds in (2, 3, lu.MAX_ROUNDS):
        r = lazy.plan(g, truth, q, L, rounds)
        assert r["status"][0] == ru.FOUND and r["rounds"] == 2 and r["checked"] == 4
        lu.assert_theorem("detour", r, _eager(ref, g, truth, q, L))
        assert np.array_equal(r["path"][:5, 0], np.stack([q["start"][:, 0], g["nodes"][:, 3], g["nodes"][:, 1],
                                                          g["nodes"][:, 0], q["goal"][:, 0]]))
    # the verdicts are kept: the same plan again checks nothing
    again = lazy.plan(g, truth, q, L, 0, state=(r["w"], r["verdict"]))
    assert again["status"][0] == ru.FOUND and again["checked"] == 0 and again["cost"][0] == 2.5


def test_prescribed_graphs(ref, lazy):
    cases = lu.prescribed_cases()
    g, truth, q, L = cases["shared_edge"]
    r = lazy.plan(g, truth, q, L, 8)
    assert r["status"].tolist() == [ru.FOUND, ru.FOUND] and r["checked"] == 2 and r["rounds"] == 1
    g, truth, q, L = cases["twin_slots"]
    r = lazy.plan(g, truth, q, L, 8)
    # 2 -> 1 by slot 1: slot 0 costs more, slot 2 is the same motion in a later slot
    assert r["status"][0] == ru.FOUND and r["cost"][0] == 2.0 and r["checked"] == 2
    assert r["verdict"][:, 2].tolist() == [lu.UNKNOWN, lu.FREE, lu.UNKNOWN]
    g, truth, q, L = cases["twin_slots_blocked"]
    r = lazy.plan(g, truth, q, L, 8)
    assert r["status"][0] == ru.FOUND and r["cost"][0] == 2.0 and r["rounds"] == 2 and r["checked"] == 3
    assert r["verdict"][:, 2].tolist() == [lu.UNKNOWN, lu.BLOCKED, lu.FREE]
    lu.assert_theorem("twin_slots_blocked", r, _eager(ref, g, truth, q, L))
    g, truth, q, L = cases["exactly_lmax"]
    r = lazy.plan(g, truth, q, L, 8)
    assert r["status"][0] == ru.FOUND and r["len"][0] == L == 6 and r["checked"] == 3
    assert np.all(r["verdict"][0, 1:] == lu.FREE)
    g, truth, q, L = cases["one_too_long"]
    r = lazy.plan(g, truth, q, L, 8)
    assert r["status"][0] == ru.TOO_LONG and r["checked"] == 0 and r["rounds"] == 0 and r["cost"][0] == 2.0
    assert np.all(r["verdict"][0, 1:] == lu.UNKNOWN)


def test_reset_forgets_the_verdicts(ref, lazy):
    g, truth, q, L = lu.prescribed_cases()["detour_blocked"]
    first = lazy.plan(g, truth, q, L, 8)
    assert first["cost"][0] == 2.5
    free = lu.all_free(g)
    kept = lazy.plan(g, free, q, L, 8, state=(first["w"], first["verdict"]))
    assert kept["cost"][0] == 2.5 and kept["checked"] == 0        # without a reset the old verdict stands
    fresh = lazy.plan(g, free, q, L, 8)
    assert fresh["status"][0] == ru.FOUND and fresh["cost"][0] == 2.0 and fresh["checked"] == 2
    assert fresh["verdict"][0, 3] == lu.FREE
    # a node that is not free blocks its slots at the reset, before any check
    truth = lu.all_free(g)
    truth["node_free"][2] = 0
    r = lazy.plan(g, truth, q, L, 0)
    assert r["verdict"][0, 3] == lu.BLOCKED and r["verdict"][0, 2] == lu.BLOCKED and r["verdict"][1, 3] == lu.UNKNOWN
    assert r["status"][0] == lu.UNSETTLED and r["cost"][0] == 2.5


@pytest.fixture(scope="module")
def wall(ref, oracle, chains, tmp_path_factory):
    """The wall scene as a lazy graph with the host motion check's truth table over all its slots, and the two pairs
    of roadmap_lazy_util.wall_pairs as queries."""
    sc = ru.wall_scene()
    motion = build_motion(str(tmp_path_factory.mktemp("motion")))
    n, N, k = 7, sc["N"], sc["k"]
    ch = chains["panda"][1]
    nodes = np.array([oracle.restart_seed(ch, sc["first"] + i) for i in range(N)]).T.copy()
    nbr, _ = ref.knn(nodes, nodes, k, True)
    frm, to = np.repeat(nodes.T[None], k, 0).reshape(-1, n), nodes.T[nbr.ravel()]
    w_eager = ru.host_checked_weights(sc, motion, frm, to).reshape(k, N)
    node_free = np.isfinite(ru.host_checked_weights(sc, motion, nodes.T, nodes.T))
    starts, goals = lu.wall_pairs(sc)
    s, g = starts.T.copy(), goals.T.copy()
    sidx, _ = ref.knn(s, nodes, k)
    gidx, _ = ref.knn(g, nodes, k)
    q = dict(start=s, goal=g, sidx=sidx, gidx=gidx,
             sw=np.stack([ru.host_checked_weights(sc, motion, starts, nodes.T[sidx[i]]) for i in range(k)]),
             gw=np.stack([ru.host_checked_weights(sc, motion, nodes.T[gidx[i]], goals) for i in range(k)]),
             direct=ru.host_checked_weights(sc, motion, starts, goals))
    graph = dict(nodes=nodes, nbr=nbr, w0=ru.np_weights(frm.T, to.T).reshape(k, N))
    truth = dict(edge_free=np.isfinite(w_eager).astype(np.uint8), node_free=node_free.astype(np.uint8))
    return graph, truth, q, w_eager


def test_wall_scene_lazy_equals_eager_and_checks_less(ref, lazy, wall):
    """The expectations of tests/test_gpu_roadmap_lazy.py's end-to-end test, from the host alone.  The scene's own
    pair has a route of one node (len 3): no graph edge, so nothing to check -- rounds 0, checked 0 --; the wide pair
    of roadmap_lazy_util.wall_pairs is the one whose first optimistic route is blocked."""
    graph, truth, q, w_eager = wall
    # the reset's rule agrees with the motion check: an edge with an end in collision is blocked by both
    assert np.array_equal(lu.eager_weights(graph, truth), w_eager)
    assert np.all(np.isinf(q["direct"]))
    eager = ref.query(dict(nodes=graph["nodes"], nbr=graph["nbr"], w=w_eager), q, 64)
    res = lazy.plan(graph, truth, q, 64, lu.MAX_ROUNDS)
    slots = int((graph["nbr"] >= 0).sum())
    print(f"wall scene: rounds {res['rounds']}, checked {res['checked']} of {slots} slots; eager len {eager['len']}")
    assert res["status"].tolist() == [ru.FOUND, ru.FOUND] == eager["status"].tolist()
    lu.assert_theorem("wall", res, eager)
    assert 0 < res["checked"] < slots and res["len"][0] == 3 and res["len"][1] > 3
    own = lazy.plan(graph, truth, ru.take_queries(q, [0]), 64, 0)
    assert own["status"][0] == ru.FOUND and own["checked"] == 0
    # the wide pair: its first optimistic route has a blocked edge, and one round does not settle it
    wide = ru.take_queries(q, [1])
    reset, one = lazy.plan(graph, truth, wide, 64, 0), lazy.plan(graph, truth, wide, 64, 1)
    assert int(((one["verdict"] == lu.BLOCKED) & (reset["verdict"] == lu.UNKNOWN)).sum()) >= 1
    assert reset["status"][0] == lu.UNSETTLED and one["status"][0] == lu.UNSETTLED and one["rounds"] == 1
    assert reset["cost"][0] <= one["cost"][0] <= res["cost"][1]
    both = lazy.plan(graph, truth, q, 64, 1)
    assert both["status"].tolist() == [ru.FOUND, lu.UNSETTLED]


# ---- the library: symbols and the refusals that need no device -----------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from optik_amd import build
    build.build()
    from optik_amd import _native
    return _native.lib()


def test_lazy_symbols_are_exported(lib):
    for name in ("optik_hip_roadmap_query_route", "optik_hip_roadmap_lazy_reset", "optik_hip_roadmap_lazy_plan",
                 "optik_hip_roadmap_lazy_plan_from_flags", "optik_robot_roadmap_build_lazy",
                 "optik_robot_roadmap_plan_lazy"):
        assert hasattr(lib, name), name


def test_argument_rules_on_the_host(lib):
    from optik_amd import _native as nat
    assert (nat.ROADMAP_SLOT_UNKNOWN, nat.ROADMAP_SLOT_FREE, nat.ROADMAP_SLOT_BLOCKED) == (lu.UNKNOWN, lu.FREE, lu.BLOCKED)
    assert nat.ROADMAP_UNSETTLED == lu.UNSETTLED and nat.ROADMAP_LAZY_MAX_ROUNDS == lu.MAX_ROUNDS
    assert nat.check_lazy_rounds(None) == nat.ROADMAP_LAZY_ROUNDS and nat.check_lazy_rounds(0) == 0
    assert nat.check_lazy_rounds(4096) == 4096
    for bad in (-1, 4097, 2.5, True):
        with pytest.raises(ValueError):
            nat.check_lazy_rounds(bad)
    # the kernel layer refuses a missing chain before any device work
    assert lib.optik_hip_roadmap_lazy_reset(None, None, None, 4, None, 4, 0, None, None, None, None, None) != 0
    assert lib.optik_hip_roadmap_lazy_plan(None, None, None, 4, None, None, None, 4, 0.1, None, None, 0, None, None, 4,
                                           None, None, 4, None, 8, 1, None, None, None, None, None, None, None) != 0
