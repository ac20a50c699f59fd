"""CPU-only: the arithmetic of roadmap planning (optik_amd/csrc/roadmap_measure.hpp, built with g++).  The serial
reference's distances against a heapq Dijkstra on Python floats, bit for bit; the order of the neighbours against a
numpy sort; the successor, first-hop and status rules on graphs whose answers are known; the wall scene of the -m gpu
end-to-end test, chosen here with the host motion check; the exported symbols and the host-side refusals."""
import math

import numpy as np
import pytest

import roadmap_util as ru
from motion_util import build_motion


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ru.build_roadmap_ref(str(tmp_path_factory.mktemp("roadmap_measure")))


@pytest.fixture(scope="module")
def cases(ref):
    return {name: (g, q, L, ref.query(g, q, L)) for name, g, q, L in ru.synthetic_cases()}


def test_weight_is_the_motion_distance(ref):
    rng = np.random.default_rng(3)
    a, b = rng.uniform(-3, 3, (50, 7)), rng.uniform(-3, 3, (50, 7))
    a[0, 2] = math.nan
    b[1, 6] = math.nan
    b[2, 0] = math.inf
    got = ref.weight(a, b)
    assert np.array_equal(ru.bits(got[3:]), ru.bits(ru.np_weights(a.T, b.T)[3:]))
    assert math.isnan(got[0]) and math.isnan(got[1]) and got[2] == math.inf


def test_order_of_distance_and_index(ref):
    nan, inf = math.nan, math.inf
    rows = [(1.0, 5, 2.0, 3, True), (2.0, 3, 1.0, 5, False), (1.0, 3, 1.0, 5, True), (1.0, 5, 1.0, 3, False),
            (inf, 9, nan, 0, True), (nan, 0, inf, 9, False), (nan, 1, nan, 2, True), (nan, 2, nan, 1, False),
            (0.0, 1, -0.0, 2, True), (-0.0, 2, 0.0, 1, False), (nan, 7, inf, -1, True), (1.0, 4, 1.0, 4, False)]
    got = ref.ranks_before(np.array([r[:4] for r in rows], dtype=np.float64))
    assert got.tolist() == [r[4] for r in rows]


@pytest.mark.parametrize("k", [1, 8, 16])
def test_knn_reference_matches_numpy_sort(ref, k):
    rng = np.random.default_rng(11)
    n, N = 4, 70
    nodes = rng.uniform(-2, 2, (n, N))
    nodes[:, 10] = nodes[:, 3]   # exact duplicates: the index decides
    nodes[:, 40] = nodes[:, 3]
    nodes[2, 25] = math.nan      # a NaN node ranks after every number
    for q, self in ((nodes, True), (rng.uniform(-2, 2, (n, 5)), False)):
        idx, dist = ref.knn(q, nodes, k, self)
        widx, wdist = ru.np_knn(q, nodes, k, self)
        assert np.array_equal(idx, widx)
        assert np.array_equal(ru.bits(dist)[~np.isnan(wdist)], ru.bits(wdist)[~np.isnan(wdist)])
        assert np.array_equal(np.isnan(dist), np.isnan(wdist))
    idx, _ = ref.knn(nodes[:, 3:4], nodes, 16)
    assert idx[:3, 0].tolist() == [3, 10, 40] and 25 not in idx[:, 0]
    idx, dist = ref.knn(nodes[:, :1], nodes[:, :5], 16, False)
    assert idx[5:, 0].tolist() == [-1] * 11 and np.all(dist[5:, 0] == math.inf) and np.all(idx[:5, 0] >= 0)
    # with fewer numbers than k the NaN node is listed, after them
    idx, dist = ref.knn(nodes[:, 24:25], nodes[:, 24:27], 3, False)
    assert idx[:, 0].tolist() == [0, 2, 1] and math.isnan(dist[2, 0])


def test_distances_equal_dijkstra_bit_for_bit(cases):
    for name, (g, q, L, res) in cases.items():
        for j in range(q["start"].shape[1]):
            d, cost = ru.dijkstra_cost(g, q, j)
            assert np.array_equal(ru.bits(res["d"][j]), ru.bits(d)), (name, j)
            if res["status"][j] != ru.QUERY_NAN:
                assert ru.bits(res["cost"][j]) == ru.bits(cost), (name, j)


def test_ring_needs_every_sweep_and_reports_the_true_cost(cases):
    g, q, L, res = cases["ring130"]
    # node v is v hops from node 0: 0.5 at the goal link, then 0.25 a hop, added from the goal backwards
    want = [0.5]
    for _ in range(129):
        want.append(0.25 + want[-1])
    assert np.array_equal(ru.bits(res["d"][0]), ru.bits(np.array(want)))
    assert res["status"][0] == ru.TOO_LONG and res["len"][0] == 2 and res["cost"][0] == 0.5 + want[129]
    assert np.array_equal(res["path"][0, 0], q["start"][:, 0]) and np.all(res["path"][1:, 0] == q["goal"][:, 0])
    g, q, L, res = cases["ring130_near"]
    assert res["status"][0] == ru.FOUND and res["len"][0] == 43
    assert np.array_equal(res["path"][1:42, 0, 0], g["nodes"][0, 40::-1])


def test_two_components(cases):
    g, q, L, res = cases["two_components"]
    assert res["status"][:2].tolist() == [ru.NO_ROUTE, ru.NO_ROUTE] and np.all(res["cost"][:2] == math.inf)
    assert np.all(np.isinf(res["d"][:, :20]))          # the goals are all in the second half
    assert np.all(res["len"][:2] == 2)


def test_successor_and_first_hop_ties(cases):
    g, q, L, res = cases["equal_routes"]
    assert res["status"][0] == ru.FOUND and res["len"][0] == 5 and res["cost"][0] == 2.0
    # start, node 3, then node 1 -- the lower index, though node 2 sits in the earlier slot --, node 0, goal
    want = np.stack([q["start"][:, 0], g["nodes"][:, 3], g["nodes"][:, 1], g["nodes"][:, 0], q["goal"][:, 0]])
    assert np.array_equal(res["path"][:5, 0], want) and np.all(res["path"][5:, 0] == q["goal"][:, 0])
    g, q, L, res = cases["direct_tie"]                   # the same cost directly: the direct edge wins
    assert res["status"][0] == ru.FOUND and res["len"][0] == 2 and res["cost"][0] == 2.0
    g, q, L, res = cases["slot_tie"]                     # two start links of the same cost: the lower slot
    assert res["status"][0] == ru.FOUND and res["len"][0] == 4 and res["cost"][0] == 2.0
    assert np.array_equal(res["path"][1, 0], g["nodes"][:, 2])


def test_each_status_and_the_waypoint_cap(cases):
    seen = set()
    for name, (g, q, L, res) in cases.items():
        seen |= set(res["status"].tolist())
        for j, st in enumerate(res["status"]):
            if st != ru.FOUND:
                assert res["len"][j] == 2 and np.all(res["path"][1:, j] == q["goal"][:, j][None]), (name, j)
            assert ru.bits(res["path"][0, j]).tolist() == ru.bits(q["start"][:, j]).tolist()
    assert seen == {ru.FOUND, ru.NO_ROUTE, ru.TOO_LONG, ru.QUERY_NAN}
    _, _, _, res = cases["lmax2_route"]
    assert res["status"][0] == ru.TOO_LONG and res["cost"][0] == 1.0   # 0.25 + 0.5 + 0.25, not the direct 5.0
    _, _, _, res = cases["lmax2_direct"]
    assert res["status"][0] == ru.FOUND and res["len"][0] == 2 and res["cost"][0] == 5.0
    for name in ("nan_start", "nan_link"):
        _, _, _, res = cases[name]
        assert res["status"][0] == ru.QUERY_NAN and math.isnan(res["cost"][0]) and res["len"][0] == 2


def test_wall_scene_is_blocked_and_has_a_route(ref, oracle, chains, tmp_path):
    """The expectation of tests/test_gpu_roadmap.py's end-to-end test, from the host alone: the straight move is not
    free, and the serial reference finds a route over the scene's N nodes."""
    sc = ru.wall_scene()
    motion = build_motion(str(tmp_path))
    n, N, k = 7, sc["N"], sc["k"]
    assert N <= 1024 and k <= 16
    ch = chains["panda"][1]
    nodes = np.array([oracle.restart_seed(ch, sc["first"] + i) for i in range(N)]).T.copy()
    s, g = sc["start"][:, None], sc["goal"][:, None]
    direct = ru.host_checked_weights(sc, motion, s.T, g.T)
    assert direct[0] == math.inf
    # the ends themselves are free: a motion of length 0 from each
    assert np.all(np.isfinite(ru.host_checked_weights(sc, motion, np.stack([s[:, 0], g[:, 0]]),
                                                       np.stack([s[:, 0], g[:, 0]]))))
    nbr, _ = ref.knn(nodes, nodes, k, True)
    w = ru.host_checked_weights(sc, motion, np.repeat(nodes.T[None], k, 0).reshape(-1, n),
                                nodes.T[nbr.ravel()]).reshape(k, N)
    sidx, _ = ref.knn(s, nodes, k)
    gidx, _ = ref.knn(g, nodes, k)
    sw = ru.host_checked_weights(sc, motion, np.repeat(s.T, k, 0), nodes.T[sidx[:, 0]])[:, None]
    gw = ru.host_checked_weights(sc, motion, nodes.T[gidx[:, 0]], np.repeat(g.T, k, 0))[:, None]
    res = ref.query(dict(nodes=nodes, nbr=nbr, w=w),
                    dict(start=s, goal=g, sidx=sidx, sw=sw, gidx=gidx, gw=gw, direct=direct), 64)
    assert res["status"][0] == ru.FOUND and 3 <= res["len"][0] <= 64 and math.isfinite(res["cost"][0])


# ---- the library: symbols and the refusals that need no device -----------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from optik_amd import build
    build.build()
    from optik_amd import _native
    return _native.lib()


def test_roadmap_symbols_are_exported(lib):
    for name in ("optik_hip_roadmap_knn", "optik_hip_roadmap_edges", "optik_hip_roadmap_query",
                 "optik_robot_roadmap_build", "optik_robot_roadmap_plan"):
        assert hasattr(lib, name), name


def test_argument_rules_on_the_host(lib):
    from optik_amd import _native as nat
    assert nat.ROADMAP_MAX_NODES == ru.MAX_NODES and nat.ROADMAP_MAX_K == ru.K_MAX
    nat.check_roadmap_args(N=8192, k=16, max_waypoints=64)
    nat.check_roadmap_args(N=1, k=1, max_waypoints=2)
    for kw in (dict(k=0), dict(k=17), dict(N=8193), dict(N=0), dict(max_waypoints=1), dict(max_waypoints=65),
               dict(k=True), dict(N=2.5)):
        with pytest.raises(ValueError):
            nat.check_roadmap_args(**kw)
    # the kernel layer refuses the same before any device work
    assert lib.optik_hip_roadmap_knn(None, None, 0, None, 4, 4, 0, None, None, None) != 0
