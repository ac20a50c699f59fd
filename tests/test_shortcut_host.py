"""CPU-only: the arithmetic of path shortcutting and resampling (optik_amd/csrc/shortcut_measure.hpp, built with g++).
The route of the serial reference against a heapq Dijkstra on Python floats, bit for bit, over random visibility
matrices; the tie, penalty and status rules on inputs whose answers are known; the subdivision's budget; the
resampler's waypoints against the formula; the jagged route of the -m gpu end-to-end test, chosen here with the host
motion check; the exported symbols and the host-side refusals."""
import math

import numpy as np
import pytest

import shortcut_util as su
from motion_util import build_motion


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return su.build_shortcut_ref(str(tmp_path_factory.mktemp("shortcut_measure")))


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all(su.bits(got) == su.bits(want)))


# ---- the route --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [2, 3, 17, 64])
def test_route_matches_dijkstra(ref, V):
    rng = np.random.default_rng(V)
    P, n, hop = 6, 3, 0.05
    paths = su.random_polylines(rng, P, V, n)             # len = V: the vertices are the waypoints
    free = rng.random((P, su.pair_count(V))) > 0.3
    free[0] = True
    out = ref.shortcut(paths, None, V, free, hop, V)
    st, le, nv, verts = ref.vertices(paths, None, V)
    assert np.all(nv == V) and _same(verts[:, :V], paths)
    for p in range(P):
        d = su.dag_dijkstra(paths[p], V, V, free[p], hop)
        assert _same(out["d"][p, :V], d), p
        if not d[0] < math.inf:
            assert out["status"][p] == su.NO_ROUTE and _same(out["path"][p], paths[p]) and out["len"][p] == V
            continue
        assert out["status"][p] == su.FOUND
        r = su.route_of(out["path"][p], out["len"][p], paths[p], V)
        assert r[0] == 0 and r[-1] == V - 1 and all(a < b for a, b in zip(r, r[1:]))
        assert all(free[p, su.pair_index(V, a, b)] for a, b in zip(r, r[1:])), "every hop of the walk is a free motion"
        w = [float(np.max(np.abs(paths[p, b] - paths[p, a]))) for a, b in zip(r, r[1:])]
        assert su.bits(out["cost"][p]) == su.bits(su.path_cost_backwards(w))
        obj = 0.0
        for wt in reversed(w):
            obj = (wt + hop) + obj
        assert su.bits(obj) == su.bits(d[0]), "the walked route attains the objective"
        assert np.all(out["path"][p, out["len"][p]:] == paths[p, V - 1])
    assert out["status"][0] == su.FOUND and out["len"][0] == 2, "everything visible: the single hop"


def test_equal_routes_go_through_the_higher_vertex(ref):
    # 0 -> 3 is blocked; 0 -> 1 -> 3 and 0 -> 2 -> 3 both cost 1 + 2 = 2 + 1 = 3 exactly
    path = np.array([[[0.0], [1.0], [2.0], [3.0]]])
    free = np.ones((1, 6), dtype=bool)
    free[0, su.pair_index(4, 0, 3)] = False
    out = ref.shortcut(path, None, 4, free, 0.0, 4)
    assert out["status"][0] == su.FOUND and out["len"][0] == 3 and out["cost"][0] == 3.0
    assert out["path"][0, :3, 0].tolist() == [0.0, 2.0, 3.0]
    # and the route of fewer hops wins the tie against 0 -> 1 -> 2 -> 3
    free[0, su.pair_index(4, 0, 2)] = False
    free[0, su.pair_index(4, 1, 3)] = True
    out = ref.shortcut(path, None, 4, free, 0.0, 4)
    assert out["len"][0] == 3 and out["path"][0, :3, 0].tolist() == [0.0, 1.0, 3.0]


def test_hop_penalty_decides_between_collinear_routes(ref):
    # 0.2 + (0.9 - 0.2) rounds below 0.9, the direct hop: without a penalty the last bit decides
    path = np.array([[[0.0], [0.2], [0.9]]])
    free = np.ones((1, 3), dtype=bool)
    assert (0.2 - 0.0) + ((0.9 - 0.2) + 0.0) < 0.9
    out = ref.shortcut(path, None, 3, free, 0.0, 3)
    assert out["status"][0] == su.FOUND and out["len"][0] == 3, "the detour through the collinear vertex is one ulp shorter"
    out = ref.shortcut(path, None, 3, free, 0.05, 3)
    assert out["status"][0] == su.FOUND and out["len"][0] == 2 and out["cost"][0] == 0.9
    assert out["path"][0, :, 0].tolist() == [0.0, 0.9, 0.9]


def test_statuses(ref):
    rng = np.random.default_rng(5)
    paths = su.random_polylines(rng, 4, 6, 2, lens=[6, 6, 4, 6])
    free = np.ones((4, su.pair_count(6)), dtype=bool)
    for i in range(5):
        free[0, su.pair_index(6, i, 5)] = False           # nothing reaches the goal
    paths[1, 2, 1] = math.nan
    out = ref.shortcut(paths, [6, 6, 4, 6], 6, free, 0.01, 6)
    assert out["status"].tolist() == [su.NO_ROUTE, su.PATH_NAN, su.FOUND, su.FOUND]
    for p in (0, 1):
        assert np.array_equal(su.bits(out["path"][p]), su.bits(paths[p])) and out["len"][p] == 6
    assert math.isnan(out["cost_in"][1]) and math.isinf(out["d"][0, 0])
    assert out["len"][2] == 2 and out["len"][3] == 2
    assert np.array_equal(out["path"][2, 1], paths[2, 3]), "the goal is waypoint len - 1, not the padding's end"
    inf_path = paths[2:3].copy()
    inf_path[0, 1, 0] = math.inf
    assert ref.shortcut(inf_path, [4], 6, free[:1], 0.01, 6)["status"][0] == su.PATH_NAN
    # len > V, len < 2 and len > Lin: status 2 and the input back, or start and goal where it does not fit
    out = ref.shortcut(paths[2:], [6, 6], 5, np.ones((2, 10), dtype=bool), 0.0, 6)
    assert out["status"].tolist() == [su.BAD_LENGTH] * 2 and np.array_equal(out["path"][1], paths[3]) and out["len"][1] == 6
    out = ref.shortcut(paths[2:], [1, 9], 6, free[:2], 0.0, 3)
    assert out["status"].tolist() == [su.BAD_LENGTH] * 2 and out["len"].tolist() == [2, 2]
    assert np.array_equal(out["path"][1], paths[3][[0, 5, 5]])
    # a route that does not fit Lout: status 2, the route's true cost, the input back if it fits
    path = np.array([[[0.0], [1.0], [2.0], [3.0]]])
    chain_only = np.zeros((1, 6), dtype=bool)
    for i in range(3):
        chain_only[0, su.pair_index(4, i, i + 1)] = True
    out = ref.shortcut(path, None, 4, chain_only, 0.0, 3)
    assert out["status"][0] == su.BAD_LENGTH and out["cost"][0] == 3.0 and out["len"][0] == 2
    assert out["path"][0, :, 0].tolist() == [0.0, 3.0, 3.0]


# ---- the subdivision --------------------------------------------------------------------------------------------

def test_subdivision_keeps_the_budget_and_the_waypoints(ref):
    rng = np.random.default_rng(11)
    grew = 0
    for trial in range(200):
        L = int(rng.integers(2, 65))
        V = int(rng.integers(L, 65))
        path = su.random_polylines(rng, 1, L, 3)
        if L > 2 and trial % 3 == 0:
            path[0, L // 2] = path[0, L // 2 - 1]                    # a segment of length zero
        if trial % 4 == 0:
            path[0, L - 1:] += 50.0                                  # one segment far longer than the rest
        if trial % 50 == 7:
            path[0, :] = path[0, 0]                                  # T = 0: nothing to cut
        st, le, nv, verts = ref.vertices(path, None, V)
        assert st[0] == -1 and le[0] == L and L <= nv[0] <= V, (trial, L, V, nv[0])
        assert np.all(np.isnan(verts[0, nv[0]:])) and not np.any(np.isnan(verts[0, :nv[0]]))
        assert su.route_of(path[0], L, verts[0], nv[0])[-1] == nv[0] - 1, "every waypoint is a vertex, in order"
        if V == L or trial % 50 == 7:
            assert nv[0] == L
        grew += nv[0] > L
        # the pieces of a segment are evenly spaced along it: all on the polyline
        seg = np.max(np.abs(np.diff(verts[0, :nv[0]], axis=0)), axis=1)
        assert seg.sum() <= np.max(np.abs(np.diff(path[0], axis=0)), axis=1).sum() * (1 + 1e-12)
    assert grew > 100
    # len > V
    st, le, nv, _ = ref.vertices(su.random_polylines(rng, 1, 9, 3), None, 8)
    assert st[0] == su.BAD_LENGTH and nv[0] == 0


def test_subdivision_follows_the_spacing(ref):
    # lengths 1, 3 and 0 with V = 12: sp = 4 / 8, pieces 2, 6 and 1: 10 vertices
    path = np.array([[[0.0, 0.0], [1.0, 0.5], [1.0, 3.5], [1.0, 3.5]]])
    st, le, nv, verts = ref.vertices(path, None, 12)
    assert nv[0] == 10
    assert verts[0, :10, 1].tolist() == [0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 3.5]
    assert verts[0, 1, 0] == 0.5


# ---- resampling ---------------------------------------------------------------------------------------------------

def _check_resampled(path, L, out):
    """Every waypoint between the ends is qa + t (qb - qa) of the segment that holds its arc, with 0 <= t <= 1 as the
    header's step 7 forms it on Python floats, and the arcs do not decrease."""
    w = [float(np.max(np.abs(path[s + 1] - path[s]))) for s in range(L - 1)]
    c = [0.0]
    for ws in w:
        c.append(c[-1] + ws)
    T, last = c[-1], 0.0
    for j in range(1, len(out) - 1):
        a = T * (float(j) / float(len(out) - 1))
        s = max(u for u in range(L - 1) if c[u] <= a)
        t = min((a - c[s]) / w[s], 1.0) if w[s] > 0.0 else 0.0
        assert 0.0 <= t <= 1.0 and a >= last
        last = a
        want = path[0] if T == 0.0 else path[s] + t * (path[s + 1] - path[s])
        assert np.array_equal(su.bits(out[j]), su.bits(want)), j


@pytest.mark.parametrize("L,Lout", [(2, 2), (2, 64), (3, 3), (17, 32), (64, 2), (64, 64), (5, 33)])
def test_resample_waypoints_lie_on_the_input(ref, L, Lout):
    rng = np.random.default_rng(100 * L + Lout)
    paths = su.random_polylines(rng, 3, L, 4)
    if L > 3:
        paths[1, 2] = paths[1, 1]
    out, st = ref.resample(paths, None, Lout)
    assert st.tolist() == [0, 0, 0]
    for p in range(3):
        assert np.array_equal(su.bits(out[p, 0]), su.bits(paths[p, 0]))
        assert np.array_equal(su.bits(out[p, -1]), su.bits(paths[p, L - 1]))
        _check_resampled(paths[p], L, out[p])


def test_resample_spacing_and_edge_cases(ref):
    a, b = np.array([0.3, -1.0, 2.0]), np.array([1.7, 0.25, 2.0])
    out, st = ref.resample(np.array([[a, b]]), None, 64)
    T = np.max(np.abs(b - a))
    step = np.max(np.abs(np.diff(out[0], axis=0)), axis=1)
    assert st[0] == 0 and np.all(np.abs(step - T / 63) <= 4 * np.spacing(T)), "equal spacing to a few ulp of T"
    # a lens below the padded length: the goal is waypoint len - 1
    paths = su.random_polylines(np.random.default_rng(2), 1, 8, 2, lens=[3])
    out, st = ref.resample(paths, [3], 5)
    assert st[0] == 0 and np.array_equal(out[0, -1], paths[0, 2])
    _check_resampled(paths[0], 3, out[0])
    # equal ends, T = 0: the start everywhere
    same = np.array([[a, a], [a, a]])
    same[1, 1, 2] = -same[1, 1, 2] * 0.0 + a[2]
    out, st = ref.resample(same, None, 7)
    assert st.tolist() == [0, 0] and np.all(out == a[None, None])
    out, st = ref.resample(np.array([[a, a, a, a]]), None, 7)
    assert st[0] == 0 and np.all(out == a[None, None])
    # a NaN and an infinity: status 3, the start, then the goal repeated
    bad = np.array([[a, b, a], [a, b, a]])
    bad[0, 1, 0] = math.nan
    bad[1, 2, 1] = math.inf
    out, st = ref.resample(bad, None, 4)
    assert st.tolist() == [su.PATH_NAN] * 2
    for p in range(2):
        assert np.array_equal(su.bits(out[p, 0]), su.bits(bad[p, 0]))
        assert all(np.array_equal(su.bits(out[p, t]), su.bits(bad[p, 2])) for t in (1, 2, 3))
    # a bad length is read as clamped
    out, st = ref.resample(np.array([[a, b, a]]), [7], 3)
    assert st[0] == su.BAD_LENGTH and np.array_equal(out[0, -1], a)


# ---- the scene of the end-to-end test -----------------------------------------------------------------------------

def test_wall_route_is_free_and_gets_shorter(ref, tmp_path):
    """The expectation of tests/test_gpu_path_shortcut.py's end-to-end test, from the host alone."""
    sc = su.wall_scene()
    motion = build_motion(str(tmp_path))
    route = np.array(su.WALL_ROUTE)
    assert np.array_equal(route[0], sc["start"]) and np.array_equal(route[-1], sc["goal"])
    assert np.all(np.isfinite(su.host_checked_weights(sc, motion, route[:-1], route[1:]))), "the input is a free path"
    assert su.host_checked_weights(sc, motion, route[:1], route[-1:])[0] == math.inf, "and the straight move is not"
    V = su.WALL_VERTICES
    st, le, nv, verts = ref.vertices(route[None], None, V)
    assert len(route) < nv[0] <= V
    qa, qb = su.pair_segments(verts[0], V)
    real = ~np.isnan(qa[:, 0])
    free = np.zeros(len(qa), dtype=bool)
    free[real] = np.isfinite(su.host_checked_weights(sc, motion, qa[real], qb[real]))
    out = ref.shortcut(route[None], None, V, free[None], sc["h"], len(route))
    assert out["status"][0] == su.FOUND
    assert out["len"][0] < len(route) and out["cost"][0] < out["cost_in"][0]
    r = su.route_of(out["path"][0], out["len"][0], verts[0], nv[0])
    assert r == su.WALL_SHORTCUT
    assert all(free[su.pair_index(V, a, b)] for a, b in zip(r, r[1:])), "every hop is free"


# ---- the library: symbols and the refusals that need no device -----------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from optik_amd import build
    build.build()
    from optik_amd import _native
    return _native.lib()


def test_shortcut_symbols_are_exported(lib):
    for name in ("optik_hip_path_shortcut", "optik_hip_path_resample", "optik_hip_path_shortcut_chunk",
                 "optik_robot_path_shortcut", "optik_robot_path_resample"):
        assert hasattr(lib, name), name


def test_argument_rules_on_the_host(lib):
    from optik_amd import _native as nat
    assert nat.PATH_SHORTCUT_MAX_VERTICES == su.MAX_POINTS
    assert nat.check_shortcut_args(64, 64, 64, 0.05, None) == (0.05, 0.05)
    assert nat.check_shortcut_args(2, 2, 2, 0.1, 0.0) == (0.1, 0.0)
    for kw in (dict(vertices=1), dict(vertices=65), dict(max_waypoints=1), dict(max_waypoints=65), dict(L=1),
               dict(L=65), dict(vertices=True), dict(vertices=2.5), dict(resolution=0.0), dict(resolution=-1.0),
               dict(resolution=math.nan), dict(hop_penalty=-1.0), dict(hop_penalty=math.nan),
               dict(hop_penalty=math.inf)):
        with pytest.raises(ValueError):
            nat.check_shortcut_args(**kw)
    # the kernel layer refuses a null chain before any device work
    assert lib.optik_hip_path_shortcut(None, None, None, None, 4, 0, 4, 0.05, 0.0, 4, None, None, None, None, None,
                                       None) != 0
    assert lib.optik_hip_path_resample(None, None, None, 4, 0, 4, None, None, None) != 0
