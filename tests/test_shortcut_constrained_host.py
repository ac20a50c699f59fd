"""The rules of shortcutting and resampling under a pose constraint (csrc/shortcut_constrained_measure.hpp) on the host:
the serial references with g++ and Python callbacks (shortcut_constrained_util), the constraint with
constraint_measure.hpp on the host.  No GPU."""
import math

import numpy as np
import pytest

import shortcut_constrained_util as xu
import shortcut_util as su

LENS = [2, 3, 9, 9, 7, 12]


def _paths():
    """The random walks of tests/test_shortcut_host.py's route test (seed, P = 6, n = 3) with mixed lengths: one longer
    than its L allows and one with a NaN."""
    rng = np.random.default_rng(17)
    paths = su.random_polylines(rng, 6, 9, 3, lens=[min(v, 9) for v in LENS])
    paths[4, 3, 1] = math.nan
    return paths


IDENTITY = lambda x: (x, xu.PROJECTED, 0)  # noqa: E731


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return xu.build_shortcut_constrained_ref(str(tmp_path_factory.mktemp("shortcut_constrained_measure")))


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return su.build_shortcut_ref(str(tmp_path_factory.mktemp("shortcut_measure")))


@pytest.fixture(scope="module")
def cmlib(tmp_path_factory):
    return xu.build_host_constraint_lib(str(tmp_path_factory.mktemp("constraint_host")))


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((su.bits(a) == su.bits(b)) | (np.isnan(a) & np.isnan(b))))


# ---- callbacks that change nothing: the unconstrained references, bit for bit -------------------------------------------

@pytest.mark.parametrize("V", [2, 9, 33, 64])
def test_idle_callbacks_give_the_unconstrained_shortcut(ref, plain, V):
    paths = _paths()
    P = len(paths)
    rng = np.random.default_rng(V)
    free = rng.random((P, su.pair_count(V))) < 0.7
    for Lout in (2, 64):
        want = plain.shortcut(paths, LENS, V, free, 0.01, Lout)
        got = ref.shortcut(paths, LENS, V, IDENTITY, xu.flags_open(free, V), 0.01, Lout)
        for key in ("status", "len"):
            assert np.array_equal(got[key], want[key]), (V, Lout, key)
        for key in ("cost", "cost_in", "path", "d"):
            assert _same(got[key], want[key]), (V, Lout, key)
    st, le, nv, verts = plain.vertices(paths, LENS, V)
    gv = ref.vertices(paths, LENS, V, IDENTITY)
    assert np.array_equal(gv["status"], st) and np.array_equal(gv["nv"], nv) and _same(gv["verts"], verts)
    # rule 8: one projection per vertex that is not an input waypoint, none where prepare gave a status
    want_count = np.where(st == -1, nv - le, 0)
    assert np.array_equal(gv["projected"][:, 0], want_count) and np.array_equal(gv["projected"][:, 1], want_count)
    assert np.array_equal(got["projected"], gv["projected"])
    # rule 3': every pair i < j < nv is asked once, vertex i -> vertex j
    for p in range(P):
        asked = got["asked"][p]
        n_v = int(nv[p]) if st[p] == -1 else 0
        assert sorted(asked) == [(i, j) for i in range(n_v) for j in range(i + 1, n_v)] and len(set(asked)) == len(asked)


@pytest.mark.parametrize("Lout", [2, 3, 17, 64])
def test_idle_callbacks_give_the_unconstrained_resampling(ref, plain, Lout):
    paths = _paths()
    want, wst = plain.resample(paths, LENS, Lout)
    got, st, projected = ref.resample(paths, LENS, Lout, IDENTITY)
    assert np.array_equal(st, wst) and _same(got, want)
    inner = np.where(wst == su.PATH_NAN, 0, Lout - 2)
    assert np.array_equal(projected[:, 0], inner) and np.array_equal(projected[:, 1], inner)


# ---- rule 2': a dead vertex ---------------------------------------------------------------------------------------------

def test_a_dead_vertex_is_nan_and_on_no_route(ref, plain):
    """Vertex 2 of 5 on a straight two-waypoint path does not project (the status of a spent budget): it is NaN, it is
    counted as attempted and not as projected, pairs with it are closed because no motion check samples a NaN end,
    and the route goes round it."""
    path = np.zeros((1, 2, 3))
    path[0, 1] = [0.4, -0.2, 0.1]
    V = 6                                     # four pieces of the one segment: five vertices

    def project(x):
        return (x, xu.BUDGET_SPENT, 0) if abs(x[0] - 0.2) < 1e-12 else (x + [0.0, 0.5, 0.0], xu.PROJECTED, 1)

    v = ref.vertices(path, None, V, project)
    assert v["nv"][0] == 5 and v["projected"][0].tolist() == [3, 2]
    assert np.isnan(v["verts"][0, 2]).all() and np.isfinite(v["verts"][0, [0, 1, 3, 4]]).all()
    assert v["iterations"][0, :5].tolist() == [-1, 1, 0, 1, -1]
    assert _same(v["verts"][0, 0], path[0, 0]) and _same(v["verts"][0, 4], path[0, 1]), "the ends never move"
    unprojected = plain.vertices(path, None, V)[3]
    assert _same(v["verts"][0, [1, 3]], unprojected[0, [1, 3]] + [0.0, 0.5, 0.0]), "a vertex is its projection's result"
    # what both motion checks say of a NaN end: not sampled, so not open; only neighbours two apart at most are open
    res = ref.shortcut(path, None, V, project,
                       lambda p, i, j, qa, qb: bool(np.isfinite(qa).all() and np.isfinite(qb).all() and j - i <= 2),
                       0.0, 8)
    assert res["status"][0] == su.FOUND and res["projected"][0].tolist() == [3, 2]
    L = int(res["len"][0])
    assert np.isfinite(res["path"][0]).all()
    route = su.route_of(res["path"][0], L, res["verts"][0], 5)
    assert route == [0, 1, 3, 4] and 2 not in route
    assert math.isinf(res["d"][0, 2]), "nothing leaves a dead vertex"
    # the cost is taken over the projected vertices and may exceed the input's
    assert res["cost"][0] > res["cost_in"][0] == 0.4


def test_a_spent_budget_on_the_panda_makes_a_dead_vertex(ref, cmlib, chains, oracle):
    """piters = 0 and a ptol the interpolated vertex violates: constraint_measure.hpp's own status BUDGET_SPENT."""
    d, ch = chains["panda"]
    home = _home(d)
    hc = xu.HostConstraint(cmlib, d, xu.upright_constraint(np.asarray(oracle.fk(ch, home)[1]), 0.01))
    path = np.stack([home, home + 0.4])[None]
    project = lambda x: hc.project(x, 1e-9, 0, xu.DAMPING, xu.MAX_STEP)  # noqa: E731
    assert project(0.5 * (path[0, 0] + path[0, 1]))[1] == xu.BUDGET_SPENT
    v = ref.vertices(path, None, 4, project)
    assert v["projected"][0].tolist() == [1, 0] and np.isnan(v["verts"][0, 1]).all()
    res = ref.shortcut(path, None, 4, project, lambda p, i, j, qa, qb: bool(np.isfinite(qa + qb).all()), 0.0, 4)
    assert res["status"][0] == su.FOUND and res["len"][0] == 2 and _same(res["path"][0, :2], path[0])
    # and when the ends do not see each other there is no route at all
    res = ref.shortcut(path, None, 4, project, lambda p, i, j, qa, qb: bool(np.isfinite(qa + qb).all()) and j - i < 2,
                       0.0, 4)
    assert res["status"][0] == su.NO_ROUTE and _same(res["path"][0, :2], path[0])


# ---- rule 3': one verdict closes one pair, in its direction -------------------------------------------------------------

def test_a_constraint_verdict_closes_exactly_its_pair(ref, plain):
    paths = _paths()[2:3]
    lens, V = LENS[2:3], 9
    free = np.ones((1, su.pair_count(V)), dtype=bool)
    base = ref.shortcut(paths, lens, V, IDENTITY, xu.flags_open(free, V), 0.0, 64)
    nv = int(ref.vertices(paths, lens, V, IDENTITY)["nv"][0])
    assert base["status"][0] == su.FOUND and base["len"][0] == 2 and nv > 3
    seen = []

    def open_but(i0, j0):
        def f(p, i, j, qa, qb):
            seen.append((i, j))
            return free[p, su.pair_index(V, i, j)] and not (i == i0 and j == j0)  # collision verdict AND constraint verdict
        return f

    got = ref.shortcut(paths, lens, V, IDENTITY, open_but(0, nv - 1), 0.0, 64)
    cok = free.copy()
    cok[0, su.pair_index(V, 0, nv - 1)] = False
    want = plain.shortcut(paths, lens, V, free & cok, 0.0, 64)
    assert got["len"][0] == 3 and np.array_equal(got["len"], want["len"]) and _same(got["path"], want["path"])
    assert _same(got["d"], want["d"])
    # only that pair: every other objective that does not use it is what it was
    assert _same(got["d"][0, 1:], base["d"][0, 1:])
    assert all(i < j for i, j in seen), "a pair is only ever asked in the direction of travel, i -> j"
    # the reversed pair does not exist: closing (j, i) changes nothing
    same = ref.shortcut(paths, lens, V, IDENTITY, open_but(nv - 1, 0), 0.0, 64)
    assert _same(same["path"], base["path"]) and _same(same["d"], base["d"])


# ---- rule 7': the status precedence ---------------------------------------------------------------------------------------

def test_resample_status_precedence(ref):
    rng = np.random.default_rng(4)
    paths = su.random_polylines(rng, 4, 6, 3, scale=0.3)
    paths[2, 1, 0] = math.nan
    lens = [6, 7, 6, 1]                       # fine, too long, NaN, too short
    fail = lambda x: (x + 1.0, xu.BUDGET_SPENT, 0)  # noqa: E731
    out, st, projected = ref.resample(paths, lens, 5, fail)
    assert st.tolist() == [xu.UNPROJECTED, su.BAD_LENGTH, su.PATH_NAN, su.BAD_LENGTH]
    assert projected.tolist() == [[3, 0], [3, 0], [0, 0], [3, 0]], "a PATH_NAN row is not projected; a BAD_LENGTH row is"
    plain_out, plain_st, _ = ref.resample(paths, lens, 5, IDENTITY)
    assert plain_st.tolist() == [0, su.BAD_LENGTH, su.PATH_NAN, su.BAD_LENGTH]
    assert _same(out, plain_out), "a projection that is not PROJECTED leaves the interpolated value"
    # a projection that works moves the interior waypoints and only them
    out, st, projected = ref.resample(paths, lens, 5, lambda x: (x + 1.0, xu.PROJECTED, 2))
    assert st.tolist() == plain_st.tolist() and projected.tolist() == [[3, 3], [3, 3], [0, 0], [3, 3]]
    assert _same(out[0, 1:4], plain_out[0, 1:4] + 1.0) and _same(out[0, [0, 4]], plain_out[0, [0, 4]])
    # one failure among successes is enough for status 4; Lout = 2 projects nothing
    calls = []
    out, st, projected = ref.resample(paths[:1], lens[:1], 5,
                                      lambda x: (x, xu.FAILED if len(calls) == 1 else xu.PROJECTED, calls.append(0) or 0))
    assert st.tolist() == [xu.UNPROJECTED] and projected.tolist() == [[3, 2]]
    out, st, projected = ref.resample(paths[:1], lens[:1], 2, fail)
    assert st.tolist() == [0] and projected.tolist() == [[0, 0]]


# ---- the scene of the GPU parity tests ------------------------------------------------------------------------------------

def _home(d):
    lo, hi = np.asarray(d["lb"]), np.asarray(d["ub"])
    return np.clip(0.5 * (lo + hi) + 0.1, lo + 0.2, hi - 0.2)


@pytest.mark.parametrize("name, V, Lin", [("panda", 8, 8), ("panda", 64, 64), ("arm10", 8, 8)])
def test_the_gpu_scene_has_what_parity_needs(ref, cmlib, chains, oracle, name, V, Lin):
    """A parity test on a scene where no vertex moves, no pair is closed by the constraint and nothing is shortened
    shows nothing: the scene the GPU tests use (no collision model: every sampled motion is free) has a) a vertex
    that moved under projection, b) a pair only the constraint closes, c) a FOUND route with fewer vertices than its
    input."""
    d, ch = chains[name]
    home = _home(d)
    c = xu.upright_constraint(np.asarray(oracle.fk(ch, home)[1]), xu.TILT)
    hc = xu.HostConstraint(cmlib, d, c)
    paths, lens = xu.scene_paths(hc, d["lb"], d["ub"], 11, V, Lin, home)
    project = lambda x: hc.project(x, xu.PTOL, xu.PITERS, xu.DAMPING, xu.MAX_STEP)  # noqa: E731
    v = ref.vertices(paths, lens, V, project)
    if V > 8:
        assert (v["iterations"] >= 1).any(), "a): a vertex moved under projection"
        assert (v["projected"][:, 1] > 0).any()
    closed = []

    def pair_open(p, i, j, qa, qb):
        ok = bool(hc.motion_ok(qa, qb, xu.H, xu.TOL)[0])
        if not ok and np.isfinite(qa + qb).all():
            closed.append((p, i, j))
        return ok

    res = ref.shortcut(paths, lens, V, project, pair_open, xu.H, Lin)
    assert closed, "b): a pair of finite vertices that only the constraint closes (there is no collision model)"
    found = res["status"] == su.FOUND
    assert (found & (res["len"] < np.array(lens))).any(), "c): a found route with fewer vertices than its input"
    assert res["status"][4] in (su.PATH_NAN, su.BAD_LENGTH)
