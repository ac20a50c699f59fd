"""-m gpu: roadmap planning on the device against the host.  roadmap_knn against numpy (abs, max, a stable
lexicographic sort) and roadmap_query against the serial reference of csrc/roadmap_measure.hpp (g++) and a heapq
Dijkstra, all bit for bit, on the synthetic graphs of roadmap_util; roadmap_edges against collision_motion_batch on
the same segments; build_roadmap / plan_paths end to end on the wall scene that tests/test_roadmap_host.py chooses on
the CPU; staleness and the refusals."""
import math

import numpy as np
import pytest

import roadmap_util as ru
from conftest import ROBOT_SPECS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def robots():
    from optik_amd import Robot
    made = {}

    def get(name):
        if name not in made:
            made[name] = Robot.from_urdf_file(*ROBOT_SPECS[name])
        return made[name]
    return get


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ru.build_roadmap_ref(str(tmp_path_factory.mktemp("roadmap_measure")))


@pytest.fixture(scope="module")
def cases(ref):
    return [(name, g, q, L, ref.query(g, q, L)) for name, g, q, L in ru.synthetic_cases()]


def _t(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all((ru.bits(got) == ru.bits(want)) | (np.isnan(got) & np.isnan(want))))


CHAIN_OF_N = {1: "panda1", 2: "panda2", 3: "panda3", 7: "panda", 8: "arm8", 10: "arm10"}


def _knn_check(torch, robots, n, q, nodes, k, exclude_self):
    hc = robots(CHAIN_OF_N[n]).hip_chain()
    idx, dist = hc.roadmap_knn(_t(torch, q), _t(torch, nodes), k, exclude_self)
    widx, wdist = ru.np_knn(q, nodes, k, exclude_self)
    assert np.array_equal(idx.cpu().numpy(), widx)
    assert _same(dist.cpu().numpy(), wdist)
    return widx, wdist


@pytest.mark.parametrize("n", [1, 7, 8, 10])
@pytest.mark.parametrize("k", [1, 8, 16])
def test_knn_matches_numpy(torch_dev, robots, n, k):
    rng = np.random.default_rng(100 * n + k)
    nodes = rng.uniform(-2.5, 2.5, (n, 257))     # 257: a second tile of one node, five blocks of queries
    nodes[:, 200] = nodes[:, 7]                  # exact duplicates: the index decides
    nodes[:, 256] = nodes[:, 7]
    nodes[n - 1, 100] = math.nan                 # one NaN node
    _knn_check(torch_dev, robots, n, rng.uniform(-2.5, 2.5, (n, 3)), nodes, k, False)
    widx, _ = _knn_check(torch_dev, robots, n, nodes, nodes, k, True)
    assert not np.any(widx == np.arange(257)[None])
    widx, wdist = _knn_check(torch_dev, robots, n, nodes[:, 7:8], nodes, k, False)
    assert widx[:min(k, 3), 0].tolist() == [7, 200, 256][:k]
    widx, wdist = _knn_check(torch_dev, robots, n, nodes[:, :2], nodes[:, :5], k, False)   # N = 5 < k
    assert np.all(widx[5:] == -1) and np.all(wdist[5:] == math.inf)


def _device_query(torch, robots, g, q, L):
    hc = robots(CHAIN_OF_N[g["nodes"].shape[0]]).hip_chain()
    t = lambda a: _t(torch, a)  # noqa: E731
    res = hc.roadmap_query(t(g["nodes"]), t(g["nbr"]), t(g["w"]), t(q["start"]), t(q["goal"]), t(q["sidx"]), t(q["sw"]),
                           t(q["gidx"]), t(q["gw"]), t(q["direct"]), L)
    return {k: v.cpu().numpy() for k, v in res.items()}


def test_query_matches_the_reference_and_dijkstra(torch_dev, robots, cases):
    seen = set()
    for name, g, q, L, want in cases:
        got = _device_query(torch_dev, robots, g, q, L)
        assert np.array_equal(got["status"], want["status"]), name
        assert np.array_equal(got["len"], want["len"]), name
        assert _same(got["cost"], want["cost"]), name
        assert _same(got["path"], want["path"]), name
        for j in range(len(got["cost"])):
            if got["status"][j] != ru.QUERY_NAN:
                assert ru.bits(got["cost"][j]) == ru.bits(ru.dijkstra_cost(g, q, j)[1]), (name, j)
        seen |= set(got["status"].tolist())
    assert seen == {ru.FOUND, ru.NO_ROUTE, ru.TOO_LONG, ru.QUERY_NAN}
    assert {g["nodes"].shape[1] for _, g, _, _, _ in cases} >= {1, 65, 300, 130}


def test_a_query_does_not_depend_on_the_batch(torch_dev, robots, cases):
    for name, g, q, L, want in cases:
        Q = q["start"].shape[1]
        if Q != 5:
            continue
        all5 = _device_query(torch_dev, robots, g, q, L)
        for j in (0, 3):
            one = _device_query(torch_dev, robots, g, ru.take_queries(q, [j]), L)
            for key in ("status", "len"):
                assert one[key][0] == all5[key][j], (name, j, key)
            assert _same(one["cost"][0], all5["cost"][j]) and _same(one["path"][:, 0], all5["path"][:, j]), (name, j)


def test_ring_and_waypoint_cap(torch_dev, robots, cases):
    by = {name: (g, q, L) for name, g, q, L, _ in cases}
    got = _device_query(torch_dev, robots, *by["ring130"])
    assert got["status"][0] == ru.TOO_LONG and got["len"][0] == 2
    assert got["cost"][0] == ru.path_cost_backwards([0.5] + [0.25] * 129 + [0.5])
    got = _device_query(torch_dev, robots, *by["lmax2_route"])
    assert got["status"][0] == ru.TOO_LONG and got["cost"][0] == 1.0
    got = _device_query(torch_dev, robots, *by["lmax2_direct"])
    assert got["status"][0] == ru.FOUND and got["len"][0] == 2 and got["cost"][0] == 5.0


@pytest.fixture(scope="module")
def wall(robots):
    sc = ru.wall_scene()
    sc["robot"] = robots("panda")
    return sc


def _set_wall(sc):
    sc["robot"].set_collision_model(sc["frames"], sc["centers"], sc["radii"], self_pairs=None)
    sc["robot"].set_world(boxes=sc["boxes"])


def test_edges_follow_the_motion_check(torch_dev, wall):
    torch = torch_dev
    robot = wall["robot"]
    hc = robot.hip_chain()
    hc.set_collision_model(wall["frames"], wall["centers"], wall["radii"], self_pairs=None)
    hc.set_world(boxes=wall["boxes"])
    N, k, h = 200, 5, wall["h"]
    nodes = hc.seed_batch(1, N)
    frm = hc.seed_batch(1000, 37)
    idx, _ = hc.roadmap_knn(frm, nodes, k)
    idx[2, 5] = -1
    idx[4, 36] = -1
    fn, nn, ii = frm.cpu().numpy(), nodes.cpu().numpy(), idx.cpu().numpy()
    for reverse in (False, True):
        w = hc.roadmap_edges(frm, nodes, idx, h, reverse=reverse).cpu().numpy()
        a = np.repeat(fn[:, None, :], k, axis=1).reshape(7, -1)          # segment b = s * Q + q
        b = nn[:, np.where(ii < 0, 0, ii).ravel()]
        qa, qb = (b, a) if reverse else (a, b)
        free = hc.collision_motion_batch(_t(torch, qa), _t(torch, qb), h, clearance=False)[1].cpu().numpy()
        want = np.where(free & (ii.ravel() >= 0), ru.np_weights(qa, qb), np.inf).reshape(k, -1)
        assert _same(w, want), reverse
        assert np.isinf(w).sum() > 2 and np.isfinite(w).sum() > 0, "the scene blocks some motions and not others"
    # the direct form: endpoint q against node q
    w = hc.roadmap_edges(frm, nodes[:, :37].contiguous(), None, h).cpu().numpy()
    free = hc.collision_motion_batch(frm, nodes[:, :37].contiguous(), h, clearance=False)[1].cpu().numpy()
    assert _same(w[0], np.where(free, ru.np_weights(fn, nn[:, :37]), np.inf))
    # without a model every motion is free: every weight is its length
    hc.clear_collision_model()
    w = hc.roadmap_edges(frm, nodes, idx, h).cpu().numpy()
    want = np.where(ii >= 0, ru.np_weights(np.repeat(fn[:, None, :], k, axis=1).reshape(7, -1),
                                           nn[:, np.where(ii < 0, 0, ii).ravel()]).reshape(k, -1), np.inf)
    assert _same(w, want) and np.isfinite(w).sum() == w.size - 2


def test_plan_round_the_wall(torch_dev, wall):
    """The scene tests/test_roadmap_host.py chose on the CPU: the straight move is blocked, the plan is found, and
    every segment of it passes the motion check in the direction of travel."""
    robot, h = wall["robot"], wall["h"]
    _set_wall(wall)
    s, g = wall["start"][None], wall["goal"][None]
    assert not robot.collision_motion_batch_arrays(s, g, h)[1][0]
    edges = robot.build_roadmap(wall["N"], wall["k"], h, first=wall["first"])
    assert 0 < edges <= wall["N"] * wall["k"]
    res = robot.plan_paths(s, g, 64)
    assert res["status"][0] == ru.FOUND
    L = int(res["len"][0])
    path = res["paths"][0]
    assert 3 <= L <= 64 and np.array_equal(path[0], s[0]) and np.array_equal(path[L - 1], g[0])
    assert np.all(path[L:] == g[0][None])
    free = robot.collision_motion_batch_arrays(path[:L - 1], path[1:L], h)[1]
    assert free.all()
    weights = ru.np_weights(path[:L - 1].T, path[1:L].T)
    assert ru.bits(res["cost"][0]) == ru.bits(ru.path_cost_backwards(weights))
    # many queries in one call: each is what it is alone
    rng = np.random.default_rng(4)
    lb, ub = (np.array(v) for v in robot.joint_limits())
    starts = np.concatenate([s, rng.uniform(lb, ub, (6, 7))])
    goals = np.concatenate([g, rng.uniform(lb, ub, (6, 7))])
    many = robot.plan_paths(starts, goals, 64)
    assert many["status"][0] == ru.FOUND and _same(many["paths"][0], path) and _same(many["cost"][0], res["cost"][0])


def test_stale_roadmap_and_refusals(torch_dev, wall):
    robot, h = wall["robot"], wall["h"]
    _set_wall(wall)
    s, g = wall["start"][None], wall["goal"][None]
    robot.build_roadmap(wall["N"], wall["k"], h, first=wall["first"])
    assert robot.plan_paths(s, g)["status"][0] == ru.FOUND
    robot.set_world(boxes=wall["boxes"])
    with pytest.raises(RuntimeError, match="stale"):
        robot.plan_paths(s, g)
    robot.build_roadmap(wall["N"], wall["k"], h, first=wall["first"])
    assert robot.plan_paths(s, g)["status"][0] == ru.FOUND
    robot.set_collision_model(wall["frames"], wall["centers"], wall["radii"], self_pairs=None)
    with pytest.raises(RuntimeError, match="stale"):
        robot.plan_paths(s, g)
    from optik_amd import Robot
    with pytest.raises(RuntimeError, match="no roadmap"):
        Robot.from_urdf_file(*ROBOT_SPECS["panda"]).plan_paths(s, g)
    for kw in (dict(k=0), dict(k=17), dict(N=8193), dict(resolution=0.0), dict(resolution=-1.0)):
        with pytest.raises(ValueError):
            robot.build_roadmap(**kw)
    for L in (1, 65):
        with pytest.raises(ValueError):
            robot.plan_paths(s, g, L)
    # the kernel layer itself: OPTIK_HIP_EINVAL (-1) before any device work
    import ctypes as C
    from optik_amd import _native as nat
    lib, hc = nat.lib(), robot.hip_chain()
    null = C.c_void_p(None)
    for N, k in ((8193, 4), (16, 0), (16, 17), (0, 4)):
        assert lib.optik_hip_roadmap_knn(hc._h, null, 4, null, N, k, 0, null, null, null) == -1, (N, k)
    assert lib.optik_hip_roadmap_edges(hc._h, None, null, 4, null, 16, null, 4, 0.0, 0, null, null) == -1
    assert lib.optik_hip_roadmap_edges(hc._h, None, null, 4, null, 16, null, 4, math.nan, 0, null, null) == -1
    for L in (1, 65):
        assert lib.optik_hip_roadmap_query(hc._h, null, 16, null, null, 4, null, null, 4, null, null, 4, null, null,
                                           4, null, L, null, null, null, null, null) == -1
    robot.clear_collision_model()
    robot.set_world()
