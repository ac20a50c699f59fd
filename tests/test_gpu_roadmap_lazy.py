"""-m gpu: lazy roadmaps on the device against the host.  roadmap_plan_lazy_from_flags against the serial reference of
csrc/roadmap_lazy_measure.hpp (g++) on the graphs of roadmap_lazy_util, every output bit for bit; the query with
route against roadmap_query; build_roadmap(lazy=True) / plan_paths end to end on the wall scene against the eager
roadmap, through a change of the world and back; staleness of the eager roadmap and the refusals."""
import numpy as np
import pytest

import roadmap_lazy_util as lu
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
def lazy(tmp_path_factory):
    return lu.build_lazy_ref(str(tmp_path_factory.mktemp("roadmap_lazy_measure")))


@pytest.fixture(scope="module")
def cases(lazy):
    """Every graph of the host test with the reference's answer (enough rounds), computed once."""
    out = [(name, g, truth, q, L, lu.MAX_ROUNDS) for name, g, truth, q, L, _ in lu.lazy_cases()]
    for name, (g, truth, q, L) in lu.prescribed_cases().items():
        out += [(f"{name}/r{rounds}", g, truth, q, L, rounds) for rounds in (0, 1, 8)]
    return [(name, g, truth, q, L, rounds, lazy.plan(g, truth, q, L, rounds)) for name, g, truth, q, L, rounds in out]


CHAIN_OF_N = {1: "panda1", 2: "panda2", 3: "panda3", 7: "panda", 10: "arm10"}


def _t(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all((ru.bits(got) == ru.bits(want)) | (np.isnan(got) & np.isnan(want))))


def _device_plan(torch, robots, g, truth, q, L, rounds):
    from optik_amd.device import LazyRoadmap
    hc = robots(CHAIN_OF_N[g["nodes"].shape[0]]).hip_chain()
    t = lambda a: _t(torch, a)  # noqa: E731
    k, N = g["nbr"].shape
    rm = LazyRoadmap(t(g["nodes"]), t(g["nbr"]), t(g["w0"]), torch.full((k, N), -7.0, dtype=torch.float64, device="cuda"),
                     torch.full((k, N), -7, dtype=torch.int32, device="cuda"), 0.1)
    res = hc.roadmap_plan_lazy_from_flags(rm, t(truth["edge_free"]), t(truth["node_free"]), t(q["start"]),
                                          t(q["goal"]), t(q["sidx"]), t(q["sw"]), t(q["gidx"]), t(q["gw"]),
                                          t(q["direct"]), L, rounds)
    out = {key: (v.cpu().numpy() if hasattr(v, "cpu") else v) for key, v in res.items()}
    out["w"], out["verdict"] = rm.w.cpu().numpy(), rm.verdict.cpu().numpy()
    return out


def _assert_equal(name, got, want):
    assert np.array_equal(got["status"], want["status"]), name
    assert np.array_equal(got["len"], want["len"]), name
    assert _same(got["cost"], want["cost"]), name
    assert _same(got["path"], want["path"]), name
    assert _same(got["w"], want["w"]), name
    assert np.array_equal(got["verdict"], want["verdict"]), name
    assert (got["rounds"], got["checked"]) == (want["rounds"], want["checked"]), name


def test_loop_matches_the_reference(torch_dev, robots, cases):
    seen, joints = set(), set()
    for name, g, truth, q, L, rounds, want in cases:
        _assert_equal(name, _device_plan(torch_dev, robots, g, truth, q, L, rounds), want)
        seen |= set(want["status"].tolist())
        joints.add(g["nodes"].shape[0])
    assert seen == {ru.FOUND, ru.NO_ROUTE, ru.TOO_LONG, ru.QUERY_NAN, lu.UNSETTLED}
    assert joints >= {1, 7, 10} and sum(want["checked"] for *_, want in cases) > 100


def test_a_found_query_does_not_depend_on_the_batch(torch_dev, robots, cases):
    count = 0
    for name, g, truth, q, L, rounds, want in cases:
        if q["start"].shape[1] != 5:
            continue
        for j in (0, 3):
            if want["status"][j] != ru.FOUND:
                continue
            one = _device_plan(torch_dev, robots, g, truth, ru.take_queries(q, [j]), L, rounds)
            assert one["status"][0] == ru.FOUND and one["len"][0] == want["len"][j], (name, j)
            assert _same(one["cost"][0], want["cost"][j]) and _same(one["path"][:, 0], want["path"][:, j]), (name, j)
            count += 1
    assert count >= 10


def test_query_route_equals_query_and_names_the_nodes(torch_dev, robots):
    torch = torch_dev
    for name, g, q, L in ru.synthetic_cases():
        hc = robots(CHAIN_OF_N[g["nodes"].shape[0]]).hip_chain()
        args = [_t(torch, a) for a in (g["nodes"], g["nbr"], g["w"], q["start"], q["goal"], q["sidx"], q["sw"], q["gidx"],
                                       q["gw"], q["direct"])]
        want = {key: v.cpu().numpy() for key, v in hc.roadmap_query(*args, L).items()}
        got = {key: v.cpu().numpy() for key, v in hc.roadmap_query_route(*args, L).items()}
        for key in ("status", "len"):
            assert np.array_equal(got[key], want[key]), (name, key)
        assert _same(got["cost"], want["cost"]) and _same(got["path"], want["path"]), name
        for j, ln in enumerate(got["len"]):
            route, hop = got["route"][:, j], got["hop"][:, j]
            inner = np.arange(L)
            inner = (inner >= 1) & (inner < ln - 1)
            assert np.all(route[~inner] == -1) and np.all(hop[~inner] == -1), (name, j)
            assert np.all(route[inner] >= 0) and _same(got["path"][inner, j], g["nodes"][:, route[inner]].T), (name, j)
            for t in np.flatnonzero(inner):
                if t + 1 < ln - 1:   # a graph hop: its slot names the next node, and no lower slot does at that cost
                    s = hop[t]
                    assert 0 <= s < g["nbr"].shape[0] and g["nbr"][s, route[t]] == route[t + 1], (name, j, t)
                else:
                    assert hop[t] == -1, (name, j, t)


# ---- end to end on the wall scene ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wall(robots):
    sc = ru.wall_scene()
    sc["robot"] = robots("panda")
    sc["starts"], sc["goals"] = lu.wall_pairs(sc)
    return sc


def _set_model(sc):
    sc["robot"].set_collision_model(sc["frames"], sc["centers"], sc["radii"], self_pairs=None)


def _eager(sc):
    sc["robot"].build_roadmap(sc["N"], sc["k"], sc["h"], first=sc["first"])
    return sc["robot"].plan_paths(sc["starts"], sc["goals"], 64)


def _assert_same_plan(got, want):
    for key in ("status", "len"):
        assert np.array_equal(got[key], want[key]), key
    assert _same(got["cost"], want["cost"]) and _same(got["paths"], want["paths"])


def test_lazy_plan_equals_the_eager_plan_and_follows_the_world(torch_dev, wall):
    """The pairs of roadmap_lazy_util.wall_pairs (tests/test_roadmap_lazy_host.py states on the CPU what they do): the
    scene's own pair needs no graph edge, the wide pair's first optimistic route is blocked by the wall."""
    robot = wall["robot"]
    _set_model(wall)
    robot.set_world(boxes=wall["boxes"])
    walled = _eager(wall)
    assert walled["status"].tolist() == [ru.FOUND, ru.FOUND]
    robot.set_world()
    open_world = _eager(wall)
    assert not _same(open_world["cost"], walled["cost"])
    cells = wall["N"] * wall["k"]

    robot.set_world(boxes=wall["boxes"])
    slots = robot.build_roadmap(wall["N"], wall["k"], wall["h"], first=wall["first"], lazy=True)
    assert 0 < slots <= cells
    res = robot.plan_paths(wall["starts"], wall["goals"], 64)
    print(f"wall scene: rounds {res['rounds']}, checked {res['checked']} of {cells} slots")
    _assert_same_plan(res, walled)
    assert 0 < res["checked"] < cells and 1 < res["rounds"] <= res["checked"]
    again = robot.plan_paths(wall["starts"], wall["goals"], 64, rounds=0)     # the verdicts are kept
    _assert_same_plan(again, walled)
    assert again["checked"] == 0 and again["rounds"] == 0

    # the wall removed: the same roadmap plans in the new world, no rebuild
    robot.set_world()
    res = robot.plan_paths(wall["starts"], wall["goals"], 64)
    _assert_same_plan(res, open_world)
    # the wall put back: the first answer again, and one round alone leaves the wide pair unsettled
    robot.set_world(boxes=wall["boxes"])
    one = robot.plan_paths(wall["starts"], wall["goals"], 64, rounds=1)
    assert one["status"].tolist() == [ru.FOUND, lu.UNSETTLED] and one["rounds"] == 1 and one["len"][1] == 2
    assert one["cost"][1] <= walled["cost"][1] and _same(one["paths"][0], walled["paths"][0])
    assert np.array_equal(one["paths"][1, 0], wall["starts"][1]) and np.all(one["paths"][1, 1:] == wall["goals"][1])
    res = robot.plan_paths(wall["starts"], wall["goals"], 64)
    _assert_same_plan(res, walled)
    assert 0 < res["checked"] < cells
    robot.clear_collision_model()
    robot.set_world()


def test_device_tensors_end_to_end(torch_dev, wall):
    """HipChain.roadmap_build_lazy / roadmap_plan_lazy / roadmap_lazy_reset against roadmap_build / roadmap_plan."""
    torch = torch_dev
    hc = wall["robot"].hip_chain()
    hc.set_collision_model(wall["frames"], wall["centers"], wall["radii"], self_pairs=None)
    hc.set_world(boxes=wall["boxes"])
    nodes = hc.seed_batch(wall["first"], wall["N"])
    s, g = _t(torch, wall["starts"].T), _t(torch, wall["goals"].T)
    nbr, w = hc.roadmap_build(nodes, wall["k"], wall["h"])
    want = hc.roadmap_plan((nodes, nbr, w), s, g, wall["k"], 64, wall["h"])
    rm = hc.roadmap_build_lazy(nodes, wall["k"], wall["h"])
    assert torch.equal(rm.nbr, nbr) and torch.all(rm.w <= w) and torch.equal(torch.isinf(rm.w), rm.verdict == lu.BLOCKED)
    at_reset = rm.verdict.clone()
    got = hc.roadmap_plan_lazy(rm, s, g, wall["k"], 64)
    for key in ("status", "len", "cost", "path"):
        assert _same(got[key].cpu().numpy(), want[key].cpu().numpy()), key
    assert 0 < got["checked"] == int((rm.verdict != at_reset).sum()) and int((rm.verdict == 3).sum()) == 0
    assert torch.equal(torch.isinf(rm.w), rm.verdict == lu.BLOCKED)
    assert torch.all(rm.w <= w)      # the eager graph is a subgraph of the lazy one
    hc.set_world()
    hc.roadmap_lazy_reset(rm)
    assert int((rm.verdict == lu.FREE).sum()) == 0
    nbr2, w2 = hc.roadmap_build(nodes, wall["k"], wall["h"])
    want2 = hc.roadmap_plan((nodes, nbr2, w2), s, g, wall["k"], 64, wall["h"])
    got2 = hc.roadmap_plan_lazy(rm, s, g, wall["k"], 64)
    for key in ("status", "len", "cost", "path"):
        assert _same(got2[key].cpu().numpy(), want2[key].cpu().numpy()), key
    hc.clear_collision_model()


def test_eager_roadmap_still_goes_stale_and_the_refusals(torch_dev, wall):
    import ctypes as C
    from optik_amd import _native as nat
    from optik_amd.robot import _dp
    robot, h = wall["robot"], wall["h"]
    _set_model(wall)
    robot.set_world(boxes=wall["boxes"])
    s, g = wall["starts"], wall["goals"]
    robot.build_roadmap(wall["N"], wall["k"], h, first=wall["first"])
    with pytest.raises(ValueError, match="lazy"):
        robot.plan_paths(s, g, rounds=4)
    paths, cost = np.zeros((2, 64, 7)), np.zeros(2)
    ln, st = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    L = robot._L
    assert L.optik_robot_roadmap_plan_lazy(robot._h, _dp(s), _dp(g), 2, 64, 4, _dp(paths), ln.ctypes.data_as(ip),
                                           _dp(cost), st.ctypes.data_as(ip), None, None) == -1
    assert "optik_robot_roadmap_plan" in L.optik_robot_last_error().decode()
    robot.set_world(boxes=wall["boxes"])
    with pytest.raises(RuntimeError, match="stale"):
        robot.plan_paths(s, g)
    robot.build_roadmap(wall["N"], wall["k"], h, first=wall["first"], lazy=True)
    assert L.optik_robot_roadmap_plan(robot._h, _dp(s), _dp(g), 2, 64, _dp(paths), ln.ctypes.data_as(ip), _dp(cost),
                                      st.ctypes.data_as(ip)) == -1
    assert "optik_robot_roadmap_plan_lazy" in L.optik_robot_last_error().decode()
    for rounds in (-1, 4097):
        with pytest.raises(ValueError):
            robot.plan_paths(s, g, rounds=rounds)
        assert L.optik_robot_roadmap_plan_lazy(robot._h, _dp(s), _dp(g), 2, 64, rounds, _dp(paths),
                                               ln.ctypes.data_as(ip), _dp(cost), st.ctypes.data_as(ip), None, None) == -1
    for L_bad in (1, 65):
        with pytest.raises(ValueError):
            robot.plan_paths(s, g, L_bad)
    assert robot.plan_paths(s, g)["status"].tolist() == [ru.FOUND, ru.FOUND]
    # the kernel layer itself: OPTIK_HIP_EINVAL (-1) before any device work
    lib, hc = nat.lib(), robot.hip_chain()
    null = C.c_void_p(None)

    def plan(N=16, k=4, Lmax=8, rounds=1, res=0.1, ks=4, Q=0):
        return lib.optik_hip_roadmap_lazy_plan(hc._h, None, null, N, null, null, null, k, res, null, null, Q, null, null,
                                               ks, null, null, 4, null, Lmax, rounds, null, null, null, null, None, None,
                                               null)
    assert plan() == 0 and plan(rounds=0) == 0 and plan(rounds=4096) == 0      # (no queries: nothing to do)
    assert plan(Q=-1) == -1 and plan(Q=4) == -1                                # (null arrays)
    for kw in (dict(N=8193), dict(N=0), dict(k=0), dict(k=17), dict(Lmax=1), dict(Lmax=65), dict(rounds=-1),
               dict(rounds=4097), dict(res=0.0), dict(res=float("nan")), dict(ks=0)):
        assert plan(**kw) == -1, kw
    for N, k in ((8193, 4), (16, 0), (16, 17), (0, 4)):
        assert lib.optik_hip_roadmap_lazy_reset(hc._h, None, null, N, null, k, 0, null, null, null, null, null) == -1
        assert lib.optik_hip_roadmap_lazy_plan_from_flags(hc._h, null, N, null, null, null, null, k, null, null, null,
                                                          null, 0, null, null, 4, null, null, 4, null, 8, 1, null, null,
                                                          null, null, None, None, null) == -1
    for rounds, rc in ((4097, -1), (-1, -1), (4096, 0)):
        assert lib.optik_hip_roadmap_lazy_plan_from_flags(hc._h, null, 16, null, null, null, null, 4, null, null, null,
                                                          null, 0, null, null, 4, null, null, 4, null, 8, rounds, null,
                                                          null, null, null, None, None, null) == rc
    for Lmax, rc in ((65, -1), (1, -1), (64, 0)):
        assert lib.optik_hip_roadmap_query_route(hc._h, null, 16, null, null, 4, null, null, 0, null, null, 4, null,
                                                 null, 4, null, Lmax, null, null, null, null, null, null, null) == rc
    robot.clear_collision_model()
    robot.set_world()
