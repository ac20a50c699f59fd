"""-m gpu: goal-set planning on the device.  roadmap_query_goals against the serial reference of
csrc/roadmap_goals_measure.hpp (g++), bit for bit in every output, on random graphs of the three kernel sizes and on the
prescribed tie, NaN and Lmax cases; G = 1 against roadmap_query_route; roadmap_plan_goals, Robot.plan_to_goals and the
pose forms end to end in the wall scene of roadmap_util against the single-goal plans they replace."""
import ctypes as C

import numpy as np
import pytest

import roadmap_goals_util as gu
import roadmap_util as ru
from conftest import ROBOT_SPECS

pytestmark = pytest.mark.gpu

CHAIN_OF_N = {2: "panda2", 3: "panda3", 7: "panda"}
KEYS_INT, KEYS_F64 = ("status", "len", "which", "route", "hop"), ("cost", "path")


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
def goals_ref(tmp_path_factory):
    return gu.build_goals_ref(str(tmp_path_factory.mktemp("roadmap_goals_measure")))


def _t(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all((ru.bits(got) == ru.bits(want)) | (np.isnan(got) & np.isnan(want))))


def _device_goals(torch, robots, g, q, L):
    hc = robots(CHAIN_OF_N[g["nodes"].shape[0]]).hip_chain()
    t = lambda a: _t(torch, a)  # noqa: E731
    res = hc.roadmap_query_goals(t(g["nodes"]), t(g["nbr"]), t(g["w"]), t(q["start"]), t(q["goals"]), t(q["gcount"]),
                                 t(q["sidx"]), t(q["sw"]), t(q["gidx"]), t(q["gw"]), t(q["direct"]), L, route=True)
    return {k: v.cpu().numpy() for k, v in res.items()}


def _assert_equals_reference(name, got, want):
    for key in KEYS_INT:
        assert np.array_equal(got[key], want[key]), (name, key)
    for key in KEYS_F64:
        assert _same(got[key], want[key]), (name, key)


def test_device_matches_the_reference_on_random_graphs(torch_dev, robots, goals_ref):
    seen, sizes = set(), set()
    for name, g, q, L in gu.random_cases():
        want = goals_ref.query(g, q, L)
        _assert_equals_reference(name, _device_goals(torch_dev, robots, g, q, L), want)
        seen |= set(want["status"].tolist())
        sizes.add(g["nodes"].shape[1])
        if q["start"].shape[1] > 1:
            assert q["gcount"].min() == 0 and q["gcount"].max() == q["goals"].shape[0]
            assert ((q["gcount"] > 0) & (q["gcount"] < q["goals"].shape[0])).any() or q["goals"].shape[0] == 1
            assert (want["which"] > 0).any(), name
    assert seen >= {ru.FOUND, ru.NO_ROUTE, ru.TOO_LONG}
    assert sizes == {64, 1100, 4100}  # CAP 1024, 4096 and 8192


def test_device_matches_the_reference_on_the_prescribed_cases(torch_dev, robots, goals_ref):
    seen = set()
    for name, g, q, L, expect in gu.prescribed_cases():
        got = _device_goals(torch_dev, robots, g, q, L)
        _assert_equals_reference(name, got, goals_ref.query(g, q, L))
        gu.assert_prescribed(name, got, g, q, L, expect)
        seen.add(int(got["status"][0]))
    assert seen == {ru.FOUND, ru.NO_ROUTE, ru.TOO_LONG, ru.QUERY_NAN}


def test_one_goal_equals_roadmap_query(torch_dev, robots):
    torch = torch_dev
    rng = np.random.default_rng(526)
    hc = robots("panda3").hip_chain()
    for N, k, kg in ((64, 4, 4), (1100, 8, 16)):
        g = ru.random_graph(rng, N, k)
        q = ru.queries_for(rng, g, 65, 3, kg)
        t = lambda a: _t(torch, a)  # noqa: E731
        graph = (t(g["nodes"]), t(g["nbr"]), t(g["w"]))
        one = hc.roadmap_query_route(*graph, t(q["start"]), t(q["goal"]), t(q["sidx"]), t(q["sw"]), t(q["gidx"]),
                                     t(q["gw"]), t(q["direct"]), 16)
        got = hc.roadmap_query_goals(*graph, t(q["start"]), t(q["goal"][None]), t(np.ones(65, dtype=np.int32)),
                                     t(q["sidx"]), t(q["sw"]), t(q["gidx"][None]), t(q["gw"][None]),
                                     t(q["direct"][None]), 16, route=True)
        for key in ("status", "len", "route", "hop"):
            assert torch.equal(got[key], one[key]), (N, key)
        for key in ("cost", "path"):
            assert _same(got[key].cpu().numpy(), one[key].cpu().numpy()), (N, key)
        assert torch.equal(got["which"], torch.where(one["status"] == ru.FOUND, 0, -1).to(torch.int32)), N


# ---- end to end in the wall scene ---------------------------------------------------------------------------------------

IN_THE_WALL = [0.0, 0.4, 0.0, -1.8, 0.0, 2.2, 0.7]  # between WALL_START and WALL_GOAL: the arm is in the wall
LMAX = 64


@pytest.fixture(scope="module")
def wall(robots, torch_dev):
    """The wall scene installed in the Robot and in its HipChain, the eager roadmap built in both."""
    sc = ru.wall_scene()
    robot = sc["robot"] = robots("panda")
    robot.set_collision_model(sc["frames"], sc["centers"], sc["radii"], self_pairs=None)
    robot.set_world(boxes=sc["boxes"])
    robot.build_roadmap(sc["N"], sc["k"], sc["h"], first=sc["first"])
    hc = sc["hc"] = robot.hip_chain()
    hc.set_collision_model(sc["frames"], sc["centers"], sc["radii"], self_pairs=None)
    hc.set_world(boxes=sc["boxes"])
    nodes = hc.seed_batch(sc["first"], sc["N"])
    sc["roadmap"] = (nodes,) + tuple(hc.roadmap_build(nodes, sc["k"], sc["h"]))
    yield sc
    hc.clear_collision_model()
    hc.set_world()
    robot.clear_collision_model()
    robot.set_world()


def _wall_queries(wall, Q, G, seed):
    """starts [Q, n], goals [Q, G, n] inside the joint limits, counts [Q]; query 0 is the wall move with goal 0 in the
    wall, query 1 has no goal, query 2 NaN rows past its count."""
    rng = np.random.default_rng(seed)
    lb, ub = (np.array(v) for v in wall["robot"].joint_limits())
    starts, goals = rng.uniform(lb, ub, (Q, 7)), rng.uniform(lb, ub, (Q, G, 7))
    counts = rng.integers(1, G + 1, Q).astype(np.int32)
    starts[0], goals[0, 0], goals[0, 1], counts[0] = wall["start"], IN_THE_WALL, wall["goal"], G
    counts[1] = 0
    counts[2] = 2
    goals[2, 2:] = np.nan
    return starts, goals, counts


def _np_plan(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def test_plan_goals_is_the_minimum_over_single_plans(torch_dev, wall):
    torch, hc, G = torch_dev, wall["hc"], 4
    starts, goals, counts = _wall_queries(wall, 24, G, 527)
    st, gl = _t(torch, starts.T), _t(torch, goals.transpose(1, 2, 0))
    got = _np_plan(hc.roadmap_plan_goals(wall["roadmap"], st, gl, _t(torch, counts), wall["k"], LMAX, wall["h"]))
    per_goal = {g: _np_plan(hc.roadmap_plan(wall["roadmap"], st, gl[g].contiguous(), wall["k"], LMAX, wall["h"]))
                for g in range(G)}
    # goal 0 of the wall move cannot be reached (it is in collision), goal 1 can, round the wall
    assert per_goal[0]["status"][0] == ru.NO_ROUTE and per_goal[1]["status"][0] == ru.FOUND
    assert got["status"][0] == ru.FOUND and got["which"][0] != 0
    assert got["status"][1] == ru.NO_ROUTE and got["which"][1] == -1
    assert got["status"][2] != ru.QUERY_NAN  # (the NaN rows past the count are not read)
    q = dict(start=starts.T, goals=goals.transpose(1, 2, 0), gcount=counts)
    finite, unique = gu.assert_theorem("wall", got, per_goal, q)
    # (not vacuous: at least a quarter of the 24 random queries have a route, and random costs do not tie)
    assert finite >= 6 and unique == finite, (finite, unique)
    # every segment of a found path passes the motion check in the direction of travel
    L0 = int(got["len"][0])
    path = got["path"][:L0, 0]
    assert wall["robot"].collision_motion_batch_arrays(path[:-1], path[1:], wall["h"])[1].all()
    assert np.array_equal(path[-1], goals[0, got["which"][0]])


def test_robot_plan_to_goals_equals_the_device_form_across_two_chunks(torch_dev, wall):
    torch, hc, G, Q = torch_dev, wall["hc"], 4, 4096 + 37  # (the host API plans in chunks of 4 096 queries)
    starts, goals, counts = _wall_queries(wall, Q, G, 528)
    host = wall["robot"].plan_to_goals(starts, goals, counts, max_waypoints=LMAX)
    dev = _np_plan(hc.roadmap_plan_goals(wall["roadmap"], _t(torch, starts.T), _t(torch, goals.transpose(1, 2, 0)),
                                         _t(torch, counts), wall["k"], LMAX, wall["h"]))
    for a, b in (("status", "status"), ("len", "len"), ("goal", "which")):
        assert np.array_equal(host[a], dev[b]), a
    assert _same(host["cost"], dev["cost"]) and _same(host["paths"], dev["path"].transpose(1, 0, 2))
    assert set(host["status"].tolist()) >= {ru.FOUND, ru.NO_ROUTE}
    assert (host["status"][4096:] == ru.FOUND).any() and (host["goal"][4096:] > 0).any()
    # counts None: every goal exists
    full = wall["robot"].plan_to_goals(starts[3:40], goals[3:40], max_waypoints=LMAX)
    want = wall["robot"].plan_to_goals(starts[3:40], goals[3:40], np.full(37, G), max_waypoints=LMAX)
    assert np.array_equal(full["goal"], want["goal"]) and _same(full["paths"], want["paths"])
    # the paths go on as plan_paths' do
    found = host["status"][:64] == ru.FOUND
    assert found.any()
    short = wall["robot"].shortcut_paths(host["paths"][:64][found], host["len"][:64][found])
    assert short is not None


def _pose7(m44):
    """The Python front end's reading of a 4x4 target (include/optik.h: optik_pose_from_matrix, flags 0)."""
    from optik_amd import _native as nat
    dp = C.POINTER(C.c_double)
    L = nat.lib()
    L.optik_pose_from_matrix.argtypes = [dp, C.c_uint32, dp]
    mc = np.ascontiguousarray(np.asarray(m44, dtype=np.float64).T).ravel()  # column-major
    p = np.zeros(7)
    assert L.optik_pose_from_matrix(mc.ctypes.data_as(dp), 0, p.ctypes.data_as(dp)) == 0
    return p


def test_plan_to_poses(torch_dev, wall):
    from optik_amd import SolverConfig
    torch, robot, hc, K, R = torch_dev, wall["robot"], wall["hc"], 4, 64
    cfg = SolverConfig("quality", max_time=0.0, max_restarts=R)
    # four reachable targets -- the poses of collision-free configurations on both sides of the wall -- and one
    # that is out of reach
    behind = [wall["goal"], wall["goal"] + np.array([0.2, 0.1, 0, 0.2, 0, 0, 0]), wall["start"],
              wall["start"] + np.array([-0.2, 0.1, 0, 0.2, 0, 0, 0])]
    far = np.eye(4)
    far[:3, 3] = 5.0
    targets = np.array([np.array(robot.fk(x)) for x in behind] + [far])
    starts = np.array([wall["start"]] * 2 + [wall["goal"]] * 2 + [wall["start"]])
    res = robot.plan_to_poses(cfg, starts, targets, k=K, min_dist=0.1, max_waypoints=LMAX)
    x, _, _, count = robot.ik_solutions_batch_arrays(cfg, targets, starts, k=K, min_dist=0.1)
    assert np.array_equal(res["count"], count) and _same(res["goals"], x)
    assert (count[:4] >= 1).all() and count[4] == 0
    assert res["status"][4] == ru.NO_ROUTE and res["goal"][4] == -1 and res["len"][4] == 2
    plan = robot.plan_to_goals(starts, x, count, max_waypoints=LMAX)
    for key in ("status", "len", "goal"):
        assert np.array_equal(res[key], plan[key]), key
    assert _same(res["cost"], plan["cost"]) and _same(res["paths"], plan["paths"])
    # never worse than planning to the solution nearest the start alone
    first = robot.plan_paths(starts[:4], x[:4, 0], LMAX)
    assert (res["cost"][:4] <= first["cost"]).all(), (res["cost"], first["cost"])
    assert ((res["goal"][:4] >= 0) == (res["status"][:4] == ru.FOUND)).all()
    assert (res["status"][:4] == ru.FOUND).any()
    # the device form: both stages on the current stream, the solutions never leave the device
    t7 = np.array([_pose7(m) for m in targets])
    dev = hc.roadmap_plan_poses(wall["roadmap"], cfg.to_c(), _t(torch, t7), _t(torch, starts.T), 0, R, K, 0.1, wall["k"],
                                LMAX, wall["h"])
    dev = _np_plan(dev)
    assert np.array_equal(dev["count"], count) and _same(dev["goals"].transpose(2, 0, 1), x)
    for a, b in (("status", "status"), ("len", "len"), ("goal", "which")):
        assert np.array_equal(res[a], dev[b]), a
    assert _same(res["cost"], dev["cost"]) and _same(res["paths"], dev["path"].transpose(1, 0, 2))


def test_refusals(torch_dev, wall):
    torch, hc = torch_dev, wall["hc"]
    starts, goals, counts = _wall_queries(wall, 3, 2, 529)
    st = _t(torch, starts.T)
    with pytest.raises(ValueError):
        hc.roadmap_plan_goals(wall["roadmap"], st, _t(torch, np.zeros((17, 7, 3))), _t(torch, counts), wall["k"], LMAX,
                              wall["h"])
    with pytest.raises(ValueError):
        hc.roadmap_plan_goals(wall["roadmap"], st, _t(torch, np.zeros((2, 7, 4))), _t(torch, counts), wall["k"], LMAX,
                              wall["h"])
    # the kernel layer itself: OPTIK_HIP_EINVAL (-1) before any device work
    from optik_amd import _native as nat
    null = C.c_void_p(None)

    def raw(N=16, k=4, G=2, ks=4, kg=4, L=8):
        return nat.lib().optik_hip_roadmap_query_goals(hc._h, null, N, null, null, k, null, null, null, G, 4, null,
                                                       null, ks, null, null, kg, null, L, null, null, null, null, null,
                                                       null, null, null)
    assert raw() == 0  # (no output asked for: a no-op)
    for bad in (dict(G=0), dict(G=17), dict(N=8193), dict(k=17), dict(ks=0), dict(kg=17), dict(L=1), dict(L=65)):
        assert raw(**bad) == -1, bad
    # a lazy roadmap in the robot: plan_to_goals says so and names plan_paths
    from optik_amd import Robot
    lazy = Robot.from_urdf_file(*ROBOT_SPECS["panda"])
    lazy.build_roadmap(32, 4, wall["h"], lazy=True)
    with pytest.raises(RuntimeError, match="lazy.*plan_paths"):
        lazy.plan_to_goals(starts, goals, counts)
    n = lazy.num_positions()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    assert lazy._L.optik_robot_roadmap_plan_goals(lazy._h, starts.ctypes.data_as(dp), goals.ctypes.data_as(dp),
                                                  counts.ctypes.data_as(ip), 2, 3, 8, None, None, None, None,
                                                  np.zeros(3, dtype=np.int32).ctypes.data_as(ip)) == -1
    assert n == 7
    with pytest.raises(RuntimeError, match="no roadmap"):
        Robot.from_urdf_file(*ROBOT_SPECS["panda"]).plan_to_goals(starts, goals, counts)
