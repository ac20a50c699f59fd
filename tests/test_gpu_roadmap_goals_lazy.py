"""-m gpu: goal-set planning on lazy roadmaps on the device against the host.  The loop's test hook against the serial
reference of csrc/roadmap_goals_lazy_measure.hpp (g++) on the cases of roadmap_goals_lazy_util, with skip_settled 0 and
1: every output (sentinel-filled beforehand), the final w and verdict and both counters, bit for bit; batch sizes that
cross a block of the live list, gather and scatter; batch independence; NULL outputs, Q = 0 and the refusals; the wall
scene end to end through HipChain and Robot against the eager forms, through a change of the world; poses and
regions."""
import ctypes as C

import numpy as np
import pytest

import roadmap_goals_lazy_util as glu
import roadmap_goals_util as gu
import roadmap_lazy_util as lu
import roadmap_util as ru
from conftest import ROBOT_SPECS
from gpu_util import _out, _sentinels_left

pytestmark = pytest.mark.gpu

CHAIN_OF_N = {2: "panda2", 3: "panda3", 7: "panda"}
OUT_KEYS = ("path", "len", "cost", "status", "which")
LMAX = 64


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
    return glu.build_goals_lazy_ref(str(tmp_path_factory.mktemp("roadmap_goals_lazy_measure")))


@pytest.fixture(scope="module")
def cases(ref):
    """Every case of the host test with the specification's answer, computed once."""
    return [(name, g, t, q, L, rounds, ref.plan(g, t, q, L, rounds)) for name, g, t, q, L, rounds in glu.device_cases()]


def _t(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_plan(torch, robots, g, truth, q, L, rounds, skip, null=(), state=None):
    """optik_hip_roadmap_lazy_plan_goals_from_flags itself: the outputs sentinel-filled beforehand, those named in
    `null` not passed.  state = (w, verdict): no reset."""
    from optik_amd import _native as nat
    hc = robots(CHAIN_OF_N[g["nodes"].shape[0]]).hip_chain()
    t = lambda a: _t(torch, a)  # noqa: E731
    k, N = g["nbr"].shape
    n = g["nodes"].shape[0]
    G, _, Q = q["goals"].shape
    ks, kg = q["sidx"].shape[0], q["gidx"].shape[1]
    if state is None:
        w, verdict = _out((k, N), torch.float64), _out((k, N), torch.int32)
    else:
        w, verdict = t(state[0]), t(state[1].astype(np.int32))
    ins = [t(a) for a in (g["nodes"], g["nbr"].astype(np.int32), g["w0"], truth["edge_free"], truth["node_free"],
                          q["start"], q["goals"], q["gcount"].astype(np.int32), q["sidx"].astype(np.int32), q["sw"],
                          q["gidx"].astype(np.int32), q["gw"], q["direct"])]
    nodes, nbr, w0, edge_free, node_free, start, goals, gcount, sidx, sw, gidx, gw, direct = ins
    outs = dict(path=_out((L, Q, n), torch.float64), len=_out((Q,), torch.int32), cost=_out((Q,), torch.float64),
                status=_out((Q,), torch.int32), which=_out((Q,), torch.int32))
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    o = lambda key: None if key in null else p(outs[key])  # noqa: E731
    used, checked = C.c_int32(-1), C.c_int64(-1)
    rc = nat.lib().optik_hip_roadmap_lazy_plan_goals_from_flags(
        hc._h, p(nodes), N, p(nbr), p(w0), p(w), p(verdict), k, p(edge_free), None if state is not None else p(node_free),
        p(start), p(goals), p(gcount), G, Q, p(sidx), p(sw), ks, p(gidx), p(gw), kg, p(direct), L, rounds,
        1 if skip else 0, o("path"), o("len"), o("cost"), o("status"), o("which"), C.byref(used), C.byref(checked),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, nat.lib().optik_hip_last_error()
    torch.cuda.synchronize()
    res = {key: v.cpu().numpy() for key, v in outs.items()}
    res.update(w=w.cpu().numpy(), verdict=verdict.cpu().numpy(), rounds=int(used.value), checked=int(checked.value))
    return res


def _assert_equal(name, got, want, null=()):
    for key in OUT_KEYS:
        if key in null:
            assert _sentinels_left(got[key]) == got[key].size, (name, key)    # (not touched)
        else:
            assert _sentinels_left(got[key]) == 0, (name, key)
            assert glu.same_or_nan(got[key], want[key]), (name, key)
    assert _sentinels_left(got["w"]) == 0 and _sentinels_left(got["verdict"]) == 0, name
    assert glu.same_or_nan(got["w"], want["w"]) and np.array_equal(got["verdict"], want["verdict"]), name
    assert (got["rounds"], got["checked"]) == (want["rounds"], want["checked"]), (name, got["rounds"], got["checked"])


@pytest.mark.parametrize("skip", (0, 1))
def test_loop_matches_the_reference(torch_dev, robots, cases, skip):
    seen, traces = set(), {}
    for name, g, truth, q, L, rounds, want in cases:
        _assert_equal((name, skip), _device_plan(torch_dev, robots, g, truth, q, L, rounds, skip), want)
        seen |= set(want["status"].tolist())
        if rounds == glu.MAX_ROUNDS:
            traces.setdefault(g["nodes"].shape[1], []).append(glu.trace_of(want))
    assert seen == {ru.FOUND, ru.NO_ROUTE, ru.TOO_LONG, ru.QUERY_NAN, glu.UNSETTLED}
    glu.assert_draws_exercise_the_loop({N: traces[N] for N, _ in glu.RANDOM_SIZES})


@pytest.mark.parametrize("Q,kind", [(1, "mixed"), (65, "mixed"), (300, "mixed"), (300, "one_live"), (300, "all_frozen")])
def test_batch_sizes(torch_dev, robots, ref, Q, kind):
    g, truth, q, L = glu.batch_case(Q, kind, ref)
    want = ref.plan(g, truth, q, L, glu.MAX_ROUNDS)
    assert q["start"].shape[1] == Q
    fa, passes = want["frozen_after"], want["rounds"] + 1
    if kind == "one_live":      # one query among 299 that pass 1 froze keeps the loop going for three passes or more
        assert passes >= 3 and fa[Q // 2] >= 3 and np.all(np.delete(fa, Q // 2) == 1)
    if kind == "all_frozen":
        assert passes == 1 and np.all(fa == 1) and np.all(want["status"] == ru.FOUND)
    if kind == "mixed" and Q > 1:
        assert passes >= 3 and (fa == 1).any() and (np.where(fa == 0, passes, fa) >= 3).any()
    for skip in (0, 1):
        _assert_equal((Q, kind, skip), _device_plan(torch_dev, robots, g, truth, q, L, glu.MAX_ROUNDS, skip), want)


def test_a_found_query_does_not_depend_on_the_batch(torch_dev, robots, cases):
    count = 0
    for name, g, truth, q, L, rounds, want in cases:
        if rounds != glu.MAX_ROUNDS or count >= 12:
            continue
        for j in np.flatnonzero(want["status"] == ru.FOUND)[:2]:
            one = _device_plan(torch_dev, robots, g, truth, gu.take(q, [j]), L, rounds, 1)
            for key in OUT_KEYS:
                assert glu.same_or_nan(one[key][..., 0] if key != "path" else one[key][:, 0],
                                       want[key][..., j] if key != "path" else want[key][:, j]), (name, j, key)
            count += 1
    assert count >= 10


def test_null_outputs_q0_and_refusals(torch_dev, robots, ref):
    torch = torch_dev
    g, truth, q, L = glu.batch_case(65, "mixed", ref)
    want = ref.plan(g, truth, q, L, glu.MAX_ROUNDS)
    assert want["rounds"] >= 2
    for skip in (0, 1):
        for key in OUT_KEYS:
            _assert_equal((key, skip), _device_plan(torch, robots, g, truth, q, L, glu.MAX_ROUNDS, skip, null=(key,)),
                          want, null=(key,))
        _assert_equal(("all", skip), _device_plan(torch, robots, g, truth, q, L, glu.MAX_ROUNDS, skip, null=OUT_KEYS),
                      want, null=OUT_KEYS)
    from optik_amd import _native as nat
    hc = robots("panda3").hip_chain()
    null = C.c_void_p(None)
    used, checked = C.c_int32(-1), C.c_int64(-1)

    def raw(N=16, k=4, G=2, Q=0, ks=4, kg=4, Lm=8, rounds=4, h=0.1, chain=hc):
        return nat.lib().optik_hip_roadmap_lazy_plan_goals(
            chain._h, None, null, N, null, null, null, k, h, null, null, null, G, Q, null, null, ks, null, null, kg, null,
            Lm, rounds, 1, null, null, null, null, null, C.byref(used), C.byref(checked), null)
    assert raw() == 0 and (used.value, checked.value) == (0, 0)     # Q = 0: a no-op after the checks
    for bad in (dict(G=0), dict(G=17), dict(N=8193), dict(k=17), dict(ks=0), dict(kg=17), dict(Lm=1), dict(Lm=65),
                dict(rounds=-1), dict(rounds=4097), dict(h=0.0), dict(h=float("nan")), dict(Q=-1),
                dict(Q=(1 << 30) + 1), dict(Q=3)):      # (Q = 3 with null arrays: bad argument)
        assert raw(**bad) == -1, bad
    assert nat.lib().optik_hip_roadmap_lazy_plan_goals_from_flags(
        hc._h, null, 16, null, null, null, null, 4, null, null, null, null, null, 2, 0, null, null, 4, null, null, 4,
        null, 8, 4097, 1, null, null, null, null, null, None, None, null) == -1
    # the Python layer's own checks
    from optik_amd.device import LazyRoadmap
    t = lambda a: _t(torch, a)  # noqa: E731
    rm = LazyRoadmap(t(g["nodes"]), t(g["nbr"]), t(g["w0"]), t(g["w0"]), t(np.zeros(g["nbr"].shape, dtype=np.int32)), 0.1)
    args = [t(truth["edge_free"]), t(truth["node_free"]), t(q["start"]), t(q["goals"]), t(q["gcount"]), t(q["sidx"]),
            t(q["sw"]), t(q["gidx"]), t(q["gw"]), t(q["direct"])]
    res = hc.roadmap_plan_goals_lazy_from_flags(rm, *args, L, None)
    assert (res["rounds"], res["checked"]) == (want["rounds"], want["checked"])
    assert np.array_equal(res["status"].cpu().numpy(), want["status"])
    for rounds in (-1, 4097):
        with pytest.raises(ValueError):
            hc.roadmap_plan_goals_lazy_from_flags(rm, *args, L, rounds)
    with pytest.raises(ValueError):
        hc.roadmap_plan_goals_lazy_from_flags(rm, *args[:3], t(np.zeros((17, 3, 65))), *args[4:], L, 4)


# ---- end to end in the wall scene ---------------------------------------------------------------------------------

IN_THE_WALL = [0.0, 0.4, 0.0, -1.8, 0.0, 2.2, 0.7]  # between WALL_START and WALL_GOAL: the arm is in the wall


@pytest.fixture(scope="module")
def wall(robots):
    sc = ru.wall_scene()
    sc["robot"] = robots("panda")
    assert (sc["N"], sc["k"]) == (128, 8)
    return sc


def _wall_queries(wall, Q, G, seed):
    """starts [Q, n], goals [Q, G, n] inside the joint limits, counts [Q]; query 0 is the wide wall move of
    roadmap_lazy_util.wall_pairs with goal 0 in the wall, goal 1 its own and no other, query 1 has no goal, query 2 NaN
    rows past its count."""
    rng = np.random.default_rng(seed)
    lb, ub = (np.array(v) for v in wall["robot"].joint_limits())
    starts, goals = rng.uniform(lb, ub, (Q, 7)), rng.uniform(lb, ub, (Q, G, 7))
    counts = rng.integers(1, G + 1, Q).astype(np.int32)
    ws, wg = lu.wall_pairs(wall)
    starts[0], goals[0, 0], goals[0, 1], counts[0] = ws[1], IN_THE_WALL, wg[1], 2
    counts[1] = 0
    counts[2] = 2
    goals[2, 2:] = np.nan
    return starts, goals, counts


def _np_plan(res):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def _assert_theorem_on_the_device(name, lazy, eager, keys=("status", "len", "which", "cost", "path")):
    settled = np.isin(lazy["status"], (ru.FOUND, ru.NO_ROUTE, ru.QUERY_NAN))
    assert not (lazy["status"] == glu.UNSETTLED).any(), name
    for key in keys:
        a, b = np.moveaxis(lazy[key], 1 if key == "path" else 0, 0), np.moveaxis(eager[key], 1 if key == "path" else 0, 0)
        assert glu.same_or_nan(a[settled], b[settled]), (name, key)
    rest = ~settled
    assert (lazy["status"][rest] == ru.TOO_LONG).all() and (lazy["cost"][rest] <= eager["cost"][rest]).all(), name
    return int(settled.sum())


def test_device_tensors_end_to_end(torch_dev, wall):
    """HipChain.roadmap_plan_goals_lazy against roadmap_plan_goals over roadmap_build's graph, before and after the
    wall moves."""
    torch, G = torch_dev, 4
    hc = wall["robot"].hip_chain()
    hc.set_collision_model(wall["frames"], wall["centers"], wall["radii"], self_pairs=None)
    hc.set_world(boxes=wall["boxes"])
    try:
        nodes = hc.seed_batch(wall["first"], wall["N"])
        starts, goals, counts = _wall_queries(wall, 24, G, 534)
        st, gl, gc = _t(torch, starts.T), _t(torch, goals.transpose(1, 2, 0)), _t(torch, counts)
        cells = wall["N"] * wall["k"]
        rm = hc.roadmap_build_lazy(nodes, wall["k"], wall["h"])
        for step, boxes in enumerate((wall["boxes"], [[0.55, 0.3, 0.45, 0.0, 0.0, 0.0, 1.0, 0.2, 0.01, 0.25]])):
            if step:
                hc.set_world(boxes=boxes)      # the wall moved: forget the verdicts, keep the roadmap
                hc.roadmap_lazy_reset(rm)
                assert int((rm.verdict == lu.FREE).sum()) == 0
            nbr, w = hc.roadmap_build(nodes, wall["k"], wall["h"])
            want = _np_plan(hc.roadmap_plan_goals((nodes, nbr, w), st, gl, gc, wall["k"], LMAX, wall["h"]))
            at_reset = rm.verdict.clone()
            got = _np_plan(hc.roadmap_plan_goals_lazy(rm, st, gl, gc, wall["k"], LMAX, glu.MAX_ROUNDS))
            print(f"wall scene {step}: rounds {got['rounds']}, checked {got['checked']} of {cells} slots; status",
                  np.bincount(got["status"], minlength=5).tolist())
            assert _assert_theorem_on_the_device(step, got, want) >= 12
            if step == 0:   # (goal 0 of the wall move is in the wall, goal 1 lies round it)
                assert got["status"][0] == ru.FOUND and got["which"][0] == 1 and got["len"][0] > 3
            assert got["status"][1] == ru.NO_ROUTE and got["status"][2] != ru.QUERY_NAN
            # (with the wall out of its way the wall move is a direct motion: nothing may be left to check then)
            assert (step or got["checked"] > 0) and got["checked"] < cells
            assert got["checked"] == int((rm.verdict != at_reset).sum())
            assert int((rm.verdict == 3).sum()) == 0 and torch.all(rm.w <= w)
            assert torch.equal(torch.isinf(rm.w), rm.verdict == lu.BLOCKED)
            # every pass on all queries: the same answers
            hc.roadmap_lazy_reset(rm)
            full = _np_plan(hc.roadmap_plan_goals_lazy(rm, st, gl, gc, wall["k"], LMAX, glu.MAX_ROUNDS,
                                                       _skip_settled=False))
            for key in ("status", "len", "which", "cost", "path"):
                assert glu.same_or_nan(full[key], got[key]), (step, key)
            assert (full["rounds"], full["checked"]) == (got["rounds"], got["checked"])
    finally:
        hc.clear_collision_model()
        hc.set_world()


def _set_scene(robot, wall, boxes):
    robot.set_collision_model(wall["frames"], wall["centers"], wall["radii"], self_pairs=None)
    robot.set_world(boxes=boxes)


def _assert_robot_plans(name, lazy, eager):
    got = dict(status=lazy["status"], len=lazy["len"], which=lazy["goal"], cost=lazy["cost"],
               path=lazy["paths"].transpose(1, 0, 2))
    want = dict(status=eager["status"], len=eager["len"], which=eager["goal"], cost=eager["cost"],
                path=eager["paths"].transpose(1, 0, 2))
    return _assert_theorem_on_the_device(name, got, want)


def test_robot_plan_to_goals_lazy_equals_the_eager_twin_and_follows_the_world(torch_dev, wall):
    from optik_amd import Robot
    lazy, eager = wall["robot"], Robot.from_urdf_file(*ROBOT_SPECS["panda"])
    moved = [[0.55, 0.3, 0.45, 0.0, 0.0, 0.0, 1.0, 0.2, 0.01, 0.25]]
    starts, goals, counts = _wall_queries(wall, 24, 4, 535)
    try:
        for r in (lazy, eager):
            _set_scene(r, wall, wall["boxes"])
        lazy.build_roadmap(wall["N"], wall["k"], wall["h"], first=wall["first"], lazy=True)
        cells = wall["N"] * wall["k"]
        with pytest.raises(RuntimeError, match="lazy.*plan_paths"):       # (the eager call keeps refusing)
            lazy.plan_to_goals(starts, goals, counts)
        for step, boxes in enumerate((wall["boxes"], moved, wall["boxes"])):
            lazy.set_world(boxes=boxes)                                       # no rebuild on the lazy side
            eager.set_world(boxes=boxes)
            eager.build_roadmap(wall["N"], wall["k"], wall["h"], first=wall["first"])
            want = eager.plan_to_goals(starts, goals, counts, max_waypoints=LMAX)
            got = lazy.plan_to_goals_lazy(starts, goals, counts, max_waypoints=LMAX, rounds=glu.MAX_ROUNDS)
            assert _assert_robot_plans(step, got, want) >= 12
            assert 0 < got["checked"] < cells and 0 < got["rounds"] <= got["checked"]
            again = lazy.plan_to_goals_lazy(starts, goals, counts, max_waypoints=LMAX, rounds=0)   # verdicts kept
            assert again["checked"] == 0 and np.array_equal(again["status"], got["status"])
        # counts None: every goal exists
        full = lazy.plan_to_goals_lazy(starts[3:20], goals[3:20], max_waypoints=LMAX, rounds=glu.MAX_ROUNDS)
        same = lazy.plan_to_goals_lazy(starts[3:20], goals[3:20], np.full(17, 4), max_waypoints=LMAX,
                                       rounds=glu.MAX_ROUNDS)
        assert np.array_equal(full["goal"], same["goal"]) and glu.same_or_nan(full["paths"], same["paths"])
        # one round alone leaves the wall move unsettled: the start, then goal 0, goal -1, a lower bound
        lazy.set_world(boxes=moved)
        lazy.set_world(boxes=wall["boxes"])
        one = lazy.plan_to_goals_lazy(starts[:1], goals[:1], counts[:1], max_waypoints=LMAX, rounds=1)
        assert one["status"][0] == glu.UNSETTLED and one["goal"][0] == -1 and one["len"][0] == 2 and one["rounds"] == 1
        assert one["cost"][0] <= got["cost"][0] and np.array_equal(one["paths"][0, 0], starts[0])
        assert glu.same_or_nan(one["paths"][0, 1:], np.broadcast_to(goals[0, 0], (LMAX - 1, 7)))
        # refusals: an eager roadmap names plan_to_goals, no roadmap says so, rounds out of range
        with pytest.raises(RuntimeError, match="plan_to_goals"):
            eager.plan_to_goals_lazy(starts, goals, counts)
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        assert eager._L.optik_robot_roadmap_plan_goals_lazy(
            eager._h, starts.ctypes.data_as(dp), goals.ctypes.data_as(dp), counts.ctypes.data_as(ip), 4, 24, 8, 4, None,
            None, None, None, np.zeros(24, dtype=np.int32).ctypes.data_as(ip), None, None) == -1
        assert "optik_robot_roadmap_plan_goals" in eager._L.optik_robot_last_error().decode()
        with pytest.raises(RuntimeError, match="no roadmap"):
            Robot.from_urdf_file(*ROBOT_SPECS["panda"]).plan_to_goals_lazy(starts, goals, counts)
        for rounds in (-1, 4097):
            with pytest.raises(ValueError):
                lazy.plan_to_goals_lazy(starts, goals, counts, rounds=rounds)
    finally:
        for r in (lazy, eager):
            r.clear_collision_model()
            r.set_world()


def test_plan_to_poses_and_regions_lazy(torch_dev, wall):
    from optik_amd import SolverConfig
    from optik_amd.constraint import PoseConstraint
    robot, K, R = wall["robot"], 4, 64
    cfg = SolverConfig("quality", max_time=0.0, max_restarts=R)
    try:
        _set_scene(robot, wall, wall["boxes"])
        robot.build_roadmap(wall["N"], wall["k"], wall["h"], first=wall["first"], lazy=True)
        behind = [wall["goal"], wall["goal"] + np.array([0.2, 0.1, 0, 0.2, 0, 0, 0]), wall["start"]]
        far = np.eye(4)
        far[:3, 3] = 5.0
        targets = np.array([np.array(robot.fk(x)) for x in behind] + [far])
        starts = np.array([wall["start"]] * 2 + [wall["goal"]] + [wall["start"]])
        res = robot.plan_to_poses_lazy(cfg, starts, targets, k=K, min_dist=0.1, max_waypoints=LMAX)
        x, _, _, count = robot.ik_solutions_batch_arrays(cfg, targets, starts, k=K, min_dist=0.1)
        assert np.array_equal(res["count"], count) and glu.same_or_nan(res["goals"], x)
        assert (count[:3] >= 1).all() and count[3] == 0
        assert res["status"][3] == ru.NO_ROUTE and res["goal"][3] == -1
        plan = robot.plan_to_goals_lazy(starts, x, count, max_waypoints=LMAX)
        for key in ("status", "len", "goal"):
            assert np.array_equal(res[key], plan[key]), key
        assert glu.same_or_nan(res["cost"], plan["cost"]) and glu.same_or_nan(res["paths"], plan["paths"])
        assert (res["status"][:3] == ru.FOUND).any() and "rounds" in res and "checked" in res
        # regions: a box of +-5 cm and +-0.1 rad round the poses of the first three targets
        regions = [PoseConstraint(m, [-0.05] * 3 + [-0.1] * 3, [0.05] * 3 + [0.1] * 3) for m in targets[:3]]
        reg = robot.plan_to_region_lazy(cfg, starts[:3], regions, k=K, min_dist=0.1, max_waypoints=LMAX)
        rr = robot.ik_region_batch_arrays(cfg, regions, starts[:3], k=K, min_dist=0.1)
        assert np.array_equal(reg["count"], rr["count"]) and glu.same_or_nan(reg["goals"], rr["x"])
        plan = robot.plan_to_goals_lazy(starts[:3], rr["x"], rr["count"], max_waypoints=LMAX)
        for key in ("status", "len", "goal"):
            assert np.array_equal(reg[key], plan[key]), key
        assert glu.same_or_nan(reg["cost"], plan["cost"]) and glu.same_or_nan(reg["paths"], plan["paths"])
        with pytest.raises(RuntimeError, match="lazy.*plan_paths"):
            robot.plan_to_poses(cfg, starts, targets, k=K)
    finally:
        robot.clear_collision_model()
        robot.set_world()
