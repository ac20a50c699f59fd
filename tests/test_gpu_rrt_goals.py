"""-m gpu: the tree planner with a goal set on the device against the serial reference of csrc/rrt_goals_measure.hpp
(g++, rrt_goals_util).  As in test_gpu_rrt.py the reference's verdicts and samples are the device's own, already
tested answers (Robot.collision_clearance_batch_arrays, Robot.collision_motion_batch_arrays, HipChain.seed_batch), so
what is compared bit for bit is the new code alone: the gather, rule 0 with its roots, and the walk to a root.  The
Panda wall scene of test_gpu_rrt.py at its parameters: step 0.3, first 1, the pair that joins after 33 iterations."""
import ctypes as C
import importlib
import math
import os
import sys

import numpy as np
import pytest

import rrt_goals_util as gu
import rrt_util as tu
from gpu_util import _out, _sentinels_left, assert_bit_equal
from test_gpu_rrt import WALL, _install, _scene, torch_dev, wall  # noqa: F401  (the scene and its fixtures)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("path", "len", "cost", "status", "iters", "nodes", "which")


@pytest.fixture(scope="module")
def gref(tmp_path_factory):
    return gu.build_rrt_goals_ref(str(tmp_path_factory.mktemp("rrt_goals_measure")))


def _reference(gref, sc, starts, goals, counts, iters, step, first, max_nodes, Lmax):
    """The serial reference per query, with the device's own verdicts and samples."""
    robot, h = sc["robot"], sc["h"]
    samples = sc["hc"].seed_batch(first, iters).cpu().numpy().T.copy()
    config_free = lambda q: bool(robot.collision_clearance_batch_arrays(q[None])[1][0])  # noqa: E731
    motions_free = lambda qa, qb: robot.collision_motion_batch_arrays(qa, qb, h)[1]       # noqa: E731
    rows = [gref.plan(sc["lo"], sc["hi"], s, g, c, samples, step, max_nodes, Lmax, config_free, motions_free)
            for s, g, c in zip(starts, goals, counts)]
    return dict(path=np.stack([r["path"] for r in rows], axis=1), len=np.array([r["len"] for r in rows]),
                cost=np.array([r["cost"] for r in rows]), status=np.array([r["status"] for r in rows]),
                iters=np.array([r["iters"] for r in rows]), nodes=np.stack([r["nodes"] for r in rows], axis=1),
                which=np.array([r["which"] for r in rows]), roots=np.array([r["roots"] for r in rows]))


def _device(torch, sc, starts, goals, counts, iters, step, first, max_nodes, Lmax, poll=32):
    """optik_hip_rrt_plan_goals on sentinel-filled outputs: every element is written.  goals [Q, G, n]."""
    from optik_amd import _native as nat
    from optik_amd.device import _ptr, _stream_ptr
    hc, (Q, G, n) = sc["hc"], goals.shape
    s = torch.from_numpy(np.ascontiguousarray(starts.T)).cuda()
    g = torch.from_numpy(np.ascontiguousarray(goals.transpose(1, 2, 0))).cuda()
    c = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).cuda()
    res = dict(path=_out((Lmax, Q, n), torch.float64), len=_out((Q,), torch.int32), cost=_out((Q,), torch.float64),
               status=_out((Q,), torch.int32), iters=_out((Q,), torch.int32), nodes=_out((2, Q), torch.int32),
               which=_out((Q,), torch.int32))
    nat.check(nat.lib().optik_hip_rrt_plan_goals(
        hc._h, None, _ptr(s), _ptr(g), _ptr(c), Q, G, iters, step, sc["h"], first, max_nodes, Lmax, poll,
        _ptr(res["path"]), _ptr(res["len"]), _ptr(res["cost"]), _ptr(res["status"]), _ptr(res["iters"]),
        _ptr(res["nodes"]), _ptr(res["which"]), _stream_ptr()))
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in res.items()}
    for k, v in res.items():
        assert _sentinels_left(v) == 0, k
    return res


def _assert_parity(got, want, what):
    for key in ("len", "status", "iters", "nodes", "which"):
        assert np.array_equal(got[key], want[key]), (what, key, got[key], want[key])
    assert_bit_equal(got["cost"], want["cost"], f"{what}: cost")
    assert_bit_equal(got["path"], want["path"], f"{what}: path")


def _rows(res, rows):
    return {k: (res[k][:, rows] if res[k].ndim > 1 else res[k][rows]) for k in KEYS}


def test_one_goal_is_rrt_plan_bit_for_bit(torch_dev, wall):
    torch = torch_dev
    _install(wall)
    starts, goals = wall["starts"], wall["goals"]
    s = torch.from_numpy(np.ascontiguousarray(starts.T)).cuda()
    g = torch.from_numpy(np.ascontiguousarray(goals.T)).cuda()
    one = {k: v.cpu().numpy() for k, v in wall["hc"].rrt_plan(s, g, resolution=wall["h"], Lmax=64, **WALL).items()}
    assert one["status"].tolist() == [tu.FOUND, tu.FOUND, tu.FOUND, tu.NO_ROUTE, tu.QUERY_NAN] and one["len"][0] > 2
    got = _device(torch, wall, starts, goals[:, None, :], np.ones(5, dtype=np.int32), Lmax=64, **WALL)
    for key in ("len", "status", "iters", "nodes"):
        assert np.array_equal(got[key], one[key]), key
    assert np.array_equal(got["cost"].view(np.uint64), one["cost"].view(np.uint64))
    assert np.array_equal(got["path"].view(np.uint64), one["path"].view(np.uint64))
    assert got["which"].tolist() == [0, 0, 0, -1, -1]
    # the tensor entry point is the same call
    dev = wall["hc"].rrt_plan_goals(s, g[None].contiguous(), torch.ones(5, dtype=torch.int32, device="cuda"),
                                    resolution=wall["h"], Lmax=64, **WALL)
    assert set(dev) == set(one) | {"which"}
    for key in KEYS:
        assert np.array_equal(dev[key].cpu().numpy().view(np.uint8), got[key].view(np.uint8)), key
    _install(wall, model=False)


def _goal_sets(wall):
    """Eight queries with G = 4 (chosen on the CPU with the host motion check: `inside` and `inside2` are in the wall,
    `near` is free and directly visible from the start, `goal2` is free and hidden like the goal)."""
    start, goal = wall["start"], wall["goal"]
    inside, inside2, near = start.copy(), start.copy(), start.copy()
    inside[0], inside2[0] = 0.0, 0.05
    near[0] -= 0.2
    goal2 = goal + np.array([0.2, 0.1, 0, 0.2, 0, 0, 0])
    nanrow, nan_goal = np.full(7, math.nan), goal.copy()
    nan_goal[3] = math.nan
    sets = [([inside, goal, nanrow, nanrow], 2),          # 0: goal 0 in collision, goal 1 the far-side goal
            ([inside, near, inside2, inside], 4),         # 1: a directly visible goal among blocked ones
            ([goal, goal2, nanrow, nanrow], 2),           # 2, 3: two far-side goals, in both orders
            ([goal2, goal, nanrow, nanrow], 2),
            ([inside, inside2, inside, inside2], 4),      # 4: all goals in collision
            ([goal, goal2, near, inside], 0),             # 5: no goals
            ([goal, nan_goal, near, near], 2),            # 6: a NaN in a counted goal
            ([inside, goal, nanrow, inside], 2)]          # 7: query 0 with a NaN row and a colliding row past the count
    goals = np.array([s for s, _ in sets])
    return np.tile(start, (len(sets), 1)), goals, np.array([c for _, c in sets], dtype=np.int32)


@pytest.fixture(scope="module")
def sets_want(gref, wall, torch_dev):
    """The reference's answer for the eight goal-set queries, computed once."""
    _install(wall)
    starts, goals, counts = _goal_sets(wall)
    return _reference(gref, wall, starts, goals, counts, Lmax=64, **WALL)


def test_parity_on_goal_sets(torch_dev, wall, sets_want):
    _install(wall)
    robot, h = wall["robot"], wall["h"]
    starts, goals, counts = _goal_sets(wall)
    want = sets_want
    print("goal sets: status", want["status"], "len", want["len"], "iters", want["iters"], "nodes", want["nodes"].T,
          "which", want["which"], "roots", want["roots"])
    F, N, X = tu.FOUND, tu.NO_ROUTE, tu.QUERY_NAN
    assert want["status"].tolist() == [F, F, F, F, N, N, X, F]
    assert want["roots"].tolist() == [1, 1, 2, 2, 0, 0, 0, 1]
    assert want["which"][[0, 1, 4, 5, 6, 7]].tolist() == [1, 1, -1, -1, -1, 1] and set(want["which"][2:4]) <= {0, 1}
    assert want["len"][0] > 2 and want["len"][1] == 2 and want["len"][2] > 2 and want["len"][3] > 2
    assert want["iters"][[1, 4, 5, 6]].tolist() == [0, 0, 0, 0] and want["iters"][0] > 1
    got = _device(torch_dev, wall, starts, goals, counts, Lmax=64, **WALL)
    _assert_parity(got, want, "goal sets")
    # what lies past the count changes nothing: query 7 is query 0
    for key in KEYS:
        a, b = (got[key][:, 0], got[key][:, 7]) if got[key].ndim > 1 else (got[key][0:1], got[key][7:8])
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), key
    # the host-row entry point gives the same plans
    rows = robot.plan_rrt_to_goals(starts, goals, counts, resolution=h, max_waypoints=64, **WALL)
    _assert_parity(dict(path=rows["paths"].transpose(1, 0, 2), len=rows["len"], cost=rows["cost"], status=rows["status"],
                        iters=rows["iters"], nodes=rows["nodes"].T, which=rows["goal"]), want, "Robot.plan_rrt_to_goals")
    # independent of the reference: every segment of every found path is free at the same resolution, in path order,
    # and the path ends at goals[which]
    for q in range(len(starts)):
        p, L, w = got["path"][:, q], got["len"][q], got["which"][q]
        assert np.array_equal(p[0], starts[q])
        if got["status"][q] != tu.FOUND:
            pad = goals[q, 0] if counts[q] > 0 else starts[q]
            assert w == -1 and L == 2 and np.array_equal(p[1:], np.tile(pad, (63, 1)), equal_nan=True)
            continue
        assert 0 <= w < counts[q]
        assert np.array_equal(p[L - 1:].view(np.uint64), np.tile(goals[q, w], (65 - L, 1)).view(np.uint64))
        assert robot.collision_motion_batch_arrays(p[:L - 1], p[1:L], h)[1].all(), q
        assert got["cost"][q] == tu.forward_cost(p, L)
    _install(wall, model=False)


def test_a_query_does_not_depend_on_the_batch_or_on_poll(torch_dev, wall, sets_want):
    _install(wall)
    starts, goals, counts = _goal_sets(wall)
    rng = np.random.default_rng(28)
    S = rng.uniform(wall["lo"], wall["hi"], (70, 7))
    Gs = rng.uniform(wall["lo"], wall["hi"], (70, 4, 7))
    Cn = rng.integers(0, 5, 70).astype(np.int32)
    S[37], Gs[37], Cn[37] = starts[2], goals[2], counts[2]
    S[5, 2] = math.nan
    alone = _device(torch_dev, wall, starts[2:3], goals[2:3], counts[2:3], Lmax=64, **WALL)
    _assert_parity(alone, {k: (v[:, 2:3] if v.ndim > 1 else v[2:3]) for k, v in sets_want.items()}, "alone")
    for poll in (1, 65536):
        got = _device(torch_dev, wall, S, Gs, Cn, Lmax=64, poll=poll, **WALL)
        _assert_parity(_rows(got, slice(37, 38)), alone, f"poll {poll}")
        if poll == 1:
            first = got
        else:
            _assert_parity(got, first, "poll 65536 against poll 1")
    assert got["status"][5] == tu.QUERY_NAN and (got["which"][got["status"] != tu.FOUND] == -1).all()
    _install(wall, model=False)


def test_two_chunks(torch_dev, wall):
    from optik_amd import _native as nat
    _install(wall)
    chunk = nat.rrt_chunk(wall["hc"]._h, 4096)
    assert 500 < chunk < 600
    Q, real = chunk + 40, chunk + 7
    starts, goals, counts = _goal_sets(wall)
    S, Gs = np.tile(wall["start"], (Q, 1)), np.tile(goals[0, :2], (Q, 1, 1))
    Cn = np.zeros(Q, dtype=np.int32)                      # no goals: these end before iteration 0
    Cn[real] = 2                                          # the wall pair behind a blocked goal, in the second chunk
    Cn[3] = 1                                             # only the blocked goal: status 1 at once, in the first
    args = dict(iters=64, step=tu.WALL_STEP, first=tu.WALL_FIRST, max_nodes=4096, Lmax=64)
    got = _device(torch_dev, wall, S, Gs, Cn, **args)
    one = _device(torch_dev, wall, S[real:real + 1], Gs[real:real + 1], Cn[real:real + 1], **args)
    _assert_parity(_rows(got, slice(real, real + 1)), one, "the row of the second chunk")
    assert one["status"][0] == tu.FOUND and one["which"][0] == 1 and one["len"][0] > 2
    rest = np.arange(Q) != real
    assert (got["status"][rest] == tu.NO_ROUTE).all() and (got["which"][rest] == -1).all()
    assert (got["iters"][rest] == 0).all() and (got["nodes"][:, rest] == 0).all()
    assert np.array_equal(got["path"][1:, 3], np.tile(goals[0, 0], (63, 1)))
    assert np.array_equal(got["path"][:, chunk], np.tile(wall["start"], (64, 1)))
    _install(wall, model=False)


def test_no_counts_is_every_slot_counted(torch_dev, wall):
    """gcount None (a null d_gcount: every query's count is G) against gcount full of G, Q = 5, G = 3: every output
    equal bit for bit (torch.equal on the words: query 4's cost and path are NaN).  A chunk holds hundreds of queries
    whatever the arguments (optik_hip_rrt_chunk has no knob), so the run that splits the five puts them across the
    border of a call's first chunk, behind and before rows whose start is in collision, which end before iteration 0."""
    from optik_amd import _native as nat
    torch, hc = torch_dev, wall["hc"]
    _install(wall)
    start, goal = wall["start"], wall["goal"]
    inside, inside2, near, nan_goal = start.copy(), start.copy(), start.copy(), goal.copy()
    inside[0], inside2[0], nan_goal[3] = 0.0, 0.05, math.nan
    near[0] -= 0.2
    goal2 = goal + np.array([0.2, 0.1, 0, 0.2, 0, 0, 0])
    goals = np.array([[inside, goal, goal2],        # 0, 1: two far-side roots behind and before a blocked goal
                      [goal2, goal, inside],
                      [inside, near, goal],         # 2: a directly visible goal
                      [inside, inside2, inside],    # 3: all goals in collision
                      [goal, nan_goal, near]])      # 4: a NaN in a goal, which is counted here
    starts = np.tile(start, (5, 1))

    def both(S, Gs, **args):
        s = torch.from_numpy(np.ascontiguousarray(S.T)).cuda()
        g = torch.from_numpy(np.ascontiguousarray(Gs.transpose(1, 2, 0))).cuda()
        full = torch.full((len(S),), 3, dtype=torch.int32, device="cuda")
        none, given = (hc.rrt_plan_goals(s, g, c, resolution=wall["h"], Lmax=64, **args) for c in (None, full))
        torch.cuda.synchronize()
        assert set(none) == set(given) == set(KEYS)
        for key in KEYS:
            a, b = none[key], given[key]
            if a.dtype == torch.float64:
                a, b = a.view(torch.int64), b.view(torch.int64)
            assert torch.equal(a, b), key
        return none

    res = both(starts, goals, **WALL)
    status, which = res["status"].cpu().numpy(), res["which"].cpu().numpy()
    print("no counts: status", status, "which", which, "iters", res["iters"].cpu().numpy())
    assert status.tolist() == [tu.FOUND, tu.FOUND, tu.FOUND, tu.NO_ROUTE, tu.QUERY_NAN]
    assert which[2] == 1 and which[0] in (1, 2) and which[1] in (0, 1) and (res["len"][:2] > 2).all()
    # the five across two chunks of one call
    chunk = nat.rrt_chunk(hc._h, 4096)
    Q, at = chunk + 3, chunk - 2
    S, Gs = np.tile(inside, (Q, 1)), np.tile(goals[3], (Q, 1, 1))
    S[at:at + 5], Gs[at:at + 5] = starts, goals
    split = both(S, Gs, **dict(WALL, max_nodes=4096))
    alone = both(starts, goals, **dict(WALL, max_nodes=4096))
    for key in KEYS:
        a = split[key][:, at:at + 5] if split[key].dim() > 1 else split[key][at:at + 5]
        if a.dtype == torch.float64:
            a, alone[key] = a.contiguous().view(torch.int64), alone[key].view(torch.int64)
        assert torch.equal(a, alone[key]), key
    rest = np.ones(Q, dtype=bool)
    rest[at:at + 5] = False
    assert (split["status"].cpu().numpy()[rest] == tu.NO_ROUTE).all()
    # the host-row entry point: counts None uploads nothing
    robot = wall["robot"]
    none, given = (robot.plan_rrt_to_goals(starts, goals, counts=c, resolution=wall["h"], max_waypoints=64, **WALL)
                   for c in (None, [3] * 5))
    assert set(none) == set(given)
    for key in none:
        assert torch.equal(torch.from_numpy(none[key].view(np.uint8)), torch.from_numpy(given[key].view(np.uint8))), key
        dev = res["path" if key == "paths" else "which" if key == "goal" else key].cpu().numpy()
        dev = dev.transpose(1, 0, 2) if key == "paths" else dev.T if key == "nodes" else dev
        assert np.array_equal(np.ascontiguousarray(dev).view(np.uint8), none[key].view(np.uint8)), key
    _install(wall, model=False)


def test_caps(torch_dev, wall, sets_want):
    _install(wall)
    starts, goals, counts = _goal_sets(wall)
    s, g, c = starts[2:3], goals[2:3], counts[2:3]
    # max_nodes == G: with two of the four slots roots tree 1 still has room; with four free goals it is full of roots
    got = _device(torch_dev, wall, s, g, c, iters=64, step=tu.WALL_STEP, first=tu.WALL_FIRST, max_nodes=4, Lmax=64)
    assert (got["nodes"] <= 4).all() and got["status"][0] in (tu.FOUND, tu.NO_ROUTE)
    far = np.stack([wall["goal"] + np.array([0.05 * j, 0, 0, 0, 0, 0, 0]) for j in range(4)])[None]
    got = _device(torch_dev, wall, s, far, np.array([4], dtype=np.int32), iters=64, step=tu.WALL_STEP,
                  first=tu.WALL_FIRST, max_nodes=4, Lmax=64)
    assert got["nodes"][1, 0] <= 4 and got["nodes"][0, 0] <= 4 and got["status"][0] in (tu.FOUND, tu.NO_ROUTE)
    if got["status"][0] == tu.NO_ROUTE:
        assert got["iters"][0] == 64 and got["cost"][0] == math.inf and got["which"][0] == -1
    # Lmax = 2: status 2 keeps the cost, which is -1, the path is the start and goal 0
    got = _device(torch_dev, wall, s, g, c, Lmax=2, **WALL)
    assert got["status"][0] == tu.TOO_LONG and got["len"][0] == 2 and got["which"][0] == -1
    assert_bit_equal(got["cost"], sets_want["cost"][2:3], "status 2 keeps the cost")
    assert np.array_equal(got["path"][:, 0], np.stack([s[0], g[0, 0]]))
    assert got["iters"][0] == sets_want["iters"][2] and np.array_equal(got["nodes"][:, 0], sets_want["nodes"][:, 2])
    _install(wall, model=False)


def test_trees_larger_than_a_wave(torch_dev, gref, wall):
    """test_gpu_rrt.py's large-tree case with G = 3 -- a goal in the wall, the goal, the goal moved: on the host 574
    iterations at step 0.1, 262 and 233 nodes, 39 waypoints, goal 1."""
    _install(wall)
    start, goal = wall["start"], wall["goal"]
    inside = start.copy()
    inside[0] = 0.0
    goals = np.stack([inside, goal, goal + np.array([0.2, 0.1, 0, 0.2, 0, 0, 0])])[None]
    counts, args = np.array([3], dtype=np.int32), dict(iters=640, step=0.1, first=tu.WALL_FIRST, max_nodes=4096, Lmax=64)
    want = _reference(gref, wall, start[None], goals, counts, **args)
    print("large trees: status", want["status"], "len", want["len"], "iters", want["iters"], "nodes", want["nodes"].T,
          "which", want["which"], "roots", want["roots"])
    assert want["roots"][0] == 2 and want["nodes"].max() > 128
    _assert_parity(_device(torch_dev, wall, start[None], goals, counts, **args), want, "large trees")
    _install(wall, model=False)


def test_duplicate_goals(torch_dev, gref, wall, sets_want):
    """G = 16 with the slots g, g, h, g, h, ...: tree 1 begins with roots that are copies of each other, so every
    nearest search over it meets exact ties from its first node on, and the lower index has to win each: `which` is
    the lowest slot among equal goals.  A copy never wins a search, so it never gets a child: but for the slots, the
    answer is that of the set (g, h), query 2 of the goal sets above."""
    _install(wall)
    g, h = wall["goal"], wall["goal"] + np.array([0.2, 0.1, 0, 0.2, 0, 0, 0])
    row = np.stack([g, g] + [h if k % 2 == 0 else g for k in range(14)])
    goals, counts = np.tile(row, (3, 1, 1)), np.array([16, 3, 1], dtype=np.int32)
    starts = np.tile(wall["start"], (3, 1))
    want = _reference(gref, wall, starts, goals, counts, Lmax=64, **WALL)
    print("duplicate goals: status", want["status"], "which", want["which"], "roots", want["roots"], "iters",
          want["iters"], "nodes", want["nodes"].T)
    assert want["roots"].tolist() == [16, 3, 1]
    assert (want["status"] == tu.FOUND).all() and (want["len"] > 2).all()
    for q in range(3):
        w = want["which"][q]
        assert w == min(k for k in range(counts[q]) if np.array_equal(row[k], row[w])), (q, w)
    for q in (0, 1):
        assert want["len"][q] == sets_want["len"][2] and want["iters"][q] == sets_want["iters"][2]
        assert_bit_equal(want["cost"][q:q + 1], sets_want["cost"][2:3], "the cost of the set (g, h)")
    _assert_parity(_device(torch_dev, wall, starts, goals, counts, Lmax=64, **WALL), want, "duplicate goals")
    _install(wall, model=False)


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


def test_rrt_plan_poses_is_ik_solutions_then_rrt_plan_goals(torch_dev, wall):
    from optik_amd import SolverConfig
    torch, robot, hc, K, R = torch_dev, wall["robot"], wall["hc"], 4, 64
    _install(wall)
    cfg = SolverConfig("quality", max_time=0.0, max_restarts=R).to_c()
    far = np.eye(4)
    far[:3, 3] = 5.0
    targets = np.array([_pose7(m) for m in (np.array(robot.fk(wall["goal"])), np.array(robot.fk(wall["start"])), far)])
    t = torch.from_numpy(targets).cuda()
    s = torch.from_numpy(np.ascontiguousarray(np.tile(wall["start"], (3, 1)).T)).cuda()
    got = hc.rrt_plan_poses(cfg, t, s, 0, R, K, 0.1, resolution=wall["h"], Lmax=64, **WALL)
    sol = hc.ik_solutions(cfg, t, s.t().contiguous(), 0, R, K, 0.1)
    goals = sol["x"].permute(1, 2, 0).contiguous()
    want = hc.rrt_plan_goals(s, goals, sol["count"], resolution=wall["h"], Lmax=64, **WALL)
    torch.cuda.synchronize()
    assert tuple(got["goals"].shape) == (K, 7, 3)
    assert np.array_equal(got["goals"].cpu().numpy().view(np.uint64), goals.cpu().numpy().view(np.uint64))
    assert np.array_equal(got["count"].cpu().numpy(), sol["count"].cpu().numpy())
    for key in KEYS:
        assert np.array_equal(got[key].cpu().numpy().view(np.uint8), want[key].cpu().numpy().view(np.uint8)), key
    count, status, which = (got[k].cpu().numpy() for k in ("count", "status", "which"))
    print("rrt_plan_poses: count", count, "status", status, "which", which, "iters", got["iters"].cpu().numpy())
    assert count[0] >= 1 and count[1] >= 1 and count[2] == 0
    assert status[2] == tu.NO_ROUTE and which[2] == -1 and status[1] == tu.FOUND
    assert ((which >= 0) == (status == tu.FOUND)).all() and (which < np.maximum(count, 1)).all()
    _install(wall, model=False)


def _example():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        return importlib.import_module("plan_rrt_to_pose")
    finally:
        sys.path.remove(os.path.join(ROOT, "examples"))


def _rotation_angle(Ra, Rb):
    return math.acos(max(-1.0, min(1.0, (np.trace(Ra.T @ Rb) - 1.0) / 2.0)))


def test_plan_rrt_to_poses_where_the_roadmap_finds_nothing(torch_dev):
    from conftest import ROBOT_SPECS
    from optik_amd import Robot
    ex = _example()
    results = []
    for roadmap in ("eager", "lazy", None):
        robot = Robot.from_urdf_file(*ROBOT_SPECS["panda"])
        start, target, config = ex.setup(robot)
        if roadmap is not None:
            robot.build_roadmap(ex.NODES, ex.K, ex.RESOLUTION, lazy=roadmap == "lazy")
        if roadmap == "eager":
            over = robot.plan_to_poses(config, start[None], target[None], k=ex.SOLUTIONS, min_dist=ex.MIN_DIST)
            assert over["status"][0] == tu.NO_ROUTE and over["count"][0] >= 1
        if roadmap == "lazy":
            with pytest.raises(RuntimeError):
                robot.plan_to_poses(config, start[None], target[None], k=ex.SOLUTIONS, min_dist=ex.MIN_DIST)
        res = robot.plan_rrt_to_poses(config, start[None], target[None], k=ex.SOLUTIONS, min_dist=ex.MIN_DIST,
                                      resolution=ex.RESOLUTION)
        results.append(res)
        assert set(res) == {"paths", "len", "cost", "status", "iters", "nodes", "goal", "goals", "count"}
        print(roadmap, "status", res["status"], "goal", res["goal"], "count", res["count"], "len", res["len"], "iters",
              res["iters"], "nodes", res["nodes"])
        assert res["status"][0] == tu.FOUND and 0 <= res["goal"][0] < res["count"][0] <= ex.SOLUTIONS
        L, w = int(res["len"][0]), int(res["goal"][0])
        last = res["paths"][0, L - 1]
        assert np.array_equal(last.view(np.uint64), res["goals"][0, w].view(np.uint64))   # "goal" indexes "goals"
        assert np.isnan(res["goals"][0, res["count"][0]:]).all()
        # the solver's objective is the squared norm of the logarithm (v, w) of the pose error with unit weights, and a
        # solution has f <= tol_f: the rotation angle |w| is at most r = sqrt(tol_f), and the translation V(w) v at
        # most |V| |v| <= (1 + r) r, since V = I + O(|w| / 2)
        r = math.sqrt(config.tol_f)
        T = np.array(robot.fk(last))
        assert _rotation_angle(T[:3, :3], target[:3, :3]) <= r
        assert np.linalg.norm(T[:3, 3] - target[:3, 3]) <= (1.0 + r) * r
        free = robot.collision_motion_batch_arrays(res["paths"][0, :L - 1], res["paths"][0, 1:L], ex.RESOLUTION)[1]
        assert free.all()
        short = robot.shortcut_paths(res["paths"], res["len"], resolution=ex.RESOLUTION)
        assert short["status"][0] == 0
        robot.clear_collision_model()
        robot.set_world()
    # no state in the robot, no roadmap read: the three answers are one
    for other in results[1:]:
        for key in results[0]:
            assert np.array_equal(results[0][key].view(np.uint8), other[key].view(np.uint8)), key


@pytest.mark.parametrize("name, start, goal, box", [
    ("ur10", [-0.9, -1.0, 1.2, 0, 0, 0], [0.9, -1.0, 1.2, 0, 0, 0], [0.869, 0.256, 0.415, 0, 0, 0, 1, 0.05, 0.05, 0.3]),
    ("arm10", [-0.9] + [0.3] * 9, [0.9] + [0.3] * 9, [0.058, -0.15, -0.599, 0, 0, 0, 1, 0.05, 0.05, 0.3])])
def test_other_chains(torch_dev, gref, name, start, goal, box):
    """A 6-joint chain and a chain of the general kernels (10 joints), the scenes of test_gpu_rrt.py: one goal against
    rrt_plan, and a set of three -- half-way (where the box is), the goal, the goal moved -- against the reference."""
    torch = torch_dev
    sc = _scene(name, [box])
    _install(sc)
    s, g = np.array(start, dtype=np.float64)[None], np.array(goal, dtype=np.float64)[None]
    args = dict(iters=128, step=0.3, first=1, max_nodes=64, Lmax=64)
    st, gt = (torch.from_numpy(np.ascontiguousarray(v.T)).cuda() for v in (s, g))
    one = {k: v.cpu().numpy() for k, v in sc["hc"].rrt_plan(st, gt, resolution=sc["h"], **args).items()}
    assert one["status"][0] == tu.FOUND and one["len"][0] > 2
    got = _device(torch, sc, s, g[:, None, :], np.ones(1, dtype=np.int32), **args)
    for key in ("path", "len", "cost", "status", "iters", "nodes"):
        assert np.array_equal(got[key].view(np.uint8), one[key].view(np.uint8)), (name, key)
    assert got["which"][0] == 0
    half, moved = 0.5 * (s[0] + g[0]), g[0].copy()
    moved[1] += 0.15
    goals, counts = np.stack([half, g[0], moved])[None], np.array([3], dtype=np.int32)
    want = _reference(gref, sc, s, goals, counts, **args)
    print(name, "status", want["status"], "which", want["which"], "roots", want["roots"], "iters", want["iters"])
    assert want["roots"][0] >= 1
    _assert_parity(_device(torch, sc, s, goals, counts, **args), want, name)
    _install(sc, model=False)


def test_refusals(torch_dev, wall, chains):
    from optik_amd import _native as nat
    from optik_amd import device
    from optik_amd.device import _ptr
    torch = torch_dev
    lib, hc, robot = nat.lib(), wall["hc"], wall["robot"]
    s = torch.zeros((7, 3), dtype=torch.float64, device="cuda")
    g = torch.zeros((16, 7, 3), dtype=torch.float64, device="cuda")
    c = torch.ones(3, dtype=torch.int32, device="cuda")
    path = _out((4, 3, 7), torch.float64)
    which = _out((3,), torch.int32)

    def plan(h=hc, Q=3, G=2, iters=8, step=0.3, res=0.1, max_nodes=16, Lmax=4, poll=4):
        return lib.optik_hip_rrt_plan_goals(h._h, None, _ptr(s), _ptr(g), _ptr(c), Q, G, iters, step, res, 0, max_nodes,
                                            Lmax, poll, _ptr(path), None, None, None, None, None, _ptr(which), None)
    bad = (dict(G=0), dict(G=17), dict(G=-1), dict(G=3, max_nodes=2), dict(G=16, max_nodes=15), dict(G=1, max_nodes=1),
           dict(Q=-1), dict(Q=(1 << 30) + 1), dict(iters=0), dict(iters=65537), dict(step=0.0), dict(step=-0.1),
           dict(step=math.nan), dict(step=math.inf), dict(max_nodes=4097), dict(Lmax=1), dict(Lmax=65), dict(poll=0),
           dict(poll=65537), dict(res=0.0), dict(res=math.nan), dict(res=math.inf))
    for kw in bad:
        assert plan(**kw) == -1, kw                                           # OPTIK_HIP_EINVAL
    torch.cuda.synchronize()
    assert _sentinels_left(path.cpu().numpy()) == path.numel() and _sentinels_left(which.cpu().numpy()) == 3
    assert plan(Q=0) == 0 and plan(G=16, max_nodes=16, Q=0) == 0 and plan(G=1, max_nodes=2, Q=0) == 0
    gantry = device.HipChain(**chains["gantry"][0])
    assert plan(h=gantry) == -2 and plan(h=gantry, Q=0) == -2                 # OPTIK_HIP_EUNSUPPORTED
    assert _sentinels_left(path.cpu().numpy()) == path.numel()
    # the caps themselves are accepted: 16 goals in trees of 16 nodes
    assert plan(G=16, max_nodes=16) == 0
    torch.cuda.synchronize()
    assert _sentinels_left(path.cpu().numpy()) == 0 and _sentinels_left(which.cpu().numpy()) == 0
    x, gs = np.zeros((3, 7)), np.zeros((3, 2, 7))
    for kw in (dict(iters=0), dict(iters=65537), dict(step=0.0), dict(step=math.nan), dict(max_nodes=1),
               dict(max_nodes=4097), dict(max_waypoints=1), dict(max_waypoints=65), dict(poll=0), dict(poll=65537),
               dict(resolution=0.0), dict(resolution=math.inf)):
        with pytest.raises(ValueError):
            robot.plan_rrt_to_goals(x, gs, **kw)
    for goals, kw in ((gs[:2], {}), (np.zeros((3, 17, 7)), {}), (np.zeros((3, 0, 7)), {}), (np.zeros((3, 2, 6)), {}),
                      (np.zeros((3, 3, 7)), dict(max_nodes=2)), (gs, dict(counts=np.zeros(2, dtype=np.int32)))):
        with pytest.raises(ValueError):
            robot.plan_rrt_to_goals(x, goals, **kw)
    with pytest.raises(ValueError):
        hc.rrt_plan_goals(s, g[:, :, :2].contiguous(), c, 8, 0.3, 0.1)
    with pytest.raises(ValueError):
        hc.rrt_plan_goals(s, g, c, 8, 0.3, 0.1, max_nodes=15)
    L = robot._L
    assert L.optik_robot_rrt_plan_goals(robot._h, None, None, None, 2, 0, 8, 0.3, 0.1, 0, 16, 4, 4, None, None, None,
                                        None, None, None, None, None) == -1
    empty = robot.plan_rrt_to_goals(np.zeros((0, 7)), np.zeros((0, 2, 7)))
    assert empty["paths"].shape == (0, 64, 7) and empty["nodes"].shape == (0, 2) and empty["goal"].shape == (0,)
