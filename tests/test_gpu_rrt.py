"""-m gpu: the bidirectional tree planner on the device against the serial reference of csrc/rrt_measure.hpp (g++,
rrt_util).  The reference's verdicts come from Robot.collision_clearance_batch_arrays and
Robot.collision_motion_batch_arrays and its samples from HipChain.seed_batch -- the device's own, already tested
answers --, so what is compared bit for bit is the new code alone: nearest, steer, commit and walk."""
import ctypes as C
import math

import numpy as np
import pytest

import roadmap_util as ru
import rrt_util as tu
from conftest import ROBOT_SPECS
from gpu_util import _out, _sentinels_left, assert_bit_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return tu.build_rrt_ref(str(tmp_path_factory.mktemp("rrt_measure")))


def _scene(name, boxes, h=0.1):
    from optik_amd import Robot
    from optik_amd.collision import spheres_along_chain
    robot = Robot.from_urdf_file(*ROBOT_SPECS[name])
    frames, centers, radii = spheres_along_chain(robot, 0.05, 2)
    sc = dict(robot=robot, hc=robot.hip_chain(), frames=frames, centers=centers, radii=radii, boxes=np.array(boxes),
              h=h)
    lo, hi = robot.joint_limits()
    sc["lo"], sc["hi"] = np.array(lo), np.array(hi)
    return sc


def _install(sc, model=True):
    """The same model and world on the robot's chain (Robot.plan_rrt and the reference's verdicts) and on the
    device-tensor chain (HipChain.rrt_plan)."""
    for who in (sc["robot"], sc["hc"]):
        if model:
            who.set_collision_model(sc["frames"], sc["centers"], sc["radii"], self_pairs=None)
            who.set_world(boxes=sc["boxes"])
        else:
            who.clear_collision_model()
            who.set_world()


@pytest.fixture(scope="module")
def wall():
    sc = ru.wall_scene()
    out = _scene("panda", sc["boxes"], sc["h"])
    out["start"], out["goal"] = sc["start"], sc["goal"]
    # the wall pair, the pair reversed, a pair whose direct move is free, a start in collision, a NaN goal
    inside = sc["start"].copy()
    inside[0] = 0.0   # (half-way through the sweep: the arm is in the wall)
    nan_goal = sc["goal"].copy()
    nan_goal[3] = math.nan
    near = sc["start"].copy()
    near[0] -= 0.2
    out["starts"] = np.stack([sc["start"], sc["goal"], sc["start"], inside, sc["start"]])
    out["goals"] = np.stack([sc["goal"], sc["start"], near, sc["goal"], nan_goal])
    return out


def _reference(ref, sc, starts, goals, iters, step, first, max_nodes, Lmax):
    """The serial reference per query, with the device's own verdicts and samples."""
    robot, h = sc["robot"], sc["h"]
    samples = sc["hc"].seed_batch(first, iters).cpu().numpy().T.copy()
    config_free = lambda q: bool(robot.collision_clearance_batch_arrays(q[None])[1][0])  # noqa: E731
    motions_free = lambda qa, qb: robot.collision_motion_batch_arrays(qa, qb, h)[1]       # noqa: E731
    rows = [ref.plan(sc["lo"], sc["hi"], s, g, samples, step, max_nodes, Lmax, config_free, motions_free)
            for s, g in zip(starts, goals)]
    return dict(path=np.stack([r["path"] for r in rows], axis=1), len=np.array([r["len"] for r in rows]),
                cost=np.array([r["cost"] for r in rows]), status=np.array([r["status"] for r in rows]),
                iters=np.array([r["iters"] for r in rows]), nodes=np.stack([r["nodes"] for r in rows], axis=1))


def _device(torch, sc, starts, goals, iters, step, first, max_nodes, Lmax, poll=32):
    """optik_hip_rrt_plan on sentinel-filled outputs: every element is written."""
    from optik_amd import _native as nat
    from optik_amd.device import _ptr, _stream_ptr
    hc, Q, n = sc["hc"], len(starts), starts.shape[1]
    s = torch.from_numpy(np.ascontiguousarray(starts.T)).cuda()
    g = torch.from_numpy(np.ascontiguousarray(goals.T)).cuda()
    res = dict(path=_out((Lmax, Q, n), torch.float64), len=_out((Q,), torch.int32), cost=_out((Q,), torch.float64),
               status=_out((Q,), torch.int32), iters=_out((Q,), torch.int32), nodes=_out((2, Q), torch.int32))
    nat.check(nat.lib().optik_hip_rrt_plan(hc._h, None, _ptr(s), _ptr(g), Q, iters, step, sc["h"], first, max_nodes, Lmax,
                                           poll, _ptr(res["path"]), _ptr(res["len"]), _ptr(res["cost"]),
                                           _ptr(res["status"]), _ptr(res["iters"]), _ptr(res["nodes"]), _stream_ptr()))
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in res.items()}
    for k, v in res.items():
        assert _sentinels_left(v) == 0, k
    return res


def _assert_parity(got, want, what):
    for key in ("len", "status", "iters", "nodes"):
        assert np.array_equal(got[key], want[key]), (what, key, got[key], want[key])
    assert_bit_equal(got["cost"], want["cost"], f"{what}: cost")
    assert_bit_equal(got["path"], want["path"], f"{what}: path")


WALL = dict(iters=tu.WALL_ITERS, step=tu.WALL_STEP, first=tu.WALL_FIRST, max_nodes=tu.WALL_NODES)


@pytest.fixture(scope="module")
def wall_want(ref, wall, torch_dev):
    """The reference's answer for the five queries of the wall scene, computed once."""
    _install(wall)
    return _reference(ref, wall, wall["starts"], wall["goals"], Lmax=64, **WALL)


def test_parity_on_the_wall_scene(torch_dev, wall, wall_want):
    _install(wall)
    robot, h = wall["robot"], wall["h"]
    assert not robot.collision_motion_batch_arrays(wall["start"][None], wall["goal"][None], h)[1][0]
    want = wall_want
    print("wall scene: status", want["status"], "len", want["len"], "iters", want["iters"], "nodes", want["nodes"].T)
    assert want["status"].tolist() == [tu.FOUND, tu.FOUND, tu.FOUND, tu.NO_ROUTE, tu.QUERY_NAN]
    assert want["len"][0] > 2 and want["len"][1] > 2 and want["len"][2] == 2
    assert want["iters"][2:].tolist() == [0, 0, 0] and want["iters"][0] > 1 and want["iters"][1] > 1
    got = _device(torch_dev, wall, wall["starts"], wall["goals"], Lmax=64, **WALL)
    _assert_parity(got, want, "wall scene")
    # the host-row entry point gives the same plans
    rows = robot.plan_rrt(wall["starts"], wall["goals"], resolution=h, max_waypoints=64, **WALL)
    _assert_parity(dict(path=rows["paths"].transpose(1, 0, 2), len=rows["len"], cost=rows["cost"],
                        status=rows["status"], iters=rows["iters"], nodes=rows["nodes"].T), want, "Robot.plan_rrt")
    # independent of the reference: every segment of every found path is free at the same resolution, in path order
    for q in range(5):
        if got["status"][q] != tu.FOUND:
            assert np.array_equal(got["path"][0, q], wall["starts"][q], equal_nan=True) and got["len"][q] == 2
            assert np.array_equal(got["path"][1:, q], np.tile(wall["goals"][q], (63, 1)), equal_nan=True)
            continue
        L = got["len"][q]
        p = got["path"][:, q]
        assert np.array_equal(p[0], wall["starts"][q]) and np.array_equal(p[L - 1:], np.tile(wall["goals"][q], (65 - L, 1)))
        assert robot.collision_motion_batch_arrays(p[:L - 1], p[1:L], h)[1].all(), q
        assert got["cost"][q] == tu.forward_cost(p, L)
    _install(wall, model=False)


def test_a_query_does_not_depend_on_the_batch_or_on_poll(torch_dev, wall, wall_want):
    _install(wall)
    rng = np.random.default_rng(26)
    starts = rng.uniform(wall["lo"], wall["hi"], (70, 7))
    goals = rng.uniform(wall["lo"], wall["hi"], (70, 7))
    starts[37], goals[37] = wall["start"], wall["goal"]
    starts[5, 2] = math.nan
    alone = _device(torch_dev, wall, wall["start"][None], wall["goal"][None], Lmax=64, **WALL)
    _assert_parity(alone, {k: (v[:, :1] if v.ndim > 1 else v[:1]) for k, v in wall_want.items()}, "alone")
    seen = set()
    for poll in (1, 65536):
        got = _device(torch_dev, wall, starts, goals, Lmax=64, poll=poll, **WALL)
        _assert_parity({k: (v[:, 37:38] if v.ndim > 1 else v[37:38]) for k, v in got.items()}, alone, f"poll {poll}")
        seen |= set(got["status"].tolist())
        if poll == 1:
            first = got
        else:
            _assert_parity(got, first, "poll 65536 against poll 1")
    assert {tu.FOUND, tu.QUERY_NAN} <= seen
    _install(wall, model=False)


def test_two_chunks(torch_dev, wall):
    from optik_amd import _native as nat
    _install(wall)
    chunk = nat.rrt_chunk(wall["hc"]._h, 4096)
    assert chunk == (256 << 20) // (2 * 4096 * (8 * 7 + 4)) and 500 < chunk < 600
    Q = chunk + 40
    rng = np.random.default_rng(27)
    starts = rng.uniform(wall["lo"], wall["hi"], (Q, 7))
    goals = starts + rng.uniform(-0.6, 0.6, (Q, 7))
    goals = np.clip(goals, wall["lo"], wall["hi"])
    args = dict(iters=4, step=0.3, first=3, max_nodes=4096, Lmax=16)
    got = _device(torch_dev, wall, starts, goals, **args)
    assert len(set(got["status"].tolist())) >= 2
    for q in (0, chunk - 1, chunk, Q - 1):
        one = _device(torch_dev, wall, starts[q:q + 1], goals[q:q + 1], **args)
        _assert_parity({k: (v[:, q:q + 1] if v.ndim > 1 else v[q:q + 1]) for k, v in got.items()}, one, f"row {q}")
    _install(wall, model=False)


def test_caps(torch_dev, wall, wall_want):
    _install(wall)
    s, g = wall["start"][None], wall["goal"][None]
    got = _device(torch_dev, wall, s, g, iters=64, step=tu.WALL_STEP, first=tu.WALL_FIRST, max_nodes=2, Lmax=64)
    assert got["status"][0] == tu.NO_ROUTE and (got["nodes"] <= 2).all() and got["iters"][0] == 64
    assert got["cost"][0] == math.inf
    got = _device(torch_dev, wall, s, g, Lmax=2, **WALL)
    assert got["status"][0] == tu.TOO_LONG and got["len"][0] == 2
    assert_bit_equal(got["cost"], wall_want["cost"][:1], "status 2 keeps the cost")
    assert np.array_equal(got["path"][:, 0], np.stack([wall["start"], wall["goal"]]))
    assert got["iters"][0] == wall_want["iters"][0] and np.array_equal(got["nodes"][:, 0], wall_want["nodes"][:, 0])
    _install(wall, model=False)


# ---- trees past one wave, trees that fill, the Lmax border -----------------------------------------------------------
# The wall scene at step 0.3 ends with trees of 17 and 13 nodes (23 and 22 for the pair reversed) with the host motion
# check: no lane of the nearest search ever holds a second node.  With a step of 0.1 the same pair needs 574 iterations
# and ends with 262 and 232 nodes and 39 waypoints on the host; with max_nodes = 70 the same growth fills tree 0 first
# and then tree 1, and no route is found.  (Chosen on the CPU with the host motion check; the preconditions below are
# asserted on the reference fed with the device's verdicts.)
LARGE = dict(iters=640, step=0.1, first=tu.WALL_FIRST, max_nodes=tu.MAX_NODES)
FILL_NODES = 70


def test_trees_larger_than_a_wave(torch_dev, ref, wall):
    _install(wall)
    s, g = wall["start"][None], wall["goal"][None]
    want = _reference(ref, wall, s, g, Lmax=64, **LARGE)
    print("large trees: status", want["status"], "len", want["len"], "iters", want["iters"], "nodes", want["nodes"].T)
    assert want["nodes"].max() > 128
    _assert_parity(_device(torch_dev, wall, s, g, Lmax=64, **LARGE), want, "large trees")
    _install(wall, model=False)


@pytest.mark.parametrize("iters, both", [(144, False), (256, True)])
def test_a_tree_that_fills_while_the_other_grows(torch_dev, ref, wall, iters, both):
    """max_nodes = 70 at step 0.1.  On the host tree 0 holds 69 nodes after 130 iterations and 70 after 140, tree 1 holds
    65 after 140, 67 after 150 and 70 after 160.  After 144 one tree is full and the other is not: the full tree's own
    iterations give up (cnt_a >= M), the other tree's go on, and its back-extensions into the full tree are refused
    (extends_back, and the commit's cnt_b < M).  After 256 both are full and the query ends in status 1 at the budget."""
    _install(wall)
    s, g = wall["start"][None], wall["goal"][None]
    args = dict(iters=iters, step=0.1, first=tu.WALL_FIRST, max_nodes=FILL_NODES, Lmax=64)
    want = _reference(ref, wall, s, g, **args)
    print("fill: status", want["status"], "iters", want["iters"], "nodes", want["nodes"].T)
    assert want["status"][0] == tu.NO_ROUTE and want["iters"][0] == iters
    nodes = sorted(want["nodes"][:, 0].tolist())
    assert nodes[1] == FILL_NODES and (nodes[0] == FILL_NODES if both else 2 < nodes[0] < FILL_NODES)
    _assert_parity(_device(torch_dev, wall, s, g, **args), want, f"fill after {iters}")
    _install(wall, model=False)


def test_lmax_border(torch_dev, ref, wall, wall_want):
    """found_status is W <= Lmax: Lmax = W is found with no padding row, Lmax = W - 1 is status 2 with the cost kept."""
    _install(wall)
    s, g = wall["start"][None], wall["goal"][None]
    W = int(wall_want["len"][0])
    assert wall_want["status"][0] == tu.FOUND and W >= 4
    for Lmax, status in ((W, tu.FOUND), (W - 1, tu.TOO_LONG)):
        want = _reference(ref, wall, s, g, Lmax=Lmax, **WALL)
        assert want["status"][0] == status and want["len"][0] == (W if status == tu.FOUND else 2)
        assert_bit_equal(want["cost"], wall_want["cost"][:1], "the cost is the route's either way")
        if status == tu.FOUND:
            assert_bit_equal(want["path"][:, 0], wall_want["path"][:W, 0], "the waypoints and nothing behind them")
        else:
            assert np.array_equal(want["path"][:, 0],
                                  np.concatenate([wall["start"][None], np.tile(wall["goal"], (W - 2, 1))]))
        _assert_parity(_device(torch_dev, wall, s, g, Lmax=Lmax, **WALL), want, f"Lmax {Lmax}")
    _install(wall, model=False)


def test_without_a_model_every_finite_pair_is_direct(torch_dev, wall):
    _install(wall, model=False)
    rng = np.random.default_rng(28)
    starts, goals = rng.uniform(-3, 3, (33, 7)), rng.uniform(-3, 3, (33, 7))
    got = _device(torch_dev, wall, starts, goals, iters=8, step=0.3, first=0, max_nodes=16, Lmax=5)
    assert (got["status"] == tu.FOUND).all() and (got["len"] == 2).all() and (got["iters"] == 0).all()
    assert_bit_equal(got["cost"], np.max(np.abs(goals - starts), axis=1), "direct cost")
    assert np.array_equal(got["path"][0], starts) and np.array_equal(got["path"][1:], np.broadcast_to(goals, (4, 33, 7)))


@pytest.mark.parametrize("name, start, goal, box", [
    ("ur10", [-0.9, -1.0, 1.2, 0, 0, 0], [0.9, -1.0, 1.2, 0, 0, 0], [0.869, 0.256, 0.415, 0, 0, 0, 1, 0.05, 0.05, 0.3]),
    ("arm10", [-0.9] + [0.3] * 9, [0.9] + [0.3] * 9, [0.058, -0.15, -0.599, 0, 0, 0, 1, 0.05, 0.05, 0.3])])
def test_other_chains(torch_dev, ref, name, start, goal, box):
    """A 6-joint chain and a chain of the general kernels (10 joints): the box sits where the end effector passes
    half-way through the sweep of the first joint (chosen on the CPU with the host motion check)."""
    sc = _scene(name, [box])
    _install(sc)
    s, g = np.array(start, dtype=np.float64)[None], np.array(goal, dtype=np.float64)[None]
    assert not sc["robot"].collision_motion_batch_arrays(s, g, sc["h"])[1][0]
    args = dict(iters=128, step=0.3, first=1, max_nodes=64, Lmax=64)
    want = _reference(ref, sc, s, g, **args)
    assert want["status"][0] == tu.FOUND and want["len"][0] > 2
    _assert_parity(_device(torch_dev, sc, s, g, **args), want, name)
    _install(sc, model=False)


def test_one_joint(torch_dev, ref):
    """n = 1 (panda1): only lane 0 steers and writes.  One sphere of 5 cm, 0.4 m off the joint's axis on the turning
    link, and a box where that sphere passes at q = 0: the sweep from -0.9 to 0.9 is blocked, and with one joint there is
    no way round, so the trees grow on their own sides until the budget ends (19 and 12 nodes with the host motion
    check).  The same start with a goal on its own side is a direct motion."""
    sc = _scene("panda1", [[0.4, 0.0, 0.333, 0, 0, 0, 1, 0.05, 0.05, 0.05]])
    sc["frames"], sc["centers"], sc["radii"] = np.array([1], dtype=np.int32), np.array([[0.4, 0.0, 0.0]]), np.array([0.05])
    _install(sc)
    starts, goals = np.array([[-0.9], [-0.9]]), np.array([[0.9], [-2.0]])
    assert not sc["robot"].collision_motion_batch_arrays(starts[:1], goals[:1], sc["h"])[1][0]
    args = dict(iters=64, step=0.3, first=1, max_nodes=64, Lmax=64)
    want = _reference(ref, sc, starts, goals, **args)
    print("panda1: status", want["status"], "iters", want["iters"], "nodes", want["nodes"].T)
    assert want["status"].tolist() == [tu.NO_ROUTE, tu.FOUND]
    assert want["iters"].tolist() == [64, 0] and want["nodes"][:, 0].min() > 2 and want["len"][1] == 2
    _assert_parity(_device(torch_dev, sc, starts, goals, **args), want, "panda1")
    _install(sc, model=False)


# The 16-joint arm (the general kernels at their widest), the sweep of test_other_chains: the box sits where the end
# effector passes at q0 = 0, and is small enough that both ends are free (chosen on the CPU with the host motion check,
# which joins the trees after 4 iterations with 4 waypoints).
ARM16 = dict(start=[-0.9] + [0.3] * 15, goal=[0.9] + [0.3] * 15,
             box=[-0.277, -0.501, 0.043, 0, 0, 0, 1, 0.02, 0.02, 0.1])


def test_sixteen_joints(torch_dev, ref):
    sc = _scene("arm16", [ARM16["box"]])
    _install(sc)
    s, g = (np.array(ARM16[k], dtype=np.float64)[None] for k in ("start", "goal"))
    assert not sc["robot"].collision_motion_batch_arrays(s, g, sc["h"])[1][0]
    args = dict(iters=128, step=0.3, first=1, max_nodes=64, Lmax=64)
    want = _reference(ref, sc, s, g, **args)
    print("arm16: status", want["status"], "len", want["len"], "iters", want["iters"], "nodes", want["nodes"].T)
    assert want["status"][0] == tu.FOUND and want["len"][0] > 2
    _assert_parity(_device(torch_dev, sc, s, g, **args), want, "arm16")
    _install(sc, model=False)


def test_refusals(torch_dev, wall, chains):
    from optik_amd import _native as nat
    from optik_amd import device
    from optik_amd.device import _ptr
    torch = torch_dev
    lib, hc, robot = nat.lib(), wall["hc"], wall["robot"]
    s = torch.zeros((7, 3), dtype=torch.float64, device="cuda")
    path = _out((4, 3, 7), torch.float64)
    status = _out((3,), torch.int32)

    def plan(h=hc, Q=3, iters=8, step=0.3, res=0.1, max_nodes=16, Lmax=4, poll=4):
        return lib.optik_hip_rrt_plan(h._h, None, _ptr(s), _ptr(s), Q, iters, step, res, 0, max_nodes, Lmax, poll,
                                      _ptr(path), None, None, _ptr(status), None, None, None)
    bad = (dict(Q=-1), dict(Q=(1 << 30) + 1), dict(iters=0), dict(iters=65537), dict(step=0.0), dict(step=-0.1),
           dict(step=math.nan), dict(step=math.inf), dict(max_nodes=1), dict(max_nodes=4097), dict(Lmax=1),
           dict(Lmax=65), dict(poll=0), dict(poll=65537), dict(res=0.0), dict(res=math.nan), dict(res=math.inf))
    for kw in bad:
        assert plan(**kw) == -1, kw                                           # OPTIK_HIP_EINVAL
    torch.cuda.synchronize()
    assert _sentinels_left(path.cpu().numpy()) == path.numel() and _sentinels_left(status.cpu().numpy()) == 3
    assert plan(Q=0) == 0
    gantry = device.HipChain(**chains["gantry"][0])
    assert plan(h=gantry) == -2 and plan(h=gantry, Q=0) == -2                 # OPTIK_HIP_EUNSUPPORTED
    assert _sentinels_left(path.cpu().numpy()) == path.numel()
    x = np.zeros((3, 7))
    for kw in (dict(iters=0), dict(iters=65537), dict(step=0.0), dict(step=math.nan), dict(max_nodes=1),
               dict(max_nodes=4097), dict(max_waypoints=1), dict(max_waypoints=65), dict(poll=0), dict(poll=65537),
               dict(resolution=0.0), dict(resolution=math.inf)):
        with pytest.raises(ValueError):
            robot.plan_rrt(x, x, **kw)
    with pytest.raises(ValueError):
        robot.plan_rrt(x, x[:2])
    L = robot._L
    assert L.optik_robot_rrt_plan(robot._h, None, None, 0, 0, 0.3, 0.1, 0, 16, 4, 4, None, None, None, None, None, None,
                                  None) == -1
    empty = robot.plan_rrt(np.zeros((0, 7)), np.zeros((0, 7)))
    assert empty["paths"].shape == (0, 64, 7) and empty["nodes"].shape == (0, 2)
