"""-m gpu: the tree planner under a pose constraint on the device against the serial reference of
csrc/rrt_constrained_measure.hpp (g++, rrt_constrained_util).  As in test_gpu_rrt.py the reference's verdicts, samples
and here also its projections are the device's own, already tested answers (Robot.collision_clearance_batch_arrays,
collision_motion_batch_arrays, constraint_batch_arrays, constraint_motion_batch_arrays,
constraint_project_batch_arrays, HipChain.seed_batch), so a 1-ulp host/device FK difference cannot fork the trees and
what is compared bit for bit is the new code alone: rule 0's mask, the step kernel with the projection inside, the
counters.  The Panda wall scene with upright(fk(start), 0.3) at rrt_constrained_util's parameters: the host build
joins the pair after 51 iterations and the pair reversed after 107 (tests/test_rrt_constrained_host.py)."""
import math

import numpy as np
import pytest

import constraint_util as cu
import rrt_constrained_util as xu
import rrt_util as tu
from gpu_util import _out, _sentinels_left, assert_bit_equal
from test_gpu_rrt import _install, _scene, torch_dev, wall  # noqa: F401  (the scene and its fixtures)

pytestmark = pytest.mark.gpu
KEYS = ("path", "len", "cost", "status", "iters", "nodes", "which", "projected")
PLAN = dict(iters=xu.ITERS, step=xu.STEP, first=xu.FIRST, max_nodes=xu.NODES)
CON = dict(tol=xu.TOL, ptol=xu.PTOL, piters=xu.PITERS, damping=xu.DAMPING, max_step=xu.MAX_STEP)


@pytest.fixture(scope="module")
def xref(tmp_path_factory):
    return xu.build_rrt_constrained_ref(str(tmp_path_factory.mktemp("rrt_constrained_measure")))


def _upright(robot, q, tilt, ee=None):
    from optik_amd import PoseConstraint
    return PoseConstraint.upright(np.array(robot.fk(q, ee)).reshape(4, 4), tilt)


@pytest.fixture(scope="module")
def upright(wall):
    return _upright(wall["robot"], wall["start"], xu.TILT)


def _reference(xref, sc, c, starts, goals, counts, iters, step, first, max_nodes, Lmax, tol, ptol, piters, damping,
               max_step, ee=None):
    """The serial reference per query, with the device's own verdicts, samples and projections."""
    robot, h = sc["robot"], sc["h"]
    samples = sc["hc"].seed_batch(first, iters).cpu().numpy().T.copy()

    def config_ok(q):
        return bool(robot.collision_clearance_batch_arrays(q[None], ee)[1][0]
                    and robot.constraint_batch_arrays(q[None], c, ee)[1][0] <= tol)

    def motions_ok(qa, qb):
        return (robot.collision_motion_batch_arrays(qa, qb, h, ee)[1]
                & robot.constraint_motion_batch_arrays(qa, qb, h, c, tol, ee)[1])

    def project(x):
        p = robot.constraint_project_batch_arrays(x[None], c, ptol, piters, damping, max_step, ee)
        return p["x"][0], p["status"][0], p["iterations"][0]

    rows = [xref.plan(sc["lo"], sc["hi"], s, g, n, samples, step, max_nodes, Lmax, config_ok, motions_ok, project)
            for s, g, n in zip(starts, goals, counts)]
    return dict(path=np.stack([r["path"] for r in rows], axis=1), len=np.array([r["len"] for r in rows]),
                cost=np.array([r["cost"] for r in rows]), status=np.array([r["status"] for r in rows]),
                iters=np.array([r["iters"] for r in rows]), nodes=np.stack([r["nodes"] for r in rows], axis=1),
                which=np.array([r["which"] for r in rows]), roots=np.array([r["roots"] for r in rows]),
                projected=np.stack([r["projected"] for r in rows], axis=1))


def _device(torch, sc, c, starts, goals, counts, iters, step, first, max_nodes, Lmax, tol, ptol, piters, damping,
            max_step, poll=32, ee7=None):
    """optik_hip_rrt_plan_constrained on sentinel-filled outputs: every element is written.  goals [Q, G, n]."""
    from optik_amd import _native as nat
    from optik_amd.constraint import constraint_arrays
    from optik_amd.device import _dp, _ptr, _stream_ptr
    hc, (Q, G, n) = sc["hc"], goals.shape
    s = torch.from_numpy(np.ascontiguousarray(starts.T)).cuda()
    g = torch.from_numpy(np.ascontiguousarray(goals.transpose(1, 2, 0))).cuda()
    cn = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).cuda()
    ref7, lo, hi = constraint_arrays(c)
    ee = np.ascontiguousarray(ee7, dtype=np.float64) if ee7 is not None else None
    res = dict(path=_out((Lmax, Q, n), torch.float64), len=_out((Q,), torch.int32), cost=_out((Q,), torch.float64),
               status=_out((Q,), torch.int32), iters=_out((Q,), torch.int32), nodes=_out((2, Q), torch.int32),
               which=_out((Q,), torch.int32), projected=_out((2, Q), torch.int32))
    nat.check(nat.lib().optik_hip_rrt_plan_constrained(
        hc._h, _dp(ee) if ee is not None else None, _dp(ref7), _dp(lo), _dp(hi), tol, ptol, piters, damping, max_step,
        _ptr(s), _ptr(g), _ptr(cn), Q, G, iters, step, sc["h"], first, max_nodes, Lmax, poll, _ptr(res["path"]),
        _ptr(res["len"]), _ptr(res["cost"]), _ptr(res["status"]), _ptr(res["iters"]), _ptr(res["nodes"]),
        _ptr(res["which"]), _ptr(res["projected"]), _stream_ptr()))
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in res.items()}
    for k, v in res.items():
        assert _sentinels_left(v) == 0, k
    return res


def _assert_parity(got, want, what):
    for key in ("len", "status", "iters", "nodes", "which", "projected"):
        assert np.array_equal(got[key], want[key]), (what, key, got[key], want[key])
    assert_bit_equal(got["cost"], want["cost"], f"{what}: cost")
    assert_bit_equal(got["path"], want["path"], f"{what}: path")


def _rows(res, rows):
    return {k: (res[k][:, rows] if res[k].ndim > 1 else res[k][rows]) for k in KEYS}


def nat_certify(name):
    from optik_amd import _native as nat
    return getattr(nat, "CERTIFY_" + name)


def _tipped(q):
    """q with the wrist turned by 1 rad: free where q is, and far outside upright(fk(q), 0.3)."""
    t = q.copy()
    t[5] -= 1.0
    return t


def _five(wall):
    """The pair, the pair reversed, a pair whose direct move passes both checks, a start that violates, a NaN goal."""
    start, goal = wall["start"], wall["goal"]
    near, nan_goal = start.copy(), goal.copy()
    near[0] -= 0.2
    nan_goal[3] = math.nan
    return (np.stack([start, goal, start, _tipped(start), start]),
            np.stack([goal, start, near, goal, nan_goal])[:, None, :], np.ones(5, dtype=np.int32))


@pytest.fixture(scope="module")
def five_want(xref, wall, upright, torch_dev):
    _install(wall)
    return _reference(xref, wall, upright, *_five(wall), Lmax=64, **PLAN, **CON)


def test_parity_on_five_queries(torch_dev, wall, upright, five_want):
    _install(wall)
    robot, h = wall["robot"], wall["h"]
    starts, goals, counts = _five(wall)
    want = five_want
    print("five: status", want["status"], "len", want["len"], "iters", want["iters"], "nodes", want["nodes"].T,
          "projected", want["projected"].T)
    F, N, X = tu.FOUND, tu.NO_ROUTE, tu.QUERY_NAN
    assert want["status"].tolist() == [F, F, F, N, X]
    assert want["len"][0] > 2 and want["len"][1] > 2 and want["len"][2] == 2
    assert want["iters"][2:].tolist() == [0, 0, 0] and (want["projected"][:, 2:] == 0).all()
    assert (want["projected"][0, :2] > 0).all() and (want["nodes"][:, 2:] == 0).all()
    got = _device(torch_dev, wall, upright, starts, goals, counts, Lmax=64, **PLAN, **CON)
    _assert_parity(got, want, "five queries")
    # independent of the reference: found paths pass both checks in path order, every waypoint is on the constraint
    for q in range(5):
        p, L = got["path"][:, q], got["len"][q]
        assert np.array_equal(p[0], starts[q])
        if got["status"][q] != F:
            assert got["which"][q] == -1 and L == 2
            continue
        assert robot.collision_motion_batch_arrays(p[:L - 1], p[1:L], h)[1].all(), q
        chk = robot.check_paths_constraint(p[None, :L], None, upright, tol=xu.TOL, resolution=h)
        assert chk["ok"][0] and chk["segment"][0] == -1, q
        assert (robot.constraint_batch_arrays(p[:L], upright)[1] <= xu.PTOL).all(), q
        assert got["cost"][q] == tu.forward_cost(p, L)
    # the unconstrained planner's path for the same pair tips the glass over
    plain = robot.plan_rrt(starts[:1], goals[:1, 0], resolution=h, max_waypoints=64, **PLAN)
    assert plain["status"][0] == F
    assert not robot.check_paths_constraint(plain["paths"], plain["len"], upright, tol=xu.TOL, resolution=h)["ok"][0]
    # Robot against HipChain: the host-row entry points give the same plans
    rows = robot.plan_rrt_constrained(starts, goals[:, 0], upright, resolution=h, max_waypoints=64, **PLAN, **CON)
    assert set(rows) == {"paths", "len", "cost", "status", "iters", "nodes", "goal", "projected"}
    _assert_parity(dict(path=rows["paths"].transpose(1, 0, 2), len=rows["len"], cost=rows["cost"], status=rows["status"],
                        iters=rows["iters"], nodes=rows["nodes"].T, which=rows["goal"],
                        projected=rows["projected"].T), want, "Robot.plan_rrt_constrained")
    # its paths go into certify_paths and time_paths as they are, and both accept them: certified free (with clearances
    # of 0.092 and 0.0046 m on the device), and timed
    cert = robot.certify_paths(rows["paths"][:2], rows["len"][:2])
    print("certify_paths: status", cert["status"], "clearance", cert["clearance"])
    assert (cert["status"] == nat_certify("FREE")).all() and (cert["clearance"] > 0.0).all()
    # (slowly: a tree's path has a corner at every waypoint, and at the URDF's velocity limits the profile stops at
    # two neighbouring waypoints of the pair's path, which is status 1; at 0.5 rad/s the host reference takes every
    # corner of both paths at the velocity limit, in 9.295 s and 10.786 s)
    timed = robot.time_paths(rows["paths"][:2], rows["len"][:2], a_max=np.full(7, 5.0), v_max=np.full(7, 0.5))
    print("time_paths: status", timed["status"], "duration", timed["duration"])
    assert (timed["status"] == 0).all() and (timed["duration"] > 0.0).all()
    _install(wall, model=False)


def test_goal_sets_with_counts(torch_dev, xref, wall, upright):
    """G = 3: a goal in collision, a goal that violates the constraint, a NaN slot past the count."""
    _install(wall)
    start, goal = wall["start"], wall["goal"]
    inside, nanrow = start.copy(), np.full(7, math.nan)
    inside[0] = 0.0
    goals = np.array([[inside, _tipped(goal), goal], [_tipped(goal), goal, nanrow], [inside, _tipped(goal), nanrow]])
    starts, counts = np.tile(start, (3, 1)), np.array([3, 2, 2], dtype=np.int32)
    want = _reference(xref, wall, upright, starts, goals, counts, Lmax=64, **PLAN, **CON)
    print("goal sets: status", want["status"], "which", want["which"], "roots", want["roots"], "iters", want["iters"])
    assert want["roots"].tolist() == [1, 1, 0] and want["which"].tolist() == [2, 1, -1]
    assert want["status"].tolist() == [tu.FOUND, tu.FOUND, tu.NO_ROUTE]
    got = _device(torch_dev, wall, upright, starts, goals, counts, Lmax=64, **PLAN, **CON)
    _assert_parity(got, want, "goal sets")
    rows = wall["robot"].plan_rrt_to_goals_constrained(starts, goals, upright, counts, resolution=wall["h"],
                                                       max_waypoints=64, **PLAN, **CON)
    _assert_parity(dict(path=rows["paths"].transpose(1, 0, 2), len=rows["len"], cost=rows["cost"], status=rows["status"],
                        iters=rows["iters"], nodes=rows["nodes"].T, which=rows["goal"],
                        projected=rows["projected"].T), want, "Robot.plan_rrt_to_goals_constrained")
    _install(wall, model=False)


@pytest.mark.parametrize("iters, max_nodes", [(448, 4096), (142, 70), (256, 70)])
def test_large_trees_and_full_trees(torch_dev, xref, wall, upright, iters, max_nodes):
    """The wall pair at step 0.1 (chosen with the host build: no junction within 640 iterations, 291 and 260 nodes by
    then; with max_nodes = 70 tree 0 holds 68 nodes after 130 iterations and 70 after 140, tree 1 holds 66 after 140 and
    70 after 150).  Trees past 128 nodes put every lane of the nearest search through several trips.  After 142
    iterations one tree is full while the other still grows through the commit whose guard needs cnt_a < M, the motion
    check's flag and the constraint's ok byte; after 256 both are full and every step leaves by cnt_a >= M before it
    projects anything, which the counters show."""
    _install(wall)
    starts, goals, counts = wall["start"][None], wall["goal"][None, None, :], np.ones(1, dtype=np.int32)
    args = dict(iters=iters, step=0.1, first=xu.FIRST, max_nodes=max_nodes, Lmax=64)
    want = _reference(xref, wall, upright, starts, goals, counts, **args, **CON)
    print("step 0.1: status", want["status"], "iters", want["iters"], "nodes", want["nodes"].T, "projected",
          want["projected"].T)
    if max_nodes == 70:
        assert want["status"][0] == tu.NO_ROUTE and want["iters"][0] == iters
        nodes = sorted(want["nodes"][:, 0].tolist())
        assert nodes[1] == 70 and (nodes[0] == 70 if iters == 256 else 2 < nodes[0] < 70)
    else:
        assert want["nodes"].max() > 128
    _assert_parity(_device(torch_dev, wall, upright, starts, goals, counts, **args, **CON), want, f"M {max_nodes}")
    _install(wall, model=False)


def test_a_query_does_not_depend_on_the_batch_or_on_poll(torch_dev, wall, upright, five_want):
    _install(wall)
    starts, goals, counts = _five(wall)
    rng = np.random.default_rng(30)
    S = rng.uniform(wall["lo"], wall["hi"], (70, 7))
    Gs = rng.uniform(wall["lo"], wall["hi"], (70, 1, 7))
    S[37], Gs[37] = starts[0], goals[0]
    S[5, 2] = math.nan
    Cn = np.ones(70, dtype=np.int32)
    alone = _device(torch_dev, wall, upright, starts[:1], goals[:1], counts[:1], Lmax=64, **PLAN, **CON)
    _assert_parity(alone, {k: (v[:, :1] if v.ndim > 1 else v[:1]) for k, v in five_want.items()}, "alone")
    for poll in (1, 65536):
        got = _device(torch_dev, wall, upright, S, Gs, Cn, Lmax=64, poll=poll, **PLAN, **CON)
        _assert_parity(_rows(got, slice(37, 38)), alone, f"poll {poll}")
        if poll == 1:
            first = got
        else:
            _assert_parity(got, first, "poll 65536 against poll 1")
    assert got["status"][5] == tu.QUERY_NAN
    _install(wall, model=False)


def test_free_box_is_rrt_plan_goals_bit_for_bit(torch_dev, wall):
    torch, hc = torch_dev, wall["hc"]
    _install(wall)
    start, goal = wall["start"], wall["goal"]
    inside, near, nan_goal = start.copy(), start.copy(), goal.copy()
    inside[0], nan_goal[3] = 0.0, math.nan
    near[0] -= 0.2
    goal2 = goal + np.array([0.2, 0.1, 0, 0.2, 0, 0, 0])
    goals = np.array([[inside, goal, goal2], [goal2, goal, inside], [inside, near, goal], [inside, inside, inside],
                      [goal, nan_goal, near], [start, start, start]])
    starts = np.tile(start, (6, 1))
    starts[5] = goal                                                     # (the pair reversed)
    counts = np.array([3, 3, 3, 3, 3, 1], dtype=np.int32)
    args = dict(iters=tu.WALL_ITERS, step=tu.WALL_STEP, first=tu.WALL_FIRST, max_nodes=tu.WALL_NODES)
    free = cu.free_constraint(cu.pose7_of(np.array(wall["robot"].fk(start)).reshape(4, 4)))
    got = _device(torch, wall, free, starts, goals, counts, Lmax=64, tol=0.0, ptol=0.0, piters=0, damping=0.0,
                  max_step=0.5, **args)
    s = torch.from_numpy(np.ascontiguousarray(starts.T)).cuda()
    g = torch.from_numpy(np.ascontiguousarray(goals.transpose(1, 2, 0))).cuda()
    cn = torch.from_numpy(counts).cuda()
    want = {k: v.cpu().numpy() for k, v in hc.rrt_plan_goals(s, g, cn, resolution=wall["h"], Lmax=64, **args).items()}
    assert want["status"].tolist() == [tu.FOUND, tu.FOUND, tu.FOUND, tu.NO_ROUTE, tu.QUERY_NAN, tu.FOUND]
    assert want["len"][0] > 2 and want["len"][5] > 2
    for key in want:
        assert np.array_equal(got[key].view(np.uint8), want[key].view(np.uint8)), key
    # every projection asked for ended PROJECTED, and none where the iterations never began
    assert np.array_equal(got["projected"][0], got["projected"][1])
    assert ((got["projected"][0] > 0) == (want["iters"] > 0)).all()
    # the tensor entry point is the same call
    dev = hc.rrt_plan_constrained(s, g, cn, free, 0.0, resolution=wall["h"], Lmax=64, ptol=0.0, piters=0, damping=0.0,
                                  **args)
    assert set(dev) == set(KEYS)
    for key in KEYS:
        assert np.array_equal(dev[key].cpu().numpy().view(np.uint8), got[key].view(np.uint8)), key
    _install(wall, model=False)


@pytest.mark.parametrize("ee", [False, True])
@pytest.mark.parametrize("name, start, goal, box, tilt, found", [
    ("ur10", [-0.9, -1.0, 1.2, 0, 0, 0], [0.9, -1.0, 1.2, 0, 0, 0], [0.869, 0.256, 0.415, 0, 0, 0, 1, 0.05, 0.05, 0.3],
     1.0, (3, 1, [2, 1], [2, 2])),
    ("arm10", [-0.9] + [0.3] * 9, [0.9] + [0.3] * 9, [0.058, -0.15, -0.599, 0, 0, 0, 1, 0.05, 0.05, 0.3], 2.6,
     (4, 8, [5, 2], [16, 16]))])
def test_other_chains(torch_dev, xref, name, start, goal, box, tilt, found, ee):
    """A 6-joint chain and a chain of the general kernels (10 joints, WideChainDev), the scenes of test_gpu_rrt.py,
    under upright(fk(start), tilt), with and without an ee_offset (a translation: the orientation is the flange's).
    The tilt is one the scene's goal keeps (chosen on the CPU with the host header: the 10-joint arm's first axis is
    not vertical and its goal is 1.78 rad from the start's orientation on the two bounded axes).  The scenes' ends lie
    outside the 10-joint arm's limits in joint 1, as in test_gpu_rrt.py: roots are taken as they are, only projected
    candidates are clamped.  Every case finds a path, so the commit of a found query and the walk run on both chain
    types: `found` is (waypoints, iterations, nodes, projections) of the reference fed with the device's verdicts, the
    same with and without the offset."""
    sc = _scene(name, [box])
    _install(sc)
    robot = sc["robot"]
    ee7 = np.array([0.05, 0.0, 0.1, 0.0, 0.0, 0.0, 1.0]) if ee else None
    ee44 = None
    if ee:
        ee44 = np.eye(4)
        ee44[:3, 3] = ee7[:3]
    s = np.array(start, dtype=np.float64)[None]
    c = _upright(robot, s[0], tilt, ee44)
    g = np.array(goal, dtype=np.float64)[None, None, :]
    assert robot.constraint_batch_arrays(g[0], c, ee44)[1][0] == 0.0
    args = dict(iters=64, step=0.3, first=1, max_nodes=64, Lmax=64)
    con = dict(CON, tol=0.1)
    counts = np.ones(1, dtype=np.int32)
    want = _reference(xref, sc, c, s, g, counts, ee=ee44, **args, **con)
    print(name, ee, "status", want["status"], "len", want["len"], "iters", want["iters"], "nodes", want["nodes"].T,
          "projected", want["projected"].T)
    assert want["roots"][0] == 1
    assert want["status"][0] == tu.FOUND
    assert (want["len"][0], want["iters"][0], want["nodes"][:, 0].tolist(), want["projected"][:, 0].tolist()) == found
    _assert_parity(_device(torch_dev, sc, c, s, g, counts, ee7=ee7, **args, **con), want, name)
    _install(sc, model=False)


def test_sixteen_joints(torch_dev, xref):
    """The WideChainDev table at its largest, staged in LDS by the constrained step: test_gpu_rrt.py's 16-joint scene
    under upright(fk(start), 2.0), which the goal keeps (violation 0 on the host).  Whether the trees join is left open;
    the iterations begin, so at least one candidate is projected."""
    from test_gpu_rrt import ARM16
    sc = _scene("arm16", [ARM16["box"]])
    _install(sc)
    s = np.array(ARM16["start"], dtype=np.float64)[None]
    g = np.array(ARM16["goal"], dtype=np.float64)[None, None, :]
    c = _upright(sc["robot"], s[0], 2.0)
    args, con, counts = dict(iters=32, step=0.3, first=1, max_nodes=64, Lmax=64), dict(CON, tol=0.1), np.ones(1, dtype=np.int32)
    want = _reference(xref, sc, c, s, g, counts, **args, **con)
    print("arm16: status", want["status"], "len", want["len"], "iters", want["iters"], "nodes", want["nodes"].T,
          "projected", want["projected"].T)
    assert want["projected"][0, 0] >= 1
    _assert_parity(_device(torch_dev, sc, c, s, g, counts, **args, **con), want, "arm16")
    _install(sc, model=False)


def test_two_chunks(torch_dev, wall, upright):
    from optik_amd import _native as nat
    _install(wall)
    chunk = nat.rrt_chunk(wall["hc"]._h, 4096)
    assert 500 < chunk < 586
    Q, real = 586, chunk + 7
    start, goal = wall["start"], wall["goal"]
    S, Gs = np.tile(_tipped(start), (Q, 1)), np.tile(goal, (Q, 1, 1))    # starts that violate: these end before iteration 0
    S[real], S[3] = start, start                                         # the pair in the second chunk and in the first
    Cn = np.ones(Q, dtype=np.int32)
    args = dict(iters=8, step=xu.STEP, first=xu.FIRST, max_nodes=4096, Lmax=64)
    got = _device(torch_dev, wall, upright, S, Gs, Cn, **args, **CON)
    one = _device(torch_dev, wall, upright, S[real:real + 1], Gs[real:real + 1], Cn[:1], **args, **CON)
    _assert_parity(_rows(got, slice(real, real + 1)), one, "the row of the second chunk")
    _assert_parity(_rows(got, slice(3, 4)), one, "the row of the first chunk")
    # (8 iterations do not join the trees: they grow, and the counters count)
    assert one["status"][0] == tu.NO_ROUTE and one["iters"][0] == 8 and one["projected"][0, 0] >= 8
    assert (one["nodes"][:, 0] > 1).all()
    rest = np.ones(Q, dtype=bool)
    rest[[3, real]] = False
    assert (got["status"][rest] == tu.NO_ROUTE).all() and (got["iters"][rest] == 0).all()
    assert (got["nodes"][:, rest] == 0).all() and (got["projected"][:, rest] == 0).all()
    _install(wall, model=False)


def test_refusals(torch_dev, wall, upright, chains):
    from optik_amd import PoseConstraint
    from optik_amd import _native as nat
    from optik_amd import device
    from optik_amd.device import _dp, _ptr
    torch = torch_dev
    lib, hc, robot = nat.lib(), wall["hc"], wall["robot"]
    s = torch.zeros((7, 3), dtype=torch.float64, device="cuda")
    g = torch.zeros((16, 7, 3), dtype=torch.float64, device="cuda")
    cn = torch.ones(3, dtype=torch.int32, device="cuda")
    path, proj = _out((4, 3, 7), torch.float64), _out((2, 3), torch.int32)
    ref7, lo6, hi6 = upright.ref7.copy(), upright.lo.copy(), upright.hi.copy()

    def plan(h=hc, Q=3, G=2, iters=8, step=0.3, res=0.1, max_nodes=16, Lmax=4, poll=4, ref=ref7, lo=lo6, hi=hi6,
             tol=0.05, ptol=1e-6, piters=16, damping=1e-6, max_step=0.5):
        ref, lo, hi = (np.ascontiguousarray(v, dtype=np.float64) if v is not None else None for v in (ref, lo, hi))
        return lib.optik_hip_rrt_plan_constrained(
            h._h, None, _dp(ref) if ref is not None else None, _dp(lo) if lo is not None else None,
            _dp(hi) if hi is not None else None, tol, ptol, piters, damping, max_step, _ptr(s), _ptr(g), _ptr(cn), Q, G,
            iters, step, res, 0, max_nodes, Lmax, poll, _ptr(path), None, None, None, None, None, None, _ptr(proj), None)
    nanref, unnorm, crossed = ref7.copy(), ref7.copy(), lo6.copy()
    nanref[0], crossed[3] = math.nan, 1.0
    unnorm[3:] *= 1.1
    bad = (dict(G=0), dict(G=17), dict(G=3, max_nodes=2), dict(Q=-1), dict(iters=0), dict(iters=65537), dict(step=0.0),
           dict(step=math.nan), dict(max_nodes=4097), dict(Lmax=1), dict(Lmax=65), dict(poll=0), dict(poll=65537),
           dict(res=0.0), dict(res=math.inf),
           dict(ref=None), dict(lo=None), dict(hi=None), dict(ref=nanref), dict(ref=unnorm), dict(lo=crossed),
           dict(tol=-1.0), dict(tol=math.nan), dict(tol=math.inf), dict(ptol=-1e-9), dict(ptol=math.nan),
           dict(ptol=math.inf), dict(piters=-1), dict(piters=4097), dict(damping=-1.0), dict(damping=math.nan),
           dict(max_step=0.0), dict(max_step=math.inf))
    for kw in bad:
        assert plan(**kw) == -1, kw                                           # OPTIK_HIP_EINVAL
        if "Q" not in kw:
            assert plan(Q=0, **kw) == -1, kw                                  # (before any device work, also at Q = 0)
    torch.cuda.synchronize()
    assert _sentinels_left(path.cpu().numpy()) == path.numel() and _sentinels_left(proj.cpu().numpy()) == 6
    assert plan(Q=0) == 0 and plan(piters=0, Q=0) == 0 and plan(piters=4096, ptol=0.0, tol=0.0, damping=0.0, Q=0) == 0
    gantry = device.HipChain(**chains["gantry"][0])
    assert plan(h=gantry) == -2 and plan(h=gantry, Q=0) == -2                 # OPTIK_HIP_EUNSUPPORTED
    assert _sentinels_left(path.cpu().numpy()) == path.numel()
    assert plan() == 0
    torch.cuda.synchronize()
    assert _sentinels_left(path.cpu().numpy()) == 0 and _sentinels_left(proj.cpu().numpy()) == 0
    x, gs = np.zeros((3, 7)), np.zeros((3, 2, 7))
    with pytest.raises(TypeError):
        robot.plan_rrt_to_goals_constrained(x, gs, upright)                   # tol has no default
    with pytest.raises(TypeError):
        robot.plan_rrt_constrained(x, x, upright)
    for kw in (dict(iters=0), dict(step=0.0), dict(max_nodes=1), dict(max_waypoints=65), dict(poll=0),
               dict(resolution=0.0), dict(tol=-1.0), dict(tol=math.nan), dict(ptol=-1.0), dict(piters=-1),
               dict(piters=4097), dict(damping=-1.0), dict(max_step=0.0)):
        with pytest.raises(ValueError):
            robot.plan_rrt_to_goals_constrained(x, gs, upright, **dict(dict(tol=0.05), **kw))
    for goals, kw in ((gs[:2], {}), (np.zeros((3, 17, 7)), {}), (np.zeros((3, 2, 6)), {}),
                      (np.zeros((3, 3, 7)), dict(max_nodes=2)), (gs, dict(counts=np.zeros(2, dtype=np.int32)))):
        with pytest.raises(ValueError):
            robot.plan_rrt_to_goals_constrained(x, goals, upright, tol=0.05, **kw)
    with pytest.raises(ValueError):
        PoseConstraint.upright(np.eye(4), -1.0)
    with pytest.raises(ValueError):
        hc.rrt_plan_constrained(s, g[:, :, :2].contiguous(), cn, upright, 0.05, 8, 0.3, 0.1)
    empty = robot.plan_rrt_constrained(np.zeros((0, 7)), np.zeros((0, 7)), upright, tol=0.05)
    assert empty["paths"].shape == (0, 64, 7) and empty["projected"].shape == (0, 2)
