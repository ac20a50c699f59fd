"""-m gpu: pose constraints on the device (optik_amd/csrc/ik_constraint.hip) against the host build of
constraint_measure.hpp, bit for bit in every output; the constrained roadmap against its CPU restatement; invariants
with a wall in the world; the refusals; the Robot layer against the HipChain layer."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import constraint_util as cu
import roadmap_lazy_util as lu
import roadmap_util as ru
from conftest import ROBOT_SPECS
from constraint_util import FAILED, PROJECTED, PROJECT_DEFAULTS

pytestmark = pytest.mark.gpu
ROBOT_NAMES = ("panda", "ur10", "arm10")
EE7 = np.array([0.02, -0.01, 0.1, 0.0, math.sin(0.2), 0.0, math.cos(0.2)])
EE16 = np.array([[math.cos(0.4), 0, math.sin(0.4), 0.02], [0, 1, 0, -0.01], [-math.sin(0.4), 0, math.cos(0.4), 0.1],
                 [0, 0, 0, 1.0]])
H, TOL = 0.1, 1e-6


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return cu.build_constraint(str(tmp_path_factory.mktemp("constraint_measure")))


@pytest.fixture(scope="module")
def roadmap_ref(tmp_path_factory):
    return ru.build_roadmap_ref(str(tmp_path_factory.mktemp("constraint_roadmap")))


@pytest.fixture(scope="module")
def robots():
    from optik_amd import Robot
    made = {}

    def get(name):
        if name not in made:
            made[name] = Robot.from_urdf_file(*ROBOT_SPECS[name])
        return made[name]
    return get


def _t(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all((cu.bits(got) == cu.bits(want)) | (np.isnan(got) & np.isnan(want))))


def _ref7(robot, x, ee16=None):
    return cu.pose7_of(np.asarray(robot.fk(list(x), ee16.tolist() if ee16 is not None else None)))


def _rows(robot, B, seed):
    lb, ub = (np.asarray(v) for v in robot.joint_limits())
    rng = np.random.default_rng(seed)
    x = rng.uniform(np.maximum(lb, -3.0), np.minimum(ub, 3.0), (B, len(lb)))
    if B >= 64:
        x[5, 0] = math.nan
        x[B - 1, len(lb) - 1] = math.nan
        x[17, 1] = math.inf
    return x


def _constraints(ref7):
    at = np.array([0.05, -0.1, 0.02, 0.1, -0.05, 0.2])
    return dict(free=cu.free_constraint(ref7), pinned=cu.pinned_constraint(ref7, at),
                upright=cu.upright_constraint(ref7, 0.1))


def _check_ops(torch, ref, hc, tables, c, x, ee7, what):
    q = _t(torch, x.T)
    r, v = hc.constraint_batch(q, c, ee_offset7=ee7)
    want = ref.measure(tables, c, x, ee7)
    assert _same(r.cpu().numpy().T, want["r"]) and _same(v.cpu().numpy(), want["v"]), what
    iters = 24  # (every loop length up to the budget occurs in a wave; the default budget is the same code)
    p = hc.constraint_project_batch(q, c, TOL, iters, PROJECT_DEFAULTS["damping"], PROJECT_DEFAULTS["max_step"],
                                    ee_offset7=ee7)
    wp = ref.project(tables, c, x, TOL, iters, PROJECT_DEFAULTS["damping"], PROJECT_DEFAULTS["max_step"], ee7)
    assert _same(p["x"].cpu().numpy().T, wp["x"]) and _same(p["violation"].cpu().numpy(), wp["v"]), what
    assert np.array_equal(p["status"].cpu().numpy(), wp["status"]), what
    assert np.array_equal(p["iterations"].cpu().numpy(), wp["iterations"]), what
    xb = np.roll(x, 1, axis=0) * 0.25 + x * 0.75
    got = hc.constraint_motion_batch(q, _t(torch, xb.T), H, c, 0.05, ee_offset7=ee7)
    wm = ref.motion(tables, c, x, xb, H, 0.05, ee7)
    assert _same(got[0].cpu().numpy(), wm["v"]), what
    for g, key in zip(got[1:], ("ok", "first", "steps")):
        assert np.array_equal(g.cpu().numpy(), wm[key]), (what, key)
    return wp, wm


@pytest.mark.parametrize("name", ROBOT_NAMES)
def test_operators_equal_the_host_header_bit_for_bit(torch_dev, ref, robots, name):
    robot = robots(name)
    hc, tables = robot.hip_chain(), robot.chain_tables()
    seen = set()
    for ee7 in (None, EE7):
        ref7 = _ref7(robot, _rows(robot, 1, 99)[0])
        for cname, c in _constraints(ref7).items():
            for B in (1, 64, 65, 257):
                wp, wm = _check_ops(torch_dev, ref, hc, tables, c, _rows(robot, B, B), ee7, (name, cname, B, ee7 is None))
                seen |= {(cname, int(s)) for s in wp["status"]}
                if B == 257:
                    assert (wm["steps"] == -1).sum() >= 3 and (wm["steps"] > 1).any()
                    seen |= {("motion ok", bool(o)) for o in wm["ok"]}
    # every status occurred, and the free constraint projects every finite row at once
    assert {("upright", PROJECTED), ("upright", FAILED), ("pinned", 1), ("free", PROJECTED)} <= seen
    assert ("free", 1) not in seen and {("motion ok", True), ("motion ok", False)} <= seen


def test_capped_grid_gives_the_same_bits(torch_dev, ref, robots):
    from optik_amd import _native as nat
    robot = robots("panda")
    hc, tables = robot.hip_chain(), robot.chain_tables()
    c = cu.upright_constraint(_ref7(robot, cu.PANDA_HOME), 0.1)
    with nat.options(grid_cap=2):
        assert nat.get_option("grid_cap") == 2
        _check_ops(torch_dev, ref, hc, tables, c, _rows(robot, 600, 6), None, "grid_cap 2")


def test_rows_of_a_wave_do_not_disturb_each_other(torch_dev, ref, robots):
    """Iteration counts differ within a wave: rows that already satisfy the constraint (0 iterations) and rows that
    never project (the whole budget; a pin that the arm cannot reach) alternate with ordinary rows, and every row has
    the result it has on its own."""
    torch = torch_dev
    robot = robots("panda")
    hc, tables = robot.hip_chain(), robot.chain_tables()
    ref7 = _ref7(robot, cu.PANDA_HOME)
    c = cu.upright_constraint(ref7, 0.1)
    x = _rows(robot, 64, 21)
    x[~np.isfinite(x)] = 0.0
    done = ref.project(tables, c, x, TOL, **PROJECT_DEFAULTS)
    sat = done["x"][done["status"] == PROJECTED]
    assert len(sat) >= 16
    mixed = x.copy()
    mixed[0::4] = sat[:16]
    p = hc.constraint_project_batch(_t(torch, mixed.T), c, TOL, **PROJECT_DEFAULTS)
    want = ref.project(tables, c, mixed, TOL, **PROJECT_DEFAULTS)
    its = p["iterations"].cpu().numpy()
    assert _same(p["x"].cpu().numpy().T, want["x"]) and np.array_equal(its, want["iterations"])
    assert not its[0::4].any() and _same(p["x"].cpu().numpy().T[0::4], sat[:16]) and its.max() > 4
    alone = np.array([ref.project(tables, c, mixed[b:b + 1], TOL, **PROJECT_DEFAULTS)["x"][0] for b in (1, 2, 3, 5)])
    assert _same(p["x"].cpu().numpy().T[[1, 2, 3, 5]], alone)
    # rows that never project: the end effector pinned two metres above anything the arm reaches
    far = ref7.copy()
    far[2] += 2.0
    cf = cu.pinned_constraint(far)
    mixed[1::4] = x[1::4]
    pf = hc.constraint_project_batch(_t(torch, mixed.T), cf, TOL, 16, 1e-6, 0.5)
    wf = ref.project(tables, cf, mixed, TOL, 16, 1e-6, 0.5)
    assert (wf["status"] == 1).all() and (wf["iterations"] == 16).all()
    assert _same(pf["x"].cpu().numpy().T, wf["x"]) and _same(pf["violation"].cpu().numpy(), wf["v"])


def _oracle_home7(robot):
    from oracle import binding
    binding.build()
    return np.asarray(binding.fk(binding.make_chain(**robot.chain_tables()), np.array(cu.PANDA_HOME))[1])


def test_constrained_roadmap_equals_the_cpu_plan(torch_dev, ref, roadmap_ref, robots):
    torch = torch_dev
    robot = robots("panda")
    hc, tables = robot.hip_chain(), robot.chain_tables()
    scene = cu.plan_scene(ref, tables, _oracle_home7(robot))
    graph, w0, queries, want = cu.cpu_plan(ref, roadmap_ref, tables, scene)
    nodes = _t(torch, scene["nodes"])
    nbr, w = hc.roadmap_build_constrained(nodes, cu.PLAN_K, cu.PLAN_H, scene["c"], cu.PLAN_TOL)
    assert np.array_equal(nbr.cpu().numpy(), graph["nbr"]) and _same(w.cpu().numpy(), graph["w"])
    got = hc.roadmap_plan_constrained((nodes, nbr, w), _t(torch, scene["starts"]), _t(torch, scene["goals"]),
                                      cu.PLAN_KS, cu.PLAN_LMAX, cu.PLAN_H, scene["c"], cu.PLAN_TOL)
    assert (want["status"] == ru.FOUND).any()
    for key in ("status", "len", "cost", "path"):
        assert _same(got[key].cpu().numpy(), want[key]), key


def test_with_a_wall_every_segment_passes_both_checks(torch_dev, robots):
    from optik_amd import PoseConstraint
    torch = torch_dev
    sc = ru.wall_scene()
    robot = robots("panda")
    starts, goals = lu.wall_pairs(sc)
    robot.set_collision_model(sc["frames"], sc["centers"], sc["radii"], self_pairs=None)
    robot.set_world(boxes=sc["boxes"])
    try:
        c = PoseConstraint.upright(np.asarray(robot.fk(list(sc["start"]))), 0.6)
        tol = 0.05
        rm = robot.build_constrained_roadmap(c, tol, 256, 8, sc["h"], first=sc["first"])
        assert rm.N == 256 and rm.k == 8 and 128 <= rm.projected <= 256 and rm.constraint is c
        assert int(torch.isnan(rm.nodes).any(dim=0).sum()) == 256 - rm.projected
        # starts and goals: the wall pairs projected, and one start that violates the constraint
        p = robot.constraint_project_batch_arrays(np.concatenate([starts, goals]), c, 1e-6)
        assert (p["status"] == PROJECTED).all()
        s, g = p["x"][:2], p["x"][2:]
        bad = s[0].copy()
        bad[5] -= 1.5
        assert robot.constraint_batch_arrays(bad[None], c)[1][0] > tol
        s, g = np.concatenate([s, bad[None]]), np.concatenate([g, g[:1]])
        res = robot.plan_constrained_paths(rm, s, g, 48)
        assert res["status"][2] == ru.NO_ROUTE and res["paths"].shape == (3, 48, 7)
        for j in np.nonzero(res["status"] == ru.FOUND)[0]:
            path = res["paths"][j, :res["len"][j]]
            assert robot.collision_motion_batch_arrays(path[:-1], path[1:], sc["h"])[1].all()
            assert robot.constraint_motion_batch_arrays(path[:-1], path[1:], sc["h"], c, tol)[1].all()
        chk = robot.check_paths_constraint(res["paths"], res["len"], c, tol, sc["h"])
        found = res["status"] == ru.FOUND
        assert chk["ok"][found].all() and (chk["segment"][found] == -1).all() and not chk["ok"][2]
        assert chk["segment"][2] == 0
    finally:
        robot.clear_collision_model()
        robot.set_world()


def test_refusals(torch_dev, robots):
    from optik_amd import PoseConstraint, Robot
    from optik_amd import _native as nat
    torch = torch_dev
    robot = robots("panda")
    hc = robot.hip_chain()
    q = torch.zeros((7, 2), dtype=torch.float64, device="cuda")
    ident = [0.0, 0, 0, 0, 0, 0, 1]
    inf6 = [math.inf] * 6

    def raw(ref7=ident, lo=[-v for v in inf6], hi=inf6):
        return types.SimpleNamespace(ref7=ref7, lo=lo, hi=hi)
    bad = [raw(lo=[0, 0, 0, 0.2, 0, 0], hi=[0, 0, 0, 0.1, 0, 0]), raw(lo=[math.nan] + [0.0] * 5, hi=[0.0] * 6),
           raw(ref7=[math.nan, 0, 0, 0, 0, 0, 1]), raw(ref7=[0, 0, 0, 0, 0, 0, 1.001]), raw(ref7=[0, 0, math.inf, 0, 0, 0, 1])]
    for c in bad:
        for call in (lambda: hc.constraint_batch(q, c), lambda: hc.constraint_project_batch(q, c),
                     lambda: hc.constraint_motion_batch(q, q, 0.1, c)):
            with pytest.raises(nat.OptikHipError, match="pose constraint"):
                call()
        with pytest.raises(RuntimeError, match="pose constraint"):
            robot.constraint_batch_arrays(np.zeros((2, 7)), c)
    with pytest.raises(ValueError):
        PoseConstraint(np.eye(4), [0.0] * 3 + [0.2, 0, 0], [0.0] * 3 + [0.1, 0, 0])
    with pytest.raises(ValueError):
        PoseConstraint(np.eye(4), [math.nan] * 6, [0.0] * 6)
    with pytest.raises(ValueError):
        PoseConstraint(np.diag([1.0, 1.0, 1.001, 1.0]), [0.0] * 6, [0.0] * 6)
    ok = raw()
    for tol in (-1e-9, math.nan, math.inf):
        with pytest.raises(ValueError, match="tol"):
            hc.constraint_project_batch(q, ok, tol)
        with pytest.raises(ValueError, match="tol"):
            hc.constraint_motion_batch(q, q, 0.1, ok, tol)
    # the C layer itself, past the Python checks
    L, dp = nat.lib(), lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    r7, lo, hi = dp(ident), dp([-v for v in inf6]), dp(inf6)
    assert L.optik_hip_constraint_project_batch(hc._h, None, r7, lo, hi, None, 0, -1.0, 8, 1e-6, 0.5, None, None, None,
                                                None, None) == -1 and b"tol" in L.optik_hip_last_error()
    assert L.optik_hip_constraint_motion_batch(hc._h, None, r7, lo, hi, None, None, 0, 0.1, -1.0, None, None, None,
                                               None, None) == -1
    assert L.optik_hip_constraint_motion_batch(hc._h, None, r7, lo, hi, None, None, 0, 0.0, 0.0, None, None, None,
                                               None, None) == -1 and b"resolution" in L.optik_hip_last_error()
    assert L.optik_hip_constraint_project_batch(hc._h, None, r7, lo, hi, None, 0, 0.0, 5000, 1e-6, 0.5, None, None,
                                                None, None, None) == -1
    assert L.optik_hip_constraint_batch(hc._h, None, r7, lo, hi, None, 0, None, None, None) == 0
    # a prismatic chain: the motion check's message, also with B = 0
    gantry = Robot.from_urdf_file(*ROBOT_SPECS["gantry"])
    n = gantry.num_positions()
    with pytest.raises(RuntimeError, match="prismatic joints are not supported"):
        gantry.collision_motion_batch_arrays(np.zeros((1, n)), np.zeros((1, n)), 0.1)
    for call in (lambda: gantry.constraint_batch_arrays(np.zeros((1, n)), ok),
                 lambda: gantry.constraint_project_batch_arrays(np.zeros((1, n)), ok),
                 lambda: gantry.constraint_motion_batch_arrays(np.zeros((1, n)), np.zeros((1, n)), 0.1, ok)):
        with pytest.raises(RuntimeError, match="prismatic joints are not supported"):
            call()
    gq = torch.zeros((n, 1), dtype=torch.float64, device="cuda")
    with pytest.raises(nat.OptikHipError, match="prismatic joints are not supported"):
        gantry.hip_chain().constraint_batch(gq, ok)


@pytest.mark.parametrize("name", ("panda", "arm10"))
def test_robot_layer_equals_the_chain_layer(torch_dev, robots, name):
    from optik_amd import PoseConstraint
    torch = torch_dev
    robot = robots(name)
    hc = robot.hip_chain()
    x = _rows(robot, 300, 31)
    xb = np.roll(x, 1, axis=0) * 0.25 + x * 0.75
    ee7 = cu.pose7_of(EE16)
    c = PoseConstraint.upright(np.asarray(robot.fk(list(_rows(robot, 1, 98)[0]), EE16.tolist())), 0.1)
    q, qb = _t(torch, x.T), _t(torch, xb.T)
    r, v = robot.constraint_batch_arrays(x, c, EE16)
    dr, dv = hc.constraint_batch(q, c, ee_offset7=ee7)
    # (the Robot layer converts the offset matrix itself; the residuals agree to rounding, and bit for bit without it)
    assert np.allclose(r, dr.cpu().numpy().T, rtol=0, atol=1e-12, equal_nan=True)
    r, v = robot.constraint_batch_arrays(x, c)
    dr, dv = hc.constraint_batch(q, c)
    assert _same(r, dr.cpu().numpy().T) and _same(v, dv.cpu().numpy())
    p = robot.constraint_project_batch_arrays(x, c, TOL, 16)
    dp_ = hc.constraint_project_batch(q, c, TOL, 16)
    assert _same(p["x"], dp_["x"].cpu().numpy().T) and _same(p["violation"], dp_["violation"].cpu().numpy())
    assert np.array_equal(p["status"], dp_["status"].cpu().numpy())
    assert np.array_equal(p["iterations"], dp_["iterations"].cpu().numpy())
    m = robot.constraint_motion_batch_arrays(x, xb, H, c, 0.05)
    dm = hc.constraint_motion_batch(q, qb, H, c, 0.05)
    assert _same(m[0], dm[0].cpu().numpy())
    for a, b in zip(m[1:], dm[1:]):
        assert np.array_equal(a, b.cpu().numpy())
