"""-m gpu: IK into pose regions on the device (optik_amd/csrc/ik_region.hip) against the host build of
region_measure.hpp and against the library's own pieces composed (seed_batch, constraint_project_batch,
solutions_from_keys, collision_batch, constraint_batch), bit for bit; the properties of the returned rows; the planners
that take a region as their goal; the refusals of the three layers; the Robot layer against the HipChain layer."""
import ctypes as C
import math

import numpy as np
import pytest

import constraint_util as cu
import region_util as gu
from conftest import ROBOT_SPECS
from constraint_util import FAILED, PROJECTED
from gpu_util import _out, _sentinels_left
from selection_util import NONE, solutions_ref

pytestmark = pytest.mark.gpu
BEGINS = (0, 5)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return gu.build_region(str(tmp_path_factory.mktemp("region_measure")))


def _t(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all((cu.bits(got) == cu.bits(want)) | (np.isnan(got) & np.isnan(want))))


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


@pytest.fixture(scope="module")
def scenes(ref):
    """name -> the robot, its chain, the three regions around fk(mid), their starts, and the host header's rows for
    both restart ranges and both key modes: computed once, left unchanged."""
    from optik_amd import Robot
    made = {}

    def get(name):
        if name not in made:
            robot = Robot.from_urdf_file(*ROBOT_SPECS[name])
            tables = robot.chain_tables()
            ref7 = cu.pose7_of(np.asarray(robot.fk(list(gu.mid_config(tables)))).reshape(4, 4))
            regs, x0 = gu.make_regions(ref7), gu.x0_rows(tables)
            rows = np.array([gu.region_row(c) for c in regs])
            host = {(b, m): ref.restarts(tables, rows, x0, b, gu.R, gu.TOL, mode=m, **gu.PROJECT)
                    for b in BEGINS for m in (gu.MODE_QUALITY, gu.MODE_SPEED)}
            made[name] = dict(robot=robot, hc=robot.hip_chain(), tables=tables, regs=regs, rows=rows, x0=x0, host=host)
        return made[name]
    return get


def _run(torch, sc, begin, mode="quality", k=gu.K, R=gu.R, rows=None, x0=None, hc=None, **kw):
    hc = hc or sc["hc"]
    return _np(hc.ik_region(_t(torch, sc["rows"] if rows is None else rows), _t(torch, sc["x0"] if x0 is None else x0),
                            begin, begin + R, k, gu.MIN_DIST, tol=gu.TOL, mode=mode, per_restart=True,
                            **dict(gu.PROJECT, **kw)))


def _check_selection(got, begin, k, R, T):
    """The per-region outputs against selection_util's greedy pick over the per-restart arrays just returned."""
    n = got["restart_x"].shape[0]
    for t in range(T):
        sl = slice(t * R, (t + 1) * R)
        want = solutions_ref(got["restart_key"][sl], got["restart_x"][:, sl], begin, k, gu.MIN_DIST)
        assert got["count"][t] == len(want), t
        for j, (idx, key, col) in enumerate(want):
            assert got["idx"][t, j] == idx and _same(got["key"][t, j], key), (t, j)
            assert _same(got["x"][t, j], got["restart_x"][:, t * R + col]), (t, j)
            assert _same(got["violation"][t, j], got["restart_violation"][t * R + col]), (t, j)
        pad = slice(len(want), k)
        assert np.isnan(got["x"][t, pad]).all() and np.isnan(got["violation"][t, pad]).all(), t
        assert (got["idx"][t, pad].view(np.uint64) == NONE).all() and np.isposinf(got["key"][t, pad]).all(), t
    assert got["x"].shape == (T, k, n)


@pytest.mark.parametrize("name", gu.ROBOTS)
@pytest.mark.parametrize("begin", BEGINS)
def test_per_restart_arrays_equal_the_host_header_and_the_composed_calls(torch_dev, scenes, name, begin):
    torch, sc = torch_dev, scenes(name)
    hc = sc["hc"]
    for mode, m in (("quality", gu.MODE_QUALITY), ("speed", gu.MODE_SPEED)):
        want = sc["host"][(begin, m)]
        # the precondition on the inputs, on the reference alone
        for t in range(gu.T):
            sl = slice(t * gu.R, (t + 1) * gu.R)
            assert int((want["status"][sl] == PROJECTED).sum()) >= 4, (name, t)
            assert len(solutions_ref(want["key"][sl], want["x"][sl].T, begin, gu.K, gu.MIN_DIST)) >= 2, (name, t)
        got = _run(torch, sc, begin, mode)
        assert _same(got["restart_x"].T, want["x"]) and _same(got["restart_violation"], want["v"]), (name, mode)
        assert np.array_equal(got["restart_status"], want["status"]), (name, mode)
        assert np.array_equal(got["restart_iterations"], want["iterations"]), (name, mode)
        assert _same(got["restart_key"], want["key"]), (name, mode)
        _check_selection(got, begin, gu.K, gu.R, gu.T)
    # the library's own pieces composed: x0 | seed_batch rows through constraint_project_batch, region_util's keys
    seeds = hc.seed_batch(begin, gu.R).cpu().numpy().T
    for t, c in enumerate(sc["regs"]):
        starts = seeds.copy()
        if begin == 0:
            starts[0] = sc["x0"][t]
        p = _np(hc.constraint_project_batch(_t(torch, starts.T), c, gu.TOL, **gu.PROJECT))
        sl = slice(t * gu.R, (t + 1) * gu.R)
        assert _same(got["restart_x"][:, sl], p["x"]) and _same(got["restart_violation"][sl], p["violation"]), (name, t)
        assert np.array_equal(got["restart_status"][sl], p["status"]), (name, t)
        keys = gu.np_keys(p["x"].T, np.tile(sc["x0"][t], (gu.R, 1)), p["status"], np.arange(begin, begin + gu.R),
                          gu.MODE_SPEED)
        assert _same(got["restart_key"][sl], keys), (name, t)


def test_selection_equals_solutions_from_keys_and_the_multi_tile_form(torch_dev, scenes):
    from optik_amd import _native as nat
    torch, sc = torch_dev, scenes("panda")
    hc = sc["hc"]

    def hook(got, begin, R, T, k):
        key = _t(torch, got["restart_key"]).clone()
        x, v = _t(torch, got["restart_x"]), _t(torch, got["restart_violation"])
        o = nat.IkSolutionsOutputs()
        bufs = dict(count=_out((T,), torch.int32), x=_out((T, k, hc.n), torch.float64),
                    f=_out((T, k), torch.float64), idx=_out((T, k), torch.int64), key=_out((T, k), torch.float64))
        o.d_count, o.d_x, o.d_f = bufs["count"].data_ptr(), bufs["x"].data_ptr(), bufs["f"].data_ptr()
        o.d_idx, o.d_key = bufs["idx"].data_ptr(), bufs["key"].data_ptr()
        nat.check(nat.lib().optik_hip_solutions_from_keys(hc._h, key.data_ptr(), x.data_ptr(), v.data_ptr(), T, begin, R,
                                                          k, gu.MIN_DIST, C.byref(o), None))
        torch.cuda.synchronize()
        w = _np(bufs)
        assert np.array_equal(got["count"], w["count"]) and np.array_equal(got["idx"], w["idx"])
        assert _same(got["x"], w["x"]) and _same(got["violation"], w["f"]) and _same(got["key"], w["key"])

    got = _run(torch, sc, 5)
    hook(got, 5, gu.R, gu.T, gu.K)
    # T = 1, R = 4097: two selection tiles
    big = _run(torch, sc, 0, rows=sc["rows"][1:2], x0=sc["x0"][1:2], R=4097, k=6)
    assert big["count"][0] >= 2
    _check_selection(big, 0, 6, 4097, 1)
    hook(big, 0, 4097, 1, 6)
    # restarts 0 .. 66 of the long launch are the short launch's
    short = _run(torch, sc, 0)
    assert _same(big["restart_x"][:, :gu.R], short["restart_x"][:, gu.R:2 * gu.R])


@pytest.mark.parametrize("name", ("panda", "arm10"))
def test_capped_grid_gives_the_same_bits_into_sentinel_filled_outputs(torch_dev, scenes, name):
    from optik_amd import _native as nat
    torch, sc = torch_dev, scenes(name)
    hc, n, cols = sc["hc"], sc["hc"].n, gu.T * gu.R

    def call(cap):
        bufs = dict(x=_out((n, cols), torch.float64), violation=_out((cols,), torch.float64),
                    status=_out((cols,), torch.int32), iterations=_out((cols,), torch.int32),
                    key=_out((cols,), torch.float64), count=_out((gu.T,), torch.int32),
                    sol_x=_out((gu.T, gu.K, n), torch.float64), sol_violation=_out((gu.T, gu.K), torch.float64),
                    sol_idx=_out((gu.T, gu.K), torch.int64), sol_key=_out((gu.T, gu.K), torch.float64))
        o = nat.IkRegionOutputs()
        for k, v in bufs.items():
            setattr(o, "d_" + k, v.data_ptr())
        regions, x0 = _t(torch, sc["rows"]), _t(torch, sc["x0"])
        with nat.options(grid_cap=cap):
            nat.check(nat.lib().optik_hip_ik_region(
                hc._h, None, regions.data_ptr(), x0.data_ptr(), gu.T, 5, 5 + gu.R, gu.TOL, gu.PROJECT["iters"],
                gu.PROJECT["damping"], gu.PROJECT["max_step"], gu.MODE_QUALITY, None, None, None, 0.0, gu.K,
                gu.MIN_DIST, C.byref(o), None))
            torch.cuda.synchronize()
        out = _np(bufs)
        for k, v in out.items():
            # (NaN padding past the count is written by the kernel with its own payload; the sentinel's must be gone)
            assert _sentinels_left(v) == 0, (k, cap)
        return out

    free, one, three = call(0), call(1), call(3)
    for k in free:
        assert np.array_equal(free[k].view(np.uint8), one[k].view(np.uint8)), k
        assert np.array_equal(free[k].view(np.uint8), three[k].view(np.uint8)), k
    want = sc["host"][(5, gu.MODE_QUALITY)]
    assert _same(free["x"].T, want["x"]) and _same(free["key"], want["key"])


def test_collision_model_and_world_filter_the_keys(torch_dev, scenes):
    from optik_amd.collision import spheres_along_chain
    torch, sc = torch_dev, scenes("panda")
    robot = sc["robot"]
    hc = robot.hip_chain()  # (a chain of its own: the model stays off the shared one)
    frames, centers, radii = spheres_along_chain(robot, 0.05, 2)
    base = _run(torch, sc, 0, hc=hc)
    # a world sphere where some of the projected rows of every region have their elbow (chosen on the CPU with the
    # host builds of region_measure.hpp and collision_measure.hpp: 10, 14 and 8 of the projected rows touch it)
    hc.set_collision_model(frames, centers, radii, self_pairs=None)
    hc.set_world(spheres=np.array([[0.19, -0.16, 0.62, 0.08]]))
    try:
        got = _run(torch, sc, 0, hc=hc)
        _, free = hc.collision_batch(_t(torch, base["restart_x"]))
        free = free.cpu().numpy()
        projected = base["restart_status"] == PROJECTED
        assert _same(got["restart_x"], base["restart_x"])
        assert _same(got["restart_key"], np.where(projected & ~free, np.inf, base["restart_key"]))
        assert (projected & ~free).any() and (projected & free).any()  # (the scene does both)
        _check_selection(got, 0, gu.K, gu.R, gu.T)
        for t in range(gu.T):
            c = int(got["count"][t])
            if c:
                _, f = hc.collision_batch(_t(torch, got["x"][t, :c].T))
                assert f.cpu().numpy().all(), t
    finally:
        hc.clear_collision_model()
        hc.set_world()


@pytest.mark.parametrize("name", ("panda", "arm10"))
def test_keep_filters_the_keys_where_its_violation_exceeds_its_tol(torch_dev, scenes, name):
    torch, sc = torch_dev, scenes(name)
    hc = sc["hc"]
    keep, ktol = cu.upright_constraint(sc["regs"][0].ref7, 0.3), 0.05
    base = _run(torch, sc, 0)
    got = _run(torch, sc, 0, keep=(keep, ktol))
    _, v = hc.constraint_batch(_t(torch, base["restart_x"]), keep)
    v = v.cpu().numpy()
    assert _same(got["restart_key"], np.where(v <= ktol, base["restart_key"], np.inf))
    assert _same(got["restart_x"], base["restart_x"]) and np.array_equal(got["restart_status"], base["restart_status"])
    dropped = np.isfinite(base["restart_key"]) & ~np.isfinite(got["restart_key"])
    assert dropped.any() and np.isfinite(got["restart_key"]).any()
    _check_selection(got, 0, gu.K, gu.R, gu.T)


@pytest.mark.parametrize("name", gu.ROBOTS)
def test_properties_of_the_returned_rows(torch_dev, scenes, name):
    torch, sc = torch_dev, scenes(name)
    robot = sc["robot"]
    lb, ub = (np.asarray(v) for v in robot.joint_limits())
    got = _run(torch, sc, 0)
    for t, c in enumerate(sc["regs"]):
        cnt = int(got["count"][t])
        assert cnt >= 2, (name, t)
        x = got["x"][t, :cnt]
        _, v = robot.constraint_batch_arrays(x, c)
        assert (v <= gu.TOL).all(), (name, t)
        assert ((x >= lb) & (x <= ub)).all(), (name, t)
        for a in range(cnt):
            for b in range(a):
                assert np.abs(x[a] - x[b]).max() > gu.MIN_DIST, (name, t, a, b)
    # Speed, K = 1, the pinned region: the lowest PROJECTED index
    one = _run(torch, sc, 0, mode="speed", k=1)
    first = int(np.nonzero(one["restart_status"][:gu.R] == PROJECTED)[0][0])
    assert one["count"][0] == 1 and one["idx"][0, 0] == first and one["key"][0, 0] == float(first)
    assert _same(one["x"][0, 0], one["restart_x"][:, first])
    # a box free on every axis: status 0 after 0 iterations, x the clamped start
    free = np.tile(gu.region_row(cu.free_constraint(sc["regs"][0].ref7)), (gu.T, 1))
    fr = _run(torch, sc, 0, rows=free)
    assert (fr["restart_status"] == PROJECTED).all() and (fr["restart_iterations"] == 0).all()
    seeds = sc["hc"].seed_batch(0, gu.R).cpu().numpy().T
    for t in range(gu.T):
        starts = seeds.copy()
        starts[0] = sc["x0"][t]
        assert _same(fr["restart_x"][:, t * gu.R:(t + 1) * gu.R].T, np.clip(starts, lb, ub)), (name, t)
    # a region with a NaN in its reference: FAILED rows, count 0
    bad = sc["rows"].copy()
    bad[1, 1] = math.nan
    nb = _run(torch, sc, 0, rows=bad)
    assert (nb["restart_status"][gu.R:2 * gu.R] == FAILED).all() and nb["count"][1] == 0
    assert nb["count"][0] == got["count"][0] and _same(nb["x"][2], got["x"][2])


@pytest.mark.parametrize("name", ("panda", "arm10"))
def test_robot_layer_equals_chain_layer(torch_dev, scenes, name):
    from optik_amd import PoseConstraint, SolverConfig
    torch, sc = torch_dev, scenes(name)
    robot = sc["robot"]
    pose = np.asarray(robot.fk(list(gu.mid_config(sc["tables"])))).reshape(4, 4)
    regs = [PoseConstraint.around(pose, 0.0, 0.0), PoseConstraint.axis_free(pose, "z"),
            PoseConstraint.position_only(pose, gu.POS_BOX)]
    for mode in ("quality", "speed"):
        got = robot.ik_region_batch_arrays(SolverConfig(solution_mode=mode), regs, sc["x0"], k=gu.K,
                                           min_dist=gu.MIN_DIST, restarts=gu.R, tol=gu.TOL, **gu.PROJECT)
        from optik_amd.constraint import region_rows
        want = _run(torch, sc, 0, mode, rows=region_rows(regs, gu.T))
        assert np.array_equal(got["count"], want["count"]) and _same(got["x"], want["x"]), (name, mode)
        assert _same(got["violation"], want["violation"]) and _same(got["key"], want["key"]), (name, mode)
        assert np.array_equal(got["idx"].view(np.int64), want["idx"]), (name, mode)
    one = robot.ik_region(SolverConfig(solution_mode="quality"), regs[1], sc["x0"][1], k=gu.K, min_dist=gu.MIN_DIST,
                          restarts=gu.R, tol=gu.TOL, **gu.PROJECT)
    q = robot.ik_region_batch_arrays(SolverConfig(solution_mode="quality"), regs[1], sc["x0"][1:2], k=gu.K,
                                     min_dist=gu.MIN_DIST, restarts=gu.R, tol=gu.TOL, **gu.PROJECT)
    assert len(one) == q["count"][0] >= 2 and _same(np.array(one), q["x"][0, :len(one)])


def test_planners_equal_ik_region_followed_by_the_goal_set_planners(torch_dev, scenes):
    from optik_amd import PoseConstraint, SolverConfig
    sc = scenes("panda")
    robot = sc["robot"]
    cfg = SolverConfig(solution_mode="quality")
    Q = 3
    starts = np.tile(np.array(cu.PANDA_HOME), (Q, 1)) + 0.1 * np.arange(Q)[:, None] * np.array([1, 0, 0, 0, 0, 0, 1.0])
    home = np.asarray(robot.fk(cu.PANDA_HOME)).reshape(4, 4)
    shelf = home.copy()
    shelf[:3, 3] += [0.0, 0.25, -0.1]
    b, inf = 0.3 / math.sqrt(2.0), math.inf
    regs = [PoseConstraint(shelf, [-0.1, -0.1, 0, -b, -b, -inf], [0.1, 0.1, 0, b, b, inf]),
            PoseConstraint.position_only(shelf, 0.02), PoseConstraint.axis_free(shelf, "z")]
    ik = dict(k=4, min_dist=gu.MIN_DIST)
    reg = dict(restarts=gu.R, tol=gu.TOL)
    sol = robot.ik_region_batch_arrays(cfg, regs, starts, **ik, **reg)
    assert (sol["count"] >= 1).all()
    rrt = dict(iters=128, step=0.3, first=1, max_nodes=128, resolution=0.1)
    got = robot.plan_rrt_to_region(cfg, starts, regs, **ik, **rrt, region_args=reg)
    want = robot.plan_rrt_to_goals(starts, sol["x"], counts=sol["count"], **rrt)
    assert _same(got["goals"], sol["x"]) and np.array_equal(got["count"], sol["count"])
    for key in want:
        assert np.array_equal(np.asarray(got[key]).view(np.uint8), np.asarray(want[key]).view(np.uint8)), key
    assert (got["status"] == 0).all()
    for q in range(Q):
        last = got["paths"][q, got["len"][q] - 1]
        assert robot.constraint_batch_arrays(last[None], regs[q])[1][0] <= gu.TOL, q
        assert _same(last, sol["x"][q, got["goal"][q]])
    # under a path constraint: the goals satisfy it, the paths keep it
    c, ctol = PoseConstraint.upright(home, 0.3), 0.05
    con = robot.plan_rrt_to_region_constrained(cfg, starts, regs[0], c, tol=ctol, region_args=reg, **ik, **rrt)
    kept = robot.ik_region_batch_arrays(cfg, regs[0], starts, keep=(c, ctol), **ik, **reg)
    assert _same(con["goals"], kept["x"]) and np.array_equal(con["count"], kept["count"])
    wantc = robot.plan_rrt_to_goals_constrained(starts, kept["x"], c, kept["count"], tol=ctol, **rrt)
    for key in wantc:
        assert np.array_equal(np.asarray(con[key]).view(np.uint8), np.asarray(wantc[key]).view(np.uint8)), key
    found = con["status"] == 0
    assert found.any()
    chk = robot.check_paths_constraint(con["paths"][found], con["len"][found], c, tol=ctol, resolution=0.1)
    assert chk["ok"].all()
    for q in np.nonzero(found)[0]:
        last = con["paths"][q, con["len"][q] - 1]
        assert robot.constraint_batch_arrays(last[None], regs[0])[1][0] <= gu.TOL, q
    # over a roadmap: eager equals the composition, lazy raises
    robot.build_roadmap(128, 8, 0.1)
    rm = robot.plan_to_region(cfg, starts, regs, **ik, region_args=reg)
    wr = robot.plan_to_goals(starts, sol["x"], counts=sol["count"])
    for key in wr:
        assert np.array_equal(np.asarray(rm[key]).view(np.uint8), np.asarray(wr[key]).view(np.uint8)), key
    assert _same(rm["goals"], sol["x"])
    for q in np.nonzero(rm["status"] == 0)[0]:
        last = rm["paths"][q, rm["len"][q] - 1]
        assert robot.constraint_batch_arrays(last[None], regs[q])[1][0] <= gu.TOL, q
    robot.build_roadmap(128, 8, 0.1, lazy=True)
    with pytest.raises(RuntimeError, match="eager roadmaps only"):
        robot.plan_to_region(cfg, starts, regs, **ik, region_args=reg)
    with pytest.raises(RuntimeError, match="eager roadmaps only"):
        robot.plan_to_goals(starts, sol["x"], counts=sol["count"])


def test_device_planners_keep_both_stages_on_the_stream(torch_dev, scenes):
    torch, sc = torch_dev, scenes("panda")
    hc = sc["hc"]
    starts = _t(torch, sc["x0"].T)
    regions = _t(torch, sc["rows"])
    reg = dict(tol=gu.TOL, **gu.PROJECT)
    sol = hc.ik_region(regions, starts.t().contiguous(), 0, gu.R, 4, gu.MIN_DIST, **reg)
    goals = sol["x"].permute(1, 2, 0).contiguous()
    got = hc.rrt_plan_region(regions, starts, 0, gu.R, 4, gu.MIN_DIST, 64, 0.3, 0.1, first=1, max_nodes=64,
                             region_args=reg)
    want = hc.rrt_plan_goals(starts, goals, sol["count"], 64, 0.3, 0.1, first=1, max_nodes=64)
    assert torch.equal(got["count"], sol["count"]) and _same(got["goals"].cpu().numpy(), goals.cpu().numpy())
    for key in want:
        assert np.array_equal(got[key].cpu().numpy().view(np.uint8), want[key].cpu().numpy().view(np.uint8)), key
    keep = cu.upright_constraint(sc["regs"][0].ref7, 0.3)
    con = hc.rrt_plan_region_constrained(regions, starts, keep, 0.05, 0, gu.R, 4, gu.MIN_DIST, 64, 0.3, 0.1, first=1,
                                         max_nodes=64, region_args=reg)
    ksol = hc.ik_region(regions, starts.t().contiguous(), 0, gu.R, 4, gu.MIN_DIST, keep=(keep, 0.05), **reg)
    assert torch.equal(con["count"], ksol["count"])
    wc = hc.rrt_plan_constrained(starts, ksol["x"].permute(1, 2, 0).contiguous(), ksol["count"], keep, 0.05, 64, 0.3,
                                 0.1, first=1, max_nodes=64)
    for key in wc:
        assert np.array_equal(con[key].cpu().numpy().view(np.uint8), wc[key].cpu().numpy().view(np.uint8)), key
    nodes = hc.seed_batch(1, 64)
    nbr, w = hc.roadmap_build(nodes, 6, 0.1)
    rm = hc.roadmap_plan_region((nodes, nbr, w), regions, starts, 0, gu.R, 4, gu.MIN_DIST, 4, 32, 0.1,
                                region_args=reg)
    wr = hc.roadmap_plan_goals((nodes, nbr, w), starts, goals, sol["count"], 4, 32, 0.1)
    for key in wr:
        assert np.array_equal(rm[key].cpu().numpy().view(np.uint8), wr[key].cpu().numpy().view(np.uint8)), key


def test_refusals_of_the_three_layers(torch_dev, scenes):
    from optik_amd import PoseConstraint, Robot, SolverConfig
    from optik_amd import _native as nat
    torch, sc = torch_dev, scenes("panda")
    hc, robot = sc["hc"], sc["robot"]
    regions, x0 = _t(torch, sc["rows"]), _t(torch, sc["x0"])
    o = nat.IkRegionOutputs()
    z6, ref7 = np.zeros(6), sc["regs"][0].ref7
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731

    def c_call(T=gu.T, begin=0, end=gu.R, tol=gu.TOL, iters=8, damping=1e-6, max_step=0.5, mode=1, keep=None,
               keep_tol=0.0, K=4, min_dist=0.1, chain=None, out=o):
        kr, kl, kh = keep if keep is not None else (None, None, None)
        return nat.lib().optik_hip_ik_region(
            chain if chain is not None else hc._h, None, regions.data_ptr(), x0.data_ptr(), T, begin, end, tol, iters,
            damping, max_step, mode, dp(kr) if kr is not None else None, dp(kl) if kl is not None else None,
            dp(kh) if kh is not None else None, keep_tol, K, min_dist, C.byref(out) if out is not None else None, None)

    bad_ref, ones = ref7.copy(), np.ones(6)
    bad_ref[6] = 1.5
    cases = [dict(T=-1), dict(begin=5, end=5), dict(tol=-1.0), dict(tol=math.nan), dict(iters=-1), dict(iters=4097),
             dict(damping=-1.0), dict(max_step=0.0), dict(max_step=math.inf), dict(mode=0), dict(mode=5), dict(K=0),
             dict(K=257), dict(min_dist=-0.1), dict(min_dist=math.nan), dict(end=1 << 40),
             dict(keep=(ref7, z6, None)), dict(keep=(bad_ref, z6, z6)), dict(keep=(ref7, ones, z6)),
             dict(keep=(ref7, z6, z6), keep_tol=-1.0), dict(keep=(ref7, z6, z6), keep_tol=math.nan), dict(out=None)]
    for kw in cases:
        for T in ((kw["T"],) if "T" in kw else (gu.T, 0)):  # (refused at T = 0 too)
            assert c_call(**dict(kw, T=T)) != 0, (kw, T)
            assert nat.lib().optik_hip_last_error()
    assert c_call(T=0) == 0 and c_call(T=0, keep=(ref7, z6, z6), keep_tol=0.1) == 0
    gantry = Robot.from_urdf_file(*ROBOT_SPECS["gantry"])
    g = gantry.hip_chain()
    assert c_call(T=0, chain=g._h) != 0 and b"prismatic" in nat.lib().optik_hip_last_error()
    # HipChain
    for kw in (dict(k=0), dict(min_dist=-1.0), dict(tol=-1.0), dict(iters=5000), dict(mode="fast"),
               dict(keep=(sc["regs"][0], -1.0)), dict(begin=3, end=3)):
        args = dict(dict(begin=0, end=gu.R, k=4, min_dist=0.1), **kw)
        b, e, k, md = (args.pop(key) for key in ("begin", "end", "k", "min_dist"))
        with pytest.raises(ValueError):
            hc.ik_region(regions, x0, b, e, k, md, **args)
    with pytest.raises(ValueError):
        hc.ik_region(regions[:, :18].contiguous(), x0, 0, gu.R, 4, 0.1)
    with pytest.raises(ValueError):
        hc.ik_region(regions, x0[:2], 0, gu.R, 4, 0.1)
    # Robot, and the host rows beneath it
    cfg, good = SolverConfig(solution_mode="quality"), PoseConstraint.position_only(np.eye(4), 0.02)
    for kw in (dict(k=0), dict(restarts=0), dict(restarts=(1 << 22) + 1), dict(min_dist=math.inf), dict(tol=-1.0),
               dict(keep=(good, math.nan)), dict(keep=good)):
        with pytest.raises(ValueError):
            robot.ik_region_batch_arrays(cfg, good, sc["x0"], **kw)
    with pytest.raises(ValueError, match="sequence of T"):
        robot.ik_region_batch_arrays(cfg, [good], sc["x0"])
    with pytest.raises(ValueError):
        robot.plan_rrt_to_region(cfg, sc["x0"], good, k=17)
    L = robot._L
    rows = sc["rows"].copy()
    rows[2, 9] = math.nan  # lo of region 2
    cnt = np.zeros(gu.T, dtype=np.int32)

    def r_call(rows, restarts=gu.R, K=4):
        return L.optik_robot_ik_region(robot._h, gu.T, dp(rows), dp(sc["x0"]), restarts, gu.TOL, 8, 1e-6, 0.5, 1, None,
                                       None, None, 0.0, K, 0.1, None, cnt.ctypes.data_as(C.POINTER(C.c_int32)), None,
                                       None, None, None)
    assert r_call(rows) != 0 and b"region 2" in L.optik_robot_last_error()
    rows = sc["rows"].copy()
    rows[1, 3:7] *= 1.01
    assert r_call(rows) != 0 and b"region 1" in L.optik_robot_last_error()
    assert r_call(sc["rows"], restarts=0) != 0 and r_call(sc["rows"], K=0) != 0
    assert r_call(sc["rows"]) == 0 and (cnt >= 2).all()
    with pytest.raises(RuntimeError, match="prismatic"):
        gantry.ik_region_batch_arrays(cfg, good, np.zeros((1, gantry.num_positions())))
