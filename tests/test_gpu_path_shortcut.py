"""-m gpu: path shortcutting and resampling on the device against the host.  path_shortcut against the serial reference
of csrc/shortcut_measure.hpp (g++), fed the visibility that collision_motion_batch gives on the same pairs, bit for
bit; a path's independence of the batch and of the chunking; path_resample against the reference; shortcut_paths /
resample_paths end to end on the wall scene and on the jagged route tests/test_shortcut_host.py chooses on the CPU;
the refusals."""
import math

import numpy as np
import pytest

import shortcut_util as su
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
    return su.build_shortcut_ref(str(tmp_path_factory.mktemp("shortcut_measure")))


@pytest.fixture(scope="module")
def wall(robots):
    sc = su.wall_scene()
    sc["robot"] = robots("panda")
    return sc


def _t(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all((su.bits(got) == su.bits(want)) | (np.isnan(got) & np.isnan(want))))


def _device(torch, hc, paths, lens, V, h, hop, Lout):
    """hc.path_shortcut on paths [P, L, n]: numpy results, the path back as [P, Lout, n]."""
    res = hc.path_shortcut(_t(torch, su.to_device_layout(paths)),
                           None if lens is None else _t(torch, np.asarray(lens, dtype=np.int32)), h, V, hop, Lout)
    out = {k: v.cpu().numpy() for k, v in res.items()}
    out["path"] = np.ascontiguousarray(np.transpose(out["path"], (1, 0, 2)))
    return out


def _reference(torch, ref, hc, paths, lens, V, h, hop, Lout):
    """The serial reference over the visibility collision_motion_batch gives on the same pairs."""
    P, _, n = paths.shape
    _, _, _, verts = ref.vertices(paths, lens, V)
    seg = [su.pair_segments(verts[p], V) for p in range(P)]
    qa = np.concatenate([s[0] for s in seg]).T
    qb = np.concatenate([s[1] for s in seg]).T
    free = np.zeros((P, su.pair_count(V)), dtype=bool)
    if qa.shape[1]:
        free = hc.collision_motion_batch(_t(torch, qa), _t(torch, qb), h, clearance=False)[1].cpu().numpy().reshape(P, -1)
    return ref.shortcut(paths, lens, V, free, hop, Lout), free


def _agree(got, want, tag):
    for key in ("status", "len"):
        assert np.array_equal(got[key], want[key]), (tag, key, got[key], want[key])
    for key in ("cost", "cost_in", "path"):
        assert _same(got[key], want[key]), (tag, key)


LENS = [2, 3, 17, 64, 64]


def _five_paths(n, seed, span):
    """P = 5 random walks of 2, 3, 17, 64 and 64 waypoints in [*, 64, n]; the last holds a NaN."""
    rng = np.random.default_rng(seed)
    paths = su.random_polylines(rng, 5, 64, n, lens=LENS, scale=span)
    paths[4, 40, n - 1] = math.nan
    return paths


@pytest.mark.parametrize("chain,model", [("panda1", False), ("panda", False), ("panda", True), ("arm8", False),
                                         ("arm10", False)])
def test_device_matches_the_reference(torch_dev, robots, ref, wall, chain, model):
    hc = robots(chain).hip_chain()
    n, h = hc.n, 0.05
    if model:
        hc.set_collision_model(wall["frames"], wall["centers"], wall["radii"], self_pairs=None)
        hc.set_world(boxes=wall["boxes"])
    else:
        hc.clear_collision_model()
    paths = _five_paths(n, 7 * n + model, 0.15)
    if model:
        # walks that start on the two sides of the wall: some motions are blocked, some are not
        paths[:4] = paths[:4] * 0.5 + np.array(su.WALL_ROUTE)[[0, 2, 5, 6], None, :]
    else:
        # a motion of more than 4096 steps is not sampled: the two-waypoint path has no single hop
        paths[0, 1:] = paths[0, 0] + 500.0
    seen, share = set(), []
    for V in (2, 33, 64):
        for Lout in (2, 64):
            got = _device(torch_dev, hc, paths, LENS, V, h, h, Lout)
            want, free = _reference(torch_dev, ref, hc, paths, LENS, V, h, h, Lout)
            _agree(got, want, (chain, model, V, Lout))
            seen |= set(got["status"].tolist())
            share.append(free.mean())
            ok = got["status"] == su.FOUND
            assert np.all(got["len"][ok] <= Lout)
            if not model:
                assert np.all(got["len"][ok] == 2) or V > 2, "without a model the route is the single hop"
                for p in np.nonzero(ok)[0]:
                    if p != 0:
                        assert got["len"][p] == 2, (V, Lout, p)
            assert got["status"][4] == (su.PATH_NAN if V == 64 else su.BAD_LENGTH)
            assert got["status"][3] == su.BAD_LENGTH or V == 64
    if model:
        assert su.FOUND in seen and any(0.0 < s < 1.0 for s in share), "the scene blocks some motions and not others"
    else:
        assert seen == {su.FOUND, su.NO_ROUTE, su.BAD_LENGTH, su.PATH_NAN}
    hc.clear_collision_model()
    hc.set_world()


def test_a_path_does_not_depend_on_the_batch(torch_dev, robots, wall):
    hc = robots("panda").hip_chain()
    hc.set_collision_model(wall["frames"], wall["centers"], wall["radii"], self_pairs=None)
    hc.set_world(boxes=wall["boxes"])
    paths = _five_paths(7, 3, 0.15)
    paths[:4] = paths[:4] * 0.5 + np.array(su.WALL_ROUTE)[[0, 2, 5, 6], None, :]
    all5 = _device(torch_dev, hc, paths, LENS, 64, 0.05, 0.05, 64)
    for p in (0, 3):
        one = _device(torch_dev, hc, paths[p:p + 1], LENS[p:p + 1], 64, 0.05, 0.05, 64)
        _agree(one, {k: v[p:p + 1] for k, v in all5.items()}, p)
    hc.clear_collision_model()
    hc.set_world()


def test_a_path_does_not_depend_on_the_chunking(torch_dev, robots):
    hc = robots("panda").hip_chain()
    hc.clear_collision_model()
    chunk = hc.path_shortcut_chunk(64)
    assert 1 <= chunk <= 4096, "the test crosses one chunk: a chunk must stay small enough to cross quickly"
    P = chunk + 3
    rng = np.random.default_rng(9)
    # T about 0.1 rad at resolution 0.05: at most three samples per pair
    paths = su.random_polylines(rng, P, 4, 7, scale=0.03)
    paths[chunk, 2, 0] = math.nan
    lens = np.full(P, 4, dtype=np.int32)
    lens[chunk - 1] = 3
    many = _device(torch_dev, hc, paths, lens, 64, 0.05, 0.0, 64)
    assert many["status"][chunk] == su.PATH_NAN and np.all(np.delete(many["status"], chunk) == su.FOUND)
    for p in (0, chunk - 1, chunk, P - 1):
        one = _device(torch_dev, hc, paths[p:p + 1], lens[p:p + 1], 64, 0.05, 0.0, 64)
        _agree(one, {k: v[p:p + 1] for k, v in many.items()}, p)


@pytest.mark.parametrize("chain", ["panda1", "panda", "arm10"])
def test_resample_matches_the_reference(torch_dev, robots, ref, chain):
    torch = torch_dev
    hc = robots(chain).hip_chain()
    rng = np.random.default_rng(hc.n)
    lens = [2, 3, 64, 64, 5]
    paths = su.random_polylines(rng, 5, 64, hc.n, lens=lens, scale=0.4)
    paths[3, 10, 0] = math.nan
    paths[4, :5] = paths[4, 0]                            # T = 0
    for Lout in (2, 3, 64):
        out, st = hc.path_resample(_t(torch, su.to_device_layout(paths)), _t(torch, np.array(lens, dtype=np.int32)), Lout)
        want, wst = ref.resample(paths, lens, Lout)
        assert np.array_equal(st.cpu().numpy(), wst) and wst.tolist() == [0, 0, 0, su.PATH_NAN, 0]
        assert _same(np.transpose(out.cpu().numpy(), (1, 0, 2)), want), Lout
    # lens None: every path has L waypoints
    out, st = hc.path_resample(_t(torch, su.to_device_layout(paths[:3, :9])), None, 17)
    want, wst = ref.resample(np.ascontiguousarray(paths[:3, :9]), None, 17)
    assert np.array_equal(st.cpu().numpy(), wst) and _same(np.transpose(out.cpu().numpy(), (1, 0, 2)), want)


def _set_wall(sc):
    sc["robot"].set_collision_model(sc["frames"], sc["centers"], sc["radii"], self_pairs=None)
    sc["robot"].set_world(boxes=sc["boxes"])


def test_shortcut_and_resample_round_the_wall(torch_dev, ref, wall):
    robot, h = wall["robot"], wall["h"]
    _set_wall(wall)
    s, g = wall["start"][None], wall["goal"][None]
    robot.build_roadmap(wall["N"], wall["k"], h, first=wall["first"])
    plan = robot.plan_paths(s, g, 64)
    assert plan["status"][0] == su.FOUND
    # a stale roadmap does not matter to either call
    robot.set_world(boxes=wall["boxes"])
    res = robot.shortcut_paths(plan["paths"], plan["len"], resolution=h)
    assert res["status"][0] == su.FOUND and res["paths"].shape == (1, 64, 7)
    L = int(res["len"][0])
    assert 2 <= L <= plan["len"][0] and res["cost"][0] <= plan["cost"][0]
    assert su.bits(res["cost_in"][0]) == su.bits(plan["cost"][0])
    path = res["paths"][0]
    assert np.array_equal(su.bits(path[0]), su.bits(s[0])) and np.array_equal(su.bits(path[L - 1]), su.bits(g[0]))
    assert np.all(path[L:] == g[0][None])
    assert robot.collision_motion_batch_arrays(path[:L - 1], path[1:L], h)[1].all(), "every segment is a free motion"
    dense, st, free = robot.resample_paths(res["paths"], res["len"], 32, resolution=h)
    assert dense.shape == (1, 32, 7) and st[0] == 0
    assert np.array_equal(dense[0, 0], s[0]) and np.array_equal(dense[0, -1], g[0])
    seg = robot.collision_motion_batch_arrays(dense[0, :-1], dense[0, 1:], h)[1]
    assert free.shape == (1,) and bool(free[0]) == bool(seg.all())
    want, _ = ref.resample(res["paths"], res["len"], 32)
    assert _same(dense, want)
    out = robot.optimize_paths(dense, iters=2, step=0.001)
    assert out[0].shape == (1, 32, 7) and out[4][0] == 0
    # the jagged route chosen on the CPU: what tests/test_shortcut_host.py predicted
    route = np.array(su.WALL_ROUTE)[None]
    res = robot.shortcut_paths(route, None, resolution=h, vertices=su.WALL_VERTICES)
    _, _, nv, verts = ref.vertices(route, None, su.WALL_VERTICES)
    assert res["status"][0] == su.FOUND and res["len"][0] == len(su.WALL_SHORTCUT) < route.shape[1]
    assert res["cost"][0] < res["cost_in"][0]
    assert _same(res["paths"][0, :3], verts[0, su.WALL_SHORTCUT])
    assert robot.collision_motion_batch_arrays(res["paths"][0, :2], res["paths"][0, 1:3], h)[1].all()
    robot.clear_collision_model()
    robot.set_world()


def test_refusals(torch_dev, robots):
    import ctypes as C
    from optik_amd import _native as nat
    robot = robots("panda")
    paths = np.zeros((2, 4, 7))
    for kw in (dict(vertices=1), dict(vertices=65), dict(max_waypoints=1), dict(max_waypoints=65), dict(resolution=0.0),
               dict(resolution=-0.05), dict(resolution=math.nan), dict(hop_penalty=-1.0), dict(hop_penalty=math.nan)):
        with pytest.raises(ValueError):
            robot.shortcut_paths(paths, **kw)
    for kw in (dict(waypoints=1), dict(waypoints=65), dict(resolution=0.0)):
        with pytest.raises(ValueError):
            robot.resample_paths(paths, **kw)
    with pytest.raises(ValueError):
        robot.shortcut_paths(np.zeros((2, 4, 6)))
    with pytest.raises(ValueError):
        robot.shortcut_paths(paths, lens=[4])
    # the kernel layer itself: OPTIK_HIP_EINVAL (-1) before any device work
    lib, hc = nat.lib(), robot.hip_chain()
    null = C.c_void_p(None)

    def shortcut(V=8, Lin=8, Lout=8, h=0.05, hop=0.0, chain=hc):
        return lib.optik_hip_path_shortcut(chain._h, None, null, null, Lin, 4, V, h, hop, Lout, null, null, null, null,
                                           null, null)
    for kw in (dict(V=1), dict(V=65), dict(Lout=1), dict(Lout=65), dict(Lin=1), dict(Lin=65), dict(h=0.0),
               dict(h=-0.05), dict(h=math.nan), dict(hop=-1.0), dict(hop=math.nan), dict(hop=math.inf)):
        assert shortcut(**kw) == -1, kw
    assert lib.optik_hip_path_shortcut(hc._h, None, null, null, 8, -1, 8, 0.05, 0.0, 8, null, null, null, null, null,
                                       null) == -1
    for Lin, Lout in ((1, 8), (65, 8), (8, 1), (8, 65)):
        assert lib.optik_hip_path_resample(hc._h, null, null, Lin, 4, Lout, null, null, null) == -1
    assert shortcut() == 0, "nothing to write: a no-op"
    gantry = robots("gantry").hip_chain()
    EUNSUPPORTED = -2
    assert shortcut(chain=gantry) == EUNSUPPORTED
    assert lib.optik_hip_path_shortcut(gantry._h, None, null, null, 8, 0, 8, 0.05, 0.0, 8, null, null, null, null,
                                       null, null) == EUNSUPPORTED
    assert lib.optik_hip_path_resample(gantry._h, null, null, 8, 0, 8, null, null, null) == EUNSUPPORTED
