"""-m gpu: the distance-field world (include/optik_hip.h; csrc/collision_measure.hpp steps 5 - 7).

The bake is compared bit for bit with the g++-built primitive_field cast to float32.  collision_batch under a grid is
compared bit for bit with fmin(clearance(...), clearance_grid(...)) of the g++-built header applied to
link_frames_batch's frames.  The motion check under a grid is compared with its definition by composition, and a
filtered solver launch with the winner selected on the host, as tests/test_gpu_collision_motion.py and
tests/test_gpu_ik_collision.py do for the primitives."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from collision_util import build_measure
from conftest import ROBOT_SPECS, ROBOTS, ROOT
from gpu_util import assert_bit_equal, make_targets
from grid_util import build_grid_measure

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CHAINS = ["panda", "ur10", "arm10"]
MARGIN = 0.01
ORIGIN, VOXEL, SHAPE = np.array([-1.5, -1.5, -1.5]), 0.1, (31, 31, 31)       # [-1.5, 1.5]^3
SMALL_ORIGIN, SMALL_SHAPE = np.array([0.0, 0.0, 0.0]), (9, 9, 9)             # [0, 0.8]^3


@pytest.fixture(scope="module")
def measure(tmp_path_factory):
    return build_measure(str(tmp_path_factory.mktemp("collision_measure")))


@pytest.fixture(scope="module")
def gm(tmp_path_factory):
    return build_grid_measure(str(tmp_path_factory.mktemp("grid_measure")))


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _robot(name):
    from optik_amd import Robot
    return Robot.from_urdf_file(*ROBOT_SPECS[name])


def model_of(name):
    """Spheres of 4 cm along the links, "auto" pairs: 36 on the Panda (12 on each of its three long segments), and
    as near to 36 as equal counts per segment get on the other chains."""
    from optik_amd.collision import auto_pairs, spheres_along_chain
    robot = _robot(name)
    segments = len(spheres_along_chain(robot, 0.04, 1)[0])
    frames, centers, radii = spheres_along_chain(robot, 0.04, max(1, round(36 / segments)))
    if name == "panda":
        assert len(frames) == 36
    return dict(frames=frames, centers=centers, radii=radii, self_pairs=auto_pairs(frames), margin=MARGIN)


def world():
    """3 spheres and 2 turned boxes inside the robots' reach."""
    sph = np.array([[0.45, 0.10, 0.50, 0.12], [-0.30, 0.40, 0.30, 0.08], [0.10, -0.50, 0.70, 0.10]])
    q = np.array([[0.2, -0.1, 0.4, 0.9], [-0.5, 0.3, 0.1, 0.7]])
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    box = np.array([np.concatenate([[0.30, -0.30, 0.25], q[0], [0.10, 0.15, 0.05]]),
                    np.concatenate([[-0.40, -0.20, 0.60], q[1], [0.05, 0.20, 0.12]])])
    return sph, box


def _rot(q):
    i, j, k, w = q
    return np.array([[1 - 2 * (j * j + k * k), 2 * (i * j - k * w), 2 * (i * k + j * w)],
                     [2 * (i * j + k * w), 1 - 2 * (i * i + k * k), 2 * (j * k - i * w)],
                     [2 * (i * k - j * w), 2 * (j * k + i * w), 1 - 2 * (i * i + j * j)]])


def sphere_centres(fr, model):
    """[B, S, 3]: the model's sphere centres in the base frame, from link_frames_batch's frames (numpy)."""
    out = np.empty((fr.shape[0], len(model["frames"]), 3))
    for b in range(fr.shape[0]):
        for s, (f, c) in enumerate(zip(model["frames"], model["centers"])):
            out[b, s] = fr[b, f, :3] + _rot(fr[b, f, 3:]) @ c
    return out


@pytest.fixture(scope="module")
def scene(chains, gm):
    """The primitives, the 31^3 grid and the 9^3 grid baked from them (by the g++ header: the GPU bake has its own
    test), computed once."""
    sph, box = world()
    return dict(sph=sph, box=box, big=gm.bake(ORIGIN, VOXEL, SHAPE, sph, box),
                small=gm.bake(SMALL_ORIGIN, VOXEL, SMALL_SHAPE, sph, box))


def test_bake_equals_the_header(chains, gm):
    from optik_amd import device
    hc = device.HipChain(**chains["panda"][0])
    sph, box = world()
    hc.set_world(sph, box)
    origin, voxel, shape = np.array([-0.43, -0.52, -0.07]), 0.11, (9, 10, 11)
    got = hc.bake_world_grid(origin, voxel, shape)
    assert got.dtype == torch.float32 and tuple(got.shape) == shape and got.is_cuda
    got = got.cpu().numpy()
    want = gm.bake(origin, voxel, shape, sph, box)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
    assert (want < 0).any() and (want > 0.3).any()  # (nodes inside obstacles and far from them)
    # the robot's bake (host output) is the chain's, and nothing was installed by either
    r = _robot("panda")
    r.set_world(sph, box)
    got_r = r.bake_world_grid(origin, voxel, shape)
    assert got_r.dtype == np.float32 and np.array_equal(got_r.view(np.uint32), want.view(np.uint32))
    from optik_amd import _native as nat
    hc.set_world()
    with pytest.raises(nat.OptikHipError, match="no spheres and no boxes"):
        hc.bake_world_grid(origin, voxel, shape)
    with pytest.raises(nat.OptikHipError, match="NaN or infinite"):
        hc.set_world_grid(origin, voxel, np.full(shape, math.nan))


@pytest.mark.parametrize("name", CHAINS)
def test_collision_batch_equals_the_header(chains, scene, measure, gm, name):
    from optik_amd import device
    d = chains[name][0]
    m = model_of(name)
    hc = device.HipChain(**d)
    hc.set_collision_model(**m)
    rng = np.random.default_rng(2)
    B = 300  # more than one block of 256, ending in a partial wave
    q = rng.uniform(d["lb"], d["ub"], size=(B, len(d["lb"])))
    q[0, 0] = math.nan
    fr = hc.link_frames_batch(_dev(q.T)).cpu().numpy()
    args = (fr, m["frames"], m["centers"], m["radii"])
    prim_none = measure.clearance(*args, m["self_pairs"])
    prim = measure.clearance(*args, m["self_pairs"], scene["sph"], scene["box"])
    grid_big = gm.clearance_grid(*args, ORIGIN, VOXEL, scene["big"])
    grid_small = gm.clearance_grid(*args, SMALL_ORIGIN, VOXEL, scene["small"])
    cases = [("grid alone", None, (ORIGIN, VOXEL, scene["big"]), np.fmin(prim_none, grid_big)),
             ("grid and primitives", (scene["sph"], scene["box"]), (ORIGIN, VOXEL, scene["big"]), np.fmin(prim, grid_big)),
             ("small grid", None, (SMALL_ORIGIN, VOXEL, scene["small"]), np.fmin(prim_none, grid_small))]
    for what, prims, grid, want in cases:
        hc.set_world(*(prims or ()))
        hc.set_world_grid(*grid)
        clr, free = (t.cpu().numpy() for t in hc.collision_batch(_dev(q.T)))
        assert_bit_equal(clr, want, f"{name} {what} clearance")
        assert math.isnan(clr[0]) and not free[0]
        assert np.array_equal(free, clr >= MARGIN)
    # the grid terms decide some configurations and the pairs others; the grid is in the way of some, not all
    both = np.fmin(prim_none, grid_big)[1:]
    assert (grid_big[1:] < prim_none[1:]).any() and (grid_big[1:] > prim_none[1:]).any()
    assert 0.0 < (both >= MARGIN).mean() < 1.0, (both >= MARGIN).mean()
    # the small grid: spheres inside and spheres outside both occur
    p = sphere_centres(fr[1:], m)
    inside = ((p >= 0.0) & (p <= 0.8)).all(-1)
    assert inside.any() and (~inside).any() and (grid_small[1:] < math.inf).any()
    assert (grid_small[1:] != grid_big[1:]).any()


def test_grid_clearance_approximates_the_primitives(chains, scene):
    """|grid-only clearance - primitives-only clearance| <= sqrt(3) * voxel + 2^-23 * max|value| for every configuration:
    the world's distance field is 1-Lipschitz, the trilinear value is a convex combination of corners within one cell
    diagonal of the centre, and the stored values are float32.  (The minimum over the spheres of terms that differ by
    at most e differs by at most e.)  Without self pairs, so that both clearances are minima over the same spheres."""
    from optik_amd import device
    d = chains["panda"][0]
    m = dict(model_of("panda"), self_pairs=None)
    hc = device.HipChain(**d)
    hc.set_collision_model(**m)
    rng = np.random.default_rng(3)
    B = 300
    q = rng.uniform(d["lb"], d["ub"], size=(B, 7))
    fr = hc.link_frames_batch(_dev(q.T)).cpu().numpy()
    p = sphere_centres(fr, m)
    hi = ORIGIN + VOXEL * (np.array(SHAPE) - 1)
    assert ((p >= ORIGIN) & (p <= hi)).all(), "every sphere centre of every configuration lies inside the grid"
    hc.set_world(scene["sph"], scene["box"])
    prim = hc.collision_batch(_dev(q.T))[0].cpu().numpy()
    hc.set_world()
    hc.set_world_grid(ORIGIN, VOXEL, scene["big"])
    grid = hc.collision_batch(_dev(q.T))[0].cpu().numpy()
    bound = math.sqrt(3.0) * VOXEL + 2.0 ** -23 * float(np.abs(scene["big"]).max())
    err = np.abs(grid - prim)
    print(f"grid vs primitives: max {err.max():.4f} mean {err.mean():.4f} bound {bound:.4f}")
    assert np.isfinite(grid).all() and np.isfinite(prim).all()
    assert (err <= bound).all(), err.max()
    assert err.max() > 0.0


def _segments(d, B, seed):
    """K = 1 (a few thousandths of a radian at h = 0.005), short ones and K of about 300, mixed."""
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    rng = np.random.default_rng(seed)
    qa = rng.uniform(lb, ub, (B, len(lb)))
    scale = rng.choice([0.004, 0.05, 1.5], size=(B, 1), p=[0.3, 0.4, 0.3])
    qb = np.clip(qa + rng.uniform(-1.0, 1.0, (B, len(lb))) * scale, lb, ub)
    return qa, qb


def test_clearing_the_grid_restores_the_bits(chains, scene):
    from optik_amd import device
    d = chains["panda"][0]
    m = model_of("panda")
    a, b = device.HipChain(**d), device.HipChain(**d)
    for hc in (a, b):
        hc.set_collision_model(**m)
        hc.set_world(scene["sph"], scene["box"])
    rng = np.random.default_rng(4)
    q = rng.uniform(d["lb"], d["ub"], size=(300, 7))
    qa, qb = _segments(d, 200, seed=5)
    b.set_world_grid(SMALL_ORIGIN, VOXEL, scene["small"] - np.float32(0.2))
    with_grid = b.collision_batch(_dev(q.T))[0].cpu().numpy()
    b.clear_world_grid()
    ca, fa = (t.cpu().numpy() for t in a.collision_batch(_dev(q.T)))
    cb, fb = (t.cpu().numpy() for t in b.collision_batch(_dev(q.T)))
    assert_bit_equal(cb, ca, "collision_batch after clear_world_grid")
    assert np.array_equal(fa, fb)
    assert (with_grid != ca).any()  # (the grid did something while it was set)
    ma = [t.cpu().numpy() for t in a.collision_motion_batch(_dev(qa.T), _dev(qb.T), 0.005)]
    mb = [t.cpu().numpy() for t in b.collision_motion_batch(_dev(qa.T), _dev(qb.T), 0.005)]
    assert_bit_equal(mb[0], ma[0], "collision_motion_batch after clear_world_grid")
    for k in (1, 2, 3):
        assert np.array_equal(ma[k], mb[k]), k
    # set_world leaves the grid alone
    b.set_world_grid(SMALL_ORIGIN, VOXEL, scene["small"] - np.float32(0.2))
    b.set_world(scene["sph"], scene["box"])
    assert_bit_equal(b.collision_batch(_dev(q.T))[0].cpu().numpy(), with_grid, "set_world keeps the grid")


def test_motion_batch_equals_the_composition(chains, scene):
    from test_gpu_collision_motion import compose
    from optik_amd import device
    d = chains["panda"][0]
    hc = device.HipChain(**d)
    hc.set_collision_model(**model_of("panda"))
    hc.set_world(spheres=scene["sph"][:1])
    hc.set_world_grid(ORIGIN, VOXEL, scene["big"])
    hc._test_margin = MARGIN
    B, h = 200, 0.005
    qa, qb = _segments(d, B, seed=6)
    want = compose(hc, qa, qb, h)
    got = [t.cpu().numpy() for t in hc.collision_motion_batch(_dev(qa.T), _dev(qb.T), h)]
    cls = [t.cpu().numpy() for t in hc.collision_motion_batch(_dev(qa.T), _dev(qb.T), h, clearance=False)[1:]]
    assert_bit_equal(got[0], want[0], "motion clearance")
    for k, what in ((1, "free"), (2, "first"), (3, "steps")):
        assert np.array_equal(got[k], want[k]), what
        assert np.array_equal(cls[k - 1], want[k]), "classify-only " + what
    K = want[3]
    assert (K == 1).any() and ((K > 1) & (K < 30)).any() and (K >= 250).any()
    assert 0.0 < want[1].mean() < 1.0, want[1].mean()


def test_filter_end_to_end_in_a_grid_only_world(oracle, chains):
    """The winner of a filtered launch in a world that is a grid alone: the (key, index) minimum over the successes the
    grid leaves free, selected on the host from the oracle's per-restart results (tests/test_gpu_ik_collision.py)."""
    from test_gpu_ik_collision import candidates, check_batch
    from optik_amd import _native as nat
    from optik_amd import device
    d, ch = chains["panda"]
    hc = device.HipChain(**d)
    from optik_amd.collision import auto_pairs, spheres_along_chain
    frames, centers, radii = spheres_along_chain(_robot("panda"), 0.04, 4)
    hc.set_collision_model(frames, centers, radii, self_pairs=auto_pairs(frames), margin=MARGIN)
    T, R = 4, 256
    tg, x0 = make_targets(oracle, d, ch, np.random.default_rng(77), T)
    cfg = nat.make_config(solution_mode="quality")
    before = _np(hc.ik_batch(cfg, _dev(tg), _dev(x0), 0, R, per_restart=False))
    assert before["win_idx"][0] >= 0
    # a wall of 10 cm through the elbow of target 0's winner, baked at 5 cm; then the primitives go
    xw = before["win_x"][0]
    elbow = hc.link_frames_batch(_dev(xw[:, None]))[0, 4, :3].cpu().numpy()
    hc.set_world(boxes=[np.concatenate([elbow, [0.0, 0.0, 0.0, 1.0], [0.05, 0.25, 0.25]])])
    field = hc.bake_world_grid([-1.5, -1.5, -1.5], 0.05, (61, 61, 61))
    hc.set_world()
    hc.set_world_grid([-1.5, -1.5, -1.5], 0.05, field)
    assert hc.collision_batch(_dev(xw[:, None]))[0].item() < MARGIN
    rejected = 0
    for mode in ("quality", "speed"):
        got, found = check_batch(oracle, chains, hc, "panda", mode, tg, x0, 0, R, None, f"grid world {mode}")
        assert found >= 1
        won = got["win_idx"] >= 0
        clr, free = hc.collision_batch(_dev(got["win_x"][won].T))
        assert bool((clr >= MARGIN).all()) and bool(free.all())
        for t in range(T):
            every = candidates(oracle, hc, ch, mode, tg[t], x0[t], 0, R, None, free_only=False)
            rejected += len(every) - len(candidates(oracle, hc, ch, mode, tg[t], x0[t], 0, R, None))
    assert rejected >= 1, "no success was rejected by the grid: the test would pass without the filter"
    after = _np(hc.ik_batch(cfg, _dev(tg), _dev(x0), 0, R, per_restart=False))
    assert after["win_idx"][0] != before["win_idx"][0]
    # one path of 8 waypoints on the seed's side of the wall, with the motion check on: every waypoint it accepts is
    # free under the grid, and so is the move to it from the waypoint before
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    rng = np.random.default_rng(8)
    L, h = 8, 0.02
    for _ in range(200):
        qa = rng.uniform(lb, ub)
        qb = np.clip(qa + rng.uniform(-0.4, 0.4, 7), lb, ub)
        qs = np.array([(1.0 - s) * qa + s * qb for s in np.linspace(0.0, 1.0, L)])
        if bool(hc.collision_motion_batch(_dev(qs[:-1].T), _dev(qs[1:].T), h)[1].all()):
            break
    else:
        raise AssertionError("no free joint-space line found")
    ptg = np.array([oracle.fk(ch, qq)[1] for qq in qs])[:, None, :]
    hc.set_motion_resolution(h)
    path = _np(hc.ik_path(nat.make_config(solution_mode="quality"), _dev(ptg), _dev(qa[None]), 0, 64, math.inf))
    ok = path["idx"][:, 0] >= 0
    assert ok.sum() >= L // 2, path["idx"][:, 0]
    seeds, xs = [], []
    c = qa
    for w in range(L):
        if ok[w]:
            seeds.append(c); xs.append(path["x"][w, 0])
            c = path["x"][w, 0]
    _, mfree, _, _ = hc.collision_motion_batch(_dev(np.array(seeds).T), _dev(np.array(xs).T), h)
    assert bool(mfree.all())
    assert bool(hc.collision_batch(_dev(np.array(xs).T))[1].all())


def test_robot_surface_and_set_devices(chains, scene):
    """The robot's grid is the chain's, and it follows the robot onto the chains set_devices creates later (two logical
    chains on one GPU)."""
    from optik_amd import SolverConfig
    from optik_amd import device
    d = chains["panda"][0]
    m = model_of("panda")
    hc = device.HipChain(**d)
    hc.set_collision_model(**m)
    hc.set_world(spheres=scene["sph"][:1])
    hc.set_world_grid(ORIGIN, VOXEL, scene["big"])
    robots = []
    for devices in (None, [0, 0]):
        r = _robot("panda")
        r.set_collision_model(**m)
        r.set_world(spheres=scene["sph"][:1])
        r.set_world_grid(ORIGIN, VOXEL, scene["big"].astype(np.float64))  # (before any device chain exists)
        if devices:
            r.set_devices(devices)
        robots.append(r)
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    rng = np.random.default_rng(17)
    T = 6
    qs = rng.uniform(lb, ub, size=(T, 7))
    clr_h = hc.collision_batch(_dev(qs.T))[0].cpu().numpy()
    for r in robots:
        assert_bit_equal(r.collision_clearance_batch_arrays(qs)[0], clr_h, "robot clearance under the grid")
    poses = np.array([robots[0].fk(q) for q in qs])
    x0 = rng.uniform(lb, ub, size=(T, 7))
    cfg = SolverConfig("quality", max_time=0.0, max_restarts=256)
    xs, fs, found = robots[0].ik_batch_arrays(cfg, poses, x0)
    assert found.sum() >= 2
    assert robots[0].collision_clearance_batch_arrays(xs[found])[1].all()
    x2, f2, found2 = robots[1].ik_batch_arrays(cfg, poses, x0)
    assert np.array_equal(found2, found)
    assert_bit_equal(x2, xs, "set_devices")
    # a grid set after the chains exist reaches them too; clearing restores the primitives' bits
    for r in robots:
        r.set_world_grid(SMALL_ORIGIN, VOXEL, scene["small"])
    hc.set_world_grid(SMALL_ORIGIN, VOXEL, scene["small"])
    clr_s = hc.collision_batch(_dev(qs.T))[0].cpu().numpy()
    x3 = [r.ik_batch_arrays(cfg, poses, x0) for r in robots]
    assert_bit_equal(robots[1].collision_clearance_batch_arrays(qs)[0], clr_s, "replaced grid")
    assert_bit_equal(x3[1][0], x3[0][0], "set_devices, replaced grid")
    hc.clear_world_grid()
    clr_p = hc.collision_batch(_dev(qs.T))[0].cpu().numpy()
    for r in robots:
        r.clear_world_grid()
        assert_bit_equal(r.collision_clearance_batch_arrays(qs)[0], clr_p, "cleared grid")


def test_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ik_world_grid.py"),
                          os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"],
                         env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    assert "all free: True" in res.stdout, res.stdout
