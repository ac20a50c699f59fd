"""GPU: from occupancy grids and point clouds to a distance-field world -- the distance
transform and the voxelization of ik_occupancy.hip bit for bit against numpy on brute-force integer squared distances
(tests/occupancy_util.py), through HipChain and Robot; the self-filter; set_world_points end to end.  No tolerance
anywhere: every comparison is exact."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROBOT_SPECS, ROBOTS, ROOT
from gpu_util import assert_bit_equal
from occupancy_util import brute_d2, field_reference, special_points, voxelize_reference

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VOXEL = 0.07


def _robot(name="panda"):
    from optik_amd import Robot
    return Robot.from_urdf_file(*ROBOT_SPECS[name])


def _occupancy(shape, fraction, seed=11):
    rng = np.random.default_rng(seed)
    occ = rng.random(shape) < fraction
    if not occ.any():
        occ.flat[rng.integers(occ.size)] = True
    return occ


def _corner():
    occ = np.zeros((1024, 2, 2), dtype=bool)
    occ[0, 0, 0] = True
    return occ


def _diagonal(voxel, shape):
    return voxel * math.sqrt(sum(s * s for s in shape))


# name -> (occupancy, max_distance or None for the default)
CASES = {
    "13x9x17": lambda: (_occupancy((13, 9, 17), 0.05), None),        # z is not a multiple of anything
    "5x4x130": lambda: (_occupancy((5, 4, 130), 0.01), None),        # z spans three waves
    "3x70x5": lambda: (_occupancy((3, 70, 5), 0.02), None),          # lines with no source in the first pass
    "2x2x2": lambda: (_occupancy((2, 2, 2), 0.5), None),
    "corner": lambda: (_corner(), None),                             # the longest axis, D2 = 1023^2 + 2, the sentinel
    "all-free": lambda: (np.zeros((6, 5, 7), dtype=bool), 0.9),
    "all-occupied": lambda: (np.ones((6, 5, 7), dtype=bool), 0.9),
    "clamped": lambda: (_occupancy((13, 9, 17), 0.02, seed=5) | _slab((13, 9, 17)), 2.5 * VOXEL),
}


def _slab(shape):
    s = np.zeros(shape, dtype=bool)
    s[2:9, :, 3:12] = True  # thick enough for the negative clamp
    return s


@pytest.fixture(scope="module")
def references():
    """Every case's occupancy, clamp and numpy field from brute-force D2, computed once."""
    out = {}
    for name, make in CASES.items():
        occ, md = make()
        md = _diagonal(VOXEL, occ.shape) if md is None else md
        out[name] = (occ, md, field_reference(VOXEL, occ, md))
    ref = out["clamped"][2]
    assert ref.max() == np.float32(2.5 * VOXEL) and ref.min() == np.float32(-2.5 * VOXEL)
    assert brute_d2(out["corner"][0]).max() == 1023 ** 2 + 2
    return out


@pytest.fixture(scope="module")
def hc(chains):
    from optik_amd import device
    return device.HipChain(**chains["panda"][0])


@pytest.fixture(scope="module")
def panda():
    return _robot()


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def _chain_field(hc, occ, md, default=False):
    t = torch.tensor(occ.astype(np.uint8), device="cuda")
    out = hc.world_grid_from_occupancy(VOXEL, t, None if default else md)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_transform_equals_the_reference(hc, panda, references, name):
    occ, md, want = references[name]
    default = CASES[name]()[1] is None
    got = _chain_field(hc, occ, md, default)
    assert got.shape == occ.shape and np.isfinite(got).all()
    assert np.array_equal(_bits(got), _bits(want)), f"HipChain, {name}: {(got != want).sum()} nodes differ"
    got_r = panda.world_grid_from_occupancy(VOXEL, occ, None if default else md)
    assert np.array_equal(_bits(got_r), _bits(want)), f"Robot, {name}: {(got_r != want).sum()} nodes differ"


def test_transform_workspace_growth_and_reuse(chains, references):
    """A fresh chain: the small grid, then a larger one (the workspace grows), then the small one again (in a
    workspace that now holds the larger grid's leftovers)."""
    from optik_amd import device
    fresh = device.HipChain(**chains["panda"][0])
    for name in ("2x2x2", "13x9x17", "5x4x130", "2x2x2", "3x70x5", "13x9x17"):
        occ, md, want = references[name]
        assert np.array_equal(_bits(_chain_field(fresh, occ, md)), _bits(want)), name


def test_transform_on_a_side_stream(hc, references):
    occ, md, want = references["5x4x130"]
    side = torch.cuda.Stream()
    t = torch.tensor(occ.astype(np.uint8), device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out = hc.world_grid_from_occupancy(VOXEL, t, md)
    side.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))


def test_kernel_layer_refusals(hc):
    from optik_amd._native import OptikHipError
    occ = torch.zeros((2, 3, 4), dtype=torch.uint8, device="cuda")
    pts = torch.zeros((4, 3), dtype=torch.float64, device="cuda")
    for md in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(OptikHipError, match="max_distance"):
            hc.world_grid_from_occupancy(0.1, occ, md)
    for voxel in (0.0, -0.1, math.nan, math.inf):
        with pytest.raises(OptikHipError, match="voxel"):
            hc.world_grid_from_occupancy(voxel, occ)
        with pytest.raises(OptikHipError, match="voxel"):
            hc.occupancy_from_points([0, 0, 0], voxel, (2, 3, 4), pts)
    with pytest.raises(OptikHipError, match=r"2\.\.1024"):
        hc.world_grid_from_occupancy(0.1, torch.zeros((1, 3, 4), dtype=torch.uint8, device="cuda"))
    with pytest.raises(OptikHipError, match=r"2\.\.1024"):
        hc.occupancy_from_points([0, 0, 0], 0.1, (2, 1025, 2), pts)
    with pytest.raises(OptikHipError, match=r"more than 2\^24"):
        hc.occupancy_from_points([0, 0, 0], 0.1, (512, 512, 65), pts)
    with pytest.raises(OptikHipError, match="origin"):
        hc.occupancy_from_points([0, math.nan, 0], 0.1, (2, 3, 4), pts)
    with pytest.raises(OptikHipError, match=r"0\.\.1024"):
        hc.occupancy_from_points([0, 0, 0], 0.1, (2, 3, 4), pts,
                                 exclude=torch.zeros((1025, 4), dtype=torch.float64, device="cuda"))


def test_kernel_layer_refuses_counts_and_null_buffers(hc):
    """The refusals HipChain cannot express: negative counts and null buffers, by the C ABI on the chain's handle.
    Each is refused with OPTIK_HIP_EINVAL before any device work; N = 0 needs no buffer and does nothing."""
    import ctypes as C
    from optik_amd import _native as nat
    L = nat.lib()
    einval = -1  # OPTIK_HIP_EINVAL
    assert L.optik_hip_occupancy_from_points(hc._h, None, 0.1, 2, 3, 4, None, 0, None, 0, None, None) == einval  # origin
    o3 = (C.c_double * 3)(0.0, 0.0, 0.0)
    occ = torch.zeros((2, 3, 4), dtype=torch.uint8, device="cuda")
    val = torch.zeros((2, 3, 4), dtype=torch.float32, device="cuda")
    pts = torch.zeros((4, 3), dtype=torch.float64, device="cuda")
    exc = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())

    def points(N, E, d_pts=p(pts), d_exc=None, d_occ=p(occ)):
        return L.optik_hip_occupancy_from_points(hc._h, o3, 0.1, 2, 3, 4, d_pts, N, d_exc, E, d_occ, None)

    def message():
        return L.optik_hip_last_error().decode()

    assert points(-1, 0) == einval and "negative" in message()
    assert points(4, -1) == einval and "0..1024" in message()
    assert points(4, 1025, d_exc=p(exc)) == einval and "0..1024" in message()
    assert points(4, 0, d_pts=None) == einval and "null buffer" in message()
    assert points(4, 0, d_occ=None) == einval and "null buffer" in message()
    assert points(4, 1, d_exc=None) == einval and "null buffer" in message()   # E > 0 needs the spheres
    assert points(0, 0, d_pts=None, d_occ=None) == 0                            # N = 0: nothing is needed
    assert points(0, 1, d_pts=None, d_exc=None, d_occ=None) == 0
    assert points(4, 1, d_exc=p(exc)) == 0                                      # the same call with its buffers
    field = lambda d_occ, d_val, md=1.0: L.optik_hip_world_grid_from_occupancy(hc._h, 0.1, 2, 3, 4, d_occ, md, d_val,
                                                                              None)
    assert field(None, p(val)) == einval and "null buffer" in message()
    assert field(p(occ), None) == einval and "null buffer" in message()
    assert L.optik_hip_world_grid_from_occupancy(None, 0.1, 2, 3, 4, p(occ), 1.0, p(val), None) == einval
    assert field(p(occ), p(val)) == 0
    torch.cuda.synchronize()
    # the points (the origin, four times) lie in the sphere: nothing was marked by any of the calls above
    assert not occ.cpu().numpy().any()


# ---- voxelize ---------------------------------------------------------------------------------------------------------
# dyadic, so the special points are exact; 11 286 nodes, so the 5000 points leave most of them free
V_ORIGIN, V_VOXEL, V_SHAPE = np.array([1.0, -0.5, 0.25]), 0.25, (22, 19, 27)


def _cloud(N, seed):
    """N points: the special points of step 9 first (as many as fit), random ones in and around the grid after."""
    rng = np.random.default_rng(seed)
    span = V_VOXEL * np.asarray(V_SHAPE)
    sp = special_points(V_ORIGIN, V_VOXEL, V_SHAPE)[:N]
    rnd = rng.uniform(V_ORIGIN - 0.2 * span, V_ORIGIN + 1.2 * span, (N - len(sp), 3))
    return np.concatenate([sp, rnd])


def _exclusions(E, seed):
    """E spheres in the grid: a dyadic one first whose surface holds a point of the cloud of _cloud_on, then random
    ones, a NaN one among them."""
    if E == 0:
        return None
    rng = np.random.default_rng(seed)
    span = V_VOXEL * np.asarray(V_SHAPE)
    e = np.concatenate([rng.uniform(V_ORIGIN, V_ORIGIN + span, (E, 3)), rng.uniform(0.1, 0.5, (E, 1))], 1)
    e[0] = [1.5, 0.0, 1.0, 0.625]
    if E > 2:
        e[2, 1] = math.nan
    return e


ON_SURFACE = np.array([[1.5 + 0.625, 0.0, 1.0], [1.5 + 0.375, 0.5, 1.0], [1.5 + 0.625 + 2.0 ** -40, 0.0, 1.0]])


def _chain_voxelize(hc, pts, exc, into=None):
    out = hc.occupancy_from_points(V_ORIGIN, V_VOXEL, V_SHAPE, torch.tensor(pts, dtype=torch.float64, device="cuda"),
                                   None if exc is None else torch.tensor(exc, dtype=torch.float64, device="cuda"),
                                   into=into)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("N", [1, 257, 5000])
@pytest.mark.parametrize("E", [0, 1, 300])
def test_voxelize_equals_numpy(hc, panda, N, E):
    pts = np.concatenate([ON_SURFACE, _cloud(N, 3)])[:N] if N > 1 else ON_SURFACE[:1]
    exc = _exclusions(E, 4)
    want = voxelize_reference(V_ORIGIN, V_VOXEL, V_SHAPE, pts, exc)
    if N > 1:
        assert want.any() and not want.all()
    got = _chain_voxelize(hc, pts, exc).cpu().numpy()
    assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got.astype(bool), want), f"{(got.astype(bool) != want).sum()} nodes differ"
    if E != 300:  # (the robot layer refuses the NaN sphere that the 300 hold: its own test below)
        got_r = panda.occupancy_from_points(V_ORIGIN, V_VOXEL, V_SHAPE, pts, exc)
        assert got_r.dtype == bool and np.array_equal(got_r, want)


def test_voxelize_surface_points_and_robot_refusal(hc, panda):
    exc = _exclusions(1, 4)
    got = _chain_voxelize(hc, ON_SURFACE, exc).cpu().numpy().astype(bool)
    # the two points on the surface are dropped (<=), the one 2^-40 beyond it is kept
    assert got.sum() == 1 and np.array_equal(got, voxelize_reference(V_ORIGIN, V_VOXEL, V_SHAPE, ON_SURFACE[2:]))
    with pytest.raises(ValueError, match="non-finite exclusion sphere"):
        panda.occupancy_from_points(V_ORIGIN, V_VOXEL, V_SHAPE, ON_SURFACE, _exclusions(300, 4))
    finite = np.nan_to_num(_exclusions(300, 4), nan=0.3)
    pts = _cloud(5000, 3)
    assert np.array_equal(panda.occupancy_from_points(V_ORIGIN, V_VOXEL, V_SHAPE, pts, finite),
                          voxelize_reference(V_ORIGIN, V_VOXEL, V_SHAPE, pts, finite))


def test_voxelize_accumulates_and_n0(hc, panda):
    a, b = _cloud(257, 5)[40:], _cloud(300, 6)[40:]   # (random points only: sparse enough to differ)
    exc = _exclusions(1, 4)
    first = _chain_voxelize(hc, a, exc)
    want_a = voxelize_reference(V_ORIGIN, V_VOXEL, V_SHAPE, a, exc)
    assert np.array_equal(first.cpu().numpy().astype(bool), want_a)
    both = _chain_voxelize(hc, b, None, into=first)
    assert both is first
    want = voxelize_reference(V_ORIGIN, V_VOXEL, V_SHAPE, b, None, into=want_a)
    assert (want != want_a).any()
    assert np.array_equal(both.cpu().numpy().astype(bool), want)
    # N = 0: not an error, nothing changes
    again = _chain_voxelize(hc, np.zeros((0, 3)), exc, into=both)
    assert np.array_equal(again.cpu().numpy().astype(bool), want)
    assert not _chain_voxelize(hc, np.zeros((0, 3)), None).cpu().numpy().any()
    # the robot's form
    r_a = panda.occupancy_from_points(V_ORIGIN, V_VOXEL, V_SHAPE, a, exc)
    r_both = panda.occupancy_from_points(V_ORIGIN, V_VOXEL, V_SHAPE, b, into=r_a)
    assert np.array_equal(r_a, want_a) and np.array_equal(r_both, want)
    assert np.array_equal(panda.occupancy_from_points(V_ORIGIN, V_VOXEL, V_SHAPE, np.zeros((0, 3)), into=r_both), want)


# ---- the self-filter and the whole path ---------------------------------------------------------------------------------
W_ORIGIN, W_VOXEL, W_SHAPE = np.array([-1.0, -1.0, -0.5]), 0.0625, (33, 33, 33)   # [-1, 1]^2 x [-0.5, 1.5]


def _sphere_points(spheres, per, rng):
    d = rng.normal(size=(len(spheres), per, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return (spheres[:, None, :3] + spheres[:, None, 3:] * d).reshape(-1, 3)


def _scene_cloud(panda, x, model, rng):
    """What a camera would return of the robot itself (points on its model's spheres at x) and of one far cluster."""
    from optik_amd.collision import spheres_at
    own = spheres_at(panda, x, *model)
    self_pts = _sphere_points(own, 40, rng)
    far = np.array([0.55, -0.45, 0.9]) + rng.uniform(-0.08, 0.08, (200, 3))
    return self_pts, far


def test_spheres_at_against_fk_and_the_collision_filter():
    """spheres_at pinned by two things that do not go through it: fk's translation, and the filter's own clearance
    (the kernels place the spheres from quaternion frames; spheres_at rotates 4x4 frames in numpy).  The bound: both
    sides are f64 forward kinematics of one chain, whose coordinates are below 2 m and carry a few hundred roundings at
    most, so they agree to 1e-12 m; a transposed rotation or a wrong frame is off by centimetres."""
    from optik_amd.collision import spheres_at
    robot = _robot()
    n = robot.num_positions()
    x = np.array([0.3, -0.4, 0.2, -1.8, 0.1, 1.5, 0.6])
    tip = spheres_at(robot, x, [n + 1], [[0.0, 0.0, 0.0]], [0.03], pad=0.01)
    assert tip.shape == (1, 4) and tip[0, 3] == 0.03 + 0.01
    assert np.abs(tip[0, :3] - np.array(robot.fk(x))[:3, 3]).max() <= 1e-12
    # one model sphere at a time, off its frame's origin on all three axes; a world sphere 0.5 m beside where
    # spheres_at says it is: the clearance is 0.5 - r - R
    c, r, R = np.array([0.11, -0.07, 0.05]), 0.04, 0.1
    for f in range(n + 2):
        at = spheres_at(robot, x, [f], [c], [r])
        assert at[0, 3] == r
        robot.set_collision_model([f], [c], [r], self_pairs=None, margin=0.0)
        robot.set_world(spheres=[[at[0, 0] + 0.5, at[0, 1], at[0, 2], R]])
        assert abs(robot.collision_clearance(x) - (0.5 - r - R)) <= 1e-12, f


def test_self_filter_keeps_only_the_far_cluster(panda):
    from optik_amd.collision import spheres_along_chain, spheres_at
    model = spheres_along_chain(panda, 0.05, 12)
    rng = np.random.default_rng(8)
    x = np.array([0.3, -0.4, 0.2, -1.8, 0.1, 1.5, 0.6])
    self_pts, far = _scene_cloud(panda, x, model, rng)
    own = spheres_at(panda, x, *model)
    assert own.shape == (len(model[0]), 4) and (own[:, 3] == 0.05).all()
    # (the far cluster keeps clear of the padded model)
    assert (np.linalg.norm(far[:, None] - own[None, :, :3], axis=-1) > own[:, 3] + 0.02).all()
    cloud = np.concatenate([self_pts, far])
    want = voxelize_reference(W_ORIGIN, W_VOXEL, W_SHAPE, far)
    unfiltered = panda.occupancy_from_points(W_ORIGIN, W_VOXEL, W_SHAPE, cloud)
    assert unfiltered.sum() > want.sum() > 0
    exclude = spheres_at(panda, x, *model, pad=0.02)
    assert np.array_equal(exclude[:, :3], own[:, :3]) and np.array_equal(exclude[:, 3], own[:, 3] + 0.02)
    got = panda.occupancy_from_points(W_ORIGIN, W_VOXEL, W_SHAPE, cloud, exclude)
    assert np.array_equal(got, want)


def test_set_world_points_end_to_end():
    from optik_amd import SolverConfig
    from optik_amd.collision import auto_pairs, spheres_along_chain, spheres_at
    rng = np.random.default_rng(9)
    x_cam = np.array([0.3, -0.4, 0.2, -1.8, 0.1, 1.5, 0.6])
    robots = [_robot(), _robot()]
    frames, centers, radii = spheres_along_chain(robots[0], 0.05, 12)
    for r in robots:
        r.set_collision_model(frames, centers, radii, self_pairs=auto_pairs(frames), margin=0.01)
    self_pts, far = _scene_cloud(robots[0], x_cam, (frames, centers, radii), rng)
    cloud = np.concatenate([self_pts, far, [[math.nan, 0.0, 0.0]]])
    exclude = spheres_at(robots[0], x_cam, frames, centers, radii, pad=0.02)
    values = robots[0].set_world_points(W_ORIGIN, W_VOXEL, W_SHAPE, cloud, exclude)
    occ = robots[0].occupancy_from_points(W_ORIGIN, W_VOXEL, W_SHAPE, cloud, exclude)
    composed = robots[0].world_grid_from_occupancy(W_VOXEL, occ)
    assert values.dtype == np.float32 and np.array_equal(_bits(values), _bits(composed))
    assert (values < 0).sum() == occ.sum() > 0
    robots[1].set_world_grid(W_ORIGIN, W_VOXEL, values)

    lb, ub = (np.array(v) for v in robots[0].joint_limits())
    T = 8
    qs = rng.uniform(lb, ub, size=(T, 7))
    qb = rng.uniform(lb, ub, size=(T, 7))
    poses = np.array([robots[0].fk(q) for q in qs])
    x0 = rng.uniform(lb, ub, size=(T, 7))
    cfg = SolverConfig("quality", max_time=0.0, max_restarts=64)

    def everything(r):
        clr, free = r.collision_clearance_batch_arrays(qs)
        motion = r.collision_motion_batch_arrays(qs, qb, 0.05)
        xs, fs, found = r.ik_batch_arrays(cfg, poses, x0)
        return [clr, free, *motion, xs, fs, found]

    def same(a, b, what):
        for k, (u, v) in enumerate(zip(a, b)):
            u, v = np.asarray(u), np.asarray(v)
            if u.dtype == np.float64:
                assert_bit_equal(u, v, f"{what}, output {k}")
            else:
                assert np.array_equal(u, v), f"{what}, output {k}"

    first = everything(robots[0])
    assert np.isfinite(first[0]).all() and first[-1].any()
    same(first, everything(robots[1]), "set_world_points against set_world_grid(values)")
    # ... and on the chains set_devices creates (two logical chains on one GPU).  set_devices is refused after a
    # robot's first GPU call, so it never replaces chains that exist: "after set_devices" can only mean new robots
    # whose first chains are the ones set_devices asked for.  multi[0] gets its grid from the cloud on those chains;
    # multi[1] was handed the values before any chain existed, which shows an installed grid reaching them.
    multi = [_robot(), _robot()]
    for r in multi:
        r.set_collision_model(frames, centers, radii, self_pairs=auto_pairs(frames), margin=0.01)
    multi[1].set_world_grid(W_ORIGIN, W_VOXEL, values)
    for r in multi:
        r.set_devices([0, 0])
    again = multi[0].set_world_points(W_ORIGIN, W_VOXEL, W_SHAPE, cloud, exclude)
    assert np.array_equal(_bits(again), _bits(values))
    on_two = everything(multi[0])
    same(on_two, everything(multi[1]), "after set_devices")
    same(on_two, first, "set_devices against one chain")


def test_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ik_world_points.py"),
                          os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"],
                         env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    assert "all free: True" in res.stdout, res.stdout
