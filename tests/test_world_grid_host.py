"""CPU-only: the distance-field world's arithmetic (optik_amd/csrc/collision_measure.hpp steps 5 - 7, built with g++)
against numpy and against constructed cases with exact answers, the exported symbols, and the refusals of a grid, which
happen on the host before any device work."""
import math
import os

import numpy as np
import pytest

from conftest import ROBOTS
from grid_util import build_grid_measure


@pytest.fixture(scope="module")
def built():
    from optik_amd import build
    build.build()
    from optik_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def gm(tmp_path_factory):
    return build_grid_measure(str(tmp_path_factory.mktemp("grid_measure")))


@pytest.fixture(scope="module")
def panda(built):
    from optik_amd import Robot
    return Robot.from_urdf_file(os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8")


def _np_trilinear(p, origin, voxel, values):
    """The textbook weighted sum of the 8 corners (another operation order than the header's nested lerps)."""
    n = np.array(values.shape)
    u = (p - origin) / voxel
    i = np.minimum(np.floor(u).astype(int), n - 2)
    f = u - i
    total = 0.0
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                w = (f[0] if a else 1 - f[0]) * (f[1] if b else 1 - f[1]) * (f[2] if c else 1 - f[2])
                total += w * float(values[i[0] + a, i[1] + b, i[2] + c])
    return total


def test_grid_distance_matches_numpy(gm):
    rng = np.random.default_rng(5)
    shape = (5, 6, 7)  # unequal, so that a mixed-up stride shows
    values = rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    origin, voxel = np.array([-0.3, 0.2, -0.1]), 0.07
    N = 3000
    hi = origin + voxel * (np.array(shape) - 1)
    p = rng.uniform(origin, hi, (N, 3))
    r = rng.uniform(0.0, 0.2, N)
    got = gm.grid_distance(p, r, origin, voxel, values)
    want = np.array([_np_trilinear(p[k], origin, voxel, values) for k in range(N)]) - r
    # The margin: the value scale is V = max|value| <= 1.  u = (p - origin) * inv carries about 2 roundings at a
    # magnitude of up to 6, so f is off by up to ~2 * 6 * eps, and one unit of f moves a lerp by up to 2 V, on three
    # axes: 72 eps V.  The seven lerps of three operations each on numbers of at most 2 V add at most 7 * 3 * 2 eps V
    # = 42 eps V, the subtraction of r one more; numpy's own weighted sum errs by as much again.  256 eps V covers
    # both sides; a wrong corner or stride is off by a large part of V.
    eps = 2.0 ** -52
    bound = 256 * eps * max(1.0, float(np.abs(values).max()))
    assert np.isfinite(got).all()
    assert (np.abs(got - want) <= bound).all(), np.abs(got - want).max() / eps


def test_grid_distance_exact_cases(gm):
    # dyadic everything: values k / 8, origin (1, 1, 1), voxel 1 / 4 (inv = 4 exactly)
    rng = np.random.default_rng(6)
    shape = (3, 4, 5)
    values = (rng.integers(-16, 17, shape) / 8.0).astype(np.float32)
    v64 = values.astype(np.float64)
    origin, voxel = np.array([1.0, 1.0, 1.0]), 0.25
    top = origin + voxel * (np.array(shape) - 1)  # (1.5, 1.75, 2.0)
    pts, want = [], []
    # on a node
    pts.append(origin + voxel * np.array([1, 2, 3])); want.append(v64[1, 2, 3])
    pts.append(origin.copy()); want.append(v64[0, 0, 0])
    # on the upper boundary (u = n - 1: cell n - 2 with f = 1), on all axes and on one axis at a time
    pts.append(top.copy()); want.append(v64[2, 3, 4])
    pts.append(np.array([top[0], 1.25, 1.5])); want.append(v64[2, 1, 2])
    pts.append(np.array([1.25, top[1], 1.5])); want.append(v64[1, 3, 2])
    pts.append(np.array([1.25, 1.5, top[2]])); want.append(v64[1, 2, 4])
    # a cell centre: the mean of its 8 corners (exact: dyadic values, f = 1 / 2)
    pts.append(origin + voxel * np.array([1.5, 2.5, 3.5])); want.append(v64[1:3, 2:4, 3:5].sum() / 8.0)
    pts.append(origin + voxel * np.array([0.5, 0.5, 0.5])); want.append(v64[0:2, 0:2, 0:2].sum() / 8.0)
    # half way along z only, on a node in x and y
    pts.append(origin + voxel * np.array([1, 2, 2.5])); want.append((v64[1, 2, 2] + v64[1, 2, 3]) / 2.0)
    pts, want = np.array(pts), np.array(want)
    got = gm.grid_distance(pts, 0.0, origin, voxel, values)
    assert np.array_equal(got, want), (got, want)
    got_r = gm.grid_distance(pts, 0.125, origin, voxel, values)
    assert np.array_equal(got_r, want - 0.125)
    # one ulp outside, on each side of each axis: the grid says nothing (+inf).  (p - origin is exact here: p lies
    # within a factor of two of the origin's coordinates, so the ulp survives the subtraction)
    inside = origin + voxel * np.array([1, 1, 1])
    outs = []
    for a in range(3):
        lo, hi = inside.copy(), inside.copy()
        lo[a] = np.nextafter(origin[a], -math.inf)
        hi[a] = np.nextafter(top[a], math.inf)
        outs += [lo, hi]
    assert (gm.grid_distance(np.array(outs), 0.0, origin, voxel, values) == math.inf).all()
    # ... and exactly on those boundaries it does
    ons = []
    for a in range(3):
        lo, hi = inside.copy(), inside.copy()
        lo[a] = origin[a]
        hi[a] = top[a]
        ons += [lo, hi]
    assert np.isfinite(gm.grid_distance(np.array(ons), 0.0, origin, voxel, values)).all()
    # a NaN centre reads nothing
    assert gm.grid_distance(np.array([[math.nan, 1.25, 1.25]]), 0.0, origin, voxel, values)[0] == math.inf


def test_clearance_grid_is_the_minimum_over_the_spheres(gm):
    rng = np.random.default_rng(7)
    shape = (5, 6, 7)
    values = rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    origin, voxel = np.array([-0.5, -0.5, -0.5]), 0.2
    ident = [0.0, 0.0, 0.0, 1.0]
    frames = np.array([[[0, 0, 0] + ident, [0.1, 0.2, 0.3] + ident]])
    centers = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.1], [5.0, 0.0, 0.0]])  # (the last one: outside the grid)
    radii = np.array([0.05, 0.1, 0.2])
    got = gm.clearance_grid(frames, [0, 1, 1], centers, radii, origin, voxel, values)
    pts = np.array([[0.0, 0.0, 0.0], [0.1 + 0.1, 0.2, 0.3 + 0.1]])
    terms = gm.grid_distance(pts, radii[:2], origin, voxel, values)
    assert got[0] == terms.min()
    # only the outside sphere: +inf; a NaN frame: NaN
    assert gm.clearance_grid(frames, [1], centers[2:], radii[2:], origin, voxel, values)[0] == math.inf
    bad = frames.copy()
    bad[0, 0, 4] = math.nan
    assert math.isnan(gm.clearance_grid(bad, [0, 1, 1], centers, radii, origin, voxel, values)[0])


def test_baked_field_of_a_dyadic_box_and_sphere(gm):
    ident = [0.0, 0.0, 0.0, 1.0]
    box = np.array([0.5, -0.25, 1.0] + ident + [0.25, 0.5, 0.125])
    sph = np.array([4.5, -0.25, 1.0, 1.0])
    origin, voxel, shape = np.array([-0.5, -1.25, 0.0]), 0.25, (24, 12, 9)
    field = gm.bake(origin, voxel, shape, [sph], [box])
    assert field.dtype == np.float32 and field.shape == shape
    # node (i, j, k) = (-0.5 + i / 4, -1.25 + j / 4, k / 4)
    assert field[4, 4, 4] == -0.125          # the box's centre: 0.125 inside its nearest (z) face
    assert field[7, 4, 4] == 0.5             # 0.5 off the box's +x face
    assert field[8, 10, 4] == 1.25           # off the box's edge by (0.75, 1.0): a 3-4-5 triangle
    assert field[20, 4, 4] == -1.0           # the sphere's centre
    assert field[23, 8, 4] == 0.25           # (0.75, 1.0) from the sphere's centre: 1.25 - 1
    assert field[16, 4, 4] == 0.0            # on the sphere
    assert field[5, 4, 4] == 0.0             # on the box's +x face
    # the whole field against numpy (the primitives themselves are tested in test_collision_host.py)
    ii, jj, kk = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")
    p = origin + voxel * np.stack([ii, jj, kk], -1)
    e = np.abs(p - box[:3]) - box[7:]
    dbox = np.linalg.norm(np.maximum(e, 0.0), axis=-1) + np.minimum(e.max(-1), 0.0)
    dsph = np.linalg.norm(p - sph[:3], axis=-1) - sph[3]
    want = np.minimum(dbox, dsph)
    # (f32 rounding of values below 8: half an ulp there is 2^-22; the f64 arithmetic adds ~1e-15)
    assert np.abs(field.astype(np.float64) - want).max() <= 2.0 ** -22 + 1e-12


def test_world_grid_symbols_are_exported(built):
    for s in ("optik_hip_chain_set_world_grid", "optik_hip_world_grid_bake", "optik_robot_set_world_grid",
              "optik_robot_world_grid_bake"):
        assert hasattr(built, s), f"{s} is not exported by liboptik_amd.so"


def test_grid_arrays_shapes():
    from optik_amd.collision import grid_arrays
    o, v, vals, shape = grid_arrays([0, 0, 0], 0.1, np.zeros((2, 3, 4), dtype=np.float64))
    assert o.dtype == np.float64 and vals.dtype == np.float32 and vals.flags.c_contiguous and shape == (2, 3, 4)
    # a transposed view is laid out again in C order, z fastest
    t = np.arange(24, dtype=np.float32).reshape(4, 3, 2).transpose(2, 1, 0)
    _, _, vals, shape = grid_arrays([0, 0, 0], 0.1, t)
    assert shape == (2, 3, 4) and vals.flags.c_contiguous and vals[1, 2, 3] == t[1, 2, 3]
    _, _, none, shape = grid_arrays([0, 0, 0], 0.1, shape=(5, 6, 7))
    assert none is None and shape == (5, 6, 7)
    for bad in (dict(origin=[0, 0], voxel=0.1, values=np.zeros((2, 2, 2))),
                dict(origin=[0, 0, 0], voxel=0.1, values=np.zeros((2, 2))),
                dict(origin=[0, 0, 0], voxel=0.1),
                dict(origin=[0, 0, 0], voxel=0.1, shape=(2, 2))):
        with pytest.raises(ValueError):
            grid_arrays(**bad)


def test_refusals_happen_before_any_device_work(panda):
    """None of these calls touches a device (the robot has created no device context: no chain exists)."""
    ok = np.zeros((2, 3, 4), dtype=np.float32)
    o = [0.0, 0.0, 0.0]
    nan_value, inf_value = ok.copy(), ok.copy()
    nan_value[1, 2, 3] = math.nan
    inf_value[0, 1, 0] = -math.inf
    for args, what in [
        ((o, 0.1, np.zeros((1, 3, 4))), r"2\.\.1024"),
        ((o, 0.1, np.zeros((2, 1, 4))), r"2\.\.1024"),
        ((o, 0.1, np.zeros((2, 3, 1025), dtype=np.float32)), r"2\.\.1024"),
        ((o, 0.1, np.zeros((1025, 2, 2), dtype=np.float32)), r"2\.\.1024"),
        ((o, 0.1, np.zeros((512, 512, 65), dtype=np.float32)), r"more than 2\^24"),
        ((o, 0.0, ok), "voxel"),
        ((o, -0.1, ok), "voxel"),
        ((o, math.nan, ok), "voxel"),
        ((o, math.inf, ok), "voxel"),
        (([0.0, math.nan, 0.0], 0.1, ok), "origin"),
        (([math.inf, 0.0, 0.0], 0.1, ok), "origin"),
        ((o, 0.1, nan_value), r"node \(1, 2, 3\) is NaN or infinite"),
        ((o, 0.1, inf_value), r"node \(0, 1, 0\) is NaN or infinite"),
        ((o, 0.1, np.full((2, 2, 2), 1e39)), "NaN or infinite"),  # (beyond float32: it arrives as +inf)
    ]:
        with pytest.raises(ValueError, match=what):
            panda.set_world_grid(*args)
    # the bake: the same geometry checks, and an empty world
    panda.set_world()
    for args, what in [
        ((o, 0.1, (1, 3, 4)), r"2\.\.1024"),
        ((o, 0.1, (2, 3, 1025)), r"2\.\.1024"),
        ((o, 0.1, (512, 512, 65)), r"more than 2\^24"),
        ((o, 0.0, (2, 3, 4)), "voxel"),
        (([0.0, 0.0, math.nan], 0.1, (2, 3, 4)), "origin"),
        ((o, 0.1, (2, 3, 4)), "no spheres and no boxes"),
    ]:
        with pytest.raises(ValueError, match=what):
            panda.bake_world_grid(*args)
    # accepted: the limits themselves (2 and 1024 per axis, exactly 2^24 nodes), then cleared
    panda.set_world_grid(o, 0.1, np.zeros((2, 2, 2)))
    panda.set_world_grid([-1.0, 2.0, 0.5], 1e-3, np.zeros((1024, 2, 2), dtype=np.float32))
    panda.set_world_grid(o, 0.1, np.zeros((256, 256, 256), dtype=np.float32))
    panda.clear_world_grid()
