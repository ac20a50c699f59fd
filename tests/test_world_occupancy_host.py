"""CPU-only: from occupancy grids and point clouds to a distance-field world (optik_amd/csrc/collision_measure.hpp
steps 8 and 9, built with g++) bit for bit against numpy on brute-force integer squared distances, constructed cases
with exact answers, the exported symbols, and the refusals, which happen on the host before any device work."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import ROBOTS
from occupancy_util import (brute_d2, build_occupancy_measure, field_reference, special_points, voxelize_reference)

# (shape, fraction of occupied nodes): the shapes of the GPU tests
RANDOM_SHAPES = [((13, 9, 17), 0.05), ((5, 4, 130), 0.01), ((3, 70, 5), 0.02), ((2, 2, 2), 0.5)]


def random_occupancy(shape, fraction, seed):
    rng = np.random.default_rng(seed)
    occ = rng.random(shape) < fraction
    if not occ.any():
        occ.flat[rng.integers(occ.size)] = True
    return occ


def corner_occupancy():
    occ = np.zeros((1024, 2, 2), dtype=bool)
    occ[0, 0, 0] = True
    return occ


@pytest.fixture(scope="module")
def built():
    from optik_amd import build
    build.build()
    from optik_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def om(tmp_path_factory):
    return build_occupancy_measure(str(tmp_path_factory.mktemp("occupancy_measure")))


@pytest.fixture(scope="module")
def panda(built):
    from optik_amd import Robot
    return Robot.from_urdf_file(os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8")


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("shape,fraction", RANDOM_SHAPES)
def test_field_matches_numpy_on_brute_force_d2(om, shape, fraction):
    occ = random_occupancy(shape, fraction, 11)
    voxel = 0.07
    md = voxel * math.sqrt(sum(s * s for s in shape))
    d2o, d2f = brute_d2(occ), brute_d2(~occ)
    got = om.field(voxel, occ, md)
    assert _same_bits(got, field_reference(voxel, occ, md, d2o, d2f))
    assert np.isfinite(got).all() and (got[occ] < 0).all() and (got[~occ] > 0).all()
    # the test's own reference, where scipy is there to pin it
    try:
        from scipy.ndimage import distance_transform_edt
    except ImportError:
        return
    assert np.array_equal(d2o, np.rint(distance_transform_edt(~occ) ** 2).astype(np.int64))
    if not occ.all():
        assert np.array_equal(d2f, np.rint(distance_transform_edt(occ) ** 2).astype(np.int64))


def test_field_of_one_corner_node_on_the_longest_axis(om):
    occ = corner_occupancy()
    voxel = 2.0 ** -6
    md = voxel * math.sqrt(1024 ** 2 + 8)
    d2o = brute_d2(occ)
    assert d2o.max() == 1023 ** 2 + 2
    got = om.field(voxel, occ, md)
    assert _same_bits(got, field_reference(voxel, occ, md, d2o))
    assert got[1023, 1, 1] == np.float32(voxel * (math.sqrt(1023 ** 2 + 2) - 0.5))
    assert got[0, 0, 0] == np.float32(-0.5 * voxel)


def test_field_exact_cases(om):
    voxel, shape, i0 = 0.25, (9, 4, 5), 3
    md = 100.0
    plane = np.zeros(shape, dtype=bool)
    plane[i0] = True
    got = om.field(voxel, plane, md)
    for i in range(shape[0]):
        want = -0.5 * voxel if i == i0 else voxel * (abs(i - i0) - 0.5)
        assert (got[i] == np.float32(want)).all(), i
    # the zero level lies midway between a free node and its occupied neighbour
    assert got[i0 + 1, 0, 0] == -got[i0, 0, 0] == np.float32(voxel / 2)
    # no occupied node / no free node anywhere: the clamp itself, assigned
    assert (om.field(voxel, np.zeros(shape, dtype=bool), 0.7) == np.float32(0.7)).all()
    assert (om.field(voxel, np.ones(shape, dtype=bool), 0.7) == np.float32(-0.7)).all()
    # max_distance = 2.5 voxels clamps both signs: a thick slab (7 planes) in a long grid
    slab = np.zeros((16, 3, 3), dtype=bool)
    slab[2:9] = True
    got = om.field(voxel, slab, 2.5 * voxel)
    assert got.max() == np.float32(2.5 * voxel) and got.min() == np.float32(-2.5 * voxel)
    assert (got[13:] == np.float32(2.5 * voxel)).all()        # 4.5 voxels and more: clamped
    assert (got[5] == np.float32(-2.5 * voxel)).all()          # the middle plane, 4 nodes from the nearest free one
    assert (got[4] == np.float32(-2.5 * voxel)).all()          # 3 nodes: -(3 - 0.5), the clamp itself
    assert (got[3] == np.float32(-1.5 * voxel)).all()          # 2 nodes deep: not clamped
    assert (got[10] == np.float32(1.5 * voxel)).all()
    assert _same_bits(got, field_reference(voxel, slab, 2.5 * voxel))


def _cloud(origin, voxel, shape, n_random, seed):
    rng = np.random.default_rng(seed)
    span = voxel * np.asarray(shape)
    rnd = rng.uniform(origin - 0.2 * span, origin + 1.2 * span, (n_random, 3))
    return np.concatenate([special_points(origin, voxel, shape), rnd])


def test_voxelize_matches_numpy(om):
    origin, voxel, shape = np.array([1.0, -0.5, 0.25]), 0.25, (6, 5, 7)
    pts = _cloud(origin, voxel, shape, 400, 3)
    got = om.voxelize(origin, voxel, shape, pts)
    assert np.array_equal(got, voxelize_reference(origin, voxel, shape, pts))
    # constructed: a half-voxel boundary goes up, w = 0 is inside, w = n is outside
    mid = np.floor(np.asarray(shape) / 2).astype(int)
    one = om.voxelize(origin, voxel, shape, [origin + voxel * mid + 0.5 * voxel])
    assert one.sum() == 1 and one[tuple(mid + 1)]
    one = om.voxelize(origin, voxel, shape, [origin + voxel * mid - 0.5 * voxel])
    assert one.sum() == 1 and one[tuple(mid)]
    assert om.voxelize(origin, voxel, shape, [origin - 0.5 * voxel])[0, 0, 0]
    assert not om.voxelize(origin, voxel, shape, [origin + voxel * (np.asarray(shape) - 0.5)]).any()
    bad = [[math.nan, 0, 0.5], [1.5, math.inf, 0.5], [1.5, 0, -math.inf], [math.nan] * 3]
    assert not om.voxelize(origin, voxel, shape, bad).any()


def test_voxelize_exclusion_spheres(om):
    origin, voxel, shape = np.array([0.0, 0.0, 0.0]), 0.25, (8, 8, 8)
    c, r = np.array([1.0, 1.0, 1.0]), 0.625
    on = np.array([c + [r, 0, 0], c - [0, r, 0], c + [0, 0, r], c + [0.375, 0.5, 0.0]])  # exactly on the surface (3-4-5)
    off = np.array([c + [r + 2.0 ** -40, 0, 0], c + [0.5, 0.5, 0.0]])                    # just outside, and outside
    pts = np.concatenate([on, off, _cloud(origin, voxel, shape, 300, 4)])
    exclude = np.array([[*c, r], [math.nan, 1.0, 1.0, 0.5], [1.0, 1.0, 1.0, math.nan], [0.25, 1.5, 0.5, 0.3]])
    assert ((on - c) ** 2).sum(1).tolist() == [r * r] * 4
    got = om.voxelize(origin, voxel, shape, pts, exclude)
    assert np.array_equal(got, voxelize_reference(origin, voxel, shape, pts, exclude))
    # <= drops a point on the surface; a NaN sphere excludes nothing
    assert not om.voxelize(origin, voxel, shape, on, exclude[:1]).any()
    assert om.voxelize(origin, voxel, shape, off, exclude[:1]).sum() == 2
    assert np.array_equal(om.voxelize(origin, voxel, shape, on, exclude[1:3]), om.voxelize(origin, voxel, shape, on))
    # marks and never clears
    first = om.voxelize(origin, voxel, shape, pts[:50], exclude)
    both = om.voxelize(origin, voxel, shape, pts[50:], exclude, into=first)
    assert np.array_equal(both, got) and (both >= first).all()


def test_occupancy_symbols_are_exported(built):
    for s in ("optik_hip_world_grid_from_occupancy", "optik_hip_occupancy_from_points",
              "optik_robot_world_grid_from_occupancy", "optik_robot_occupancy_from_points"):
        assert hasattr(built, s), f"{s} is not exported by liboptik_amd.so"


def test_python_helpers():
    from optik_amd.collision import cloud_arrays, default_max_distance, occupancy_array
    assert default_max_distance(0.5, (3, 4, 12)) == 6.5
    occ = occupancy_array(np.arange(24).reshape(2, 3, 4).transpose(0, 1, 2) % 3)
    assert occ.dtype == np.uint8 and occ.flags.c_contiguous and set(np.unique(occ)) == {0, 1}
    p, e = cloud_arrays(np.zeros((5, 3), dtype=np.float32))
    assert p.dtype == np.float64 and e.shape == (0, 4)
    for bad in (dict(points=np.zeros((5, 2))), dict(points=np.zeros((5, 3)), exclude=np.zeros((2, 3)))):
        with pytest.raises(ValueError):
            cloud_arrays(**bad)
    with pytest.raises(ValueError):
        occupancy_array(np.zeros((2, 2)))


def test_refusals_happen_before_any_device_work(panda):
    """None of these calls touches a device (the robot has created no device context: no chain exists)."""
    ok = np.zeros((2, 3, 4), dtype=bool)
    for args, what in [
        ((0.1, np.zeros((1, 3, 4), dtype=bool)), r"2\.\.1024"),
        ((0.1, np.zeros((2, 3, 1025), dtype=bool)), r"2\.\.1024"),
        ((0.1, np.zeros((512, 512, 65), dtype=bool)), r"more than 2\^24"),
        ((0.0, ok), "voxel"),
        ((-0.1, ok), "voxel"),
        ((math.nan, ok), "voxel"),
        ((math.inf, ok), "voxel"),
        ((0.1, ok, 0.0), "max_distance"),
        ((0.1, ok, -1.0), "max_distance"),
        ((0.1, ok, math.nan), "max_distance"),
        ((0.1, ok, math.inf), "max_distance"),
    ]:
        with pytest.raises(ValueError, match=what):
            panda.world_grid_from_occupancy(*args)
    o, pts = [0.0, 0.0, 0.0], np.zeros((4, 3))
    for args, kw, what in [
        ((o, 0.1, (1, 3, 4), pts), {}, r"2\.\.1024"),
        ((o, 0.1, (2, 1025, 4), pts), {}, r"2\.\.1024"),
        ((o, 0.1, (512, 512, 65), pts), {}, r"more than 2\^24"),
        ((o, 0.0, (2, 3, 4), pts), {}, "voxel"),
        ((o, math.nan, (2, 3, 4), pts), {}, "voxel"),
        (([0.0, math.inf, 0.0], 0.1, (2, 3, 4), pts), {}, "origin"),
        ((o, 0.1, (2, 3, 4), pts), dict(exclude=np.zeros((1025, 4))), r"0\.\.1024"),
        ((o, 0.1, (2, 3, 4), pts), dict(exclude=[[0.0, math.nan, 0.0, 1.0]]), "non-finite exclusion sphere"),
        ((o, 0.1, (2, 3, 4), pts), dict(exclude=[[0.0, 0.0, 0.0, math.inf]]), "non-finite exclusion sphere"),
    ]:
        with pytest.raises(ValueError, match=what):
            panda.occupancy_from_points(*args, **kw)
        with pytest.raises(ValueError, match=what):
            panda.set_world_points(*args, **kw)
    # the C ABI itself: negative counts and null buffers that are needed; N = 0 needs none and does nothing
    L, h = panda._L, panda._h
    o3 = (C.c_double * 3)(0.0, 0.0, 0.0)
    p3 = (C.c_double * 12)()
    e4 = (C.c_double * 4)(0.0, 0.0, 0.0, 1.0)
    occ = (C.c_uint8 * 24)()
    val = (C.c_float * 24)()
    vp = lambda a: C.cast(a, C.c_void_p)
    assert L.optik_robot_occupancy_from_points(h, o3, 0.1, 2, 3, 4, vp(p3), -1, None, 0, vp(occ)) == -1
    assert L.optik_robot_occupancy_from_points(h, o3, 0.1, 2, 3, 4, vp(p3), 4, None, -1, vp(occ)) == -1
    assert L.optik_robot_occupancy_from_points(h, o3, 0.1, 2, 3, 4, None, 4, None, 0, vp(occ)) == -1
    assert L.optik_robot_occupancy_from_points(h, o3, 0.1, 2, 3, 4, vp(p3), 4, None, 1, vp(occ)) == -1
    assert L.optik_robot_occupancy_from_points(h, o3, 0.1, 2, 3, 4, vp(p3), 4, vp(e4), 1, None) == -1
    assert L.optik_robot_occupancy_from_points(h, None, 0.1, 2, 3, 4, vp(p3), 4, None, 0, vp(occ)) == -1
    assert L.optik_robot_occupancy_from_points(h, o3, 0.1, 2, 3, 4, None, 0, None, 0, None) == 0
    assert L.optik_robot_world_grid_from_occupancy(h, 0.1, 2, 3, 4, None, 1.0, vp(val)) == -1
    assert L.optik_robot_world_grid_from_occupancy(h, 0.1, 2, 3, 4, vp(occ), 1.0, None) == -1
    assert bytes(occ) == bytes(24)
    # the kernel layer refuses the same before it looks at its chain's device: it needs a chain, so the GPU tests
    # repeat these (tests/test_gpu_world_occupancy.py)
