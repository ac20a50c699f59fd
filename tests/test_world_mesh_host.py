"""Mesh worlds on the host: optik_amd/csrc/mesh_measure.hpp compiled with g++ against an
independently formulated numpy reference and against constructed cases with exact answers, atan2m against
math.atan2, load_stl, the exported symbols and the refusals that happen before any device work.  No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import ROBOTS
from mesh_util import (box_sdf, box_triangles, build_mesh_measure, degenerate_triangles, field_reference, grid_nodes,
                       random_triangles, ulp_diff, write_stl_ascii, write_stl_binary)

# the grid of the constructed cases: no node lies on a face of the unit cube (or of the boxes inside it below)
ORIGIN, VOXEL, SHAPE = [-0.7131, -0.7131, -0.7131], 0.173, (14, 14, 14)
LO, HI = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
BIG = 100.0  # a max_distance that clamps nothing here


@pytest.fixture(scope="module")
def built():
    from optik_amd import build
    build.build()
    from optik_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def mm(tmp_path_factory):
    return build_mesh_measure(str(tmp_path_factory.mktemp("mesh_measure")))


@pytest.fixture(scope="module")
def panda(built):
    from optik_amd import Robot
    return Robot.from_urdf_file(os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8")


@pytest.fixture(scope="module")
def cube_field(mm):
    return mm.field(ORIGIN, VOXEL, SHAPE, box_triangles(LO, HI), BIG)


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("seed, shape, M", [(1, (9, 8, 7), 12), (2, (6, 11, 5), 30)])
def test_measure_matches_independent_numpy_reference(mm, seed, shape, M):
    """Ericson's closest point and np.arctan2 against the segment / face form and atan2m.  The two f64 formulations
    differ by ~1e-15, far below a float32 ulp (6e-8 relative), so only a rounding boundary can separate the float32
    values: at most one ulp apart; the sign is the same wherever |value| > 1e-6 -- and the seeds leave no node
    there, so that condition excludes nothing."""
    rng = np.random.default_rng(seed)
    tris = random_triangles(rng, M)
    origin, voxel = [-1.2137, -1.1911, -1.2291], 0.3173
    got = mm.field(origin, voxel, shape, tris, BIG)
    ref, _ = field_reference(origin, voxel, shape, tris, BIG)
    assert np.isfinite(got).all()
    assert (np.abs(got) > 1e-6).all() and (np.abs(ref) > 1e-6).all()
    assert ulp_diff(got, ref).max() <= 1
    assert np.array_equal(np.signbit(got), np.signbit(ref))


def test_closed_random_mesh_matches_reference_with_both_signs(mm):
    """The same comparison on a closed mesh (a box) among random triangles: inside nodes exist and agree."""
    rng = np.random.default_rng(3)
    tris = np.concatenate([random_triangles(rng, 6), box_triangles([-0.6, -0.5, -0.7], [0.5, 0.6, 0.4])])
    origin, voxel, shape = [-1.2137, -1.1911, -1.2291], 0.3173, (8, 8, 8)
    got = mm.field(origin, voxel, shape, tris, BIG)
    ref, _ = field_reference(origin, voxel, shape, tris, BIG)
    assert (np.abs(got) > 1e-6).all()
    assert (got < 0).any() and (got > 0).any()
    assert ulp_diff(got, ref).max() <= 1
    assert np.array_equal(np.signbit(got), np.signbit(ref))


def test_unit_cube_is_the_box_sdf(mm, cube_field):
    p = grid_nodes(ORIGIN, VOXEL, SHAPE)
    sdf = box_sdf(p, LO, HI)
    assert (np.abs(sdf) > 1e-3).all()  # the nodes avoid the faces
    want = sdf.astype(np.float32).reshape(SHAPE)
    assert ulp_diff(cube_field, want).max() <= 1
    interior = ((p > 0.0) & (p < 1.0)).all(1).reshape(SHAPE)
    assert interior.sum() == 5 ** 3 and (cube_field[interior] < 0).all() and (cube_field[~interior] > 0).all()
    # inward-oriented: the same field.  (A flipped triangle walks its edges from the other end, so a segment term may
    # round differently in f64, ~1e-16 relative: at most a float32 rounding boundary, one ulp; signs are identical.)
    flipped = mm.field(ORIGIN, VOXEL, SHAPE, box_triangles(LO, HI, flip=True), BIG)
    assert ulp_diff(flipped, cube_field).max() <= 1
    assert np.array_equal(np.signbit(flipped), np.signbit(cube_field))


def test_cube_with_a_face_removed_still_has_an_inside(mm):
    """The +z face is gone; node (7, 7, 5) at (0.498, 0.498, 0.152) sees the opening under 0.09 of the sphere: its
    winding number is 0.91 and it reads inside, 0.152 from the floor."""
    open_box = box_triangles(LO, HI, skip_face=5)
    assert len(open_box) == 10
    f = mm.field(ORIGIN, VOXEL, SHAPE, open_box, BIG)
    z = ORIGIN[2] + VOXEL * 5
    assert f[7, 7, 5] < 0 and abs(f[7, 7, 5] + z) < 1e-6
    assert (f[:, :, 0] > 0).all()  # below the floor: outside


def test_open_sheet_is_unsigned(mm):
    tri = np.array([[[0.1, 0.2, 0.3], [0.9, 0.3, 0.5], [0.4, 0.8, 0.2]]])
    f = mm.field(ORIGIN, VOXEL, SHAPE, tri, BIG)
    assert (f >= 0).all() and np.isfinite(f).all()
    ref, _ = field_reference(ORIGIN, VOXEL, SHAPE, tri, BIG)
    assert ulp_diff(f, ref).max() <= 1


def test_cavity_reads_outside(mm):
    """A cube shell: the outer surface outward, the inner cube [0.3, 0.7]^3 oriented the other way.  Nodes in the
    cavity have winding number 0 and read positive; nodes in the wall read negative."""
    ilo, ihi = [0.3, 0.3, 0.3], [0.7, 0.7, 0.7]
    shell = np.concatenate([box_triangles(LO, HI), box_triangles(ilo, ihi, flip=True)])
    f = mm.field(ORIGIN, VOXEL, SHAPE, shell, BIG)
    p = grid_nodes(ORIGIN, VOXEL, SHAPE)
    cavity = ((p > 0.3) & (p < 0.7)).all(1).reshape(SHAPE)
    wall = ((p > 0.0) & (p < 1.0)).all(1).reshape(SHAPE) & ~cavity
    assert cavity.sum() == 3 ** 3 and wall.sum() == 5 ** 3 - 3 ** 3
    assert (f[cavity] > 0).all() and (f[wall] < 0).all() and (f[~cavity & ~wall] > 0).all()
    want = np.maximum(box_sdf(p, LO, HI), -box_sdf(p, ilo, ihi)).astype(np.float32).reshape(SHAPE)
    assert ulp_diff(f, want).max() <= 1


def test_nodes_on_a_vertex_and_in_a_face_read_zero(mm):
    """Dyadic grid and box: node (2, 2, 2) is the box's corner (0.25, 0.25, 0.25) and node (3, 4, 2) lies in the
    interior of its -z face, off the diagonal the face's two triangles share."""
    f = mm.field([0.0, 0.0, 0.0], 0.125, (9, 9, 9), box_triangles([0.25] * 3, [0.75] * 3), BIG)
    assert np.isfinite(f).all()
    assert f[2, 2, 2] == 0 and f[3, 4, 2] == 0
    assert f[4, 4, 4] == np.float32(-0.25) and f[0, 4, 4] == np.float32(0.25)


def test_degenerate_triangles_change_nothing(mm, cube_field):
    """A zero-area triangle (three collinear points along a cube edge) and one with three equal vertices (a cube
    corner) lie on the surface: every value is finite and the field is the cube's, bit for bit.  Elsewhere in space
    they are finite too and count as the segment and the point they are."""
    on_surface = np.array([[[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [1.0, 0.0, 0.0]],
                           [[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [1.0, 1.0, 0.0]]])
    for tris in (np.concatenate([box_triangles(LO, HI), on_surface]), np.concatenate([on_surface, box_triangles(LO, HI)])):
        f = mm.field(ORIGIN, VOXEL, SHAPE, tris, BIG)
        assert np.isfinite(f).all() and _same_bits(f, cube_field)
    free = mm.field(ORIGIN, VOXEL, SHAPE, degenerate_triangles(), BIG)
    assert np.isfinite(free).all() and (free >= 0).all()
    p = grid_nodes(ORIGIN, VOXEL, SHAPE)
    a, c = degenerate_triangles()[0][0], degenerate_triangles()[0][2]
    s = np.clip(((p - a) @ (c - a)) / ((c - a) @ (c - a)), 0.0, 1.0)
    d_seg = np.linalg.norm(p - (a + s[:, None] * (c - a)), axis=1)
    d_pt = np.linalg.norm(p - degenerate_triangles()[1][0], axis=1)
    assert ulp_diff(free, np.minimum(d_seg, d_pt).astype(np.float32).reshape(SHAPE)).max() <= 1


def test_max_distance_clamps_both_signs(mm, cube_field):
    md = 0.1
    f = mm.field(ORIGIN, VOXEL, SHAPE, box_triangles(LO, HI), md)
    assert _same_bits(f, np.clip(cube_field.astype(np.float64), -md, md).astype(np.float32))
    assert f.min() == np.float32(-md) and f.max() == np.float32(md)
    assert (cube_field.min() < -md) and (cube_field.max() > md)


def test_atan2m_against_libm(mm):
    """|atan2m - math.atan2| <= 4.5e-16, one ulp at pi, on every quadrant, the axes and the origin."""
    mags = [0.0, 1e-300, 1e-8, 0.3, 0.4375, 0.5, 0.6875, 1.0, 1.1875, 2.0, 2.4375, 3.0, 1e8, 1e300]
    signed = sorted({s * m for m in mags for s in (1.0, -1.0) if m > 0.0} | {0.0})
    pts = [(y, x) for y in signed for x in signed] + [(0.0, 0.0), (0.0, -1.0), (1.0, 0.0), (-1.0, 0.0)]
    th = np.linspace(-math.pi, math.pi, 4001)
    pts += [(math.sin(t) * r, math.cos(t) * r) for t in th for r in (1.0, 37.5)]
    rng = np.random.default_rng(5)
    pts += [tuple(v) for v in rng.normal(size=(20000, 2))]
    y, x = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
    y, x = y + 0.0, x + 0.0  # (no -0.0: atan2m takes y == 0 and x >= 0 by value, libm by sign bit)
    got = mm.atan2m(y, x)
    want = np.array([math.atan2(a, b) for a, b in zip(y, x)])
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= 4.5e-16
    for (a, b), v in {(0.0, 0.0): 0.0, (0.0, -1.0): math.pi, (1.0, 0.0): math.pi / 2, (-1.0, 0.0): -math.pi / 2,
                      (0.0, 1.0): 0.0}.items():
        assert mm.atan2m([a], [b])[0] == v


def test_load_stl(tmp_path):
    from optik_amd.collision import load_stl
    rng = np.random.default_rng(7)
    tris = rng.normal(size=(37, 3, 3))
    f32 = tris.astype(np.float32)
    pb, pa, ps, pt = (str(tmp_path / n) for n in ("b.stl", "a.stl", "solid.stl", "trunc.stl"))
    write_stl_binary(pb, tris, header=b"binary mesh")
    got = load_stl(pb)
    assert got.dtype == np.float64 and got.shape == (37, 3, 3) and np.array_equal(got, f32.astype(np.float64))
    write_stl_ascii(pa, tris)  # repr-exact digits: the float64 values themselves come back
    got = load_stl(pa)
    assert got.dtype == np.float64 and got.shape == (37, 3, 3) and np.array_equal(got, tris)
    # a binary file whose header starts with "solid" is still binary: the size decides
    write_stl_binary(ps, tris, header=b"solid made by some CAD exporter")
    assert np.array_equal(load_stl(ps), f32.astype(np.float64))
    data = open(pb, "rb").read()
    for cut in (len(data) - 7, 84, 50, 0):
        with open(pt, "wb") as fh:
            fh.write(data[:cut])
        with pytest.raises(ValueError):
            load_stl(pt)
    text = open(pa).read()
    with open(pt, "w") as fh:
        fh.write(text[:len(text) // 2])
    with pytest.raises(ValueError):
        load_stl(pt)


def test_mesh_arrays():
    from optik_amd.collision import mesh_arrays
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    t = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int16)
    soup = mesh_arrays(v, t)
    assert soup.dtype == np.float64 and soup.shape == (2, 9) and soup.flags.c_contiguous
    assert np.array_equal(soup.reshape(2, 3, 3), v.astype(np.float64)[t])
    assert np.array_equal(mesh_arrays(soup.reshape(2, 3, 3)), soup) and np.array_equal(mesh_arrays(soup), soup)
    for bad in (dict(vertices=v), dict(vertices=v, triangles=[[0, 1, 4]]), dict(vertices=v, triangles=[[0, 1, -1]]),
                dict(vertices=v, triangles=[[0.0, 1.0, 2.0]]), dict(vertices=v, triangles=[[0, 1]]),
                dict(vertices=np.zeros((4, 2)), triangles=t), dict(vertices=np.zeros((2, 3, 2)))):
        with pytest.raises(ValueError):
            mesh_arrays(**bad)


def test_mesh_symbols_are_exported(built):
    for s in ("optik_hip_world_grid_from_mesh", "optik_robot_world_grid_from_mesh", "optik_hip_mesh_tile",
              "optik_hip_mesh_pairs_per_launch"):
        assert hasattr(built, s), f"{s} is not exported by liboptik_amd.so"
    from optik_amd import _native
    assert _native.mesh_tile() >= 1
    # the launch bound is a process-wide test hook: set for a block, restored after it
    before = built.optik_hip_mesh_pairs_per_launch(-1)
    assert before >= 1
    with _native.mesh_pairs_per_launch(12345):
        assert built.optik_hip_mesh_pairs_per_launch(-1) == 12345
    assert built.optik_hip_mesh_pairs_per_launch(-1) == before


def test_refusals_happen_before_any_device_work(panda):
    """None of these calls touches a device (the robot has created no device context: no chain exists)."""
    o, shape = [0.0, 0.0, 0.0], (2, 3, 4)
    tri = box_triangles(LO, HI)
    nan_tri = tri.copy()
    nan_tri[5, 1, 2] = math.nan
    inf_tri = tri.copy()
    inf_tri[11, 2, 0] = -math.inf
    verts = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    for args, kw, what in [
        ((o, 0.1, shape, np.zeros((0, 3, 3))), {}, r"1\.\.2\^20"),                      # M = 0
        ((o, 0.1, shape, np.zeros(((1 << 20) + 1, 3, 3))), {}, r"1\.\.2\^20"),          # M too large
        ((o, 0.1, shape, nan_tri), {}, "triangle 5 has a NaN or infinite"),
        ((o, 0.1, shape, inf_tri), {}, "triangle 11 has a NaN or infinite"),
        ((o, 0.1, (1, 3, 4), tri), {}, r"2\.\.1024"),                                   # a bad grid
        ((o, 0.1, (2, 1025, 4), tri), {}, r"2\.\.1024"),
        ((o, 0.1, (512, 512, 65), tri), {}, r"more than 2\^24"),
        ((o, 0.0, shape, tri), {}, "voxel"),
        ((o, math.nan, shape, tri), {}, "voxel"),
        (([0.0, math.inf, 0.0], 0.1, shape, tri), {}, "origin"),
        ((o, 0.1, shape, tri), dict(max_distance=0.0), "max_distance"),
        ((o, 0.1, shape, tri), dict(max_distance=-1.0), "max_distance"),
        ((o, 0.1, shape, tri), dict(max_distance=math.nan), "max_distance"),
        ((o, 0.1, shape, tri), dict(max_distance=math.inf), "max_distance"),
        ((o, 0.1, shape, verts), dict(triangles=[[0, 1, 3]]), "vertex index"),         # an index out of range
        ((o, 0.1, shape, verts), dict(triangles=[[0, -1, 2]]), "vertex index"),
    ]:
        with pytest.raises(ValueError, match=what):
            panda.world_grid_from_mesh(*args, **kw)
        with pytest.raises(ValueError, match=what):
            panda.set_world_mesh(*args, **kw)
    # the C ABI itself: each of these returns -1
    L, h = panda._L, panda._h
    o3 = (C.c_double * 3)(0.0, 0.0, 0.0)
    t9 = (C.c_double * 18)(*([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0] * 2))
    val = (C.c_float * 24)()
    vp = lambda a: C.cast(a, C.c_void_p)
    f = L.optik_robot_world_grid_from_mesh
    assert f(h, o3, 0.1, 2, 3, 4, None, 2, 1.0, vp(val)) == -1          # null buffers
    assert f(h, o3, 0.1, 2, 3, 4, vp(t9), 2, 1.0, None) == -1
    assert f(h, None, 0.1, 2, 3, 4, vp(t9), 2, 1.0, vp(val)) == -1
    assert f(None, o3, 0.1, 2, 3, 4, vp(t9), 2, 1.0, vp(val)) == -1
    assert f(h, o3, 0.1, 2, 3, 4, vp(t9), 0, 1.0, vp(val)) == -1        # M = 0, negative, too large
    assert f(h, o3, 0.1, 2, 3, 4, vp(t9), -1, 1.0, vp(val)) == -1
    assert f(h, o3, 0.1, 2, 3, 4, vp(t9), (1 << 20) + 1, 1.0, vp(val)) == -1
    assert f(h, o3, 0.1, 1, 3, 4, vp(t9), 2, 1.0, vp(val)) == -1        # a bad grid
    assert f(h, o3, 0.1, 2, 3, 4, vp(t9), 2, 0.0, vp(val)) == -1        # max_distance <= 0
    assert f(h, o3, 0.1, 2, 3, 4, vp(t9), 2, -2.0, vp(val)) == -1
    t9[13] = math.nan
    assert f(h, o3, 0.1, 2, 3, 4, vp(t9), 2, 1.0, vp(val)) == -1        # a NaN vertex
    assert bytes(val) == bytes(96)
