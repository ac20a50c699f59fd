"""Sphere models from collision geometry on the host: optik_amd/csrc/spherefit_measure.hpp
compiled with g++ against an independent numpy greedy and against solids with closed-form distances; surface_points,
primitive_mesh, urdf_collision_geometry, prune_pairs; the exported symbols and the refusals that happen before any
device work.  No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import ROBOTS, ROOT
from mesh_util import box_sdf, box_triangles, build_mesh_measure, write_stl_binary
from spherefit_util import (boundary_margin, build_spherefit, cover_matrix, grid_nodes, numpy_greedy, random_case,
                            unit_cube_case)

FIXTURE = os.path.join(ROOT, "tests", "golden", "robots", "arm_primitives.urdf")
UR3E = os.path.join(ROOT, "tests", "golden", "reference", "ur3e.urdf")


@pytest.fixture(scope="module")
def built():
    from optik_amd import build
    build.build()
    from optik_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def sf(tmp_path_factory):
    return build_spherefit(str(tmp_path_factory.mktemp("spherefit_measure")))


@pytest.fixture(scope="module")
def mm(tmp_path_factory):
    return build_mesh_measure(str(tmp_path_factory.mktemp("mesh_measure")))


@pytest.fixture(scope="module")
def panda(built):
    from optik_amd import Robot
    return Robot.from_urdf_file(os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8")


def _solid_case(mm, tris, lo, hi, voxel, spacing, pad):
    """The field and the samples Robot.fit_spheres would use, from the host builds: (values, origin, points)."""
    from optik_amd.collision import fit_grid, surface_points
    origin, shape = fit_grid(lo, hi, voxel, pad)
    values = mm.field(origin, voxel, shape, tris, 100.0)
    return values, origin, surface_points(tris, None, spacing)


@pytest.fixture(scope="module")
def cube(mm):
    tris, lo, hi, voxel, spacing, pad = unit_cube_case()
    values, origin, pts = _solid_case(mm, tris, lo, hi, voxel, spacing, pad)
    return dict(values=values, origin=origin, points=pts, voxel=voxel, spacing=spacing, pad=pad, lo=lo, hi=hi)


# ---- the header against the independent greedy ---------------------------------------------------------------------
@pytest.mark.parametrize("seed,shape,P,K", [(1, (7, 6, 5), 90, 6), (2, (5, 9, 4), 200, 12), (3, (8, 8, 8), 333, 40)])
def test_fit_reference_matches_the_numpy_greedy(sf, seed, shape, P, K):
    values, origin, voxel, pts = random_case(seed, shape, P)
    pad, slack = 2.0 * voxel, 0.3 * voxel
    # no (candidate, point) pair so close to the covered boundary that the two formulations could round apart: the
    # seeds are chosen so that this excludes nothing
    assert boundary_margin(values, origin, voxel, pts, pad, slack) > 1e-9
    want = numpy_greedy(values, origin, voxel, pts, pad, slack, K)
    got = sf.fit(values, origin, voxel, pts, pad, slack, K)
    assert want["count"] >= 4
    assert np.array_equal(got["chosen"], want["chosen"]) and np.array_equal(got["gains"], want["gains"])
    assert got["count"] == want["count"] and got["uncovered"] == want["uncovered"]
    # centres are the nodes, radii pad - value
    nodes = grid_nodes(origin, voxel, shape)
    c = got["chosen"][:got["count"]]
    assert np.array_equal(got["centers"][:got["count"]], nodes[c])
    assert np.array_equal(got["radii"][:got["count"]], pad - values.ravel()[c].astype(np.float64))
    assert np.isnan(got["centers"][got["count"]:]).all() and (got["chosen"][got["count"]:] == -1).all()


def test_unit_cube_is_covered_and_nothing_protrudes_beyond_pad(sf, cube):
    """K = the number of nodes: the greedy stops by itself.  uncovered == 0, and every chosen sphere stays within pad
    of the cube by the closed form box_sdf.  Measured: 2 spheres (pad is half the cube's side here);
    the largest box_sdf(centre) + radius - pad is 4.6e-9 (the float32 field), against the 1e-5 allowed."""
    K = cube["values"].size
    got = sf.fit(cube["values"], cube["origin"], cube["voxel"], cube["points"], cube["pad"], cube["spacing"], K)
    assert got["uncovered"] == 0 and 1 <= got["count"] < K
    assert got["gains"][:got["count"]].sum() == len(cube["points"])
    c, r = got["centers"][:got["count"]], got["radii"][:got["count"]]
    excess = box_sdf(c, cube["lo"], cube["hi"]) + r - cube["pad"]
    print("spheres", got["count"], "largest excess", excess.max())
    assert (excess <= 1e-5).all()
    # every sample lies at least `slack` inside some chosen sphere
    d = np.linalg.norm(cube["points"][:, None, :] - c[None], axis=2)
    assert ((d <= (r - cube["spacing"])[None] + 1e-12).any(axis=1)).all()


def test_unit_cube_first_pick_is_the_lowest_node_of_maximal_gain(sf, cube):
    got = sf.fit(cube["values"], cube["origin"], cube["voxel"], cube["points"], cube["pad"], cube["spacing"], 1)
    cov, _, _, _, _ = cover_matrix(cube["values"], cube["origin"], cube["voxel"], cube["points"], cube["pad"],
                                   cube["spacing"])
    gain = cov.sum(1)
    best = [c for c in range(len(gain)) if gain[c] == gain.max()]  # brute force
    assert got["count"] == 1 and got["chosen"][0] == best[0] and got["gains"][0] == gain.max()
    assert got["uncovered"] == len(cube["points"]) - gain.max()


def test_no_candidate_chooses_nothing(sf, cube):
    """pad at slack + the smallest value of a field that is positive everywhere: r = pad - value <= slack at every
    node, so there is no candidate."""
    slack = cube["spacing"]
    values = np.abs(cube["values"]) + np.float32(0.5)
    pad = float(values.min()) + slack
    assert 0.0 < slack < pad
    got = sf.fit(values, cube["origin"], cube["voxel"], cube["points"], pad, slack, 5)
    assert got["count"] == 0 and got["uncovered"] == len(cube["points"])
    assert (got["chosen"] == -1).all() and (got["gains"] == 0).all()
    assert np.isnan(got["centers"]).all() and np.isnan(got["radii"]).all()
    # a hair more pad and the node of the smallest value is one
    more = sf.fit(values, cube["origin"], cube["voxel"], cube["points"], pad * (1 + 1e-6), slack, 5)
    assert more["count"] <= 1 and (more["count"] == 0 or more["chosen"][0] == int(np.argmin(values)))


def test_a_bar_gets_its_spheres_along_its_axis(sf, mm):
    lo, hi = np.array([0.0, -0.1, -0.1]), np.array([1.0, 0.1, 0.1])
    voxel, spacing = 0.05, 0.02
    pad = 1.01 * (math.sqrt(3.0) * voxel + spacing)
    values, origin, pts = _solid_case(mm, box_triangles(lo, hi), lo, hi, voxel, spacing, pad)
    got = sf.fit(values, origin, voxel, pts, pad, spacing, 4)
    assert got["count"] == 4
    assert (np.diff(got["gains"]) <= 0).all()
    assert (np.abs(got["centers"][:, 1:]) <= voxel + 1e-12).all()
    assert got["centers"][:, 0].max() - got["centers"][:, 0].min() > 0.5


def test_non_finite_values_are_no_candidates(sf):
    values, origin, voxel, pts = random_case(5, (6, 6, 6), 50)
    pad, slack = 2.0 * voxel, 0.3 * voxel
    ref = sf.fit(values, origin, voxel, pts, pad, slack, 1)
    bad = values.copy().ravel()
    bad[ref["chosen"][0]] = -np.inf   # r = +inf would cover everything
    bad[0] = np.nan
    got = sf.fit(bad.reshape(values.shape), origin, voxel, pts, pad, slack, 3)
    assert ref["chosen"][0] not in got["chosen"] and 0 not in got["chosen"]
    assert np.isfinite(got["radii"][:got["count"]]).all()


# ---- surface_points, primitive_mesh ----------------------------------------------------------------------------------
def test_surface_points_are_dense_enough():
    from optik_amd.collision import surface_points
    rng = np.random.default_rng(7)
    tris = rng.uniform(-1.0, 1.0, (5, 3, 3))
    spacing = 0.13
    pts = surface_points(tris, None, spacing)
    w = rng.dirichlet([1.0, 1.0, 1.0], 1000)
    for t in tris:
        q = w @ t
        m = int(math.ceil(max(np.linalg.norm(t[(k + 1) % 3] - t[k]) for k in range(3)) / spacing))
        own = np.array([t[0] + (i / m) * (t[1] - t[0]) + (j / m) * (t[2] - t[0])
                        for i in range(m + 1) for j in range(m + 1 - i)])
        assert np.linalg.norm(q[:, None, :] - own[None], axis=2).min(axis=1).max() <= spacing
        # the triangle's own lattice is in the output
        assert np.linalg.norm(own[:, None, :] - pts[None], axis=2).min(axis=1).max() < 1e-12
    # indexed input is the same mesh
    verts = tris.reshape(-1, 3)
    assert np.array_equal(surface_points(verts, np.arange(15).reshape(5, 3), spacing), pts)


def test_surface_points_degenerate_triangles_and_the_cap():
    from optik_amd.collision import surface_points
    point = np.full((1, 3, 3), 0.25)
    line = np.array([[[0.0, 0, 0], [1.0, 0, 0], [0.5, 0, 0]]])
    p = surface_points(np.concatenate([point, line]), None, 0.3)
    assert np.isfinite(p).all()
    assert (np.linalg.norm(p - 0.25, axis=1) == 0.0).sum() == 3           # the point triangle: its three vertices
    for v in line[0]:
        assert (np.abs(p - v).sum(1) == 0.0).any()
    with pytest.raises(ValueError, match=r"2\^20.*raise spacing"):
        surface_points(box_triangles([0, 0, 0], [1, 1, 1]), None, 0.002)
    with pytest.raises(ValueError, match="spacing"):
        surface_points(point, None, 0.0)


def test_primitive_meshes_are_circumscribed():
    from optik_amd.collision import PRIMITIVE_SEGMENTS, primitive_mesh
    assert PRIMITIVE_SEGMENTS == 24
    box = primitive_mesh("box", (0.2, 0.4, 0.6)).reshape(-1, 3)
    assert np.array_equal(np.abs(box).max(0), [0.1, 0.2, 0.3]) and np.array_equal(np.abs(box).min(0), [0.1, 0.2, 0.3])
    R, L = 0.3, 1.1
    cyl = primitive_mesh("cylinder", (R, L))
    v = cyl.reshape(-1, 3)
    rho = np.linalg.norm(v[:, :2], axis=1)
    assert ((rho >= R) | (rho == 0.0)).all() and (np.abs(v[:, 2]) == L / 2).all()   # on or outside; cap centres
    # the side faces' planes do not cut into the cylinder either
    side = cyl[np.ptp(cyl[:, :, 2], axis=1) > 0]
    n = np.cross(side[:, 1] - side[:, 0], side[:, 2] - side[:, 0])
    assert ((n * side[:, 0]).sum(1) / np.linalg.norm(n, axis=1) >= R * (1 - 1e-12)).all()
    sph = primitive_mesh("sphere", 0.7)
    assert (np.linalg.norm(sph.reshape(-1, 3), axis=1) >= 0.7).all()
    n = np.cross(sph[:, 1] - sph[:, 0], sph[:, 2] - sph[:, 0])
    d = (n * sph[:, 0]).sum(1) / np.linalg.norm(n, axis=1)
    assert (d >= 0.7 * (1 - 1e-12)).all() and d.min() <= 0.7 * (1 + 1e-12)            # outward, touching
    with pytest.raises(ValueError):
        primitive_mesh("capsule", (1.0, 1.0))
    with pytest.raises(ValueError):
        primitive_mesh("box", (1.0, -1.0, 1.0))


# ---- the URDF ---------------------------------------------------------------------------------------------------------
def _wedge():
    return box_triangles([0.0, -0.06, -0.06], [0.2, 0.06, 0.06])


def _T(xyz=(0, 0, 0), R=None):
    T = np.eye(4)
    T[:3, 3] = xyz
    if R is not None:
        T[:3, :3] = R
    return T


def _rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    return {"y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def test_urdf_collision_geometry_on_the_fixture(tmp_path, built):
    from optik_amd import Robot
    from optik_amd.collision import urdf_collision_geometry
    text = open(FIXTURE).read()
    with pytest.raises(ValueError, match="link 'l3'.*wedge.stl.*not found"):
        urdf_collision_geometry(text, "base", "tip", mesh_dir=str(tmp_path))
    geo, rep = urdf_collision_geometry(text, "base", "tip", mesh_dir=str(tmp_path), on_missing="skip")
    assert [g[1] for g in geo] == ["box", "cylinder", "sphere", "box", "box", "sphere"]
    assert any(s["link"] == "l3" and "not found" in s["reason"] for s in rep["skipped"])
    os.makedirs(tmp_path / "meshes")
    write_stl_binary(str(tmp_path / "meshes" / "wedge.stl"), _wedge())
    geo, rep = urdf_collision_geometry(text, "base", "tip", mesh_dir=str(tmp_path))
    # hand-computed: the link, its frame, the geometry's transform in that frame
    want = [("base", 0, "box", _T((0, 0, 0.05))),
            ("l1", 1, "cylinder", _T((0, 0, 0.15))),
            ("mid", 1, "sphere", _T((0, 0, 0.3))),                      # behind the fixed joint: l1's frame
            ("l2", 2, "box", _T((0.15, 0, 0))),
            ("camera", 2, "box", _T((0.1 - 0.02 * math.sin(0.3), 0, -0.05 - 0.02 * math.cos(0.3)), _rot("y", 0.3))),
            ("l3", 3, "mesh", _T()),
            ("tip", 4, "sphere", _T())]                                 # the fixed tip: frame n + 1
    assert rep["links"] == [w[0] for w in want]
    for (frame, kind, T, data), (_, wf, wk, wT) in zip(geo, want):
        assert frame == wf and kind == wk
        assert np.allclose(T, wT, rtol=0, atol=1e-15), (kind, T, wT)
    assert np.array_equal(geo[0][3], [0.2, 0.2, 0.1]) and np.array_equal(geo[1][3], [0.04, 0.3])
    assert np.array_equal(geo[2][3], [0.05])
    assert np.array_equal(geo[5][3], _wedge().astype(np.float32).astype(np.float64) * 0.5)   # scale applied
    assert rep["frames"] == dict(base=0, l1=1, mid=1, l2=2, camera=2, l3=3, tip=4)
    assert [s["link"] for s in rep["skipped"]] == ["finger"] and "prismatic" in rep["skipped"][0]["reason"]
    assert rep["fold_order_differs"] == []
    # the frames are the chain's: the accumulated joint origins equal the loader's table
    robot = Robot.from_urdf_str(text, "base", "tip")
    tab = robot.chain_tables()
    assert robot.num_positions() == 3 and len(tab["origins"]) == 4 == len(rep["joint_origins"])
    for T, o7 in zip(rep["joint_origins"], tab["origins"]):
        x, y, z, w = o7[3:]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        assert np.allclose(T[:3, 3], o7[:3], rtol=0, atol=1e-15) and np.allclose(T[:3, :3], R, rtol=0, atol=1e-15)
    # a mesh that is no STL
    with pytest.raises(ValueError, match="link 'l3'.*not an .stl"):
        urdf_collision_geometry(text.replace("wedge.stl", "wedge.dae"), "base", "tip", mesh_dir=str(tmp_path))
    # a custom resolver
    geo2, _ = urdf_collision_geometry(text, "base", "tip",
                                      mesh_resolver=lambda f: str(tmp_path / "meshes" / os.path.basename(f)))
    assert np.array_equal(geo2[5][3], geo[5][3])


def test_urdf_collision_geometry_of_the_ur3e():
    """The reference UR3e model: its <collision> geometry is spheres and cylinders only -- the .obj files it names,
    which are not here, are <visual> geometry and are never looked for -- so it reads without a mesh directory, with
    a non-empty report, and the same under on_missing="skip".  (A collision mesh that is absent or no STL: the
    fixture's test above.)"""
    from optik_amd.collision import urdf_collision_geometry
    text = open(UR3E).read()
    assert ".obj" in text
    geo, rep = urdf_collision_geometry(text, "ur_base_link", "ur_ee_link")
    geo2, rep2 = urdf_collision_geometry(text, "ur_base_link", "ur_ee_link", on_missing="skip")
    assert len(geo) == len(geo2) == 13 and sorted({g[1] for g in geo}) == ["cylinder", "sphere"]
    assert rep["skipped"] == [] and rep["links"] == rep2["links"] and len(rep["links"]) == 13
    assert rep["frames"]["ur_base_link"] == 0 and rep["frames"]["ur_wrist_3_link"] == 6
    assert rep["frames"]["ur_tool0"] == 6 and rep["frames"]["ur_ee_link"] == 7      # off-chain fixed; the fixed tip
    assert [g[0] for g in geo] == sorted(g[0] for g in geo) and {g[0] for g in geo} == set(range(7))
    # a collision mesh in it that is absent: raises naming the link, skipped and reported on request
    bad = text.replace('<sphere radius="0.07"/>', '<mesh filename="package://drake_models/ur3e/base.stl"/>', 1)
    assert bad != text
    with pytest.raises(ValueError, match=r"link 'ur_base_link': collision mesh .*base.stl' not found"):
        urdf_collision_geometry(bad, "ur_base_link", "ur_ee_link", mesh_dir=os.path.dirname(UR3E))
    geo3, rep3 = urdf_collision_geometry(bad, "ur_base_link", "ur_ee_link", mesh_dir=os.path.dirname(UR3E),
                                         on_missing="skip")
    assert len(geo3) == 12 and [s["link"] for s in rep3["skipped"]] == ["ur_base_link"]


# ---- prune_pairs ------------------------------------------------------------------------------------------------------
class _StillRobot:
    """Three frames that never move: frame k at x = k."""

    def num_positions(self):
        return 1

    def joint_limits(self):
        return [-1.0], [1.0]

    def link_frames_batch_arrays(self, xs, ee_offset=None):
        T = np.tile(np.eye(4), (len(xs), 3, 1, 1))
        T[:, :, 0, 3] = np.arange(3)
        return T


def test_prune_pairs_drops_the_overlapping_pair():
    from optik_amd.collision import prune_pairs
    frames, centers, radii = [0, 1, 2], np.zeros((3, 3)), [0.6, 0.6, 0.3]   # 0-1 overlap by 0.2; 1-2 apart 0.1; 0-2 1.1
    pairs = [[0, 1], [1, 2], [0, 2]]
    kept, dropped = prune_pairs(_StillRobot(), frames, centers, radii, pairs)
    assert kept.tolist() == [[1, 2], [0, 2]] and dropped.tolist() == [[0, 1]]
    assert kept.dtype == np.int32 and dropped.dtype == np.int32
    kept, dropped = prune_pairs(_StillRobot(), frames, centers, radii, pairs, configs=[[0.0], [0.5]], margin=0.15)
    assert kept.tolist() == [[0, 2]] and dropped.tolist() == [[0, 1], [1, 2]]


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def test_fit_symbols_are_exported(built):
    for s in ("optik_hip_sphere_fit", "optik_robot_sphere_fit", "optik_hip_sphere_fit_workspace_bytes",
              "optik_hip_fit_tile", "optik_hip_fit_pairs_per_launch"):
        assert hasattr(built, s), f"{s} is not exported by liboptik_amd.so"
    from optik_amd import _native
    assert _native.fit_tile() >= 1
    assert built.optik_hip_sphere_fit_workspace_bytes(3, 4, 5, 7) >= 4 * (60 + 2 * 7)
    before = built.optik_hip_fit_pairs_per_launch(-1)
    assert before == 1 << 32
    with _native.fit_pairs_per_launch(4321):
        assert built.optik_hip_fit_pairs_per_launch(-1) == 4321
    assert built.optik_hip_fit_pairs_per_launch(-1) == before


def test_fit_refusals_happen_before_any_device_work(panda):
    """None of these calls touches a device (the robot has created no device context: no chain exists)."""
    o, vals, pts = [0.0, 0.0, 0.0], np.zeros((2, 3, 4), dtype=np.float32), np.zeros((5, 3))
    nan_pts = pts.copy()
    nan_pts[3, 1] = math.nan
    for args, what in [
        ((vals, o, 0.1, pts, 0.3, 0.1, 0), r"K must be in 1\.\.256"),
        ((vals, o, 0.1, pts, 0.3, 0.1, 257), r"K must be in 1\.\.256"),
        ((vals, o, 0.1, np.zeros((0, 3)), 0.3, 0.1, 4), r"1\.\.2\^20"),
        ((vals, o, 0.1, np.zeros(((1 << 20) + 1, 3)), 0.3, 0.1, 4), r"1\.\.2\^20"),
        ((vals, o, 0.1, nan_pts, 0.3, 0.1, 4), "point 3 has a NaN or infinite"),
        ((vals, o, 0.1, pts, 0.0, 0.0, 4), "pad"),
        ((vals, o, 0.1, pts, math.inf, 0.1, 4), "pad"),
        ((vals, o, 0.1, pts, math.nan, 0.1, 4), "pad"),
        ((vals, o, 0.1, pts, 0.3, -0.1, 4), "slack"),
        ((vals, o, 0.1, pts, 0.3, 0.3, 4), "slack"),
        ((vals, o, 0.1, pts, 0.3, math.nan, 4), "slack"),
        ((vals, o, 0.0, pts, 0.3, 0.1, 4), "voxel"),
        ((np.zeros((1, 3, 4), dtype=np.float32), o, 0.1, pts, 0.3, 0.1, 4), r"2\.\.1024"),
        ((vals, [0.0, math.inf, 0.0], 0.1, pts, 0.3, 0.1, 4), "origin"),
    ]:
        with pytest.raises(ValueError, match=what):
            panda.sphere_fit_arrays(*args)
    cube = box_triangles([0, 0, 0], [1, 1, 1])
    for kw, what in [(dict(count=0), "K must be"), (dict(count=300), "K must be"), (dict(voxel=0.0), "voxel"),
                     (dict(voxel=0.1, spacing=0.05, pad=0.2), "pad must be >="), (dict(spacing=-1.0), "spacing"),
                     (dict(voxel=0.0005), r"2\.\.1024|2\^24|2\^20")]:
        with pytest.raises(ValueError, match=what):
            panda.fit_spheres(cube, **kw)
    with pytest.raises(ValueError):
        panda.fit_spheres(np.zeros((0, 3, 3)))
    # the C ABI itself: each of these returns -1
    L, h = panda._L, panda._h
    o3 = (C.c_double * 3)(0.0, 0.0, 0.0)
    p3 = (C.c_double * 15)()
    val = (C.c_float * 24)()
    i4, g4, cu = (C.c_int32 * 4)(), (C.c_int32 * 4)(), (C.c_int32 * 2)()
    c12, r4 = (C.c_double * 12)(), (C.c_double * 4)()
    vp = lambda a: C.cast(a, C.c_void_p)
    f = L.optik_robot_sphere_fit
    assert f(None, o3, 0.1, 2, 3, 4, vp(val), p3, 5, 0.3, 0.1, 4, i4, c12, r4, g4, cu) == -1
    assert f(h, o3, 0.1, 2, 3, 4, None, p3, 5, 0.3, 0.1, 4, i4, c12, r4, g4, cu) == -1
    assert f(h, o3, 0.1, 2, 3, 4, vp(val), None, 5, 0.3, 0.1, 4, i4, c12, r4, g4, cu) == -1
    assert f(h, o3, 0.1, 2, 3, 4, vp(val), p3, 5, 0.3, 0.1, 4, None, c12, r4, g4, cu) == -1
    assert f(h, o3, 0.1, 2, 3, 4, vp(val), p3, 5, 0.3, 0.1, 4, i4, c12, r4, g4, None) == -1
    assert f(h, o3, 0.1, 2, 3, 4, vp(val), p3, 5, 0.3, 0.1, 0, i4, c12, r4, g4, cu) == -1
    assert f(h, o3, 0.1, 2, 3, 4, vp(val), p3, 0, 0.3, 0.1, 4, i4, c12, r4, g4, cu) == -1
    assert f(h, o3, 0.1, 2, 3, 4, vp(val), p3, 5, 0.3, 0.3, 4, i4, c12, r4, g4, cu) == -1
    assert b"slack" in L.optik_robot_last_error()


def test_fit_collision_model_refuses_too_many_spheres(panda):
    geo = [(k % 9, "sphere", np.eye(4), [0.01]) for k in range(257)]
    with pytest.raises(ValueError, match="257 spheres.*lower per_link"):
        panda.fit_collision_model(geo)
    frames, centers, radii, rep = panda.fit_collision_model(geo[:9])     # spheres pass through as themselves
    assert frames.tolist() == list(range(9)) and (radii == 0.01).all() and (centers == 0.0).all()
    assert rep["uncovered"] == 0 and rep["fits"] == {}
