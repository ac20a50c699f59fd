"""GPU: from a triangle mesh to a distance-field world -- the kernel of ik_mesh.hip bit for
bit against optik_amd/csrc/mesh_measure.hpp compiled with g++ (tests/mesh_util.py), through HipChain and Robot, at the
tile edges and with the launch bound forced small; against the bake of the same cube; set_world_mesh end to end."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROBOT_SPECS, ROBOTS, ROOT
from gpu_util import assert_bit_equal
from mesh_util import box_triangles, build_mesh_measure, degenerate_triangles, random_triangles, ulp_diff

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# node counts that are no multiple of the block (256) or the wave (64); (2, 2, 2) has fewer nodes than one wave: the
# barriers with idle lanes
GRIDS = [(13, 9, 17), (5, 4, 130), (3, 70, 5), (2, 2, 2)]
ORIGIN, VOXEL = [-0.6137, -0.4311, -0.8791], 0.0873
# the grid of the cube cases: no node on a face of the unit cube
C_ORIGIN, C_VOXEL, C_SHAPE = [-0.7131, -0.7131, -0.7131], 0.173, (14, 14, 14)


def _robot(name="panda"):
    from optik_amd import Robot
    return Robot.from_urdf_file(*ROBOT_SPECS[name])


@pytest.fixture(scope="module")
def mm(tmp_path_factory):
    return build_mesh_measure(str(tmp_path_factory.mktemp("mesh_measure")))


@pytest.fixture(scope="module")
def hc(chains):
    from optik_amd import device
    return device.HipChain(**chains["panda"][0])


@pytest.fixture(scope="module")
def panda():
    return _robot()


def _tile():
    from optik_amd import _native
    return _native.mesh_tile()


def _mesh(M, seed=21):
    """M triangles: random well-shaped ones, with the zero-area and the three-equal-vertices triangle among them
    from M = 12 on (at the front and in the middle)."""
    rng = np.random.default_rng(seed + M)
    if M < 12:
        return random_triangles(rng, M)
    t = random_triangles(rng, M - 2)
    deg = degenerate_triangles()
    return np.concatenate([deg[:1], t[:M // 2], deg[1:], t[M // 2:]])


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def _chain_field(hc, origin, voxel, shape, tris, md=None):
    t = torch.tensor(np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3), device="cuda")
    out = hc.world_grid_from_mesh(origin, voxel, shape, t, md)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(shape)
    return out.cpu().numpy()


def _default_md(voxel, shape):
    return voxel * math.sqrt(sum(s * s for s in shape))


# the tile edges are read from the library; the ids name them
M_CASES = {"1": lambda T: 1, "12": lambda T: 12, "tile-1": lambda T: T - 1, "tile": lambda T: T,
           "tile+1": lambda T: T + 1, "2tile+3": lambda T: 2 * T + 3}


@pytest.mark.parametrize("case", list(M_CASES))
def test_field_equals_the_host_measure(hc, mm, case):
    M = M_CASES[case](_tile())
    tris = _mesh(M)
    assert len(tris) == M
    for shape in GRIDS:
        want = mm.field(ORIGIN, VOXEL, shape, tris, _default_md(VOXEL, shape))
        got = _chain_field(hc, ORIGIN, VOXEL, shape, tris)
        assert np.isfinite(got).all()
        assert np.array_equal(_bits(got), _bits(want)), f"M = {M}, {shape}: {(got != want).sum()} nodes differ"


def test_robot_path_equals_the_chain_path_and_the_host(hc, panda, mm):
    M = _tile() + 1
    tris, shape = _mesh(M), GRIDS[0]
    md = 0.05  # clamps both signs: 257 random triangles leave values of -0.13 .. 0.09 on this grid
    want = mm.field(ORIGIN, VOXEL, shape, tris, md)
    assert want.max() == np.float32(md) and want.min() == np.float32(-md)
    got_c = _chain_field(hc, ORIGIN, VOXEL, shape, tris, md)
    got_r = panda.world_grid_from_mesh(ORIGIN, VOXEL, shape, tris, max_distance=md)
    assert got_r.dtype == np.float32 and got_r.shape == shape
    assert np.array_equal(_bits(got_c), _bits(want)) and np.array_equal(_bits(got_r), _bits(want))
    # indexed form: the same soup gathered by the Python layer
    verts = tris.reshape(-1, 3)
    idx = np.arange(3 * M, dtype=np.int32).reshape(M, 3)
    assert np.array_equal(_bits(panda.world_grid_from_mesh(ORIGIN, VOXEL, shape, verts, idx, max_distance=md)),
                          _bits(want))


def test_split_into_launches_changes_nothing(hc, mm):
    """The launch bound forced to 12 * 700 pairs: the 1989 nodes of (13, 9, 17) against 12 triangles go out as three
    launches of 700, 700 and 589 nodes, none a multiple of the block.  (The hook: _native.mesh_pairs_per_launch,
    optik_hip_mesh_pairs_per_launch of optik_hip.h.)"""
    from optik_amd import _native
    tris, shape = _mesh(12), GRIDS[0]
    assert int(np.prod(shape)) == 1989
    whole = _chain_field(hc, ORIGIN, VOXEL, shape, tris)
    with _native.mesh_pairs_per_launch(12 * 700):
        assert _native.lib().optik_hip_mesh_pairs_per_launch(-1) == 12 * 700
        split = _chain_field(hc, ORIGIN, VOXEL, shape, tris)
    with _native.mesh_pairs_per_launch(1):  # one node per launch on the smallest grid
        tiny = _chain_field(hc, ORIGIN, VOXEL, (2, 2, 2), tris)
    want = mm.field(ORIGIN, VOXEL, shape, tris, _default_md(VOXEL, shape))
    assert np.array_equal(_bits(split), _bits(whole)) and np.array_equal(_bits(split), _bits(want))
    assert np.array_equal(_bits(tiny), _bits(mm.field(ORIGIN, VOXEL, (2, 2, 2), tris, _default_md(VOXEL, (2, 2, 2)))))


def test_cube_mesh_against_the_bake_of_the_same_cube(panda):
    """Two independent routes to one field: the box primitive's bake and the cube's 12 triangles.  Both are f64
    distances to the same surface, rounded to float32: within one ulp, and the sign pattern is identical."""
    robot = _robot()
    robot.set_world(boxes=[[0.5, 0.5, 0.5, 0.0, 0.0, 0.0, 1.0, 0.5, 0.5, 0.5]])
    baked = robot.bake_world_grid(C_ORIGIN, C_VOXEL, C_SHAPE)
    mesh = panda.world_grid_from_mesh(C_ORIGIN, C_VOXEL, C_SHAPE, box_triangles([0, 0, 0], [1, 1, 1]), max_distance=100.0)
    assert ulp_diff(mesh, baked).max() <= 1
    assert np.array_equal(np.signbit(mesh), np.signbit(baked)) and (mesh < 0).sum() == 5 ** 3


def test_back_to_back_calls_on_one_stream(hc, mm):
    """Two meshes, two grids, queued without a synchronisation between them: neither disturbs the other."""
    a, b = _mesh(_tile() + 1, seed=31), _mesh(12, seed=32)
    ta = torch.tensor(a, device="cuda")
    tb = torch.tensor(b, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out_a = hc.world_grid_from_mesh(ORIGIN, VOXEL, GRIDS[0], ta)
        out_b = hc.world_grid_from_mesh(ORIGIN, VOXEL, GRIDS[1], tb)
        out_a2 = hc.world_grid_from_mesh(ORIGIN, VOXEL, GRIDS[0], ta.reshape(-1, 9))
    side.synchronize()
    want_a = mm.field(ORIGIN, VOXEL, GRIDS[0], a, _default_md(VOXEL, GRIDS[0]))
    want_b = mm.field(ORIGIN, VOXEL, GRIDS[1], b, _default_md(VOXEL, GRIDS[1]))
    assert np.array_equal(_bits(out_a.cpu().numpy()), _bits(want_a))
    assert np.array_equal(_bits(out_b.cpu().numpy()), _bits(want_b))
    assert np.array_equal(_bits(out_a2.cpu().numpy()), _bits(want_a))


def test_kernel_layer_refusals(hc):
    import ctypes as C
    from optik_amd import _native as nat
    from optik_amd._native import OptikHipError
    tri = torch.zeros((2, 3, 3), dtype=torch.float64, device="cuda")
    for md in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(OptikHipError, match="max_distance"):
            hc.world_grid_from_mesh([0, 0, 0], 0.1, (2, 3, 4), tri, md)
    with pytest.raises(OptikHipError, match="voxel"):
        hc.world_grid_from_mesh([0, 0, 0], 0.0, (2, 3, 4), tri)
    with pytest.raises(OptikHipError, match=r"2\.\.1024"):
        hc.world_grid_from_mesh([0, 0, 0], 0.1, (1, 3, 4), tri)
    with pytest.raises(OptikHipError, match=r"1\.\.2\^20"):
        hc.world_grid_from_mesh([0, 0, 0], 0.1, (2, 3, 4), tri[:0])
    with pytest.raises(ValueError):
        hc.world_grid_from_mesh([0, 0, 0], 0.1, (2, 3, 4), tri.to(torch.float32))
    L, einval = nat.lib(), -1
    o3 = (C.c_double * 3)(0.0, 0.0, 0.0)
    val = torch.zeros((2, 3, 4), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    f = lambda d_t, M, d_v: L.optik_hip_world_grid_from_mesh(hc._h, o3, 0.1, 2, 3, 4, d_t, M, 1.0, d_v, None)
    assert f(None, 2, p(val)) == einval and "null buffer" in L.optik_hip_last_error().decode()
    assert f(p(tri), 2, None) == einval and "null buffer" in L.optik_hip_last_error().decode()
    assert f(p(tri), (1 << 20) + 1, p(val)) == einval and f(p(tri), -3, p(val)) == einval
    assert L.optik_hip_world_grid_from_mesh(None, o3, 0.1, 2, 3, 4, p(tri), 2, 1.0, p(val), None) == einval
    assert f(p(tri), 2, p(val)) == 0
    torch.cuda.synchronize()
    assert np.isfinite(val.cpu().numpy()).all()


# ---- the whole path ---------------------------------------------------------------------------------------------------
W_ORIGIN, W_VOXEL, W_SHAPE = [-1.0, -1.0, -0.2], 0.05, (41, 41, 33)
SLAB = ([0.40, -0.30, -0.10], [0.44, 0.30, 0.30])  # a low wall in front of the robot: the arm reaches over it


def test_set_world_mesh_end_to_end(mm):
    from optik_amd import SolverConfig
    from optik_amd.collision import spheres_along_chain
    rng = np.random.default_rng(9)
    robots = [_robot(), _robot()]
    frames, centers, radii = spheres_along_chain(robots[0], 0.05, 8)
    margin = math.sqrt(3.0) * W_VOXEL
    for r in robots:
        r.set_collision_model(frames, centers, radii, self_pairs=None, margin=margin)
    slab = box_triangles(*SLAB)
    values = robots[0].set_world_mesh(W_ORIGIN, W_VOXEL, W_SHAPE, slab)
    host = mm.field(W_ORIGIN, W_VOXEL, W_SHAPE, slab, _default_md(W_VOXEL, W_SHAPE))
    assert values.dtype == np.float32 and np.array_equal(_bits(values), _bits(host))
    assert (values < 0).any()
    robots[1].set_world_grid(W_ORIGIN, W_VOXEL, host)

    lb, ub = (np.array(v) for v in robots[0].joint_limits())
    qs = rng.uniform(lb, ub, size=(512, 7))
    clr0, free0 = robots[0].collision_clearance_batch_arrays(qs)
    clr1, free1 = robots[1].collision_clearance_batch_arrays(qs)
    assert_bit_equal(clr0, clr1, "set_world_mesh against set_world_grid(host measure)")
    assert np.array_equal(free0, free1) and free0.any() and not free0.all()

    # targets behind the slab: the poses of free configurations whose end effector is beyond it
    poses = np.array([robots[0].fk(q) for q in qs])
    behind = free0 & (clr0 > margin + 0.02) & (poses[:, 0, 3] > 0.5) & (np.abs(poses[:, 1, 3]) < 0.25)
    assert behind.any()
    targets = poses[behind][:4]
    x0 = rng.uniform(lb, ub, size=(len(targets), 7))
    cfg = SolverConfig("quality", max_time=0.0, max_restarts=256)
    xs, fs, found = robots[0].ik_batch_arrays(cfg, targets, x0)
    assert found.any()
    c, ok = robots[0].collision_clearance_batch_arrays(np.asarray(xs)[found])
    assert (c >= margin).all() and ok.all()


def test_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ik_world_mesh.py"),
                          os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"],
                         env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    m = re.search(r"clearance (-?\d+\.\d+)", res.stdout)
    assert m and float(m.group(1)) >= 0.0, res.stdout
    assert "all free: True" in res.stdout, res.stdout
