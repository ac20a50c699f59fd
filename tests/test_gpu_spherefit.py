"""GPU: sphere models from collision geometry -- the kernels of ik_spherefit.hip against
optik_amd/csrc/spherefit_measure.hpp's fit_reference compiled with g++ (tests/spherefit_util.py), every output exact,
into sentinel-filled buffers: at the tile edges, on grids below a wave and past a block, with a tie across blocks,
under a capped grid and with the launch bound forced small; Robot.fit_spheres on the unit cube against the closed
form; set_collision_model_from_urdf end to end."""
import math
import os

import numpy as np
import pytest

from conftest import ROBOT_SPECS, ROOT
from gpu_util import _out, _sentinels_left
from mesh_util import box_sdf, box_triangles, write_stl_binary
from spherefit_util import assert_fit_equal, build_spherefit, grid_nodes, random_case, unit_cube_case

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FIXTURE = os.path.join(ROOT, "tests", "golden", "robots", "arm_primitives.urdf")
# node counts below one wave (24), just past a block (258 = 256 + 2: a grid has at least 2 nodes per axis, so 257 is
# none), past four blocks (1028) and no multiple of the block or the wave (693)
GRIDS = {"below-a-wave": (2, 3, 4), "past-a-block": (3, 43, 2), "past-four-blocks": (257, 2, 2), "odd": (7, 9, 11)}


def _robot(name="panda"):
    from optik_amd import Robot
    return Robot.from_urdf_file(*ROBOT_SPECS[name])


@pytest.fixture(scope="module")
def sf(tmp_path_factory):
    return build_spherefit(str(tmp_path_factory.mktemp("spherefit_measure")))


@pytest.fixture(scope="module")
def hc(chains):
    from optik_amd import device
    return device.HipChain(**chains["panda"][0])


def _tile():
    from optik_amd import _native
    return _native.fit_tile()


def _device_fit(hc, values, origin, voxel, pts, pad, slack, K):
    """HipChain.sphere_fit_into sentinel-filled outputs; the outputs as host arrays, no sentinel left."""
    out = dict(chosen=_out((K,), torch.int32), centers=_out((K, 3), torch.float64), radii=_out((K,), torch.float64),
               gains=_out((K,), torch.int32), count_uncovered=_out((2,), torch.int32))
    v = torch.tensor(np.ascontiguousarray(values, dtype=np.float32), device="cuda")
    p = torch.tensor(np.ascontiguousarray(pts, dtype=np.float64), device="cuda")
    hc.sphere_fit_into(v, origin, voxel, p, pad, slack, K, out)
    torch.cuda.synchronize()
    got = {k: t.cpu().numpy() for k, t in out.items()}
    for k, a in got.items():
        assert _sentinels_left(a) == 0, f"{k}: a sentinel is left"
    got["count"], got["uncovered"] = int(got["count_uncovered"][0]), int(got["count_uncovered"][1])
    return got


P_CASES = {"1": lambda T: 1, "63": lambda T: 63, "64": lambda T: 64, "65": lambda T: 65, "tile": lambda T: T,
           "tile+1": lambda T: T + 1}


@pytest.mark.parametrize("case", list(P_CASES))
def test_fit_equals_the_host_reference_at_the_point_counts(hc, sf, case):
    P = P_CASES[case](_tile())
    for name, shape in GRIDS.items():
        values, origin, voxel, pts = random_case(100 + P, shape, P)
        pad, slack, K = 2.0 * voxel, 0.3 * voxel, 7
        want = sf.fit(values, origin, voxel, pts, pad, slack, K)
        got = _device_fit(hc, values, origin, voxel, pts, pad, slack, K)
        assert_fit_equal(got, want, f"P = {P}, grid {name}")


def test_k_of_one_and_k_larger_than_needed(hc, sf):
    values, origin, voxel, pts = random_case(7, (6, 7, 8), 150)
    pad, slack = 2.0 * voxel, 0.3 * voxel
    one = sf.fit(values, origin, voxel, pts, pad, slack, 1)
    assert one["count"] == 1
    assert_fit_equal(_device_fit(hc, values, origin, voxel, pts, pad, slack, 1), one, "K = 1")
    many = sf.fit(values, origin, voxel, pts, pad, slack, 64)
    assert 4 <= many["count"] < 60 and many["chosen"][-1] == -1       # the greedy stops by itself: trailing -1 / NaN
    assert_fit_equal(_device_fit(hc, values, origin, voxel, pts, pad, slack, 64), many, "K = 64")
    # through the robot's host arrays too
    panda = _robot()
    ch, ce, ra, ga, cnt, unc = panda.sphere_fit_arrays(values, origin, voxel, pts, pad, slack, 64)
    assert_fit_equal(dict(chosen=ch, centers=ce, radii=ra, gains=ga, count=cnt, uncovered=unc), many, "Robot")


def test_no_candidate(hc, sf):
    values, origin, voxel, pts = random_case(8, (5, 5, 5), 70)
    values = np.abs(values) + np.float32(1.0)
    pad, slack = 1.0 + 0.3 * voxel, 0.3 * voxel      # r = pad - value <= slack everywhere
    want = sf.fit(values, origin, voxel, pts, pad, slack, 5)
    assert want["count"] == 0 and want["uncovered"] == 70
    got = _device_fit(hc, values, origin, voxel, pts, pad, slack, 5)
    assert_fit_equal(got, want, "no candidate")
    assert (got["chosen"] == -1).all() and np.isnan(got["radii"]).all() and (got["gains"] == 0).all()


def test_a_tie_across_two_blocks_goes_to_the_lower_node(hc, sf):
    """Two identical blobs far apart on a (40, 4, 4) grid, 640 nodes: the best nodes of the two, 2 * 16 + 5 = 37 and
    37 + 32 * 16 = 549, are in different blocks (0 and 2) and cover the same number of points."""
    shape, voxel, origin = (40, 4, 4), 0.1, np.zeros(3)
    nodes = grid_nodes(origin, voxel, shape)
    a, b = nodes[37], nodes[549]
    assert np.array_equal(b - a, [3.2, 0.0, 0.0])
    d = np.minimum(np.linalg.norm(nodes - a, axis=1), np.linalg.norm(nodes - b, axis=1)) - 0.12
    values = d.astype(np.float32).reshape(shape)
    rng = np.random.default_rng(3)
    u = rng.normal(size=(40, 3))
    off = np.round(0.12 * u / np.linalg.norm(u, axis=1)[:, None] * 1024) / 1024    # exactly representable offsets
    pts = np.concatenate([a + off, b + off])
    pad, slack, K = 0.2, 0.02, 3
    want = sf.fit(values, origin, voxel, pts, pad, slack, K)
    assert want["chosen"][0] == 37 and want["chosen"][1] == 549 and want["gains"][0] == want["gains"][1] == 40
    got = _device_fit(hc, values, origin, voxel, pts, pad, slack, K)
    assert_fit_equal(got, want, "tie")


def test_the_launch_bound_and_the_capped_grid_change_nothing(hc, sf):
    from optik_amd import _native as nat
    values, origin, voxel, pts = random_case(9, (9, 10, 11), 300)     # 990 nodes
    pad, slack, K = 2.0 * voxel, 0.3 * voxel, 12
    want = sf.fit(values, origin, voxel, pts, pad, slack, K)
    assert want["count"] >= 6
    before = nat.lib().optik_hip_fit_pairs_per_launch(-1)
    with nat.fit_pairs_per_launch(300 * 256 + 17):                    # 256 candidates a launch: 4 launches a pass
        got = _device_fit(hc, values, origin, voxel, pts, pad, slack, K)
    assert nat.lib().optik_hip_fit_pairs_per_launch(-1) == before
    assert_fit_equal(got, want, "launch bound")
    for cap in (1, 3):                                                 # the pick's and the mark's grid-stride trips
        with nat.options(grid_cap=cap):
            got = _device_fit(hc, values, origin, voxel, pts, pad, slack, K)
        assert_fit_equal(got, want, f"grid_cap = {cap}")


def test_fit_spheres_on_the_unit_cube(sf):
    """uncovered == 0 and no sphere beyond pad by the closed form; the field fed to the fit is world_grid_from_mesh's:
    the host reference on that field gives the spheres fit_spheres returns."""
    panda = _robot()
    tris, lo, hi, voxel, spacing, pad = unit_cube_case()
    centers, radii, info = panda.fit_spheres(tris, None, count=8, voxel=voxel, pad=pad, spacing=spacing)
    assert info["uncovered"] == 0 and 1 <= len(radii) <= 8 and info["gains"].sum() == info["points"]
    excess = box_sdf(centers, lo, hi) + radii - pad
    print("spheres", len(radii), "largest excess", excess.max())
    assert (excess <= 1e-5).all()
    from optik_amd.collision import surface_points
    values = panda.world_grid_from_mesh(info["origin"], info["voxel"], info["shape"], tris)
    want = sf.fit(values, info["origin"], voxel, surface_points(tris, None, spacing), pad, spacing, 8)
    assert np.array_equal(info["chosen"], want["chosen"][:want["count"]])
    assert np.array_equal(centers, want["centers"][:want["count"]]) and np.array_equal(radii, want["radii"][:want["count"]])
    # the fit does not depend on the chain: a UR10 and the 10-joint chain give the same spheres and accept the model
    for name in ("ur10", "arm10"):
        other = _robot(name)
        c2, r2, i2 = other.fit_spheres(tris, None, count=8, voxel=voxel, pad=pad, spacing=spacing)
        assert np.array_equal(c2, centers) and np.array_equal(r2, radii) and i2["uncovered"] == 0
        other.set_collision_model(np.full(len(r2), 1, dtype=np.int32), c2 * 0.05, r2 * 0.05, self_pairs=None)
        other.set_world(spheres=[[2.0, 0.0, 0.0, 0.1]])
        assert math.isfinite(other.collision_clearance(np.zeros(other.num_positions())))


def test_set_collision_model_from_urdf_end_to_end(tmp_path):
    from optik_amd import Robot
    from optik_amd.collision import spheres_at
    os.makedirs(tmp_path / "meshes")
    write_stl_binary(str(tmp_path / "meshes" / "wedge.stl"), box_triangles([0.0, -0.06, -0.06], [0.2, 0.06, 0.06]))
    robot = Robot.from_urdf_file(FIXTURE, "base", "tip")
    frames, centers, radii, rep = robot.set_collision_model_from_urdf(
        FIXTURE, "base", "tip", per_link=16, mesh_dir=str(tmp_path), self_pairs=None, voxel=0.02, spacing=0.01)
    assert rep["uncovered"] == 0 and set(frames.tolist()) == {0, 1, 2, 3, 4}
    assert [s["link"] for s in rep["geometry"]["skipped"]] == ["finger"]
    pad = rep["fits"][2]["pad"]
    assert pad == 1.01 * (math.sqrt(3.0) * 0.02 + 0.01)
    # a world sphere d above the top face of l2's box (0.3 x 0.08 x 0.06, centred at (0.15, 0, 0) in frame 2) at the
    # zero configuration; every other solid of the arm is further from it than d + its pad
    x0 = np.zeros(3)
    T = robot.link_frames_batch_arrays(x0[None])[0]
    d, rw = 0.1, 0.05
    centre = T[2, :3, :3] @ np.array([0.15, 0.0, 0.03 + d + rw]) + T[2, :3, 3]
    robot.set_world(spheres=[[*centre, rw]])
    clr = robot.collision_clearance(x0)
    print("clearance", clr, "d", d, "pad", pad)
    assert d - pad - 1e-5 <= clr <= d + 1e-5
    # the installed frames are link_frames_batch_arrays': the model's spheres in the base frame, by hand
    s = spheres_at(robot, x0, frames, centers, radii)
    by_hand = min(np.linalg.norm(s[:, :3] - centre, axis=1) - s[:, 3] - rw)
    assert abs(by_hand - clr) <= 1e-12
    # frame 2 is where the URDF puts l2: 0.45 up, turned by 0.5 about z
    assert np.allclose(T[2, :3, 3], [0.0, 0.0, 0.45], atol=1e-15) and np.isclose(T[2, 1, 0], math.sin(0.5))
    # with "auto" pairs the pruned model is not in self-collision at the reference configuration
    _, _, _, rep2 = robot.set_collision_model_from_urdf(FIXTURE, "base", "tip", per_link=16, mesh_dir=str(tmp_path),
                                                        voxel=0.02, spacing=0.01)
    robot.set_world()
    assert len(rep2["pairs"]) > 0 and robot.collision_clearance(np.zeros(3)) >= 0.0
