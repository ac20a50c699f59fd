"""-m gpu: depth-image worlds -- the kernels of ik_depth.hip bit for bit against the serial
reference of depth_measure.hpp (g++, tests/depth_util.py) through HipChain and Robot, the later trips of their
grid-stride loops under a capped grid into sentinel-filled outputs, set_world_depth end to end, and the example.  No
tolerance anywhere: every comparison is exact."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import depth_util as du
from conftest import ROBOT_SPECS, ROOT
from depth_util import K, ORIGIN, PARAMS, SHAPE, UNKNOWN, VOXEL
from occupancy_util import field_reference

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = du.cases()
SENTINEL = 12345  # (no update gives it: every update ends in [e_min, e_max])


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return du.build_depth_ref(str(tmp_path_factory.mktemp("gpu_depth_measure")))


@pytest.fixture(scope="module")
def wants(ref):
    """Every case's map from the serial reference, computed once."""
    return {name: ref.integrate(c["map"], ORIGIN, VOXEL, c["depth"], c["intrinsics"], c["poses"], c["exclude"],
                                **c["params"]) for name, c in CASES}


@pytest.fixture(scope="module")
def hc():
    from oracle import urdf_chain
    from optik_amd import device
    path, base, ee = ROBOT_SPECS["panda"]
    with open(path) as fh:
        return device.HipChain(**urdf_chain.chain_from_urdf(fh.read(), base, ee))


@pytest.fixture(scope="module")
def panda():
    from optik_amd import Robot
    return Robot.from_urdf_file(*ROBOT_SPECS["panda"])


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _finite(exclude):
    """The robot layer sees the numbers and refuses a non-finite exclusion sphere; such a sphere excludes nothing
    (depth_measure.hpp, step 1), so the reference's answer with it is the answer without it."""
    return None if exclude is None else exclude[np.isfinite(exclude).all(axis=1)]


def _hip_integrate(hc, c, map=None, **over):
    m = _dev(c["map"] if map is None else map)
    exc = None if c["exclude"] is None else _dev(np.asarray(c["exclude"], dtype=np.float64))
    out = hc.depth_integrate(m, ORIGIN, VOXEL, _dev(np.asarray(c["depth"], dtype=np.float32)), c["intrinsics"], c["poses"],
                             exc, **dict(PARAMS, **c["params"], **over))
    torch.cuda.synchronize()
    assert out is m
    return m.cpu().numpy()


@pytest.mark.parametrize("name,case", CASES, ids=[n for n, _ in CASES])
def test_hip_chain_integrate_equals_reference(hc, wants, name, case):
    got = _hip_integrate(hc, case)
    assert got.dtype == np.int16 and np.array_equal(got, wants[name]), name


@pytest.mark.parametrize("name,case", CASES, ids=[n for n, _ in CASES])
def test_robot_integrate_equals_reference(panda, wants, name, case):
    before = case["map"].copy()
    got = panda.depth_integrate(case["map"], ORIGIN, VOXEL, case["depth"], case["intrinsics"], case["poses"],
                                _finite(case["exclude"]), **dict(PARAMS, **case["params"]))
    assert got.dtype == np.int16 and np.array_equal(got, wants[name]), name
    assert np.array_equal(case["map"], before), "the caller's map is not modified"


def test_frames_in_one_call_equal_single_calls(hc, panda, wants):
    case = dict(CASES)["frames3"]
    m, mr = case["map"], case["map"]
    for f in range(3):
        one = dict(case, depth=case["depth"][f], intrinsics=case["intrinsics"][f], poses=case["poses"][f])
        m = _hip_integrate(hc, one, map=m)
        mr = panda.depth_integrate(mr, ORIGIN, VOXEL, one["depth"], one["intrinsics"], one["poses"],
                                   _finite(one["exclude"]), **PARAMS)
    assert np.array_equal(m, wants["frames3"]) and np.array_equal(mr, wants["frames3"])


def test_more_frames_than_one_launch_takes(hc, ref):
    """11 frames: a launch of 8 and one of 3 (ik_depth.hip: FRAMES_PER_LAUNCH)."""
    case = dict(CASES)["frames3"]
    idx = [0, 1, 2, 1, 0, 2, 2, 1, 0, 0, 1]
    many = dict(case, depth=case["depth"][idx], intrinsics=case["intrinsics"][idx], poses=case["poses"][idx])
    want = ref.integrate(many["map"], ORIGIN, VOXEL, many["depth"], many["intrinsics"], many["poses"], many["exclude"])
    assert np.array_equal(_hip_integrate(hc, many), want)


def test_occupancy_from_map(hc, panda, ref, wants):
    m = wants["tilted"]
    cloud = (np.random.default_rng(3).random(SHAPE) < 0.1).astype(np.uint8)
    for threshold in (-1, 1, 3):
        for unknown in (False, True):
            want = ref.occupancy(m, threshold, unknown)
            got = hc.occupancy_from_map(_dev(m), threshold, unknown)
            assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
            got_r = panda.occupancy_from_map(m, threshold, unknown)
            assert got_r.dtype == bool and np.array_equal(got_r.view(np.uint8), want)
            into = _dev(cloud)
            assert hc.occupancy_from_map(_dev(m), threshold, unknown, into=into) is into
            assert np.array_equal(into.cpu().numpy(), ref.occupancy(m, threshold, unknown, into=cloud))
            assert np.array_equal(panda.occupancy_from_map(m, threshold, unknown, into=cloud.view(bool)).view(np.uint8),
                                  cloud | want)


# ---- the later trips of the grid-stride loops ------------------------------------------------------------------------
# 805 = 3 * 256 + 37 nodes and as many pixels (tests/test_gpu_grid_stride.py): under grid_cap = 1 four trips of one
# block, the last with 37 live lanes; under grid_cap = 3 a ragged second trip of one block out of three.
STRIDE_SHAPE, STRIDE_IMG = (7, 5, 23), (23, 35)


def _stride_case():
    rng = np.random.default_rng(805)
    img = np.stack([rng.uniform(0.15, 0.7, STRIDE_IMG), rng.uniform(0.3, 0.5, STRIDE_IMG)]).astype(np.float32)
    img[0][rng.random(STRIDE_IMG) < 0.05] = np.nan
    img[1][rng.random(STRIDE_IMG) < 0.05] = 3.0
    k = np.array([22.0, 21.0, 17.0, 11.0])
    poses = np.stack([du.pose(), du.pose(du.rot(1, 0.3) @ du.rot(0, -0.2), (-0.15, 0.02, 0.05))])
    origin = np.array([-0.15, -0.1, 0.1])
    exclude = np.array([[0.0, 0.0, 0.4, 0.1], [0.1, 0.05, 0.3, 0.04]])
    seen = rng.integers(-7, 12, STRIDE_SHAPE).astype(np.int16)
    seen[rng.random(STRIDE_SHAPE) < 0.3] = UNKNOWN
    return dict(origin=origin, depth=img, k=k, poses=poses, exclude=exclude, seen=seen)


def test_capped_grids(hc, ref):
    from optik_amd import _native as nat
    assert np.prod(STRIDE_SHAPE) == np.prod(STRIDE_IMG) == 805
    c = _stride_case()
    args = (c["origin"], VOXEL, c["depth"], c["k"], c["poses"], c["exclude"])
    # the nodes no frame updates hold a value that no update produces, and must hold it afterwards
    touched = ref.integrate(du.new_map(STRIDE_SHAPE), *args) != UNKNOWN
    assert 200 <= touched.sum() <= 700
    start = np.where(touched, c["seen"], SENTINEL).astype(np.int16)
    want = ref.integrate(start, *args)
    assert (want[~touched] == SENTINEL).all() and (want[touched] != SENTINEL).all() and (want != start).sum() >= 150
    want_occ = ref.occupancy(want, 2, True)
    assert 0 < want_occ.sum() < want_occ.size
    d_depth, d_exc = _dev(c["depth"]), _dev(c["exclude"])
    res = {}
    for cap in (0, 1, 3):
        m = _dev(start)
        occ = torch.full(STRIDE_SHAPE, 0xAB, dtype=torch.uint8, device="cuda")
        with nat.options(grid_cap=cap):
            assert nat.get_option("grid_cap") == cap
            hc.depth_integrate(m, c["origin"], VOXEL, d_depth, c["k"], c["poses"], d_exc, **PARAMS)
            nat.check(nat.lib().optik_hip_occupancy_from_map(hc._h, *STRIDE_SHAPE, m.data_ptr(), 2, 1, 0, occ.data_ptr(),
                                                             torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
        res[cap] = (m.cpu().numpy(), occ.cpu().numpy())
        assert np.array_equal(res[cap][0], want), f"map, cap {cap}"
        assert (res[cap][1] != 0xAB).all() and np.array_equal(res[cap][1], want_occ), f"occupancy, cap {cap}"
        assert res[cap][0].tobytes() == res[0][0].tobytes() and res[cap][1].tobytes() == res[0][1].tobytes(), \
            f"cap {cap} vs the uncapped launch"


# ---- refusals of the kernel layer ----------------------------------------------------------------------------------------
def test_kernel_layer_refusals(hc):
    from optik_amd import _native as nat
    case = dict(CASES)["wall"]
    m = _dev(case["map"])
    d = _dev(case["depth"])

    def refused(what, map=m, origin=ORIGIN, voxel=VOXEL, depth=d, intrinsics=K, poses=du.pose(), **kw):
        with pytest.raises(nat.OptikHipError, match=what):
            hc.depth_integrate(map, origin, voxel, depth, intrinsics, poses, **dict(PARAMS, **kw))

    refused(r"2\.\.1024", map=_dev(du.new_map((1, 3, 4))))
    refused("voxel", voxel=0.0)
    refused("origin", origin=[0.0, math.nan, 0.0])
    refused(r"1\.\.64", depth=_dev(np.zeros((65, 2, 2), dtype=np.float32)), poses=np.stack([du.pose()] * 65))
    refused(r"1\.\.4096", depth=_dev(np.zeros((1, 4097), dtype=np.float32)))
    refused("intrinsics", intrinsics=[0.0, 20.0, 1.0, 1.0])
    refused("intrinsics", intrinsics=[20.0, 20.0, math.nan, 1.0])
    refused(r"0\.\.1024", exclude=_dev(np.zeros((1025, 4))))
    refused("z_near", z_near=0.0)
    refused("z_near", z_far=PARAMS["z_near"])
    refused("band", band=-1.0)
    refused(r"1\.\.1024", hit=0)
    refused(r"1\.\.1024", miss=1025)
    refused("e_min", e_min=1)
    refused("e_min", e_max=32768)
    with pytest.raises(nat.OptikHipError, match="threshold"):
        hc.occupancy_from_map(m, 32768)
    # the C ABI itself: null buffers that are needed (OPTIK_HIP_EINVAL = -1)
    L, dp = nat.lib(), C.POINTER(C.c_double)
    zero3, k_arr, eye = np.zeros(3), np.ascontiguousarray(K), np.eye(4).ravel()
    o3, k4, p16 = zero3.ctypes.data_as(dp), k_arr.ctypes.data_as(dp), eye.ctypes.data_as(dp)
    tail = (0.1, 0.8, 0.05, 3, 2, -7, 11, None)
    rc_map = L.optik_hip_depth_integrate(hc._h, o3, VOXEL, *SHAPE, None, d.data_ptr(), 1, *du.IMG, k4, p16, None, 0, *tail)
    rc_img = L.optik_hip_depth_integrate(hc._h, o3, VOXEL, *SHAPE, m.data_ptr(), None, 1, *du.IMG, k4, p16, None, 0, *tail)
    rc_exc = L.optik_hip_depth_integrate(hc._h, o3, VOXEL, *SHAPE, m.data_ptr(), d.data_ptr(), 1, *du.IMG, k4, p16, None, 1,
                                         *tail)
    rc_cam = L.optik_hip_depth_integrate(hc._h, o3, VOXEL, *SHAPE, m.data_ptr(), d.data_ptr(), 1, *du.IMG, None, p16, None,
                                         0, *tail)
    assert rc_map == rc_img == rc_exc == rc_cam == -1
    assert L.optik_hip_occupancy_from_map(hc._h, *SHAPE, None, 1, 0, 0, m.data_ptr(), None) == rc_map
    torch.cuda.synchronize()
    assert np.array_equal(m.cpu().numpy(), case["map"]), "a refused call does no device work"


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_set_world_depth_end_to_end(ref):
    from optik_amd import Robot
    from optik_amd.collision import default_max_distance, spheres_along_chain
    robots = [Robot.from_urdf_file(*ROBOT_SPECS["panda"]) for _ in range(2)]
    frames, centers, radii = spheres_along_chain(robots[0], 0.05, 2)
    for r in robots:
        r.set_collision_model(frames, centers, radii, self_pairs=None, margin=0.0)
    case = dict(CASES)["frames3"]
    threshold = 3
    m, values = robots[0].set_world_depth(case["map"], ORIGIN, VOXEL, case["depth"], case["intrinsics"], case["poses"],
                                          _finite(case["exclude"]), threshold=threshold, unknown_occupied=False,
                                          **PARAMS)
    want_map = ref.integrate(case["map"], ORIGIN, VOXEL, case["depth"], case["intrinsics"], case["poses"], case["exclude"])
    assert np.array_equal(m, want_map)
    occ = ref.occupancy(want_map, threshold, False)
    assert 20 <= occ.sum() < occ.size
    want = field_reference(VOXEL, occ, default_max_distance(VOXEL, SHAPE))
    assert values.dtype == np.float32 and np.array_equal(values.view(np.uint32), want.view(np.uint32))
    # the installed grid is read by the consumers: the clearance is what set_world_grid of the same values gives
    robots[1].set_world_grid(ORIGIN, VOXEL, values)
    x = np.array([[0.0, 0.3, 0.0, -1.6, 0.0, 1.9, 0.7]])
    c0, f0 = robots[0].collision_clearance_batch_arrays(x)
    c1, f1 = robots[1].collision_clearance_batch_arrays(x)
    assert np.isfinite(c0).all(), "a robot sphere lies inside the grid"
    assert np.array_equal(c0.view(np.uint64), c1.view(np.uint64)) and np.array_equal(f0, f1)


def test_ik_world_depth_example():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ik_world_depth.py"), *ROBOT_SPECS["panda"]],
                         env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-2000:]
    assert "with the box: no collision-free solution" in res.stdout, res.stdout
    assert "box removed: reachable: True" in res.stdout, res.stdout
