"""CPU-only: the collision filter's arithmetic (optik_amd/csrc/collision_measure.hpp, built with g++) against numpy and
against constructed cases with exact answers, the "auto" self pairs and spheres_along_chain, the exported symbols, and
the refusals of the model and world arguments, which happen on the host before any device work."""
import math
import os

import numpy as np
import pytest

from collision_util import build_measure
from conftest import REF_GOLDEN, ROBOTS


@pytest.fixture(scope="module")
def built():
    from optik_amd import build
    build.build()
    from optik_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def measure(tmp_path_factory):
    return build_measure(str(tmp_path_factory.mktemp("collision_measure")))


@pytest.fixture(scope="module")
def panda(built):
    from optik_amd import Robot
    return Robot.from_urdf_file(os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8")


def _rot(q):
    i, j, k, w = q
    return np.array([[1 - 2 * (j * j + k * k), 2 * (i * j - k * w), 2 * (i * k + j * w)],
                     [2 * (i * j + k * w), 1 - 2 * (i * i + k * k), 2 * (j * k - i * w)],
                     [2 * (i * k - j * w), 2 * (j * k + i * w), 1 - 2 * (i * i + j * j)]])


def _unit_quats(rng, count):
    q = rng.normal(size=(count, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _np_sphere_box(p, r, box):
    local = _rot(box[3:7]).T @ (p - box[:3])
    e = np.abs(local) - box[7:10]
    return np.linalg.norm(np.maximum(e, 0.0)) + min(e.max(), 0.0) - r


def test_sphere_and_box_distances_match_numpy(measure):
    rng = np.random.default_rng(1)
    N = 4000
    recs = np.zeros((N, 15))
    want = np.zeros(N)
    for i in range(N):
        p = rng.uniform(-1, 1, 3)
        r = rng.uniform(0, 0.2)
        if i % 2 == 0:
            c, rb = rng.uniform(-1, 1, 3), rng.uniform(0, 0.3)
            recs[i] = np.concatenate([[0.0], p, [r], c, [rb], np.zeros(6)])
            want[i] = np.linalg.norm(p - c) - r - rb
        else:
            box = np.concatenate([rng.uniform(-1, 1, 3), _unit_quats(rng, 1)[0], rng.uniform(0.01, 0.5, 3)])
            recs[i] = np.concatenate([[1.0], p, [r], box])
            want[i] = _np_sphere_box(p, r, box)
    got = measure.primitives(recs)
    scale = np.maximum(1.0, np.abs(want))
    assert (np.abs(got - want) <= 1e-14 * scale * 8).all(), np.max(np.abs(got - want) / scale)
    # (the boxes: points outside and inside both occur)
    assert (want[1::2] + recs[1::2, 4] > 0).any() and (want[1::2] + recs[1::2, 4] < 0).any()


def test_dyadic_cases_are_exact(measure):
    ident = [0.0, 0.0, 0.0, 1.0]
    box = np.array([0.5, -0.25, 1.0] + ident + [0.25, 0.5, 0.125])
    recs = [
        # a sphere touching the +x face: clearance exactly 0
        np.concatenate([[1.0], [0.5 + 0.25 + 0.125, -0.25, 1.0], [0.125], box]),
        # the centre inside, 0.0625 from the nearest (+z) face: -0.0625 - r
        np.concatenate([[1.0], [0.5, -0.25, 1.0 + 0.0625], [0.25], box]),
        # outside a corner by (0.5, 0.5, 0.25)... along x and y only: sqrt(0.25 + 0) - r
        np.concatenate([[1.0], [0.5 + 0.25 + 0.5, -0.25 + 0.5 + 0.5, 1.0], [0.0], box]),
        # two spheres 3-4-5 apart, touching
        np.concatenate([[0.0], [0.0, 0.0, 0.0], [2.0], [3.0, 4.0, 0.0], [3.0], np.zeros(6)]),
        # a box turned by 90 degrees about z: its x half extent now lies along y
        np.concatenate([[1.0], [0.0, 0.75, 0.0], [0.25],
                        [0.0, 0.0, 0.0, 0.0, 0.0, math.sqrt(0.5), math.sqrt(0.5), 0.5, 0.125, 0.125]]),
    ]
    got = measure.primitives(np.array(recs))
    assert got[0] == 0.0
    assert got[1] == -0.0625 - 0.25
    assert got[2] == math.sqrt(0.5) and got[2] > 0
    assert got[3] == 0.0
    assert abs(got[4]) < 1e-15  # (the rotation is not dyadic: sqrt(0.5) rounds)
    # free at margin 0 means clearance >= 0: the touching sphere counts as free
    frames = np.array([[[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]]])
    c = measure.clearance(frames, [0], [[0.875, -0.25, 1.0]], [0.125], boxes=[box])
    assert c[0] == 0.0 and c[0] >= 0.0
    c = measure.clearance(frames, [0], [[0.5, -0.25, 1.0625]], [0.25], boxes=[box])
    assert c[0] == -0.3125


def test_clearance_is_the_minimum_and_nan_and_inf_rules(measure):
    rng = np.random.default_rng(3)
    nf, S, B = 5, 12, 50
    frames = np.zeros((B, nf, 7))
    frames[:, :, :3] = rng.uniform(-1, 1, (B, nf, 3))
    frames[:, :, 3:] = _unit_quats(rng, B * nf).reshape(B, nf, 4)
    sf = rng.integers(0, nf, S)
    centers = rng.uniform(-0.2, 0.2, (S, 3))
    radii = rng.uniform(0, 0.1, S)
    pairs = np.array([(a, b) for a in range(S) for b in range(S) if a < b and abs(sf[a] - sf[b]) >= 2])
    spheres = np.concatenate([rng.uniform(-1, 1, (7, 3)), rng.uniform(0, 0.2, (7, 1))], axis=1)
    boxes = np.concatenate([rng.uniform(-1, 1, (5, 3)), _unit_quats(rng, 5), rng.uniform(0.05, 0.3, (5, 3))], axis=1)
    got = measure.clearance(frames, sf, centers, radii, pairs, spheres, boxes)
    for b in range(B):
        world = []
        for s in range(S):
            fr = frames[b, sf[s]]
            p = fr[:3] + _rot(fr[3:]) @ centers[s]
            world += [np.linalg.norm(p - w[:3]) - radii[s] - w[3] for w in spheres]
            world += [_np_sphere_box(p, radii[s], bx) for bx in boxes]
        for a, c in pairs:
            pa = frames[b, sf[a], :3] + _rot(frames[b, sf[a], 3:]) @ centers[a]
            pc = frames[b, sf[c], :3] + _rot(frames[b, sf[c], 3:]) @ centers[c]
            world.append(np.linalg.norm(pa - pc) - radii[a] - radii[c])
        assert abs(got[b] - min(world)) <= 1e-13, b
    # nothing to check: +inf; a NaN frame: NaN
    assert measure.clearance(frames[:2], [], np.zeros((0, 3)), [])[0] == math.inf
    assert measure.clearance(frames[:2], sf, centers, radii)[0] == math.inf  # (no world, no pairs)
    bad = frames[:1].copy()
    bad[0, nf - 1, 0] = math.nan
    assert math.isnan(measure.clearance(bad, sf, centers, radii, pairs, spheres, boxes)[0])


def test_auto_pairs_and_spheres_along_chain(panda):
    from optik_amd.collision import auto_pairs, model_arrays, spheres_along_chain
    f = np.array([0, 0, 1, 2, 2, 4])
    pairs = auto_pairs(f)
    want = [(a, b) for a in range(6) for b in range(a + 1, 6) if abs(f[a] - f[b]) >= 2]
    assert [tuple(p) for p in pairs] == want and pairs.dtype == np.int32
    assert auto_pairs([]).shape == (0, 2)
    _, _, _, p0, _ = model_arrays(f, np.zeros((6, 3)), 0.1, None)
    assert p0.shape == (0, 2)
    frames, centers, radii = spheres_along_chain(panda, 0.05, 10)
    n = panda.num_positions()
    assert frames.dtype == np.int32 and centers.shape == (len(frames), 3) and radii.shape == (len(frames),)
    assert 30 <= len(frames) <= 40 and (radii == 0.05).all()
    assert frames.min() >= 0 and frames.max() <= n + 1
    origins = panda.chain_tables()["origins"]
    for k, c in zip(frames, centers):
        off = origins[k, :3]
        # on the segment from frame k's origin to frame k + 1's, at least 1.5 radii from both joints
        s = float(np.dot(c, off) / np.dot(off, off))
        length = float(np.linalg.norm(off))
        assert np.allclose(c, s * off, atol=1e-15)
        assert 0.075 * (1 - 1e-12) <= s * length <= length - 0.075 * (1 - 1e-12)
    # zero-length segments (the Panda's joints 2 and 6) and short ones (the wrist, the flange) get no spheres
    assert set(frames.tolist()) == {0, 2, 4}
    with pytest.raises(ValueError):
        spheres_along_chain(panda, 0.0, 4)


def test_collision_symbols_are_exported(built):
    for s in ("optik_hip_chain_set_collision_model", "optik_hip_chain_set_world", "optik_hip_link_frames_batch",
              "optik_hip_collision_batch", "optik_robot_set_collision_model", "optik_robot_set_world",
              "optik_robot_link_frames_batch", "optik_robot_collision_batch"):
        assert hasattr(built, s), f"{s} is not exported by liboptik_amd.so"


def test_refusals_happen_before_any_device_work(panda):
    """None of these calls touches a device (the robot has created no device context: no chain exists)."""
    from optik_amd import Robot
    n = panda.num_positions()
    c3 = [[0.0, 0.0, 0.0]]
    for kw, what in [
        (dict(frames=[n + 2], centers=c3, radii=[0.1]), "frame"),
        (dict(frames=[-1], centers=c3, radii=[0.1]), "frame"),
        (dict(frames=[1], centers=c3, radii=[-0.1]), "radius"),
        (dict(frames=[1], centers=c3, radii=[math.nan]), "radius"),
        (dict(frames=[1], centers=[[math.nan, 0, 0]], radii=[0.1]), "centre"),
        (dict(frames=[1, 3], centers=c3 * 2, radii=[0.1, 0.1], self_pairs=[[0, 2]]), "out of range"),
        (dict(frames=[1, 3], centers=c3 * 2, radii=[0.1, 0.1], self_pairs=[[1, 1]]), "itself"),
        (dict(frames=[1], centers=c3, radii=[0.1], margin=-0.01), "margin"),
        (dict(frames=[1], centers=c3, radii=[0.1], margin=math.nan), "margin"),
        (dict(frames=[1], centers=c3, radii=[0.1], margin=math.inf), "margin"),
        (dict(frames=[1] * 257, centers=c3 * 257, radii=[0.1] * 257, self_pairs=None), "sphere count"),
        (dict(frames=list(range(9)) * 20, centers=c3 * 180, radii=[0.1] * 180), "pair count"),
    ]:
        with pytest.raises(ValueError, match=what):
            panda.set_collision_model(**kw)
    unit = [0.0, 0.0, 0.0, 1.0]
    for kw, what in [
        (dict(spheres=[[0, 0, 0, -1.0]]), "radius"),
        (dict(spheres=[[0, 0, 0, math.nan]]), "radius"),
        (dict(spheres=[[math.inf, 0, 0, 1.0]]), "centre"),
        (dict(boxes=[[0, 0, 0] + unit + [0.1, -0.1, 0.1]]), "half extent"),
        (dict(boxes=[[0, 0, 0] + unit + [0.1, math.nan, 0.1]]), "half extent"),
        (dict(boxes=[[0, 0, 0, 0.0, 0.0, 0.0, 1.0 + 1e-8, 0.1, 0.1, 0.1]]), "unit quaternion"),
        (dict(spheres=np.zeros((65537, 4))), "at most"),
    ]:
        with pytest.raises(ValueError, match=what):
            panda.set_world(**kw)
    # accepted: |q|^2 within 1e-9 of 1, a zero radius, a margin of 0; then cleared
    panda.set_world(spheres=[[0, 0, 0, 0.0]], boxes=[[0, 0, 0, 0.0, 0.0, 0.0, 1.0 + 4e-10, 0.1, 0.1, 0.1]])
    panda.set_collision_model([0, n + 1], [[0, 0, 0], [0, 0, 0]], [0.0, 0.1], margin=0.0)
    panda.clear_collision_model()
    panda.set_world()
    with pytest.raises(ValueError):
        panda.set_collision_model([1], c3, [0.1], self_pairs="all")
    # a prismatic chain: refused whatever the device
    gantry = Robot.from_urdf_file(os.path.join(os.path.dirname(REF_GOLDEN), "robots", "gantry.urdf"), "g0", "g5")
    with pytest.raises(ValueError, match="prismatic"):
        gantry.set_collision_model([1], c3, [0.1])
