"""CPU-only: the motion check's arithmetic (optik_amd/csrc/motion_measure.hpp, built with g++) against numpy written in
the documented order, against coll::clearance over the samples' frames, and against constructed scenes whose answers
are known exactly; the exported symbols and the refusals that happen on the host before any device work."""
import math
import os

import numpy as np
import pytest

from collision_util import build_measure
from conftest import ROBOTS
from motion_util import MAX_STEPS, build_motion, np_frames7, np_reduce, np_samples


@pytest.fixture(scope="module")
def built():
    from optik_amd import build
    build.build()
    from optik_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def motion(tmp_path_factory):
    return build_motion(str(tmp_path_factory.mktemp("motion_measure")))


@pytest.fixture(scope="module")
def measure(tmp_path_factory):
    return build_measure(str(tmp_path_factory.mktemp("collision_measure")))


@pytest.fixture(scope="module")
def panda(built):
    from optik_amd import Robot
    return Robot.from_urdf_file(os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_samples_match_numpy_bit_for_bit(motion):
    rng = np.random.default_rng(5)
    n, h = 7, 0.0625
    qa = rng.uniform(-2.5, 2.5, (40, n))
    qb = qa + rng.uniform(-1.0, 1.0, (40, n)) * rng.choice([0.01, 0.3, 3.0], (40, 1))
    qb[0] = qa[0]                                     # d = 0: K = 1, two samples
    qb[1] = qa[1]; qb[1, 3] = qa[1, 3] + 0.5          # maybe not exactly 8 h after the rounding of the sum ...
    qa[2] = 0.0; qb[2] = 0.0; qb[2, 2] = -0.5         # ... so: d = 8 h exactly
    qa[3] = 0.0; qb[3] = 0.0; qb[3, 5] = np.nextafter(0.5, 1.0)  # just above 8 h: one step more
    qa[4] = 0.0; qb[4] = 0.0; qb[4, 0] = h            # exactly one step
    qa[5] = 0.0; qb[5] = 0.0; qb[5, 0] = np.nextafter(h, 1.0)
    got = motion.samples(qa, qb, h)
    for b in range(len(qa)):
        d, K, s = np_samples(qa[b], qb[b], h)
        gd, gK, gs = got[b]
        assert _bits(gd) == _bits(d) and gK == K, b
        assert gs.shape == (K + 1, n)
        assert np.array_equal(_bits(gs), _bits(s)), b
        # the endpoints are reproduced, not computed
        assert np.array_equal(_bits(gs[0]), _bits(qa[b])) and np.array_equal(_bits(gs[K]), _bits(qb[b]))
    assert got[0][1] == 1 and got[0][0] == 0.0
    assert got[2][1] == 8 and got[3][1] == 9 and got[4][1] == 1 and got[5][1] == 2
    assert {g[1] for g in got} >= {1, 2, 8, 9} and max(g[1] for g in got) > 40


def test_over_limit_and_non_finite_segments_are_not_sampled(motion):
    h = 0.001
    z = np.zeros(3)
    qa = np.array([z, z, z, [math.nan, 0, 0], z, z, [0, math.nan, 0]])
    qb = np.array([[MAX_STEPS * h, 0, 0], [np.nextafter(MAX_STEPS * h, 10.0) + h, 0, 0], [0, 5.0, 0], z,
                   [0, 0, math.inf], [0, -math.inf, 0], [7.0, 0, 0]])
    got = motion.samples(qa, qb, h)
    assert got[0][1] == np_samples(qa[0], qb[0], h)[1] and 1 <= got[0][1] <= MAX_STEPS
    assert got[1][1] == -1 and got[2][1] == -1           # more than 4096 steps
    assert got[3][1] == -1 and math.isnan(got[3][0])     # NaN in qa
    assert got[4][1] == -1 and got[4][0] == math.inf     # infinite d
    assert got[5][1] == -1 and got[5][0] == math.inf
    assert got[6][1] == -1 and math.isnan(got[6][0])     # a NaN joint is not lost behind a larger finite one
    for g, a, b in zip(got, qa, qb):
        assert g[1] == np_samples(a, b, h)[1]
    clr, free, first, steps = motion.reduce([-1], [None], 0.0, [], np.zeros((0, 3)), [])
    assert math.isnan(clr[0]) and not free[0] and first[0] == -1 and steps[0] == -1


def _panda_chain(panda):
    return panda.chain_tables()


def test_motion_clearance_is_the_minimum_over_the_samples(motion, measure, panda):
    from optik_amd.collision import auto_pairs, spheres_along_chain
    d = _panda_chain(panda)
    lb, ub = (np.asarray(v) for v in panda.joint_limits())
    frames, centers, radii = spheres_along_chain(panda, 0.05, 8)
    pairs = auto_pairs(frames)
    rng = np.random.default_rng(11)
    sph = np.concatenate([rng.uniform(-0.7, 0.7, (10, 3)), rng.uniform(0.03, 0.1, (10, 1))], 1)
    q4 = rng.normal(size=(4, 4))
    box = np.concatenate([rng.uniform(-0.7, 0.7, (4, 3)), q4 / np.linalg.norm(q4, axis=1, keepdims=True),
                          rng.uniform(0.03, 0.12, (4, 3))], 1)
    margin, h = 0.01, 0.05
    B = 12
    qa = rng.uniform(lb, ub, (B, 7))
    qb = np.clip(qa + rng.uniform(-0.6, 0.6, (B, 7)), lb, ub)
    Ks, fr = [], []
    for b in range(B):
        _, K, s = np_samples(qa[b], qb[b], h)
        Ks.append(K)
        fr.append(np.array([np_frames7(d, q) for q in s]))
    clr, free, first, steps = motion.reduce(Ks, fr, margin, frames, centers, radii, pairs, sph, box)
    blocked = 0
    for b in range(B):
        per = measure.clearance(fr[b], frames, centers, radii, pairs, sph, box)
        want = np_reduce(Ks[b], per, margin)
        assert _bits(clr[b]) == _bits(want[0]) and free[b] == want[1] and first[b] == want[2] and steps[b] == want[3]
        blocked += not want[1]
        # and against plain numpy distances from the same numpy frames (world spheres and self pairs)
        lo = math.inf
        for f7 in fr[b]:
            p = np.array([f7[frames[s], :3] + _rot(f7[frames[s], 3:]) @ centers[s] for s in range(len(frames))])
            lo = min(lo, min(np.linalg.norm(p[s] - w[:3]) - radii[s] - w[3] for s in range(len(p)) for w in sph))
            lo = min(lo, min(np.linalg.norm(p[a] - p[c]) - radii[a] - radii[c] for a, c in pairs))
        per_s = measure.clearance(fr[b], frames, centers, radii, pairs, sph, None)
        assert abs(per_s.min() - lo) <= 1e-14 * max(1.0, abs(lo)) * 8
    assert 0 < blocked < B
    # a NaN sample: NaN clearance, not free, first at that sample
    bad = fr[0].copy()
    bad[2, 3, 0] = math.nan
    c, f, k, _ = motion.reduce([Ks[0]], [bad], 0.0, frames, centers, radii, None, sph[:1] + 100.0, None)
    assert math.isnan(c[0]) and not f[0] and k[0] == 2
    # nothing to check: +inf and free
    c, f, k, st = motion.reduce([Ks[0]], [fr[0]], 0.0, [], np.zeros((0, 3)), [])
    assert c[0] == math.inf and f[0] and k[0] == -1 and st[0] == Ks[0]


def _rot(q):
    i, j, k, w = q
    return np.array([[1 - 2 * (j * j + k * k), 2 * (i * j - k * w), 2 * (i * k + j * w)],
                     [2 * (i * j + k * w), 1 - 2 * (i * i + k * k), 2 * (j * k - i * w)],
                     [2 * (i * k - j * w), 2 * (j * k + i * w), 1 - 2 * (i * i + j * j)]])


def test_dyadic_sweep_through_a_unit_box(motion):
    """A 1-joint arm about z: a sphere of radius 0.25 at (2, 0, 0) in the joint's frame swings from q = -1 to q = +1
    through a unit box centred at (2, 0, 0).  Its centre is (2 cos q, 2 sin q, 0); it is not free while
    2 |sin q| - 0.5 < 0.25, that is |q| < 0.3844.  The samples are dyadic, so K and first are known exactly, and at
    q = 0 the centre is the box's: clearance -0.5 - 0.25."""
    chain = dict(origins=np.array([[0.0, 0, 0, 0, 0, 0, 1]]), axes=np.array([[0.0, 0, 1]]))
    box = [[2.0, 0, 0, 0, 0, 0, 1, 0.5, 0.5, 0.5]]
    qa, qb = np.array([[-1.0]]), np.array([[1.0]])
    for h, K, first in [(0.125, 16, 5), (0.25, 8, 3), (0.5, 4, 2), (1.0, 2, 1), (0.75, 3, 1), (2.0, 1, -1)]:
        (d, gK, s), = motion.samples(qa, qb, h)
        assert d == 2.0 and gK == K
        assert np.array_equal(s[:, 0], -1.0 + 2.0 * np.arange(K + 1) / K)
        fr = np.array([np_frames7(chain, q) for q in s])
        clr, free, gfirst, steps = motion.reduce([K], [fr], 0.0, [1], [[2.0, 0, 0]], [0.25], boxes=box)
        assert steps[0] == K and gfirst[0] == first and free[0] == (first < 0), h
        if K % 2 == 0:
            assert clr[0] == -0.75, h  # (the sample at q = 0)
        else:
            assert (clr[0] < 0.0) == (first >= 0)
    # h = 2 checks the endpoints only: both are free, and the wall between them goes unnoticed -- the case the
    # resolution is there for; a margin of 1.25 blocks the first sample already
    fr = np.array([np_frames7(chain, q) for q in np_samples(qa[0], qb[0], 0.125)[2]])
    _, free, first, _ = motion.reduce([16], [fr], 1.25, [1], [[2.0, 0, 0]], [0.25], boxes=box)
    assert not free[0] and first[0] == 0


def test_motion_symbols_are_exported(built):
    for s in ("optik_hip_collision_motion_batch", "optik_hip_chain_set_motion_resolution",
              "optik_robot_collision_motion_batch", "optik_robot_set_motion_resolution"):
        assert hasattr(built, s), f"{s} is not exported by liboptik_amd.so"


def test_refusals_happen_before_any_device_work(panda):
    """None of these calls touches a device (the robot has created no device context)."""
    n = panda.num_positions()
    for h in (math.nan, -0.1, math.inf):
        with pytest.raises(ValueError, match="resolution"):
            panda.set_motion_resolution(h)
    panda.set_motion_resolution(0.05)
    panda.set_motion_resolution(0)
    z = np.zeros((2, n))
    for h in (math.nan, 0.0, -1.0, math.inf):
        with pytest.raises(ValueError, match="resolution"):
            panda.collision_motion_batch_arrays(z, z, h)
    with pytest.raises(ValueError):
        panda.collision_motion_batch_arrays(z, np.zeros((3, n)), 0.1)
    with pytest.raises(ValueError):
        panda.collision_motion_batch_arrays(np.zeros((2, n - 1)), np.zeros((2, n - 1)), 0.1)
    # the C ABI refuses the same without a device
    L = panda._L
    for h in (math.nan, -0.1, math.inf):
        assert L.optik_robot_set_motion_resolution(panda._h, h) == -1
        assert b"resolution" in L.optik_robot_last_error()
