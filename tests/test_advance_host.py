"""CPU-only: the certified motion check's arithmetic (optik_amd/csrc/advance_measure.hpp, built with g++): the reach
table and both speed bounds against hand-written values and against the displacements a numpy FK actually produces,
the walk on constructed scenes whose answers are known, the outside-grid rule, the exported symbols and the refusals
that happen on the host before any device work."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from advance_util import BLOCKED, FREE, LIMIT, NOT_A_NUMBER, Scene, build_advance
from conftest import ROBOTS
from motion_util import np_frames7, np_samples


@pytest.fixture(scope="module")
def adv(tmp_path_factory):
    return build_advance(str(tmp_path_factory.mktemp("advance_measure")))


@pytest.fixture(scope="module")
def built():
    from optik_amd import build
    build.build()
    from optik_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def panda(built):
    from optik_amd import Robot
    return Robot.from_urdf_file(os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8")


# A planar arm: joint 1 at the base, joint 2 one metre along x behind it, both about z, and a fixed tip half a metre
# further.  Frames 0 .. 3; at q = 0 the end effector sits at (1.5, 0, 0).
PLANAR = dict(origins=np.array([[0.0, 0, 0, 0, 0, 0, 1], [1.0, 0, 0, 0, 0, 0, 1], [0.5, 0, 0, 0, 0, 0, 1]]),
              axes=np.array([[0.0, 0, 1], [0.0, 0, 1]]))


def spatial_chain(seed, n=5):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n + 1, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    ax = rng.normal(size=(n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    return dict(origins=np.concatenate([rng.uniform(-0.4, 0.4, (n + 1, 3)), q], 1), axes=ax)


def _rot(q):
    i, j, k, w = q
    return np.array([[1 - 2 * (j * j + k * k), 2 * (i * j - k * w), 2 * (i * k + j * w)],
                     [2 * (i * j + k * w), 1 - 2 * (i * i + k * k), 2 * (j * k - i * w)],
                     [2 * (i * k - j * w), 2 * (j * k + i * w), 1 - 2 * (i * i + j * j)]])


def centre(f7, f, c):
    return f7[f, :3] + _rot(f7[f, 3:]) @ np.asarray(c)


def frames_fn(chain, ee7=None):
    return lambda q: np.array([np_frames7(chain, row, ee7) for row in q])


def test_reach_and_speeds_of_a_hand_made_chain(adv):
    R = adv.reach(PLANAR, 2)
    want = np.zeros_like(R)
    want[0, 2], want[0, 3], want[1, 3] = 1.0, 1.5, 0.5
    assert np.array_equal(R, want)
    # an ee_offset lengthens the last link: |(0, 0.25, 0)| = 0.25, whatever its rotation
    R2 = adv.reach(PLANAR, 2, [0.0, 0.25, 0.0, 0.0, 0.0, math.sin(0.3), math.cos(0.3)])
    want[0, 3], want[1, 3] = 1.75, 0.75
    assert np.array_equal(R2, want)
    # without the fixed tip frame 3 is frame 2
    R3 = adv.reach(dict(origins=PLANAR["origins"][:2]), 2)
    assert R3[0, 2] == 1.0 and R3[0, 3] == 1.0 and R3[1, 3] == 0.0
    a = np.array([0.5, 0.25])
    c = [0.3, 0.4, 0.0]  # |c| = 0.5
    assert adv.lam_sphere(2, 0, a, R, c) == 0.0
    assert adv.lam_sphere(2, 1, a, R, c) == 0.5 * (0.0 + 0.5)
    assert adv.lam_sphere(2, 2, a, R, c) == 0.5 * (1.0 + 0.5) + 0.25 * (0.0 + 0.5)
    assert adv.lam_sphere(2, 3, a, R, c) == 0.5 * (1.5 + 0.5) + 0.25 * (0.5 + 0.5)
    z = [0.0, 0.0, 0.0]
    # a pair: only the joints between the frames, with the reach and |c| of the sphere on the higher frame
    assert adv.pair_lam(2, 1, z, 3, c, a, R) == 0.25 * (0.5 + 0.5)
    assert adv.pair_lam(2, 3, c, 1, z, a, R) == 0.25 * (0.5 + 0.5)          # stored the other way round
    assert adv.pair_lam(2, 0, z, 3, c, a, R) == 0.5 * (1.5 + 0.5) + 0.25 * (0.5 + 0.5)
    assert adv.pair_lam(2, 0, c, 2, z, a, R) == 0.5 * 1.0 + 0.25 * 0.0      # |c| of the LOWER sphere plays no part
    assert adv.pair_lam(2, 2, c, 2, z, a, R) == 0.0 and adv.pair_lam(2, 3, c, 3, c, a, R) == 0.0
    assert adv.pair_lam(2, 2, z, 3, c, a, R) == 0.0                          # frames 2 and 3: no joint between them


@pytest.mark.parametrize("name", ["planar", "spatial5"])
def test_speed_bounds_hold_for_random_motions(adv, name):
    chain, n = (PLANAR, 2) if name == "planar" else (spatial_chain(3), 5)
    rng = np.random.default_rng(17)
    ee7 = None if name == "planar" else np.array([0.05, -0.1, 0.2, 0.0, 0.0, math.sin(0.2), math.cos(0.2)])
    R = adv.reach(chain, n, ee7)
    worst = worst_pair = 0.0
    # The bound is on the true displacement; the two positions come from a numpy FK that rounds: about 10 operations
    # per joint on coordinates of at most 4 m, an ulp (4.4e-16 at 4 m) each, over 6 transforms and two poses.
    fk_rounding = 1e-13
    for _ in range(2000):
        qa = rng.uniform(-3.0, 3.0, n)
        dq = rng.uniform(-2.0, 2.0, n) * rng.choice([0.0, 1.0], n, p=[0.2, 0.8])
        a = np.abs(dq)
        t = rng.uniform(0.0, 1.0)
        dt = rng.uniform(0.0, 1.0 - t) * rng.choice([1e-3, 0.05, 1.0])
        f0, f1 = np_frames7(chain, qa + t * dq, ee7), np_frames7(chain, qa + (t + dt) * dq, ee7)
        fs, fo = rng.integers(0, n + 2, 2)
        cs, co = rng.uniform(-0.3, 0.3, 3), rng.uniform(-0.3, 0.3, 3)
        ps0, ps1, po0, po1 = centre(f0, fs, cs), centre(f1, fs, cs), centre(f0, fo, co), centre(f1, fo, co)
        lam = adv.lam_sphere(n, fs, a, R, cs)
        moved = np.linalg.norm(ps1 - ps0)
        assert moved <= lam * dt * (1 + 1e-12) + fk_rounding, (fs, moved, lam * dt)
        lam_p = adv.pair_lam(n, fs, cs, fo, co, a, R)
        change = abs(np.linalg.norm(ps1 - po1) - np.linalg.norm(ps0 - po0))
        assert change <= lam_p * dt * (1 + 1e-12) + fk_rounding, (fs, fo, change, lam_p * dt)
        if lam * dt > 0:
            worst = max(worst, moved / (lam * dt))
        if lam_p * dt > 0:
            worst_pair = max(worst_pair, change / (lam_p * dt))
    # the bounds are not vacuous: some motion comes within a factor of two of them
    assert worst > 0.5 and worst_pair > 0.5 if name == "planar" else worst > 0.2


def _wall(angle, half_thickness):
    """A thin plate across the end effector's circle of radius 1.5, at `angle` from the x axis."""
    return [[1.5 * math.cos(angle), 1.5 * math.sin(angle), 0.0, 0.0, 0.0, math.sin(angle / 2), math.cos(angle / 2),
             0.2, half_thickness, 0.2]]


def test_walk_stops_at_a_wall_the_samples_step_over(adv):
    n, tol, h = 2, 1e-3, 0.1
    qa, qb = np.array([[-0.5, 0.0]]), np.array([[0.5, 0.0]])
    scene = Scene(frames=[3], centers=[[0.0, 0, 0]], radii=[0.02], margin=0.0, boxes=_wall(0.05, 0.005))
    R = adv.reach(PLANAR, n)
    fr = frames_fn(PLANAR)
    # the sampled check at h = 0.1 has its samples at q1 = -0.5, -0.4 .. 0.5: the plate at 0.05 +- 0.017 rad lies
    # between two of them, and every sample is free
    _, K, s = np_samples(qa[0], qb[0], h)
    assert K == 10
    c, _, nan = adv.terms(n, fr(s), np.abs(qb - qa).repeat(K + 1, 0), scene, R, tol, math.sqrt(3.0))
    assert not nan.any() and (c >= scene.margin).all() and c.min() > 0.04
    w = adv.walk(n, qa, qb, scene, R, tol, math.sqrt(3.0), 4096, fr)
    assert w["status"][0] == BLOCKED
    q1 = -0.5 + w["t_stop"][0] * 1.0
    # inside the plate's shadow: |1.5 sin(q1 - 0.05)| < 0.005 + 0.02
    assert abs(1.5 * math.sin(q1 - 0.05)) < 0.025, q1
    assert w["clearance"][0] < 0.0 and w["steps"][0] == len(w["t"][0]) and w["t"][0][-1] == w["t_stop"][0]
    assert all(t1 > t0 for t0, t1 in zip(w["t"][0], w["t"][0][1:]))
    # the blocking sample is the walk's first non-free one: every earlier one is free, so nothing before it is missed
    cs, _, _ = adv.terms(n, fr(adv.samples(qa.repeat(len(w["t"][0]), 0), qb.repeat(len(w["t"][0]), 0), w["t"][0])),
                         np.abs(qb - qa).repeat(len(w["t"][0]), 0), scene, R, tol, math.sqrt(3.0))
    assert (cs[:-1] >= 0.0).all() and cs[-1] < 0.0 and w["clearance"][0] == cs.min()


def test_walk_certifies_a_clear_motion_within_the_step_bound(adv):
    n = 2
    qa, qb = np.array([[-0.5, 0.3], [0.2, -0.4], [0.1, 0.1]]), np.array([[0.5, -0.2], [0.2, 0.9], [0.1, 0.1]])
    scene = Scene(frames=[3, 2, 1], centers=[[0.0, 0, 0], [0.1, 0.2, 0.0], [0.5, 0, 0]], radii=[0.02, 0.05, 0.03],
                  pairs=[[0, 2]], margin=0.01, spheres=[[0.0, -3.0, 0.0, 0.5], [4.0, 0.0, 0.0, 1.0]],
                  boxes=[[0.0, 0.0, 2.0, 0, 0, 0, 1, 5.0, 5.0, 0.5]])
    R = adv.reach(PLANAR, n)
    for tol in (0.01, 0.001):
        w = adv.walk(n, qa, qb, scene, R, tol, math.sqrt(3.0), 65536, frames_fn(PLANAR))
        for b in range(3):
            a = np.abs(qb[b] - qa[b])
            lam_max = max(adv.lam_sphere(n, f, a, R, c) for f, c in zip(scene.frame, scene.centers))
            assert w["status"][b] == FREE and w["t_stop"][b] == 1.0
            assert 2 <= w["steps"][b] <= math.ceil(lam_max / tol) + 2, (b, w["steps"][b], lam_max / tol)
            assert w["t"][b][0] == 0.0 and w["t"][b][-1] == 1.0 and w["clearance"][b] >= scene.margin
        assert w["steps"][2] == 2  # qa == qb: every lam is 0, A = +inf
        assert w["steps"][0] > 2   # (and the first does take steps: the plane above it is 1.5 m away, not infinity)
    # a budget of samples that is too small says so and nothing else
    walled = Scene(frames=[3], centers=[[0.0, 0, 0]], radii=[0.02], margin=0.0, boxes=_wall(0.05, 0.005))
    w = adv.walk(n, np.array([[-0.5, 0.0]]), np.array([[0.5, 0.0]]), walled, R, 1e-4, math.sqrt(3.0), 2,
                 frames_fn(PLANAR))
    assert w["status"][0] == LIMIT and w["steps"][0] == 2 and 0.0 < w["t_stop"][0] < 1.0
    # no model at all: two samples, +inf; a NaN joint: not walked
    w = adv.walk(n, np.array([[0.0, 0.0], [math.nan, 0.0], [0.0, 1.0]]), np.array([[1.0, 2.0], [1.0, 1.0], [0.0, math.inf]]),
                 Scene(), R, 0.01, math.sqrt(3.0), 2, frames_fn(PLANAR))
    assert list(w["status"]) == [FREE, NOT_A_NUMBER, NOT_A_NUMBER] and list(w["steps"]) == [2, 0, 0]
    assert w["clearance"][0] == math.inf and np.isnan(w["clearance"][1:]).all() and np.isnan(w["t_stop"][1:]).all()
    # qa == qb in collision: blocked at sample 0
    hit = Scene(frames=[3], centers=[[0.0, 0, 0]], radii=[0.02], spheres=[[1.5, 0.0, 0.0, 0.1]])
    w = adv.walk(n, np.zeros((1, 2)), np.zeros((1, 2)), hit, R, 0.01, math.sqrt(3.0), 16, frames_fn(PLANAR))
    assert w["status"][0] == BLOCKED and w["steps"][0] == 1 and w["t_stop"][0] == 0.0
    # a NaN frame (from a NaN ee_offset): status NAN at the first sample
    w = adv.walk(n, np.zeros((1, 2)), np.ones((1, 2)), hit, R, 0.01, math.sqrt(3.0), 16,
                 frames_fn(PLANAR, [math.nan, 0, 0, 0, 0, 0, 1]))
    assert w["status"][0] == NOT_A_NUMBER and w["steps"][0] == 1 and math.isnan(w["clearance"][0])


def test_outside_grid_rule(adv):
    """A 5^3 grid over x in [1, 2], y, z in [-0.5, 0.5].  The end effector's sphere starts at q1 = 1 rad, outside it,
    and swings to (1.5, 0, 0), inside.  While it is outside the grid term is not part of the clearance, but it must
    hold the walk back: where the field behind the boundary is fine the motion is certified, where it is below the
    margin it must not be."""
    n = 2
    qa, qb = np.array([[1.0, 0.0]]), np.array([[0.0, 0.0]])
    R = adv.reach(PLANAR, n)
    fr = frames_fn(PLANAR)
    origin, voxel = [1.0, -0.5, -0.5], 0.25
    fine = Scene(frames=[3], centers=[[0.0, 0, 0]], radii=[0.02], margin=0.01, grid=(origin, voxel, np.full((5, 5, 5), 0.5)))
    w = adv.walk(n, qa, qb, fine, R, 0.01, math.sqrt(3.0), 4096, fr)
    assert w["status"][0] == FREE and w["t_stop"][0] == 1.0
    assert w["clearance"][0] == 0.5 - 0.02  # (the samples inside the grid; outside ones say +inf)
    # outside, the clamped field value lets it stride: far fewer samples than creeping up by dbox alone would take
    assert w["steps"][0] < 64
    low = Scene(frames=[3], centers=[[0.0, 0, 0]], radii=[0.02], margin=0.01, grid=(origin, voxel, np.full((5, 5, 5), -0.1)))
    w = adv.walk(n, qa, qb, low, R, 0.01, math.sqrt(3.0), 256, fr)
    assert w["status"][0] in (BLOCKED, LIMIT)
    # it has been held at the boundary (or has entered and found the field low): never past it unseen
    p = centre(np_frames7(PLANAR, qa[0] + w["t_stop"][0] * (qb[0] - qa[0])), 3, [0.0, 0, 0])
    inside = 1.0 <= p[0] <= 2.0 and -0.5 <= p[1] <= 0.5
    assert (w["status"][0] == BLOCKED) == inside
    if not inside:
        assert max(1.0 - p[0], p[1] - 0.5) < 1e-6 and w["clearance"][0] == math.inf
    # a field that is fine at the boundary and low deeper in: the walk enters and is blocked inside
    vals = np.full((5, 5, 5), 0.5)
    vals[1:4, 1:4, :] = -0.2
    deep = Scene(frames=[3], centers=[[0.0, 0, 0]], radii=[0.02], margin=0.01, grid=(origin, voxel, vals))
    from optik_amd.collision import grid_lipschitz
    G = grid_lipschitz(vals, voxel)
    assert G == math.sqrt(2 * (0.7 / 0.25) ** 2)
    w = adv.walk(n, qa, qb, deep, R, 0.001, G, 4096, fr)
    assert w["status"][0] == BLOCKED and 0.0 < w["t_stop"][0] < 1.0
    # the first non-free sample lies within tol / (G lam) of where the field crosses the margin: just below it
    assert deep.margin - w["clearance"][0] <= 0.001


def test_grid_lipschitz_numpy():
    from optik_amd.collision import grid_lipschitz
    x, y, z = np.meshgrid(np.arange(4) * 0.5, np.arange(5) * 0.5, np.arange(6) * 0.5, indexing="ij")
    assert grid_lipschitz(2.0 * x - 1.0 * y + 0.5 * z, 0.5) == pytest.approx(math.sqrt(4.0 + 1.0 + 0.25), rel=1e-15)
    d = np.sqrt(x * x + y * y + z * z)  # a true distance field
    assert grid_lipschitz(d, 0.5) <= math.sqrt(3.0)
    for bad in (np.zeros((4, 4)), np.zeros((1, 4, 4))):
        with pytest.raises(ValueError):
            grid_lipschitz(bad, 0.5)
    with pytest.raises(ValueError):
        grid_lipschitz(d, 0.0)


def test_certify_symbols_are_exported(built):
    for s in ("optik_hip_collision_motion_certify_batch", "optik_robot_collision_motion_certify_batch"):
        assert hasattr(built, s), f"{s} is not exported by liboptik_amd.so"


def test_refusals_happen_before_any_device_work(panda):
    """None of these calls touches a device (the robot has created no device context)."""
    from optik_amd import _native as nat
    n = panda.num_positions()
    z = np.zeros((2, n))
    for tol in (math.nan, 0.0, -1e-3, math.inf):
        with pytest.raises(ValueError, match="tol"):
            panda.collision_motion_certify_batch_arrays(z, z, tol)
        with pytest.raises(ValueError, match="tol"):
            panda.certify_paths(np.zeros((1, 3, n)), None, tol)
    for G in (math.nan, 0.0, -1.0, math.inf):
        with pytest.raises(ValueError, match="grid_lipschitz"):
            panda.collision_motion_certify_batch_arrays(z, z, 0.01, grid_lipschitz=G)
    for ms in (1, 0, -5, 65537, 2.5, True):
        with pytest.raises(ValueError, match="max_steps"):
            panda.collision_motion_certify_batch_arrays(z, z, 0.01, max_steps=ms)
    with pytest.raises(ValueError):
        panda.collision_motion_certify_batch_arrays(z, np.zeros((3, n)), 0.01)
    with pytest.raises(ValueError):
        panda.collision_motion_certify(np.zeros(n - 1), np.zeros(n - 1), 0.01)
    assert (nat.CERTIFY_FREE, nat.CERTIFY_BLOCKED, nat.CERTIFY_LIMIT, nat.CERTIFY_NAN) == (FREE, BLOCKED, LIMIT,
                                                                                           NOT_A_NUMBER)
    # the C ABI refuses the same without a device
    L = panda._L
    dp = C.POINTER(C.c_double)
    zp = z.ctypes.data_as(dp)
    for tol, G, ms, word in ((math.nan, 1.0, 16, b"tol"), (0.0, 1.0, 16, b"tol"), (0.01, math.inf, 16, b"grid_lipschitz"),
                             (0.01, 0.0, 16, b"grid_lipschitz"), (0.01, 1.0, 1, b"max_steps"),
                             (0.01, 1.0, 65537, b"max_steps")):
        assert L.optik_robot_collision_motion_certify_batch(panda._h, 2, zp, zp, tol, G, ms, None, None, None, None,
                                                            None) == -1
        assert word in L.optik_robot_last_error()
