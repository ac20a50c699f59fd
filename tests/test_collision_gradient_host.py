"""CPU-only: the witnesses and gradients of the clearance (optik_amd/csrc/collision_gradient.hpp, built with g++ as
plain C++) on frames from a numpy forward kinematics: the minimum over the rows is the clearance bit for bit, the
gradients are the central differences of the rows' distances, and the constructed special cases have their values."""
import math

import numpy as np
import pytest

from avoid_util import Scene, build_avoid, load_tables, numpy_frames, make_test_world
from collision_util import build_measure
from conftest import ROBOT_SPECS
from grid_util import build_grid_measure

NAMES = ["panda", "ur10", "arm8"]
H = 1e-5         # the step of the central differences
REACH = 1.5      # no point of these arms is farther than this from a joint axis: a step H moves a point by < REACH * H


@pytest.fixture(scope="module")
def avoid(tmp_path_factory):
    return build_avoid(str(tmp_path_factory.mktemp("avoid_grad")))


@pytest.fixture(scope="module")
def measures(tmp_path_factory):
    return (build_measure(str(tmp_path_factory.mktemp("avoid_cm"))),
            build_grid_measure(str(tmp_path_factory.mktemp("avoid_gm"))))


def _scene(name):
    from optik_amd import Robot
    from optik_amd.collision import auto_pairs, spheres_along_chain
    robot = Robot.from_urdf_file(*ROBOT_SPECS[name])
    tables = load_tables(*ROBOT_SPECS[name])
    n = robot.num_positions()
    frames, centers, radii = spheres_along_chain(robot, 0.05, 2)
    spheres, boxes, grid = make_test_world()
    scene = Scene(tables["axes"][:n], frames, centers, radii, auto_pairs(frames), spheres, boxes, grid)
    return robot, tables, scene


def _configs(robot, rng, B):
    lb, ub = (np.array(v) for v in robot.joint_limits())
    return rng.uniform(np.maximum(lb, -2.8), np.minimum(ub, 2.8), size=(B, robot.num_positions()))


@pytest.mark.parametrize("name", NAMES)
def test_minimum_over_rows_is_the_clearance_bit_for_bit(avoid, measures, name):
    robot, tables, scene = _scene(name)
    measure, gmeasure = measures
    q = _configs(robot, np.random.default_rng(5), 200)
    frames = np.array([numpy_frames(tables, x) for x in q])
    dist, wit, grad = avoid.witness(scene, frames)
    c = measure.clearance(frames, scene.frames, scene.centers, scene.radii, scene.pairs, scene.spheres, scene.boxes)
    cg = gmeasure.clearance_grid(frames, scene.frames, scene.centers, scene.radii, *scene.grid)
    want = np.minimum(c, cg)
    assert np.array_equal(dist.min(axis=1).view(np.uint64), want.view(np.uint64))
    # every kind of witness occurs, and rows without a sphere or pair are empty
    assert set(np.unique(wit[:, :, 1])) >= {0, 1, 2, 3}
    empty = wit[:, :, 0] < 0
    assert (np.isinf(dist[empty])).all() and (grad[empty] == 0.0).all() and (wit[empty] == -1).all()
    assert np.isfinite(dist[~empty]).all()


def _qrot(q, v):
    t = 2.0 * np.cross(q[:3], v)
    return t * q[3] + np.cross(q[:3], t) + v


def _near_a_kink(scene, frames, f, w, tol):
    """Is the witness point of row f within tol of a box face (or of the switch between two faces inside the box) or
    of a grid cell wall?"""
    s, kind, idx = w
    if kind not in (1, 2):
        return False
    p = frames[f, :3] + _qrot(frames[f, 3:], scene.centers[s])
    if kind == 1:
        box = scene.boxes[idx]
        qc = np.array([-box[3], -box[4], -box[5], box[6]])
        l = _qrot(qc, p - box[:3])
        e = np.sort(np.abs(l) - box[7:10])
        return bool((np.abs(e) <= tol).any() or (np.abs(l) <= tol).any() or (e[2] < 0 and e[2] - e[1] <= 2 * tol))
    origin, voxel, _ = scene.grid
    u = (p - origin) / voxel
    return bool((np.abs(u - np.round(u)) <= tol / voxel).any())


@pytest.mark.parametrize("name", NAMES)
def test_gradient_is_the_central_difference(avoid, name):
    """dist at q -+ H e_j against grad_j at 1e-6: the truncation error is H^2 / 6 times a third derivative of order
    1 .. 10 per m^2 (1e-10 .. 1e-9), the round-off 1e-16 / H = 1e-11.  Rows whose witness changes within the step, or
    whose point is within a step's motion of a kink, have no derivative there and are left out (at most 10 %)."""
    robot, tables, scene = _scene(name)
    n = robot.num_positions()
    q = _configs(robot, np.random.default_rng(11), 40)
    B = len(q)
    steps = np.concatenate([np.zeros((1, n)), H * np.eye(n), -H * np.eye(n)])
    frames = np.array([[numpy_frames(tables, x + d) for d in steps] for x in q])  # [B, 2n + 1, F, 7]
    dist, wit, grad = avoid.witness(scene, frames.reshape(B * (2 * n + 1), n + 2, 7))
    dist = dist.reshape(B, 2 * n + 1, n + 2)
    wit = wit.reshape(B, 2 * n + 1, n + 2, 3)
    grad = grad.reshape(B, 2 * n + 1, n + 2, n)
    finite = compared = 0
    worst = 0.0
    for b in range(B):
        for f in range(n + 2):
            if not np.isfinite(dist[b, 0, f]):
                continue
            finite += 1
            if (wit[b, :, f] != wit[b, 0, f]).any() or _near_a_kink(scene, frames[b, 0], f, wit[b, 0, f], REACH * H):
                continue
            compared += 1
            fd = (dist[b, 1:n + 1, f] - dist[b, n + 1:, f]) / (2 * H)
            err = np.abs(fd - grad[b, 0, f]).max()
            worst = max(worst, err)
            assert err <= 1e-6, (name, b, f, wit[b, 0, f], fd, grad[b, 0, f])
            assert (grad[b, 0, f, min(f, n):] == 0.0).all() or wit[b, 0, f, 1] == 3
    print(f"{name}: {compared} of {finite} finite rows compared, worst error {worst:.3g}")
    assert finite >= 100 and finite - compared <= 0.10 * finite, (finite, compared)


def test_special_rows(avoid):
    # a 2-joint planar chain about z: frame 1 at the origin, frame 2 at (1, 0, 0), the end effector at (1.5, 0, 0)
    ident = [0.0, 0.0, 0.0, 1.0]
    frames = np.array([[0, 0, 0] + ident, [0, 0, 0] + ident, [1.0, 0, 0] + ident, [1.5, 0, 0] + ident], dtype=float)
    axes = [[0, 0, 1.0], [0, 0, 1.0]]
    # a sphere on frame 2 inside a box: l = (-0.1, -0.1, 0), e = (-0.4, -0.05, -0.3): out through -y
    box = [1.1, 0.1, 0.0] + ident + [0.5, 0.15, 0.3]
    sc = Scene(axes, [2], [[0.0, 0.0, 0.0]], [0.1], boxes=[box])
    dist, wit, grad = avoid.witness(sc, frames[None])
    e1 = abs(0.0 - 0.1) - 0.15
    assert dist[0, 2] == (0.0 + e1) - 0.1 and tuple(wit[0, 2]) == (0, 1, 0)
    assert tuple(grad[0, 2]) == (-1.0, 0.0)  # joint 1 moves the point along +y, the normal is -y; joint 2 not at all
    # frames without a sphere are empty
    for f in (0, 1, 3):
        assert dist[0, f] == math.inf and tuple(wit[0, f]) == (-1, -1, -1) and (grad[0, f] == 0.0).all()
    # a sphere outside the grid: the grid says nothing, the row is empty
    grid = (np.array([5.0, 5.0, 5.0]), 0.5, np.ones((2, 2, 2), dtype=np.float32))
    sc = Scene(axes, [2], [[0.0, 0.0, 0.0]], [0.1], grid=grid)
    dist, wit, grad = avoid.witness(sc, frames[None])
    assert dist[0, 2] == math.inf and tuple(wit[0, 2]) == (-1, -1, -1) and (grad[0, 2] == 0.0).all()
    # inside it: the trilinear slope times 1 / voxel.  values = x index: d c / d x = 1 / 0.5 = 2 per metre
    vals = np.zeros((3, 2, 2), dtype=np.float32)
    vals[1], vals[2] = 1.0, 2.0
    sc = Scene(axes, [2], [[0.0, 0.0, 0.0]], [0.1], grid=(np.array([0.75, -0.25, -0.25]), 0.5, vals))
    dist, wit, grad = avoid.witness(sc, frames[None])
    assert dist[0, 2] == 0.5 - 0.1 and tuple(wit[0, 2]) == (0, 2, 0)
    assert tuple(grad[0, 2]) == (0.0, 0.0)  # (both joints move the point along y; the field slopes along x)
    # a coincident centre: the distance is -(r_a + r_b), the normal and the gradient are zero
    sc = Scene(axes, [3], [[0.25, 0.0, 0.0]], [0.1], spheres=[[1.75, 0.0, 0.0, 0.2]])
    dist, wit, grad = avoid.witness(sc, frames[None])
    assert dist[0, 3] == (0.0 - 0.1) - 0.2 and tuple(wit[0, 3]) == (0, 0, 0) and (grad[0, 3] == 0.0).all()
    # a self pair belongs to its higher frame; the witness names sphere a and the pair
    sc = Scene(axes, [0, 3], [[0.0, 2.0, 0.0], [0.0, 0.0, 0.0]], [0.1, 0.1], pairs=[[1, 0]])
    dist, wit, grad = avoid.witness(sc, frames[None])
    assert dist[0, 3] == (2.5 - 0.1) - 0.1 and tuple(wit[0, 3]) == (1, 3, 0) and dist[0, 0] == math.inf
    # p_a - p_b = (1.5, -2, 0) / 2.5; joint 1 moves p_a by (0, 1.5, 0), joint 2 by (0, 0.5, 0)
    assert np.allclose(grad[0, 3], [-0.8 * 1.5, -0.8 * 0.5], rtol=0, atol=1e-15)
    # a NaN frame: every row NaN, no witness
    bad = frames.copy()
    bad[1, 4] = math.nan
    dist, wit, grad = avoid.witness(sc, bad[None])
    assert np.isnan(dist).all() and np.isnan(grad).all() and (wit == -1).all()


def test_damper_rows_are_the_four_smallest_with_ties_to_the_lower_frame(avoid):
    """The active rows in ascending order of (dist, frame), whatever order the frames come in: exact ties, more than
    four active rows, a closer frame arriving after equal ones, rows at and beyond the influence distance, infinite and
    NaN rows."""
    inf, nan = math.inf, math.nan
    cases = [
        ([0.1, 0.1, 0.1, 0.1, 0.05], [4, 0, 1, 2]),
        ([0.1, 0.1, 0.05], [2, 0, 1, -1]),
        ([0.1] * 10, [0, 1, 2, 3]),
        ([0.1, 0.05, 0.1, 0.05, 0.1, 0.05], [1, 3, 5, 0]),
        ([0.15, 0.1, 0.1, 0.05, 0.05, 0.01, 0.15], [5, 3, 4, 1]),
        ([0.1, 0.1, 0.1, 0.1, 0.1, 0.02, 0.02, 0.02], [5, 6, 7, 0]),
        ([0.2, 0.25, inf, -inf, nan, 0.19, -0.3], [6, 5, -1, -1]),   # 0.2 is not < influence; -inf is not finite
        ([inf] * 9, [-1, -1, -1, -1]),
        ([0.0, -0.0, 0.1], [0, 1, 2, -1]),                             # -0.0 == 0.0: a tie
    ]
    rng = np.random.default_rng(3)
    for _ in range(200):  # random rows from a few values: many ties
        d = rng.choice([0.01, 0.05, 0.1, 0.15, 0.3, inf], size=int(rng.integers(1, 11))).tolist()
        order = sorted((f for f in range(len(d)) if d[f] < 0.2), key=lambda f: (d[f], f))[:4]
        cases.append((d, order + [-1] * (4 - len(order))))
    m, sel = avoid.select([c[0] for c in cases], 0.2)
    for (d, want), got_m, got in zip(cases, m, sel):
        assert got.tolist() == want and got_m == sum(w >= 0 for w in want), (d, got.tolist(), want)
