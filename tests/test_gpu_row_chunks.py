"""GPU: chunking is invisible in the row batches of the host API (robot_rows.cpp over robot_host.hpp:stage_rows).
Each of diff_ik_batch_arrays, manipulability_batch_arrays, collision_clearance_batch_arrays and
link_frames_batch_arrays gets 2^18 + 3 rows -- one full chunk and a partial one -- and collision_motion_batch_arrays
2^16 + 3 segments; the rows at the start, across the chunk boundary and at the end, resubmitted on their own, must
come back with the bits the big call gave them.  No tolerance and no reference: every comparison is exact."""
import numpy as np
import pytest

from collision_util import small_scene
from conftest import ROBOT_SPECS

pytestmark = pytest.mark.gpu

ROW_CHUNK = 1 << 18     # rows per launch of the row batches
MOTION_CHUNK = 1 << 16  # segments per launch of the motion batch


@pytest.fixture(scope="module")
def panda():
    from optik_amd import Robot
    r = Robot.from_urdf_file(*ROBOT_SPECS["panda"])
    model, spheres = small_scene(r)
    r.set_collision_model(**model)
    r.set_world(spheres=spheres)
    return r


@pytest.fixture(scope="module")
def rows(panda):
    """2^18 + 3 random configurations within the joint limits."""
    lb, ub = (np.array(v) for v in panda.joint_limits())
    return np.random.default_rng(18).uniform(lb, ub, size=(ROW_CHUNK + 3, len(lb)))


def _slices(chunk, B):
    return [slice(0, 3), slice(chunk - 2, chunk + 3), slice(B - 3, B)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.astype(np.int64)


def _assert_rows_reproduce(call, inputs, chunk, names):
    """call(*inputs) over all rows, then over each slice alone: every output of the slice bit-equal to its rows of the
    big call's.  Returns the big call's outputs."""
    B = len(inputs[0])
    assert B == chunk + 3
    big = call(*inputs)
    assert len(big) == len(names)
    for s in _slices(chunk, B):
        small = call(*(a[s] for a in inputs))
        for name, got, want in zip(names, small, big):
            assert got.shape == want[s].shape and got.dtype == want.dtype, (name, s)
            assert np.array_equal(_bits(got), _bits(want[s])), (name, s)
    return big


def test_diff_ik_rows_do_not_depend_on_the_chunk(panda, rows):
    rng = np.random.default_rng(5)
    B, n = rows.shape
    V = rng.uniform(-0.5, 0.5, size=(B, 6))
    v_max = rng.uniform(0.5, 2.0, size=(B, n))
    alpha, v, found = _assert_rows_reproduce(panda.diff_ik_batch_arrays, (rows, V, v_max), ROW_CHUNK,
                                             ("alpha", "v", "status"))
    # the status counts of the whole batch are those of its two halves
    h = B // 2
    halves = [panda.diff_ik_batch_arrays(rows[s], V[s], v_max[s])[2] for s in (slice(0, h), slice(h, B))]
    assert int(found.sum()) == sum(int(f.sum()) for f in halves)
    assert int((~found).sum()) == sum(int((~f).sum()) for f in halves)
    assert 0 < found.sum()


def test_manipulability_rows_do_not_depend_on_the_chunk(panda, rows):
    w, c = _assert_rows_reproduce(panda.manipulability_batch_arrays, (rows,), ROW_CHUNK, ("w", "c"))
    assert np.isfinite(w).all() and np.isfinite(c).all()


def test_clearance_rows_do_not_depend_on_the_chunk(panda, rows):
    clr, free = _assert_rows_reproduce(panda.collision_clearance_batch_arrays, (rows,), ROW_CHUNK,
                                       ("clearance", "free"))
    assert np.isfinite(clr).all() and 0 < free.sum() < len(free)  # (the scene bites, and not everywhere)


def test_link_frame_rows_do_not_depend_on_the_chunk(panda, rows):
    (frames,) = _assert_rows_reproduce(lambda xs: (panda.link_frames_batch_arrays(xs),), (rows,), ROW_CHUNK,
                                       ("frames",))
    assert np.isfinite(frames).all()


def test_motion_segments_do_not_depend_on_the_chunk(panda, rows):
    B = MOTION_CHUNK + 3
    lb, ub = (np.array(v) for v in panda.joint_limits())
    xa = rows[:B]
    # short segments at a coarse resolution: at most 0.2 rad per joint in steps of 0.05 -- a handful of samples each
    xb = np.clip(xa + np.random.default_rng(7).uniform(-0.2, 0.2, size=xa.shape), lb, ub)
    clr, free, first, steps = _assert_rows_reproduce(
        lambda a, b: panda.collision_motion_batch_arrays(a, b, 0.05), (xa, xb), MOTION_CHUNK,
        ("clearance", "free", "first", "steps"))
    assert np.isfinite(clr).all() and (steps >= 0).all() and steps.max() <= 5
    assert 0 < free.sum() < B
