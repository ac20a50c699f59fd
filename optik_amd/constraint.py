"""Pose constraints (include/optik_hip.h: optik_hip_constraint_batch and what precedes it)."""
from __future__ import annotations

import math

import numpy as np


def _quat_from_rotation(R):
    """The unit quaternion (i, j, k, w), w >= 0, of a rotation matrix: the largest of the four squared components is
    taken from the diagonal, the others from the off-diagonal sums and differences."""
    t = [R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1],
         R[0, 0] + R[1, 1] + R[2, 2]]
    m = int(np.argmax(t))
    s = 2.0 * math.sqrt(1.0 + t[m])
    if m == 3:
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, s / 4.0]
    else:
        a, b = (m + 1) % 3, (m + 2) % 3
        q = [0.0, 0.0, 0.0, (R[b, a] - R[a, b]) / s]
        q[m], q[a], q[b] = s / 4.0, (R[a, m] + R[m, a]) / s, (R[b, m] + R[m, b]) / s
    q = np.array(q, dtype=np.float64)
    q /= math.sqrt(float(q @ q))
    return -q if q[3] < 0.0 else q


class PoseConstraint:
    """A box on the pose error against a reference pose.

    With X = reference^-1 * fk(x) * ee_offset the error of a configuration is e(x) = (se3 log linear xyz, so3 log
    xyz) of X, in the frame of the reference -- the six numbers the IK objective forms before it weights them.  The
    residual is r_i = e_i - min(max(e_i, lo_i), hi_i), the violation max_i |r_i|; x satisfies the constraint at tol
    iff its violation is <= tol.  lo_i = -inf and hi_i = +inf free an axis, lo_i == hi_i pins it.

    reference: a 4x4 homogeneous matrix, validated as every pose of this module is (an isometry within 100 machine
    epsilons); lo, hi: six numbers each with lo <= hi and no NaN.  ValueError otherwise -- what the C layer refuses
    with OPTIK_HIP_EINVAL.  `ref7` is the reference as (t, quaternion i j k w), the layout the C layer takes."""

    def __init__(self, reference, lo, hi):
        from .robot import _pose16
        m = _pose16(reference).reshape(4, 4).T  # (validates; back to row, column)
        if not np.isfinite(m).all():
            raise ValueError("pose constraint: the reference pose must be finite")
        lo, hi = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
        if lo.shape != (6,) or hi.shape != (6,):
            raise ValueError("pose constraint: lo and hi must be six numbers each (linear xyz, angular xyz)")
        if not (lo <= hi).all():
            raise ValueError("pose constraint: needs lo <= hi on every axis, no NaN")
        self.reference = m.copy()
        self.ref7 = np.ascontiguousarray(np.concatenate([m[:3, 3], _quat_from_rotation(m[:3, :3])]))
        self.lo, self.hi = np.ascontiguousarray(lo), np.ascontiguousarray(hi)

    @staticmethod
    def upright(reference, tilt):
        """The end effector's z axis within `tilt` radians (0 <= tilt, finite) of the reference's, everything else
        free: the box +-tilt / sqrt(2) on the angular x and y components.  It guarantees the tilt because the angle
        alpha between the two z axes satisfies alpha <= sqrt(e_4^2 + e_5^2) (csrc/constraint_measure.hpp has the
        two-line proof); it is sufficient, not necessary: a square inside the circle."""
        tilt = float(tilt)
        if not (math.isfinite(tilt) and tilt >= 0.0):
            raise ValueError("pose constraint: tilt must be finite and >= 0")
        b, inf = tilt / math.sqrt(2.0), math.inf
        return PoseConstraint(reference, [-inf, -inf, -inf, -b, -b, -inf], [inf, inf, inf, b, b, inf])

    def __repr__(self):
        return f"PoseConstraint(ref7={self.ref7.tolist()}, lo={self.lo.tolist()}, hi={self.hi.tolist()})"


def constraint_arrays(c):
    """(ref7, lo, hi) of a PoseConstraint -- or of anything with those attributes -- as contiguous float64 arrays of
    7, 6 and 6 numbers: what the C layer reads (and validates)."""
    ref7, lo, hi = (np.ascontiguousarray(getattr(c, k), dtype=np.float64) for k in ("ref7", "lo", "hi"))
    if ref7.shape != (7,) or lo.shape != (6,) or hi.shape != (6,):
        raise ValueError("pose constraint: ref7 must be 7 numbers, lo and hi 6 each")
    return ref7, lo, hi


def checked_constraint_arrays(c):
    """constraint_arrays(c), with what PoseConstraint's constructor checks of the numbers checked again for an
    object that did not come from it: a finite reference and lo <= hi without a NaN.  ValueError otherwise."""
    ref7, lo, hi = constraint_arrays(c)
    if not np.isfinite(ref7).all():
        raise ValueError("pose constraint: the reference pose must be finite")
    if not (lo <= hi).all():
        raise ValueError("pose constraint: needs lo <= hi on every axis, no NaN")
    return ref7, lo, hi


class ConstrainedRoadmap:
    """What Robot.build_constrained_roadmap returns and Robot.plan_constrained_paths takes: the device tensors
    nodes [n, N] (a node whose projection failed is a NaN column), nbr [k, N] int32, w [k, N], and N, k, the
    resolution, the constraint, tol and `projected`, the number of nodes that projected.  The caller's object:
    nothing in the robot knows it, and nothing marks it stale."""

    def __init__(self, nodes, nbr, w, resolution, constraint, tol, projected):
        self.nodes, self.nbr, self.w = nodes, nbr, w
        self.N, self.k = int(nodes.shape[1]), int(nbr.shape[0])
        self.resolution, self.constraint, self.tol = float(resolution), constraint, float(tol)
        self.projected = int(projected)
