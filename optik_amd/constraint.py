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

    # -- goal regions (Robot.ik_region and the plan_*_to_region planners) --------------------
    @staticmethod
    def _tol(name, v):
        v = float(v)
        if not (math.isfinite(v) and v >= 0.0):
            raise ValueError(f"pose constraint: {name} must be finite and >= 0")
        return v

    @staticmethod
    def position_only(pose, pos_tol=0.0):
        """"Reach this point, any orientation": the three linear components within +-pos_tol, the angular ones free.
        With pos_tol = 0 the end effector's origin is the pose's exactly (the linear error V^-1 t is zero iff t is).
        With pos_tol > 0 the box is on the linear part of the se3 logarithm, not on t itself: V scales no vector up
        (its singular values are 1 along the rotation axis and 2 sin(theta / 2) / theta <= 1 across it), so
        |t| <= |V^-1 t| <= sqrt(3) pos_tol -- the origin lies within that distance of the pose's."""
        p, inf = PoseConstraint._tol("pos_tol", pos_tol), math.inf
        return PoseConstraint(pose, [-p, -p, -p, -inf, -inf, -inf], [p, p, p, inf, inf, inf])

    @staticmethod
    def axis_free(pose, axis="z", pos_tol=0.0, rot_tol=0.0):
        """"Drill here, any angle about the tool axis": the angular component about `axis` ("x", "y" or "z", of the
        pose's own frame) free, the two others within +-rot_tol, the linear ones within +-pos_tol.
        With both tolerances 0 the set is exactly {pose * R_axis(theta)}: the five pinned components say that X =
        pose^-1 * fk(x) has the rotation vector w = theta * axis and the linear logarithm V(w)^-1 t = 0, that is
        t = 0, so X = R_axis(theta); and every R_axis(theta), theta in (-pi, pi], has that error."""
        k = {"x": 0, "y": 1, "z": 2}.get(axis)
        if k is None:
            raise ValueError(f"pose constraint: axis must be 'x', 'y' or 'z', got {axis!r}")
        p, r = PoseConstraint._tol("pos_tol", pos_tol), PoseConstraint._tol("rot_tol", rot_tol)
        lo, hi = [-p, -p, -p, -r, -r, -r], [p, p, p, r, r, r]
        lo[3 + k], hi[3 + k] = -math.inf, math.inf
        return PoseConstraint(pose, lo, hi)

    @staticmethod
    def around(pose, pos_tol, rot_tol):
        """The pose within tolerances (what TRAC-IK takes as bounds): the linear components of the error within
        +-pos_tol, the angular ones within +-rot_tol.  Both 0 pins the pose."""
        p, r = PoseConstraint._tol("pos_tol", pos_tol), PoseConstraint._tol("rot_tol", rot_tol)
        return PoseConstraint(pose, [-p, -p, -p, -r, -r, -r], [p, p, p, r, r, r])

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


def region_rows(regions, T):
    """regions -- one PoseConstraint (or anything with ref7, lo, hi), broadcast over T rows, or a sequence of T of
    them -- as the [T, 19] float64 array optik_hip_ik_region reads: per row ref7, lo, hi.  Each is validated as
    checked_constraint_arrays validates it, and its quaternion for unit norm within 100 machine epsilons; ValueError
    naming the row otherwise."""
    one = hasattr(regions, "ref7")
    seq = [regions] if one else list(regions)
    if not one and len(seq) != T:
        raise ValueError(f"regions must be one PoseConstraint or a sequence of T = {T}, got {len(seq)}")
    rows = np.empty((len(seq), 19), dtype=np.float64)
    for t, c in enumerate(seq):
        try:
            ref7, lo, hi = checked_constraint_arrays(c)
            if not abs(float(ref7[3:] @ ref7[3:]) - 1.0) <= 100.0 * np.finfo(np.float64).eps:
                raise ValueError("pose constraint: the reference quaternion must have unit norm")
        except (ValueError, AttributeError) as e:
            raise ValueError(f"region {t}: {e}") from None
        rows[t, :7], rows[t, 7:13], rows[t, 13:] = ref7, lo, hi
    return np.ascontiguousarray(np.broadcast_to(rows, (T, 19))) if one else rows


def keep_arrays(keep):
    """keep = (PoseConstraint, tol) or None -> (ref7, lo, hi, tol) or None, validated; ValueError otherwise."""
    if keep is None:
        return None
    try:
        c, tol = keep
    except (TypeError, ValueError):
        raise ValueError("keep must be (PoseConstraint, tol)") from None
    if not hasattr(c, "ref7"):
        raise ValueError("keep must be (PoseConstraint, tol)")
    tol = float(tol)
    if not (math.isfinite(tol) and tol >= 0.0):
        raise ValueError(f"pose constraint: tol must be finite and >= 0, got {tol}")
    return (*checked_constraint_arrays(c), tol)


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
