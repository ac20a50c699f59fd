"""CPU-only: the arithmetic of pose constraints (optik_amd/csrc/constraint_measure.hpp, built for the host) against the
oracle, finite differences, numpy restatements and constructed cases whose answers are known; the constrained planner
restated on the CPU over the serial roadmap reference."""
import math

import numpy as np
import pytest

import constraint_util as cu
from constraint_util import BUDGET_SPENT, FAILED, PROJECTED, PROJECT_DEFAULTS, bits
from roadmap_util import FOUND, build_roadmap_ref

ROBOT_NAMES = ("panda", "ur10", "arm10")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return cu.build_constraint(str(tmp_path_factory.mktemp("constraint_measure")))


@pytest.fixture(scope="module")
def roadmap_ref(tmp_path_factory):
    return build_roadmap_ref(str(tmp_path_factory.mktemp("constraint_roadmap")))


def _qmul(a, b):
    ai, aj, ak, aw = a
    bi, bj, bk, bw = b
    return np.array([aw * bi + ai * bw + aj * bk - ak * bj, aw * bj - ai * bk + aj * bw + ak * bi,
                     aw * bk + ai * bj - aj * bi + ak * bw, aw * bw - ai * bi - aj * bj - ak * bk])


def _qrot(q, v):
    u = 2.0 * np.cross(q[:3], v)
    return v + q[3] * u + np.cross(q[:3], u)


def _home7(oracle, chains):
    return np.asarray(oracle.fk(chains["panda"][1], np.array(cu.PANDA_HOME))[1])


def _rows(d, rng, count):
    lb, ub = np.maximum(d["lb"], -3.0), np.minimum(d["ub"], 3.0)
    return rng.uniform(lb, ub, (count, len(lb)))


@pytest.mark.parametrize("name", ROBOT_NAMES)
def test_error_matches_the_oracle_and_the_jacobian_its_finite_difference(ref, oracle, chains, name):
    d, oc = chains[name]
    n = len(d["lb"])
    rng = np.random.default_rng(3)
    q = _rows(d, rng, 24)
    ee7 = np.array([0.02, -0.01, 0.1, 0.0, math.sin(0.2), 0.0, math.cos(0.2)])
    for ee in (None, ee7):
        ee_pose = oracle.Pose.make(ee[:3], ee[3:]) if ee is not None else None
        ref7 = np.asarray(oracle.fk(oc, _rows(d, rng, 1)[0], ee_pose)[1])
        c = cu.free_constraint(ref7)
        m = ref.measure(d, c, q, ee)
        checked = 0
        for b in range(len(q)):
            p = np.asarray(oracle.fk(oc, q[b], ee_pose)[1])
            qc = np.array([-ref7[3], -ref7[4], -ref7[5], ref7[6]])
            want = oracle.se3_log(_qrot(qc, p[:3] - ref7[:3]), _qmul(qc, p[3:]))
            assert np.abs(m["e"][b] - want).max() <= 1e-12, (name, b)
            theta = np.linalg.norm(m["e"][b][3:])
            if not 0.1 < theta < 3.0:  # (the logarithm is not differentiable at pi and the reference's series is noisy at 0)
                continue
            h = 1e-5
            J = np.zeros((6, n))
            for k in range(n):
                qp, qm = q[b].copy(), q[b].copy()
                qp[k] += h
                qm[k] -= h
                J[:, k] = (ref.measure(d, c, qp, ee)["e"][0] - ref.measure(d, c, qm, ee)["e"][0]) / (2 * h)
            assert np.abs(J - m["J"][b]).max() <= 1e-6 * np.abs(m["J"][b]).max(), (name, b)
            checked += 1
            if checked == 4:
                break
        assert checked == 4


def test_residual_rules(ref, oracle, chains):
    d, oc = chains["panda"]
    rng = np.random.default_rng(4)
    q = _rows(d, rng, 6)
    ref7 = _home7(oracle, chains)
    e = ref.measure(d, cu.free_constraint(ref7), q)
    # every axis free: no residual, no violation, exactly
    assert not e["r"].any() and not e["v"].any() and not np.signbit(e["r"]).any()
    # lo == hi: the residual is the distance to the pin, the violation its largest component
    at = np.array([0.1, -0.2, 0.3, 0.0, 0.05, -0.05])
    m = ref.measure(d, cu.pinned_constraint(ref7, at), q)
    assert np.array_equal(bits(m["r"]), bits(e["e"] - at))
    assert np.array_equal(bits(m["v"]), bits(np.abs(e["e"] - at).max(axis=1)))
    # an error exactly on a bound: no violation; a bound one ulp inside it: the difference
    lo, hi = np.full(6, -np.inf), np.full(6, np.inf)
    hi[4], lo[2] = e["e"][0][4], e["e"][0][2]
    m = ref.measure(d, cu.Constraint(ref7, lo, hi), q[:1])
    assert m["v"][0] == 0.0 and not m["r"][0].any()
    hi[4] = np.nextafter(hi[4], -np.inf)
    m = ref.measure(d, cu.Constraint(ref7, lo, hi), q[:1])
    assert m["v"][0] == e["e"][0][4] - hi[4] > 0.0 and m["r"][0][2] == 0.0
    # one-sided boxes
    lo, hi = np.full(6, -np.inf), np.full(6, np.inf)
    lo[0] = e["e"][:, 0].max() + 1.0
    m = ref.measure(d, cu.Constraint(ref7, lo, hi), q)
    assert np.array_equal(bits(m["r"][:, 0]), bits(e["e"][:, 0] - lo[0])) and not m["r"][:, 1:].any()
    # a NaN joint: every residual on a bounded axis and the violation are NaN -- also behind a larger finite term
    bad = q[:2].copy()
    bad[0, 3] = math.nan
    bad[1, 6] = math.nan
    m = ref.measure(d, cu.upright_constraint(ref7, 0.1), bad)
    assert np.isnan(m["v"]).all() and np.isnan(m["e"]).all()


def test_tilt_is_bounded_by_the_angular_xy_error(ref):
    """alpha <= sqrt(e_4^2 + e_5^2) on 10 000 random rotations: a 1-joint chain whose only frame is the identity and
    whose end-effector offset is the rotation (the header's FK, error and logarithm; alpha from the rotated z axis)."""
    rng = np.random.default_rng(8)
    quats = rng.normal(size=(10000, 4))
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    quats[:4] = [[0, 0, 0, 1.0], [1.0, 0, 0, 0], [0, 1.0, 0, 0], [math.sin(0.5), 0, 0, math.cos(0.5)]]
    chain = dict(origins=np.array([[0.0, 0, 0, 0, 0, 0, 1]]), axes=np.array([[0.0, 0, 1]]), lb=[-1.0], ub=[1.0])
    c = cu.free_constraint([0.0, 0, 0, 0, 0, 0, 1])
    worst = -math.inf
    for qt in quats:
        e = ref.measure(chain, c, [[0.0]], np.concatenate([[0.0, 0, 0], qt]))["e"][0]
        z = _qrot(qt, np.array([0.0, 0, 1.0]))
        alpha = math.atan2(math.hypot(z[0], z[1]), z[2])
        worst = max(worst, alpha - math.hypot(e[4], e[3]))
        assert alpha <= math.hypot(e[3], e[4]) + 1e-12
    assert worst > -1e-9  # (the bound is attained: rotations about an axis in the xy plane)


def test_projection(ref, oracle, chains):
    d, _ = chains["panda"]
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    c = cu.upright_constraint(_home7(oracle, chains), 0.1)
    rng = np.random.default_rng(12)
    x = rng.uniform(lb, ub, (512, 7))
    tol = 1e-6
    p = ref.project(d, c, x, tol, **PROJECT_DEFAULTS)
    ok = p["status"] == PROJECTED
    # a floor against a vacuous test, not a measurement
    assert ok.sum() >= 256, ok.sum()
    assert set(np.unique(p["status"])) <= {PROJECTED, BUDGET_SPENT, FAILED}
    again = ref.measure(d, c, p["x"])["v"]
    assert np.array_equal(bits(again), bits(p["v"]))
    assert (again[ok] <= tol).all() and (again[~ok] > tol).all()
    assert (p["x"] >= lb).all() and (p["x"] <= ub).all()
    assert (p["iterations"][p["status"] == BUDGET_SPENT] == PROJECT_DEFAULTS["iters"]).all()
    assert (p["iterations"][ok] <= PROJECT_DEFAULTS["iters"]).all() and p["iterations"][ok].max() > 1
    # a row that satisfies the constraint comes back unchanged after 0 iterations
    p2 = ref.project(d, c, p["x"][ok], tol, **PROJECT_DEFAULTS)
    assert np.array_equal(bits(p2["x"]), bits(p["x"][ok])) and not p2["iterations"].any()
    assert (p2["status"] == PROJECTED).all()
    # NaN and infinite rows: status 2, the row as it came, violation NaN
    bad = x[:3].copy()
    bad[0, 2], bad[1, 0], bad[2, 6] = math.nan, math.inf, -math.inf
    p3 = ref.project(d, c, bad, tol, **PROJECT_DEFAULTS)
    assert (p3["status"] == FAILED).all() and not p3["iterations"].any() and np.isnan(p3["v"]).all()
    assert np.array_equal(bits(p3["x"]), bits(bad))
    # a spent budget: iters = 0 evaluates once
    p4 = ref.project(d, c, x[:8], tol, 0, PROJECT_DEFAULTS["damping"], PROJECT_DEFAULTS["max_step"])
    assert np.array_equal(bits(p4["x"]), bits(x[:8])) and not p4["iterations"].any()
    assert (p4["status"] == np.where(ref.measure(d, c, x[:8])["v"] <= tol, PROJECTED, BUDGET_SPENT)).all()
    # a start outside the limits is clamped first
    out = x[:1].copy()
    out[0, 1] = ub[1] + 0.5
    p5 = ref.project(d, c, out, tol, 0, 1e-6, 0.5)
    assert p5["x"][0, 1] == ub[1]


def test_motion_against_numpy(ref, oracle, chains):
    d, _ = chains["panda"]
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    c = cu.upright_constraint(_home7(oracle, chains), 0.6)
    rng = np.random.default_rng(15)
    qa = rng.uniform(lb, ub, (24, 7))
    qb = np.clip(qa + rng.uniform(-0.5, 0.5, (24, 7)) * rng.choice([0.02, 0.3, 1.0], (24, 1)), lb, ub)
    qb[0] = qa[0]                      # K = 1
    qa[1, 2] = math.nan                # not sampled
    qb[2] = qa[2]; qb[2, 0] += 500.0   # more than 4096 steps
    h, tol = 0.05, 0.2
    got = ref.motion(d, c, qa, qb, h, tol)
    oks = 0
    for b in range(len(qa)):
        v, ok, first, K = cu.np_motion(ref, d, c, qa[b], qb[b], h, tol)
        assert bits(got["v"][b]) == bits(v) and got["ok"][b] == ok and got["first"][b] == first and got["steps"][b] == K
        oks += ok
    assert got["steps"][0] == 1 and got["steps"][1] == -1 and got["steps"][2] == -1
    assert math.isnan(got["v"][1]) and not got["ok"][1] and got["first"][1] == -1
    assert 0 < oks < len(qa) - 2


def test_motion_whose_ends_satisfy_and_whose_middle_does_not(ref, oracle, chains):
    """Two Panda configurations that differ by pi in the last wrist joint, which turns about the flange's z axis,
    under a constraint that bounds the angular z error to +-(pi / 2 + 0.01).  With the reference at the pose in the
    middle of the motion the whole motion is inside the box.  With that reference turned by pi about z both ends are
    still pi / 2 from it -- they satisfy the constraint -- and the middle is pi away: the motion is not ok, the first
    violating sample is sample 1, and a check of the ends alone would have passed it."""
    d, oc = chains["panda"]
    a = np.array(cu.PANDA_HOME)
    a[6] = -1.5
    b = a.copy()
    b[6] = a[6] + math.pi
    mid = (a + b) / 2
    ref7 = np.asarray(oracle.fk(oc, mid)[1])
    lo, hi = np.full(6, -np.inf), np.full(6, np.inf)
    lo[5], hi[5] = -math.pi / 2 - 0.01, math.pi / 2 + 0.01
    c_wide = cu.Constraint(ref7, lo, hi)
    h, tol = 0.1, 1e-9
    got = ref.motion(d, c_wide, [a], [b], h, tol)
    assert got["ok"][0] and got["steps"][0] == math.ceil(math.pi / h)
    ref_far = ref7.copy()
    ref_far[3:] = _qmul(ref7[3:], np.array([0.0, 0.0, 1.0, 0.0]))
    c = cu.Constraint(ref_far, lo, hi)
    ends = ref.measure(d, c, [a, b])
    assert (ends["v"] <= tol).all()
    got = ref.motion(d, c, [a], [b], h, tol)
    K = got["steps"][0]
    assert not got["ok"][0] and 0 < got["first"][0] < K
    assert abs(got["v"][0] - (math.pi / 2 - 0.01)) < h  # the middle sample is pi away from the reference
    assert got["first"][0] == cu.np_motion(ref, d, c, a, b, h, tol)[2] == 1


def test_constrained_plan_on_the_cpu(ref, roadmap_ref, oracle, chains):
    d, _ = chains["panda"]
    scene = cu.plan_scene(ref, d, _home7(oracle, chains))
    assert cu.PLAN_N > scene["projected"] >= cu.PLAN_N // 2  # (some NaN columns, most nodes)
    graph, w0, queries, plan = cu.cpu_plan(ref, roadmap_ref, d, scene)
    # at least one edge that is free of collision (no model: every sampled motion) is blocked by the constraint
    assert (np.isfinite(w0) & np.isinf(graph["w"])).sum() >= 1
    assert np.isfinite(graph["w"]).sum() >= 1
    nan_cols = np.isnan(scene["nodes"]).any(axis=0)
    assert np.isinf(graph["w"][:, nan_cols]).all()
    found = plan["status"] == FOUND
    assert found.sum() >= 1 and (plan["len"][found] > 2).any()
    # every segment of every found path passes the check in the direction of travel
    for j in np.nonzero(found)[0]:
        p = plan["path"][:plan["len"][j], j]
        assert ref.motion(d, scene["c"], p[:-1], p[1:], cu.PLAN_H, cu.PLAN_TOL)["ok"].all()
        assert np.array_equal(p[0], scene["starts"][:, j]) and np.array_equal(p[-1], scene["goals"][:, j])
