// constraint_measure.hpp -- pose constraints: the error of a configuration against a reference pose, its residual
// against a box, the projection of a configuration onto the box and the check of the box along a motion; one source
// for the host and the device (optik_hip_constraint_batch, optik_hip_constraint_project_batch and
// optik_hip_constraint_motion_batch, optik_hip.h).
//
// A pose constraint is a reference pose ref[7] (t, quaternion i j k w: the library's pose layout) and a box lo[6],
// hi[6] with lo <= hi, either end of an axis possibly infinite.  The chain has 1 <= n <= MAXN revolute joints, n known
// at run time, and an optional trailing fixed joint; CH is ChainDev or WideChainDev (or any table with their members).
// The exact operation order (the tests depend on it; -ffp-contract=off on both sides; only the correctly rounded
// + - * / sqrt, comparisons, and the functions of ik_math.hpp, which are used as they are):
//
//  1. FK (constraint::fk; the sequence of ik_eval.hpp's forward pass with the joint loop rolled): for j = 0 .. n-1,
//     sincos_dev(q_j / 2), local = (axis_j * s, c), jt = (origin_j.t, qmul(origin_j.q, local)), state = jt for j = 0 and
//     pose_mul(state, jt) after it, tf_j = state.  ee = state, then pose_mul(ee, origin_n) with a trailing fixed joint,
//     then pose_mul(ee, ee_offset) with an ee_offset.
//  2. Error (constraint::error): X = pose_inv_mul(ref, ee), w = so3_log(X.q), rt = rot_terms(w),
//     e = (se3_log_linear(rt, X.t), w): linear x y z, then angular x y z -- the six numbers ik_eval.hpp forms before it
//     weights them, with ref in the place of the target.
//  3. Residual (constraint::residual), i = 0 .. 5: c = e_i; c = lo_i if e_i < lo_i; c = hi_i if c > hi_i; r_i = e_i - c.
//     An error on a bound has r_i = 0 exactly; a NaN e_i gives a NaN r_i; lo_i = -inf and hi_i = +inf free the axis.
//  4. Violation (constraint::violation): v = 0, then for i ascending a = |r_i| and v = a if a > v or a is NaN -- the
//     maximum, NaN as soon as one e_i is, and kept.  A configuration satisfies the constraint at tol >= 0 iff v <= tol.
//  5. Task Jacobian (constraint::task_jacobian), J[6 k + r], column k = 0 .. n-1: Jr = so3_right_jacobian(rt),
//     Qm = se3_q_matrix(rt, X.t, Jr); angular = qrot(tf_k.q, axis_k), linear = cross(angular, ee.t - tf_k.t), both
//     rotated by conj(ee.q) into the body frame (the column of J_body); then for r = 0, 1, 2
//     J[6 k + r] = ((0 + Jr[r][0] lin_0 + Jr[r][1] lin_1 + Jr[r][2] lin_2) + Qm[r][0] ang_0 + ..) and
//     J[6 k + r + 3] = (0 + Jr[r][0] ang_0 + Jr[r][1] ang_1 + Jr[r][2] ang_2): Jtask = Jlog6 * J_body, the matrix
//     ik_eval.hpp builds column by column.
//  6. Projection (constraint::project), damped Gauss-Newton.  A row with a NaN or infinite joint: status 2, nothing
//     else is done (x as it came, violation NaN, 0 iterations).  Otherwise x_i = lb_i if x_i < lb_i, ub_i if x_i > ub_i
//     (a row inside the limits is not changed), it = 0, and then, repeated:
//       a. steps 1 - 4 at x give e, r, v.
//       b. v NaN: status 2, stop.  v <= tol: status 0, stop.  it == iters: status 1, stop.
//       c. A = the task Jacobian of step 5 with row i zeroed (0.0 stored) where r_i == 0.
//       d. M[a][b] for a >= b: s = 0, s = s + A[a][k] * A[b][k] for k ascending; M[a][a] = s + damping.
//       e. Cholesky M = L L', column j = 0 .. 5: acc = M[j][j], acc = acc - L[j][k] * L[j][k] for k < j ascending; unless
//          acc > 0 and finite: status 2, stop (a failed factorisation); L[j][j] = sqrt(acc); for i > j:
//          a = M[i][j], a = a - L[i][k] * L[j][k] for k < j ascending, L[i][j] = a / L[j][j].
//       f. L z = r: z_i = (r_i - L[i][k] z_k, k < i ascending) / L[i][i] for i ascending;  L' y = z:
//          y_i = (z_i - L[k][i] y_k, k = i+1 .. 5 ascending) / L[i][i] for i descending.
//       g. dx_k = -(0 + A[0][k] y_0 + .. + A[5][k] y_5);  m = max_k |dx_k| (as step 4); if m > max_step:
//          s = max_step / m and dx_k = dx_k * s.
//       h. x_k = x_k + dx_k, then clamped as above; it = it + 1.
//     The outputs are x, the violation of the last a., the status and it.  A row of status 0 satisfies the constraint
//     at tol (v was evaluated at the x that is returned) and lies within the joint limits (every x is clamped).
//  7. Motion (constraint::motion): d, K and the samples q_k of motion_measure.hpp steps 1 - 3.  K < 0 (not sampled):
//     violation NaN, ok 0, first -1, steps -1.  Otherwise for k = 0 .. K steps 1 - 4 at q_k give v_k; the violation is
//     the maximum as step 4 takes it (NaN if any v_k is), first the lowest k with v_k <= tol false, -1 if none,
//     ok = (first == -1), steps = K.  Nothing is projected: it says only what holds at the samples.
//
// Property (upright).  Let alpha be the angle between the end effector's z axis and the reference's, and theta = |w| <=
// pi the rotation angle of X with unit axis u, w = theta u = (e_3, e_4, e_5).  Then alpha <= sqrt(e_4^2 + e_5^2).
// Proof: cos alpha = (R z).z = 1 - (1 - cos theta)(u_x^2 + u_y^2), so with s = sqrt(u_x^2 + u_y^2) in [0, 1],
// sin(alpha / 2) = s sin(theta / 2), that is alpha = 2 asin(s sin(theta / 2)).  asin is convex on [0, 1] with
// asin(0) = 0, so asin(s y) <= s asin(y) for s in [0, 1]: alpha <= 2 s (theta / 2) = s theta = sqrt(e_4^2 + e_5^2).
// So the box |e_4|, |e_5| <= tilt / sqrt(2), everything else free, guarantees alpha <= tilt ("upright within tilt");
// PoseConstraint.upright builds exactly that box.
//
// Plain host C++ compiles this header too, under OPTIK_LANE_EMU as ik_math.hpp needs it (tests/constraint_util.py).
#pragma once

#include "ik_eval.hpp"
#include "motion_measure.hpp"

namespace optik {
namespace constraint {

constexpr int MAXN = 16;  // joint positions (the general solver's limit)
constexpr double CM_DBL_MAX = 1.7976931348623157e308;

enum { PROJECTED = 0, BUDGET_SPENT = 1, FAILED = 2 };  // OPTIK_HIP_CONSTRAINT_* (optik_hip.h)

struct Box {
    double ref[7];
    double lo[6], hi[6];
};

OPTIK_DEV double cm_fabs(double x) { return x < 0.0 ? -x : x; }
OPTIK_DEV bool cm_finite(double x) { return x >= -CM_DBL_MAX && x <= CM_DBL_MAX; }
OPTIK_DEV double cm_nan() { return __builtin_nan(""); }
// the running maximum v with the term a, a NaN taken and then kept
OPTIK_DEV double max_take(double v, double a) { return (a > v || a != a) ? a : v; }

// Step 1.
template <class CH>
__device__ inline Pose fk(const CH &ch, const EvalParams &ep, int n, const double *q, double *tf) {
    Pose state;
    state.t = V3{0.0, 0.0, 0.0};
    state.q = Q4{0.0, 0.0, 0.0, 1.0};
#pragma unroll 1
    for (int j = 0; j < n; ++j) {
        double s, c;
        sincos_dev(q[j] / 2.0, s, c);
        const Q4 local{ch.axis[j][0] * s, ch.axis[j][1] * s, ch.axis[j][2] * s, c};
        Pose jt;
        jt.t = V3{ch.origin[j][0], ch.origin[j][1], ch.origin[j][2]};
        jt.q = qmul(Q4{ch.origin[j][3], ch.origin[j][4], ch.origin[j][5], ch.origin[j][6]}, local);
        state = (j == 0) ? jt : pose_mul(state, jt);
        tf[7 * j + 0] = state.t.x; tf[7 * j + 1] = state.t.y; tf[7 * j + 2] = state.t.z;
        tf[7 * j + 3] = state.q.i; tf[7 * j + 4] = state.q.j; tf[7 * j + 5] = state.q.k; tf[7 * j + 6] = state.q.w;
    }
    if (ch.has_tip) state = pose_mul(state, load_pose(ch.origin[n]));
    return ep.has_ee_offset ? pose_mul(state, load_pose(ep.ee_offset)) : state;
}

// What steps 2 and 5 share for one configuration.
struct ErrorTerms {
    Pose X;
    RotTerms rt;
    double e[6];
};

// Step 2.
__device__ inline ErrorTerms error(const Box &c, const Pose ee) {
    ErrorTerms t;
    t.X = pose_inv_mul(load_pose(c.ref), ee);
    const V3 w = so3_log(t.X.q);
    t.rt = rot_terms(w);
    const V3 elin = se3_log_linear(t.rt, t.X.t);
    t.e[0] = elin.x; t.e[1] = elin.y; t.e[2] = elin.z;
    t.e[3] = w.x; t.e[4] = w.y; t.e[5] = w.z;
    return t;
}

// Step 3.
OPTIK_DEV void residual(const Box &c, const double (&e)[6], double (&r)[6]) {
    for (int i = 0; i < 6; ++i) {
        double b = e[i];
        if (e[i] < c.lo[i]) b = c.lo[i];
        if (b > c.hi[i]) b = c.hi[i];
        r[i] = e[i] - b;
    }
}

// Step 4.
OPTIK_DEV double violation(const double (&r)[6]) {
    double v = 0.0;
    for (int i = 0; i < 6; ++i) v = max_take(v, cm_fabs(r[i]));
    return v;
}

// Step 5: J[6 k + r].
template <class CH>
__device__ inline void task_jacobian(const CH &ch, int n, const double *tf, const Pose ee, const ErrorTerms &t,
                                     double *J) {
    const M3 Jr = so3_right_jacobian(t.rt);
    const M3 Qm = se3_q_matrix(t.rt, t.X.t, Jr);
    const Q4 eeqc = qconj(ee.q);
#pragma unroll 1
    for (int k = 0; k < n; ++k) {
        const V3 tk{tf[7 * k + 0], tf[7 * k + 1], tf[7 * k + 2]};
        const Q4 tq{tf[7 * k + 3], tf[7 * k + 4], tf[7 * k + 5], tf[7 * k + 6]};
        const V3 ax{ch.axis[k][0], ch.axis[k][1], ch.axis[k][2]};
        const V3 angular = qrot(tq, ax);
        const V3 d{ee.t.x - tk.x, ee.t.y - tk.y, ee.t.z - tk.z};
        const V3 linear = cross(angular, d);
        const V3 al = qrot(eeqc, angular);
        const V3 ll = qrot(eeqc, linear);
        const double lin[3] = {ll.x, ll.y, ll.z};
        const double ang[3] = {al.x, al.y, al.z};
        for (int r = 0; r < 3; ++r) {
            double acc = 0.0;
            for (int m = 0; m < 3; ++m) acc += Jr.m[r][m] * lin[m];
            for (int m = 0; m < 3; ++m) acc += Qm.m[r][m] * ang[m];
            J[6 * k + r] = acc;
            double acc2 = 0.0;  // (the lower-left block of Jlog6 is zero)
            for (int m = 0; m < 3; ++m) acc2 += Jr.m[r][m] * ang[m];
            J[6 * k + r + 3] = acc2;
        }
    }
}

// Steps 1 - 4 at q: the residual, returns the violation.
template <class CH>
__device__ inline double measure(const CH &ch, const EvalParams &ep, const Box &c, int n, const double *q,
                                 double (&r)[6]) {
    double tf[7 * MAXN];
    const Pose ee = fk(ch, ep, n, q, tf);
    const ErrorTerms t = error(c, ee);
    residual(c, t.e, r);
    return violation(r);
}

// Step 6 e - f: solves M y = r in place of r (M's lower triangle is overwritten by L); false: a failed factorisation.
__device__ inline bool cholesky_solve(double (&M)[6][6], double (&y)[6]) {
    for (int j = 0; j < 6; ++j) {
        double acc = M[j][j];
        for (int k = 0; k < j; ++k) acc = acc - M[j][k] * M[j][k];
        if (!(acc > 0.0 && acc <= CM_DBL_MAX)) return false;
        const double ljj = __builtin_sqrt(acc);
        M[j][j] = ljj;
        for (int i = j + 1; i < 6; ++i) {
            double a = M[i][j];
            for (int k = 0; k < j; ++k) a = a - M[i][k] * M[j][k];
            M[i][j] = a / ljj;
        }
    }
    for (int i = 0; i < 6; ++i) {
        double a = y[i];
        for (int k = 0; k < i; ++k) a = a - M[i][k] * y[k];
        y[i] = a / M[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double a = y[i];
        for (int k = i + 1; k < 6; ++k) a = a - M[k][i] * y[k];
        y[i] = a / M[i][i];
    }
    return true;
}

struct Projected {
    double violation;
    int status, iterations;
};

// Step 6: x [n] in and out.
template <class CH>
__device__ inline Projected project(const CH &ch, const EvalParams &ep, const Box &c, int n, double tol, int iters,
                                    double damping, double max_step, double *x) {
    Projected out{cm_nan(), FAILED, 0};
    for (int i = 0; i < n; ++i)
        if (!cm_finite(x[i])) return out;
    for (int i = 0; i < n; ++i) {
        if (x[i] < ch.lb[i]) x[i] = ch.lb[i];
        if (x[i] > ch.ub[i]) x[i] = ch.ub[i];
    }
    double tf[7 * MAXN], J[6 * MAXN], dx[MAXN];
#pragma unroll 1
    for (int it = 0;; ++it) {
        const Pose ee = fk(ch, ep, n, x, tf);
        const ErrorTerms t = error(c, ee);
        double r[6];
        residual(c, t.e, r);
        const double v = violation(r);
        out.violation = v;
        out.iterations = it;
        if (v != v) { out.status = FAILED; return out; }
        if (v <= tol) { out.status = PROJECTED; return out; }
        if (it == iters) { out.status = BUDGET_SPENT; return out; }
        task_jacobian(ch, n, tf, ee, t, J);
        for (int i = 0; i < 6; ++i)
            if (r[i] == 0.0)
                for (int k = 0; k < n; ++k) J[6 * k + i] = 0.0;
        double M[6][6];
        for (int a = 0; a < 6; ++a)
            for (int b = 0; b <= a; ++b) {
                double s = 0.0;
                for (int k = 0; k < n; ++k) s = s + J[6 * k + a] * J[6 * k + b];
                M[a][b] = s;
            }
        for (int a = 0; a < 6; ++a) M[a][a] = M[a][a] + damping;
        if (!cholesky_solve(M, r)) { out.status = FAILED; return out; }
        double m = 0.0;
        for (int k = 0; k < n; ++k) {
            double s = 0.0;
            for (int i = 0; i < 6; ++i) s = s + J[6 * k + i] * r[i];
            dx[k] = -s;
            m = max_take(m, cm_fabs(dx[k]));
        }
        if (m > max_step) {
            const double s = max_step / m;
            for (int k = 0; k < n; ++k) dx[k] = dx[k] * s;
        }
        for (int k = 0; k < n; ++k) {
            double xn = x[k] + dx[k];
            if (xn < ch.lb[k]) xn = ch.lb[k];
            if (xn > ch.ub[k]) xn = ch.ub[k];
            x[k] = xn;
        }
    }
}

struct MotionResult {
    double violation;
    int ok, first, steps;
};

// Step 7: qa_i = qa[i * sa], qb_i = qb[i * sb].
template <class CH>
__device__ inline MotionResult motion(const CH &ch, const EvalParams &ep, const Box &c, int n, const double *qa,
                                      long long sa, const double *qb, long long sb, double h, double tol) {
    const double d = optik::motion::motion_distance(n, qa, sa, qb, sb);
    const int K = optik::motion::motion_steps(d, h);
    if (K < 0) return MotionResult{cm_nan(), 0, -1, -1};
    MotionResult out{0.0, 1, -1, K};
#pragma unroll 1
    for (int k = 0; k <= K; ++k) {
        double q[MAXN], r[6];
        for (int i = 0; i < n; ++i) q[i] = optik::motion::motion_sample(qa[i * sa], qb[i * sb], k, K);
        const double v = measure(ch, ep, c, n, q, r);
        out.violation = max_take(out.violation, v);
        if (!(v <= tol) && out.first < 0) out.first = k;
    }
    out.ok = out.first < 0 ? 1 : 0;
    return out;
}

}  // namespace constraint
}  // namespace optik
