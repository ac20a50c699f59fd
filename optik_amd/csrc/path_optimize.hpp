// path_optimize.hpp -- covariant gradient smoothing of joint-space paths (after CHOMP, Ratliff et al. 2009): one source
// for the host and the device (optik_hip_path_optimize, optik_hip.h).  collision_gradient.hpp
// says, per frame, how far the closest obstacle is and which way is out; this header turns those rows into a cost of
// a whole path and one step down its gradient, measured in the metric of the first differences.
//
// A deliberate simplification of CHOMP: the obstacle cost is the hinge of the clearance rows in joint space, without
// the workspace-velocity weighting of the original (no |x'| factor, no projection orthogonal to the motion), and the
// joint limits are a plain clamp after the step, not CHOMP's covariant limit projection.
//
// A path has L waypoints q_0 .. q_{L-1} of n joints, 3 <= L <= 64; q_0 and q_{L-1} never move, M = L - 2 are free.
// Parameters: step > 0, w_smooth >= 0, w_obs >= 0, influence > safety >= 0;  e = influence - safety.
//
// The exact operation order (both sides: -ffp-contract=off, only + - * / sqrt and comparisons):
//
//  1. The hinge of a row at distance dist, d = dist - safety:
//         d != d:        c = d,                                 c' = d            (NaN stays NaN)
//         d < 0:         c = (-d) + 0.5 * e,                    c' = -1
//         0 <= d <= e:   c = ((d - e) * (d - e)) / (2.0 * e),   c' = (d - e) / e
//         otherwise:     c = 0,                                 c' = 0            (a +inf row costs nothing)
//  2. An interior waypoint t (1 <= t <= L - 2) with the witness table of q_t (collision_gradient.hpp: dist[f],
//     grad[f][j], f = 0 .. n + 1), the sums starting from 0.0 and running over f ascending:
//         o_t      = ((0.0 + c(d_0)) + c(d_1)) + ...
//         gobs_t,j = ((0.0 + c'(d_0) * grad[0][j]) + c'(d_1) * grad[1][j]) + ...
//  3. A segment t (0 <= t <= L - 2), j ascending from 0.0:   s_t = ... + (q_{t+1,j} - q_{t,j}) * (q_{t+1,j} - q_{t,j})
//  4. The costs, t ascending from 0.0:   F_smooth = 0.5 * (s_0 + s_1 + ...),   F_obs = o_1 + ... + o_{L-2},
//         U = w_smooth * F_smooth + w_obs * F_obs
//  5. The clearance of a waypoint: the smallest dist of its rows (d < best, from +inf), NaN if any row is NaN; of the
//     path: the smallest over all L waypoints (the two fixed ones included, t ascending), NaN if any is NaN.
//  6. One update, every waypoint from the same old iterate (Jacobi):
//         g_t,j = w_smooth * ((2.0 * q_t,j - q_{t-1},j) - q_{t+1},j) + w_obs * gobs_t,j
//         Ainv(i, k) = (double)(min(i, k) * (M + 1 - max(i, k))) / (double)(M + 1),   i, k = 1 .. M
//             (the inverse of the M x M tridiagonal (-1, 2, -1) matrix of the first differences, in closed form)
//         y_i,j = ((0.0 + Ainv(i, 1) * g_1,j) + Ainv(i, 2) * g_2,j) + ...              (k ascending: no serial solve)
//         x = q_i,j - step * y_i,j
//         q_i,j <- x < lb_j ? lb_j : (x > ub_j ? ub_j : x)                            (a NaN stays a NaN)
//  7. Under a pose constraint (constraint_measure.hpp: a box lo[6], hi[6] about a reference pose; DESIGN.md section
//     5.32) an update is step 6 and then, for every interior waypoint i on its own, from x_j = the stepped and clamped
//     value of step 6 for every joint j:
//         the box free on every axis (lo_a == -inf and hi_a == +inf, a = 0 .. 5):   q_i <- x; nothing is evaluated and
//             no counter moves (box_is_free, settle)
//         otherwise constraint::project(.., ptol, piters, damping, max_step, x) as it is, attempted = attempted + 1:
//             it ends PROJECTED:        q_i <- x as projected, ended = ended + 1
//             any other status:         q_i keeps its old value, copied bit for bit
//     The two end waypoints are never projected.  So a waypoint that satisfies the constraint at ptol in one iterate
//     satisfies it in the next.  Steps 1 - 5 are unchanged; the path's violation is v = 0.0, then
//     v = constraint::max_take(v, violation of q_t) (constraint::measure) for t = 0 .. L - 1 of the last iterate.
//     This header does not include constraint_measure.hpp (g++ compiles it alone): the projection comes in as a callable.
//
// Plain host C++ compiles this header too (no HIP runtime): tests/path_optimize_util.py drives path_step with g++.
#pragma once

#include "collision_gradient.hpp"

namespace optik {
namespace pathopt {

constexpr int MAX_WAYPOINTS = 64;  // one lane of a wave per waypoint
constexpr int MIN_WAYPOINTS = 3;

struct Params {
    double step, w_smooth, w_obs, influence, safety;
};

// influence > safety >= 0, step > 0, the weights >= 0, all finite (the EINVAL rule of the entry points).
inline bool params_ok(const Params &p) {
    return p.step > 0.0 && p.step < INFINITY && p.w_smooth >= 0.0 && p.w_smooth < INFINITY && p.w_obs >= 0.0
           && p.w_obs < INFINITY && p.influence > p.safety && p.influence < INFINITY && p.safety >= 0.0;
}

// Step 1: c and c' of a row at distance dist.
OPTIK_CM_HD inline void hinge(double dist, double safety, double e, double &c, double &cp) {
    const double d = dist - safety;
    if (d != d) {
        c = d; cp = d;
    } else if (d < 0.0) {
        c = (-d) + 0.5 * e; cp = -1.0;
    } else if (d <= e) {
        c = ((d - e) * (d - e)) / (2.0 * e); cp = (d - e) / e;
    } else {
        c = 0.0; cp = 0.0;
    }
}

// Step 2, one term of gobs_t,j.
OPTIK_CM_HD inline double add_scaled(double acc, double cp, double g) { return acc + cp * g; }

// Step 3, one term of s_t.
OPTIK_CM_HD inline double add_square(double acc, double qa, double qb) {
    const double d = qb - qa;
    return acc + d * d;
}

// Step 4.
OPTIK_CM_HD inline void costs(const Params &p, double sum_s, double sum_o, double *cost3) {
    cost3[1] = 0.5 * sum_s;
    cost3[2] = sum_o;
    cost3[0] = p.w_smooth * cost3[1] + p.w_obs * cost3[2];
}

// Step 5: the running minimum and the NaN flag.
OPTIK_CM_HD inline void clearance_take(double d, double &best, bool &nan) {
    if (d != d) nan = true;
    if (d < best) best = d;
}

// Step 6.
OPTIK_CM_HD inline double gradient_term(const Params &p, double qm, double q, double qp, double gobs) {
    return p.w_smooth * ((2.0 * q - qm) - qp) + p.w_obs * gobs;
}
OPTIK_CM_HD inline double ainv(int i, int k, int M) {
    const int lo = i < k ? i : k, hi = i < k ? k : i;
    return (double)(lo * (M + 1 - hi)) / (double)(M + 1);
}
OPTIK_CM_HD inline double stepped(const Params &p, double q, double y, double lb, double ub) {
    const double x = q - p.step * y;
    return x < lb ? lb : (x > ub ? ub : x);
}

// Step 7.
OPTIK_CM_HD inline bool box_is_free(const double *lo6, const double *hi6) {
    bool free_box = true;
    for (int a = 0; a < 6; ++a) free_box = free_box && lo6[a] == -INFINITY && hi6[a] == INFINITY;
    return free_box;
}
// x: step 6's values of one interior waypoint in, projected in place by project(x), which says whether it ended
// PROJECTED.  True: q_i <- x; false: q_i keeps its old value (x is then of no use).
template <class Project>
OPTIK_CM_HD inline bool settle(bool free_box, double *x, Project &&project, int &attempted, int &ended) {
    if (free_box) return true;
    attempted = attempted + 1;
    if (!project(x)) return false;
    ended = ended + 1;
    return true;
}

// The reference form (the tests' g++ driver): one evaluation of a path and, with q_new, one update.
// q [L][n]; dist [L][n + 2] and grad [L][n + 2][n] the witness tables of the L waypoints (witness_rows); lb, ub [n].
// Out: cost3 = (U, F_smooth, F_obs), the path clearance, wp_clearance [L] (may be null), g_out [L][n] the gradient of
// U with respect to the waypoints (rows 0 and L - 1 zero; may be null), q_new [L][n] (null: evaluate only).
inline void path_step(int n, int L, const double *q, const double *dist, const double *grad, const double *lb,
                      const double *ub, const Params &p, double *cost3, double *clearance, double *wp_clearance,
                      double *g_out, double *q_new) {
    const int nf = n + 2, M = L - 2;
    const double e = p.influence - p.safety;
    double o[MAX_WAYPOINTS], gobs[MAX_WAYPOINTS][8], g[MAX_WAYPOINTS][8];
    double best = INFINITY;
    bool any_nan = false;
    for (int t = 0; t < L; ++t) {
        double wb = INFINITY;
        bool wn = false;
        for (int f = 0; f < nf; ++f) clearance_take(dist[t * nf + f], wb, wn);
        if (wn) wb = NAN;
        if (wp_clearance) wp_clearance[t] = wb;
        clearance_take(wb, best, any_nan);
        o[t] = 0.0;
        for (int j = 0; j < n; ++j) gobs[t][j] = 0.0;
        if (t == 0 || t == L - 1) continue;
        for (int f = 0; f < nf; ++f) {
            double c, cp;
            hinge(dist[t * nf + f], p.safety, e, c, cp);
            o[t] = o[t] + c;
            for (int j = 0; j < n; ++j) gobs[t][j] = add_scaled(gobs[t][j], cp, grad[(t * nf + f) * n + j]);
        }
    }
    *clearance = any_nan ? NAN : best;
    double sum_s = 0.0, sum_o = 0.0;
    for (int t = 0; t + 1 < L; ++t) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) s = add_square(s, q[t * n + j], q[(t + 1) * n + j]);
        sum_s = sum_s + s;
    }
    for (int t = 1; t + 1 < L; ++t) sum_o = sum_o + o[t];
    costs(p, sum_s, sum_o, cost3);
    for (int j = 0; j < n; ++j) { g[0][j] = 0.0; g[L - 1][j] = 0.0; }
    for (int t = 1; t <= M; ++t)
        for (int j = 0; j < n; ++j)
            g[t][j] = gradient_term(p, q[(t - 1) * n + j], q[t * n + j], q[(t + 1) * n + j], gobs[t][j]);
    if (g_out)
        for (int t = 0; t < L; ++t)
            for (int j = 0; j < n; ++j) g_out[t * n + j] = g[t][j];
    if (!q_new) return;
    for (int j = 0; j < n; ++j) {
        q_new[j] = q[j];
        q_new[(L - 1) * n + j] = q[(L - 1) * n + j];
    }
    for (int i = 1; i <= M; ++i)
        for (int j = 0; j < n; ++j) {
            double y = 0.0;
            for (int k = 1; k <= M; ++k) y = y + ainv(i, k, M) * g[k][j];
            q_new[i * n + j] = stepped(p, q[i * n + j], y, lb[j], ub[j]);
        }
}

}  // namespace pathopt
}  // namespace optik
