// repair_measure.hpp -- collision repair: pushing ONE configuration out of collision along the gradient of its
// clearance, optionally keeping the end effector inside a pose box; one source for the host and the device
// (optik_hip_collision_repair_batch, optik_hip.h; ik_repair.hip).  It is the loop that
// path_optimize.hpp runs per waypoint (steps 1, 2, 5, 6 and 7 there) for a configuration without neighbours: no
// smoothness term, no metric, the step straight down the hinge's gradient, then the projection.
//
// A configuration x has n joints, 1 <= n <= 8 (the witness code's range).  Parameters: influence > safety >= 0,
// step > 0 (path_optimize.hpp's rule for the three), iters in 0 .. MAX_ITERS, max_move >= 0 or +inf (the default: no
// bound), e = influence - safety.  Optionally a pose box c (constraint_measure.hpp) with the projection's arguments
// ptol, piters, damping, max_step.  This header includes neither constraint_measure.hpp nor a forward kinematics
// (plain g++ compiles it alone): the witness table, the projection and the violation come in as callables.
//
// The exact operation order (both sides: -ffp-contract=off, only + - * / sqrt and comparisons), x_in = the input,
// k = 0, 1, ...:
//
//  1. The witness table of x (collision_gradient.hpp: rows f = 0 .. n + 1 of dist[f], grad[f][j]).  The clearance is
//     the smallest dist (d < best, from +inf, f ascending), NaN if any row is NaN: pathopt::clearance_take, step 5 of
//     path_optimize.hpp.  In the same pass over the rows, f ascending from 0.0:
//         gobs_j = ((0.0 + c'(dist_0) * grad[0][j]) + c'(dist_1) * grad[1][j]) + ...
//     with c' of pathopt::hinge(dist, safety, e) and pathopt::add_scaled, steps 1 and 2 there (called, not restated).
//     A row without a term (dist +inf) has grad 0; every row takes part, c' == 0 or not.
//  2. clearance NaN: status NAN (3), stop.  clearance >= safety: status FREE (0), stop.  At k == 0 that is an input
//     that was free already: x is never written, so it comes back bit for bit, iterations = 0, moved = 0.
//  3. k == iters: status LIMIT (1), stop.
//  4. gobs_j == 0 for every j: status STUCK (2), stop (the closest terms do not depend on any joint, or cancel).
//     Otherwise y_j = pathopt::stepped(x_j, gobs_j): t = x_j - step * gobs_j; y_j = t < lb_j ? lb_j : (t > ub_j ? ub_j
//     : t) -- step 6 there with gobs in the place of its metric's y.
//  5. The box free on every axis (pathopt::box_is_free; also: no box): y stays as it is, nothing is evaluated.
//     Otherwise project(y) -- constraint::project(.., ptol, piters, damping, max_step, y) as it is --; anything but
//     PROJECTED: status STUCK, stop, x keeps its last accepted value.
//     m = 0.0, then for j ascending a = |y_j - x_in_j|, m = a if a > m.  m > max_move: status STUCK, stop, x keeps its
//     last accepted value.  Otherwise x <- y, moved = m, k = k + 1, and again from 1.
//
// Outputs: x; clearance = step 1's of the returned x (the last evaluation was at it); violation = measure(x)
// (constraint::measure) of the returned x under a box that is not free, else 0.0; moved (0.0 until a step is
// accepted); status; iterations = k, the number of accepted steps.
//
// The invariant.  Status FREE with iterations > 0: the returned x has witness clearance >= safety (step 2 tested the
// clearance of this very x), lies within the joint limits (step 4 clamps, and the projection clamps every iterate) and,
// under a box that is not free, satisfies it at ptol (the projection ended PROJECTED at this very x; `violation` is
// that number measured again).  Status FREE with iterations == 0 says only that the input's clearance is >= safety: the
// input is returned untouched, whether or not it lies within the limits or the box; `violation` reports the box.
//
// Witness clearance and the clearance of optik_hip_collision_batch.  The minimum over the witness rows is
// coll::clearance / clearance_grid bit for bit (collision_gradient.hpp calls collision_measure.hpp's distance
// functions, every term once), which is the number optik_hip_collision_batch returns.  Neither contains the model's
// margin: the margin enters only the free flag, clearance >= margin.  So a FREE row has collision_batch's clearance
// >= safety, and it is free in the filter's sense whenever safety >= margin.
//
// Every loop is bounded: k by iters, the projection by piters, the rest by n.
#pragma once

#include "path_optimize.hpp"

namespace optik {
namespace repair {

constexpr int MAXN = 8;           // the witness code's range
constexpr int MAX_ITERS = 4096;   // OPTIK_HIP_REPAIR_MAX_ITERS (optik_hip.h)

enum : int { FREE = 0, LIMIT = 1, STUCK = 2, NOT_A_NUMBER = 3 };  // OPTIK_HIP_REPAIR_* (optik_hip.h)

struct Params {
    double influence, safety, step, max_move;
    int iters;
};

// influence > safety >= 0 and step > 0, all finite (pathopt::params_ok's rule for the three); iters in 0 .. MAX_ITERS;
// max_move >= 0, +inf allowed, no NaN (the EINVAL rule of the entry points).
inline bool params_ok(const Params &p) {
    return pathopt::params_ok(pathopt::Params{p.step, 0.0, 0.0, p.influence, p.safety}) && p.iters >= 0
           && p.iters <= MAX_ITERS && p.max_move >= 0.0;
}

struct Result {
    double clearance, violation, moved;
    int status, iterations;
};

// Step 1, one row: the running clearance and this row's c'.
OPTIK_CM_HD inline double row_take(double dist, double safety, double e, double &best, bool &nan) {
    double c, cp;
    pathopt::clearance_take(dist, best, nan);
    pathopt::hinge(dist, safety, e, c, cp);
    return cp;
}

// Step 1 over a table: dist [n + 2], grad [n + 2][n] -> the clearance and gobs [n].
OPTIK_CM_HD inline double fold_rows(int n, const double *dist, const double *grad, double safety, double e,
                                    double *gobs) {
    double best = INFINITY;
    bool nan = false;
    for (int j = 0; j < n; ++j) gobs[j] = 0.0;
    for (int f = 0; f < n + 2; ++f) {
        const double cp = row_take(dist[f], safety, e, best, nan);
        for (int j = 0; j < n; ++j) gobs[j] = pathopt::add_scaled(gobs[j], cp, grad[f * n + j]);
    }
    return nan ? NAN : best;
}

// Step 5: one term of m.
OPTIK_CM_HD inline double move_take(double m, double y, double x_in) {
    const double d = y - x_in, a = d < 0.0 ? -d : d;
    return a > m ? a : m;
}

// Steps 1 - 5 for one configuration x [n] (in and out), n <= MAXN.
//   evaluate(x, gobs) -> clearance   step 1 at x
//   project(y) -> bool               step 5: y projected in place; true: it ended PROJECTED
//   measure(x) -> violation          of the returned x (called once, and only under a box that is not free)
template <class Evaluate, class Project, class Measure>
OPTIK_CM_HD inline Result run(int n, const double *lb, const double *ub, const Params &p, bool free_box, double *x,
                              Evaluate &&evaluate, Project &&project, Measure &&measure) {
    const pathopt::Params pp{p.step, 0.0, 0.0, p.influence, p.safety};
    Result out{0.0, 0.0, 0.0, LIMIT, 0};
    double x_in[MAXN], y[MAXN], gobs[MAXN];
    for (int j = 0; j < n; ++j) x_in[j] = x[j];
    for (int k = 0;; ++k) {
        out.iterations = k;
        out.clearance = evaluate(x, gobs);
        if (out.clearance != out.clearance) { out.status = NOT_A_NUMBER; break; }
        if (out.clearance >= p.safety) { out.status = FREE; break; }
        if (k == p.iters) { out.status = LIMIT; break; }
        bool zero = true;
        for (int j = 0; j < n; ++j) zero = zero && gobs[j] == 0.0;
        if (zero) { out.status = STUCK; break; }
        for (int j = 0; j < n; ++j) y[j] = pathopt::stepped(pp, x[j], gobs[j], lb[j], ub[j]);
        if (!free_box && !project(y)) { out.status = STUCK; break; }
        double m = 0.0;
        for (int j = 0; j < n; ++j) m = move_take(m, y[j], x_in[j]);
        if (m > p.max_move) { out.status = STUCK; break; }
        for (int j = 0; j < n; ++j) x[j] = y[j];
        out.moved = m;
    }
    out.violation = free_box ? 0.0 : measure(x);
    return out;
}

// The reference form (the tests' driver), serial: x [n] in and out.  witness(x, dist [n + 2], grad [n + 2][n]) fills
// the witness table of x (coll::witness_rows on the frames of x); project and measure as run() takes them.
template <class Witness, class Project, class Measure>
inline Result repair_reference(int n, const double *lb, const double *ub, const Params &p, bool free_box, double *x,
                               Witness &&witness, Project &&project, Measure &&measure) {
    const double e = p.influence - p.safety;
    return run(n, lb, ub, p, free_box, x,
               [&](const double *xx, double *gobs) {
                   double dist[MAXN + 2], grad[(MAXN + 2) * MAXN];
                   witness(xx, dist, grad);
                   return fold_rows(n, dist, grad, p.safety, e, gobs);
               },
               project, measure);
}

}  // namespace repair
}  // namespace optik
