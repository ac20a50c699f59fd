// rrt_constrained_measure.hpp -- the rules of the bidirectional tree planner under a pose constraint, one source for
// the host and the device (optik_hip_rrt_plan_constrained, optik_hip.h; ik_rrt.hip).
//
// rrt_goals_measure.hpp's planner with every node projected onto a pose constraint (constraint_measure.hpp: a box on
// the pose error against a reference) before it joins a tree, and every motion judged by the collision motion check AND
// by constraint::motion at tol, in the direction the path travels it (a constrained bidirectional RRT with one
// projected extension per tree and iteration).  Its rules are rrt_goals_measure.hpp's with these changes and no others
// (the exact operation order; the tests depend on it; -ffp-contract=off on both sides):
//
//  0. "A configuration is free" means: free by optik_hip_collision_batch AND violation <= tol by constraint::measure.
//     "A direct motion is free" means: free by the motion check AND ok by constraint::motion at tol.  So a start that
//     violates the constraint gives status 1 and a counted goal that violates it is not a root.  The order of the
//     cases is begin_goals', unchanged.
//  3. Iteration i: a = i & 1, b = 1 - a, r = sample i (restart seed first + i, NOT projected).  p = nearest of tree a
//     to r; the iteration does nothing if the steer does nothing or tree a is full.  c = steer(p, r), clamped; then
//     constraint::project(c, ptol, piters, damping, max_step): one projection attempted.  The iteration does nothing
//     if the projection's status is not PROJECTED, or if it ran at least one iteration and its result equals p in
//     every joint (==) (takes).  Otherwise c' = the projected configuration, and c' replaces c everywhere below.
//  4. m = nearest of tree b (as it was before the iteration) to c'.  If motion_distance(m, c') > eta and tree b is
//     not full, e = steer(m, c') is projected the same way (a second projection attempted) and e' is its result; a
//     projection that is not taken -- not PROJECTED, or equal to m after at least one iteration -- means no
//     back-extension.  Then the up to three motions p - c', c' - m and m - e' are judged in travel direction, with the
//     qa / qb arrays of rrt_measure.hpp's rule 4, by BOTH checks; a motion counts only if both pass.  p - c' not free:
//     nothing is appended.  Otherwise c' is appended to tree a with parent p; c' - m free: the query is found with the
//     junction (c', m); otherwise, with a back-extension whose motion m - e' is free, e' is appended to tree b with
//     parent m.  Both projections of an iteration are attempted before any verdict of it is known, so the second one
//     is counted whether p - c' turns out free or not.
//  5. - 7. (route, status, padding): unchanged.
//  8. projected[0] = the projections attempted, projected[1] = those that ended PROJECTED, candidates and
//     back-extensions together; both 0 where the iterations never began.
//
// Consequence.  With a box that is free on all six axes (lo = -inf, hi = +inf) every projection returns its input
// after 0 iterations (the candidate is clamped already) and every constraint verdict is ok wherever the motion is
// sampled, so every shared output equals optik_hip_rrt_plan_goals' bit for bit.
//
// Every node of a tree other than the roots has violation <= ptol at the end of its projection and lies inside the
// joint limits (constraint_measure.hpp step 6); the roots have violation <= tol.  What holds BETWEEN the nodes is what
// constraint::motion found at its samples with tol: edge interiors are not projected, so tol is the caller's statement
// of how far a straight joint-space motion between two projected nodes may leave the constraint.
//
// This header does not include constraint_measure.hpp: the reference at its end takes the projection as a callback, as
// it takes the verdicts, so plain g++ compiles it (tests/rrt_constrained_util.py) and the device is compared with it
// bit for bit on the device's own verdicts and projections.
#pragma once

#include "rrt_goals_measure.hpp"

namespace optik {
namespace rrt {

constexpr int PROJECTION_OK = 0;  // constraint::PROJECTED (ik_rrt.hip asserts the two are one)

// Rule 3 / 4: is a projection's result taken as a node?  status and iterations are constraint::project's; same_as_from:
// the result equals, joint by joint, the node it was steered from.
OPTIK_CM_HD inline bool takes(int status, int iterations, bool same_as_from) {
    return status == PROJECTION_OK && !(iterations >= 1 && same_as_from);
}

// ---- the serial reference (the tests' g++ driver; the device is compared with it bit for bit) --------------------

struct ConstrainedResult {
    Result r;
    int which, roots;
    int projected[2];
};

OPTIK_CM_HD inline bool same_joints(int n, const double *a, const double *b) {
    bool same = true;
    for (int i = 0; i < n; ++i) same = same && a[i] == b[i];
    return same;
}

// Rules 3 and 4 above for the iterations 0 .. I - 1 (grow_reference under a constraint).  project(x [n] in and out,
// &iterations) -> status.  motions_ok(count, qa, qb, ok): both checks of qa -> qb, as given; count is 2 or 3.
template <class MotionsOk, class Project>
inline void grow_constrained_reference(Tree *tree, int n, const double *lo, const double *hi, const double *samples,
                                       int I, double eta, int M, MotionsOk &&motions_ok, Project &&project, Result &res,
                                       int *projected) {
    double *seg = new double[8 * (size_t)n]();  // (zeroed: without a back-extension the third segment is not asked)
    double *c = seg, *e = seg + n;
    double *qa = seg + 2 * n, *qb = seg + 5 * n;  // three segments each
    for (int i = 0; i < I && res.status == RUNNING; ++i) {
        res.iters_used = i + 1;
        const int a = i & 1, b = 1 - a;
        const double *r = samples + (size_t)i * n;
        double d;
        const int p = tree[a].nearest(r, &d);
        if (!steers(d) || tree[a].count >= M) continue;
        const double *qp = tree[a].node(p);
        steer(n, qp, r, d, eta, lo, hi, c);
        int its = 0;
        int st = project(c, &its);
        projected[0] += 1;
        if (st == PROJECTION_OK) projected[1] += 1;
        if (!takes(st, its, same_joints(n, c, qp))) continue;
        double dm;
        const int m = tree[b].nearest(c, &dm);
        const double *qm = tree[b].node(m);
        bool back = extends_back(dm, eta, tree[b].count, M);
        if (back) {
            steer(n, qm, c, dm, eta, lo, hi, e);
            its = 0;
            st = project(e, &its);
            projected[0] += 1;
            if (st == PROJECTION_OK) projected[1] += 1;
            back = takes(st, its, same_joints(n, e, qm));
        }
        for (int j = 0; j < n; ++j) {
            qa[j] = a == 0 ? qp[j] : c[j];
            qb[j] = a == 0 ? c[j] : qp[j];
            qa[n + j] = a == 0 ? c[j] : qm[j];
            qb[n + j] = a == 0 ? qm[j] : c[j];
            // (tree b's travel direction is tree a's reversed)
            qa[2 * n + j] = b == 0 ? qm[j] : e[j];
            qb[2 * n + j] = b == 0 ? e[j] : qm[j];
        }
        unsigned char ok[3] = {0, 0, 0};
        motions_ok(back ? 3 : 2, qa, qb, ok);
        if (!ok[0]) continue;
        tree[a].append(c, p);
        if (ok[1]) {
            res.junction[a] = tree[a].count - 1;
            res.junction[b] = m;
            res.status = FOUND;
        } else if (back && ok[2]) {
            tree[b].append(e, m);
        }
    }
    delete[] seg;
    if (res.status == RUNNING) res.status = NO_ROUTE;
}

// plan_goals_reference under a constraint.  config_ok(q [n]) -> bool: free and violation <= tol; motions_ok and
// project as above (rule 0 calls motions_ok with count 1).  The other arguments are plan_goals_reference's.
template <class ConfigOk, class MotionsOk, class Project>
inline ConstrainedResult plan_constrained_reference(int n, const double *lo, const double *hi, const double *start,
                                                    const double *goals, int G, int count, const double *samples,
                                                    int I, double eta, int M, int Lmax, ConfigOk &&config_ok,
                                                    MotionsOk &&motions_ok, Project &&project, double *conf,
                                                    int32_t *parent, int32_t *root_goal, double *path_out) {
    Tree tree[2] = {{n, M, 0, conf, parent}, {n, M, 0, conf + (size_t)M * n, parent + M}};
    ConstrainedResult out{{RUNNING, 2, 0, {0, 0}, {-1, -1}, roadmap::inf()}, -1, 0, {0, 0}};
    Result &res = out.r;
    const int gc = clamp_count(count, G);
    for (int g = 0; g < G; ++g) root_goal[g] = -1;
    bool ends_finite = true;
    for (int i = 0; i < n; ++i) ends_finite = ends_finite && finite(start[i]);
    for (int g = 0; g < gc; ++g)
        for (int i = 0; i < n; ++i) ends_finite = ends_finite && finite(goals[(size_t)g * n + i]);
    int R = 0, direct = -1;
    const bool start_ok = ends_finite && gc > 0 && config_ok(start);
    if (start_ok) {
        for (int g = 0; g < gc; ++g)
            if (config_ok(goals + (size_t)g * n)) root_goal[R++] = g;
        double bd = roadmap::inf();
        for (int r = 0; r < R; ++r) {
            const double *goal = goals + (size_t)root_goal[r] * n;
            unsigned char ok = 0;
            motions_ok(1, start, goal, &ok);
            if (!ok) continue;
            const double d = motion::motion_distance(n, start, 1, goal, 1);
            if (direct_better(d, bd, direct)) { bd = d; direct = root_goal[r]; }
        }
    }
    out.roots = R;
    res.status = begin_goals(ends_finite, gc, start_ok, R, direct);
    if (res.status == RUNNING) {
        tree[0].append(start, -1);
        for (int r = 0; r < R; ++r) tree[1].append(goals + (size_t)root_goal[r] * n, -1);
        grow_constrained_reference(tree, n, lo, hi, samples, I, eta, M, motions_ok, project, res, out.projected);
    }
    res.nodes[0] = tree[0].count;
    res.nodes[1] = tree[1].count;
    // rules 5 and 7
    int *order = new int[2 * (size_t)M + 2];
    long long W = 2;
    if (res.junction[0] >= 0) {
        W = route_reference(tree, n, M, Lmax, conf, res, order);
        if (res.status == FOUND) out.which = root_goal[order[W - 1] - M];
    } else if (res.status == FOUND) {
        res.cost = 0.0 + motion::motion_distance(n, start, 1, goals + (size_t)direct * n, 1);
        res.status = found_status(2, Lmax);
        if (res.status == FOUND) out.which = direct;
    } else if (res.status == QUERY_NAN) {
        res.cost = roadmap::nan_value();
    }
    res.len = res.status == FOUND && res.junction[0] >= 0 ? (int)W : 2;
    const double *pad = res.status == FOUND ? goals + (size_t)out.which * n : (gc > 0 ? goals : start);
    for (int t = 0; t < Lmax; ++t)
        for (int i = 0; i < n; ++i) {
            double v = pad[i];
            if (t == 0) v = start[i];
            else if (t < res.len - 1) v = conf[(size_t)order[t] * n + i];
            path_out[(size_t)t * n + i] = v;
        }
    delete[] order;
    return out;
}

}  // namespace rrt
}  // namespace optik
