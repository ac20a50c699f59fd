// rrt_measure.hpp -- the rules of the bidirectional tree planner, one source for the host and the device
// (optik_hip_rrt_plan, optik_hip.h; ik_rrt.hip).
//
// A query grows two trees in joint space, tree 0 from its start and tree 1 from its goal, each of at most M nodes (a
// configuration and a parent index, -1 for the root), towards the random samples r_0, r_1, ... r_{I-1} that every
// query shares (sample i is restart seed first + i, optik_hip_seed_batch), and joins them by a motion that is free.
// The metric is L-infinity in radians (motion_measure.hpp's step 1); every motion is judged by the motion check
// (motion_measure.hpp) IN THE DIRECTION THE FINAL PATH TRAVELS IT: parent -> child in tree 0, child -> parent in tree
// 1, tree-0 node -> tree-1 node for a connection.  The exact operation order (the tests depend on it;
// -ffp-contract=off on both sides, only the correctly rounded - * / +, fabs and comparisons):
//
//  0. Before iteration 0: a NaN or infinite joint in the start or the goal ends the query with status 3 (cost NaN);
//     a start or goal that is not free (optik_hip_collision_batch's flag) with status 1 (cost +inf); a free direct
//     motion start -> goal with status 0, len 2.  iters_used is 0 in all three (begin).
//  1. Nearest (nearer): the node of a tree that comes first in roadmap_measure.hpp's total order on
//     (motion_distance(node, x), index): a number before a NaN, then the smaller distance, then the smaller index.
//  2. Steer from p towards x at distance d = motion_distance(p, x) with step eta (steers, steer_joint): nothing if d
//     is 0, NaN or infinite.  If d <= eta, c_j = x_j, copied.  Otherwise s = eta / d, t_j = s * (x_j - p_j),
//     c_j = p_j + t_j: the difference, the product and the sum each rounded.  Then the clamp, in this order:
//     if (c_j < lo_j) c_j = lo_j; if (c_j > hi_j) c_j = hi_j (a NaN limit clamps nothing).
//  3. Iteration i: a = i & 1, b = 1 - a, r = sample i.  p = nearest of tree a to r; c = steer(p, r).  The iteration
//     ends here if the steer does nothing, if tree a is full, or if the motion between p and c (travel direction) is
//     not free -- a motion that is not sampled is not free.  Otherwise c is appended to tree a with parent p.
//  4. Connect: m = nearest of tree b to c.  If the motion between c and m (travel direction: c -> m for a = 0, m -> c
//     for a = 1) is free the query is found with the junction (c in tree a, m in tree b).  Otherwise, if
//     motion_distance(m, c) > eta and tree b is not full, e = steer(m, c) is appended to tree b with parent m if the
//     motion between m and e (travel direction) is free.  m, e and the two verdicts are functions of c and of tree b
//     as it was before the iteration, so all three motions of an iteration may be judged in one batch; a verdict
//     that the rules do not ask for is not looked at.
//  5. A found path: tree 0 from its root to its junction node, then tree 1 from its junction node to its root: W
//     waypoints.  cost = the sum of motion_distance over consecutive waypoints, added from the start forwards from
//     0.0 in f64.  W <= Lmax: status 0, len W; W > Lmax: status 2 with the same cost.  iters_used = i + 1.
//  6. After I iterations without a junction: status 1, cost +inf, iters_used = I.
//  7. The path [Lmax][n]: the waypoints padded with the goal for status 0; otherwise the start, then the goal repeated,
//     len 2 (what roadmap_query writes).
//
// A query's result is a function of its own start and goal and of the call's arguments: not of the other queries, of
// how many there are, of the chunking, of `poll` or of a launch shape.
//
// Plain host C++ compiles this header too (no HIP runtime): tests/rrt_util.py drives the serial reference at its end
// (plan_reference) with g++, the motion verdicts given by a callback, and the device is compared with it bit for bit.
#pragma once

#include "roadmap_measure.hpp"

#ifndef OPTIK_HIP_RRT_MAX_NODES
#define OPTIK_HIP_RRT_MAX_ITERS 65536  // (include/optik_hip.h)
#define OPTIK_HIP_RRT_MAX_NODES 4096
#define OPTIK_HIP_RRT_MAX_POLL 65536
#endif

namespace optik {
namespace rrt {

constexpr int MAX_ITERS = OPTIK_HIP_RRT_MAX_ITERS, MIN_NODES = 2, MAX_NODES = OPTIK_HIP_RRT_MAX_NODES,
              MAX_POLL = OPTIK_HIP_RRT_MAX_POLL;
constexpr int FOUND = roadmap::FOUND, NO_ROUTE = roadmap::NO_ROUTE, TOO_LONG = roadmap::TOO_LONG,
              QUERY_NAN = roadmap::QUERY_NAN;
constexpr int RUNNING = -1;  // (a query that has not ended; never an output)

OPTIK_CM_HD inline bool finite(double v) { return v - v == 0.0; }

// Rule 0: ends_finite = no NaN or infinite joint in the start and the goal; the two flags of optik_hip_collision_batch;
// the verdict of the direct motion.  RUNNING: the iterations begin.
OPTIK_CM_HD inline int begin(bool ends_finite, bool start_free, bool goal_free, bool direct_free) {
    if (!ends_finite) return QUERY_NAN;
    if (!start_free || !goal_free) return NO_ROUTE;
    return direct_free ? FOUND : RUNNING;
}

// Rule 1: does (da, ia) come before (db, ib)?  ib < 0: no candidate yet.
OPTIK_CM_HD inline bool nearer(double da, int ia, double db, int ib) { return roadmap::ranks_before(da, ia, db, ib); }

// Rule 2: does a steer over the distance d make a candidate?
OPTIK_CM_HD inline bool steers(double d) { return d > 0.0 && d < roadmap::inf(); }
// Rule 2, one joint.
OPTIK_CM_HD inline double steer_joint(double p, double x, double d, double eta, double lo, double hi) {
    double c = x;
    if (!(d <= eta)) {
        const double s = eta / d;
        const double t = s * (x - p);
        c = p + t;
    }
    if (c < lo) c = lo;
    if (c > hi) c = hi;
    return c;
}

// Rule 4: does tree b extend after a connection that is not free?
OPTIK_CM_HD inline bool extends_back(double d_mc, double eta, int count_b, int M) { return d_mc > eta && count_b < M; }

// Rule 5.
OPTIK_CM_HD inline int found_status(long long W, int Lmax) { return W <= (long long)Lmax ? FOUND : TOO_LONG; }

// ---- the serial reference (the tests' g++ driver; the device is compared with it bit for bit) --------------------

struct Result {
    int status, len, iters_used, nodes[2], junction[2];
    double cost;
};

// One tree of the reference: conf [M][n], parent [M].
struct Tree {
    int n, M, count;
    double *conf;
    int32_t *parent;
    const double *node(int j) const { return conf + (size_t)j * n; }
    int nearest(const double *x, double *dist) const {
        int best = -1;
        double bd = roadmap::inf();
        for (int j = 0; j < count; ++j) {
            const double d = motion::motion_distance(n, node(j), 1, x, 1);
            if (nearer(d, j, bd, best)) { bd = d; best = j; }
        }
        *dist = bd;
        return best;
    }
    void append(const double *c, int p) {
        for (int i = 0; i < n; ++i) conf[(size_t)count * n + i] = c[i];
        parent[count++] = p;
    }
};

inline void steer(int n, const double *p, const double *x, double d, double eta, const double *lo, const double *hi,
                  double *c) {
    for (int i = 0; i < n; ++i) c[i] = steer_joint(p[i], x[i], d, eta, lo[i], hi[i]);
}

// Rules 3 and 4 for the iterations 0 .. I - 1 over two trees that hold their roots (tree 1 may hold several:
// rrt_goals_measure.hpp); motions_free as below.  Leaves the junction, iters_used and FOUND or NO_ROUTE in res.
template <class MotionsFree>
inline void grow_reference(Tree *tree, int n, const double *lo, const double *hi, const double *samples, int I,
                           double eta, int M, MotionsFree &&motions_free, Result &res) {
    double *seg = new double[6 * (size_t)n];
    double *c = seg, *e = seg + n;             // the candidates
    double *qa = seg + 2 * n, *qb = seg + 4 * n;  // two segments each
    for (int i = 0; i < I && res.status == RUNNING; ++i) {
        res.iters_used = i + 1;
        const int a = i & 1, b = 1 - a;
        const double *r = samples + (size_t)i * n;
        double d;
        const int p = tree[a].nearest(r, &d);
        if (!steers(d) || tree[a].count >= M) continue;
        steer(n, tree[a].node(p), r, d, eta, lo, hi, c);
        unsigned char ok[2] = {0, 0};
        for (int j = 0; j < n; ++j) {
            qa[j] = a == 0 ? tree[a].node(p)[j] : c[j];
            qb[j] = a == 0 ? c[j] : tree[a].node(p)[j];
        }
        motions_free(1, qa, qb, ok);
        if (!ok[0]) continue;
        double dm;
        const int m = tree[b].nearest(c, &dm);  // (tree b as it was: c goes to tree a)
        tree[a].append(c, p);
        const double *qm = tree[b].node(m);
        const bool back = extends_back(dm, eta, tree[b].count, M);
        if (back) steer(n, qm, c, dm, eta, lo, hi, e);
        for (int j = 0; j < n; ++j) {
            qa[j] = a == 0 ? c[j] : qm[j];
            qb[j] = a == 0 ? qm[j] : c[j];
            // (tree b's travel direction is tree a's reversed)
            qa[n + j] = b == 0 ? qm[j] : e[j];
            qb[n + j] = b == 0 ? e[j] : qm[j];
        }
        ok[0] = ok[1] = 0;
        motions_free(back ? 2 : 1, qa, qb, ok);
        if (ok[0]) {
            res.junction[a] = tree[a].count - 1;
            res.junction[b] = m;
            res.status = FOUND;
        } else if (back && ok[1]) {
            tree[b].append(e, m);
        }
    }
    delete[] seg;
    if (res.status == RUNNING) res.status = NO_ROUTE;
}

// Rule 5 for a query with a junction: order [2 M + 2] receives the waypoints, node v of tree 0 or M + v of tree 1, the
// start first and the root that tree 1's branch ends in last; conf [2][M][n] the trees'.  Sets the cost and the
// status; returns W.
inline long long route_reference(const Tree *tree, int n, int M, int Lmax, const double *conf, Result &res, int *order) {
    int d0 = 0;
    for (int v = res.junction[0]; v >= 0; v = tree[0].parent[v]) ++d0;
    int t = d0;
    for (int v = res.junction[0]; v >= 0; v = tree[0].parent[v]) order[--t] = v;
    long long W = d0;
    for (int v = res.junction[1]; v >= 0; v = tree[1].parent[v]) order[W++] = M + v;
    double cost = 0.0;
    for (long long t2 = 0; t2 + 1 < W; ++t2)
        cost = cost + motion::motion_distance(n, conf + (size_t)order[t2] * n, 1, conf + (size_t)order[t2 + 1] * n, 1);
    res.cost = cost;
    res.status = found_status(W, Lmax);
    return W;
}

// config_free(q [n]) -> bool; motions_free(count, qa [count][n], qb [count][n], free_out [count]): the motion check of
// qa -> qb, as given.  samples [I][n].  conf [2][M][n] and parent [2][M] receive the trees; path_out [Lmax][n].
template <class ConfigFree, class MotionsFree>
inline Result plan_reference(int n, const double *lo, const double *hi, const double *start, const double *goal,
                             const double *samples, int I, double eta, int M, int Lmax, ConfigFree &&config_free,
                             MotionsFree &&motions_free, double *conf, int32_t *parent, double *path_out) {
    Tree tree[2] = {{n, M, 0, conf, parent}, {n, M, 0, conf + (size_t)M * n, parent + M}};
    Result res{RUNNING, 2, 0, {0, 0}, {-1, -1}, roadmap::inf()};
    bool ends_finite = true;
    for (int i = 0; i < n; ++i) ends_finite = ends_finite && finite(start[i]) && finite(goal[i]);
    {
        const bool sf = ends_finite && config_free(start), gf = ends_finite && config_free(goal);
        unsigned char direct = 0;
        if (sf && gf) motions_free(1, start, goal, &direct);
        res.status = begin(ends_finite, sf, gf, direct != 0);
    }
    if (res.status == RUNNING) {
        tree[0].append(start, -1);
        tree[1].append(goal, -1);
        grow_reference(tree, n, lo, hi, samples, I, eta, M, motions_free, res);
    }
    res.nodes[0] = tree[0].count;
    res.nodes[1] = tree[1].count;
    // rules 5 and 7
    int *order = new int[2 * (size_t)M + 2];  // (tree, node) of every waypoint, start first
    long long W = 2;
    if (res.junction[0] >= 0) {
        W = route_reference(tree, n, M, Lmax, conf, res, order);
    } else if (res.status == FOUND) {
        res.cost = 0.0 + motion::motion_distance(n, start, 1, goal, 1);
        res.status = found_status(2, Lmax);
    } else if (res.status == QUERY_NAN) {
        res.cost = roadmap::nan_value();
    }
    res.len = res.status == FOUND && res.junction[0] >= 0 ? (int)W : 2;
    for (int t = 0; t < Lmax; ++t)
        for (int i = 0; i < n; ++i) {
            double v = goal[i];
            if (t == 0) v = start[i];
            else if (t < res.len - 1) v = conf[(size_t)order[t] * n + i];
            path_out[(size_t)t * n + i] = v;
        }
    delete[] order;
    return res;
}

}  // namespace rrt
}  // namespace optik
