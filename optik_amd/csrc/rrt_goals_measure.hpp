// rrt_goals_measure.hpp -- the rules of the bidirectional tree planner with a goal set, one source for the host and
// the device (optik_hip_rrt_plan_goals, optik_hip.h; ik_rrt.hip).
//
// rrt_measure.hpp's planner with G goal slots per query, 1 <= G <= 16, in place of the one goal -- the IK solutions of
// a pose, for one: goals [G][n] and a count, clamped to 0 .. G (clamp_count).  Only the goals g < count exist; NOTHING
// of the others influences any output, so the NaN rows optik_hip_ik_solutions leaves past its count are harmless.
// Tree 1 has several roots, one per counted goal that is free; the query ends at the first junction with any of them.
// Past rule 0 the answer is the goal joined FIRST, not the cheapest one.  The exact operation order (the tests depend
// on it; -ffp-contract=off on both sides, only the correctly rounded - * / +, fabs and comparisons):
//
//  0. Before iteration 0, in this order (begin_goals):
//     a NaN or infinite joint in the start or in any counted goal: status 3, cost NaN;
//     count == 0: status 1;
//     a start that is not free (optik_hip_collision_batch's flag): status 1;
//     the counted goals that are free become the roots of tree 1 in ascending g: nodes 0 .. R - 1, parent -1 each;
//     R == 0: status 1;
//     among the R roots whose direct motion start -> goal is free, the one with the smallest
//     motion_distance(start, goal), a tie going to the lower g (direct_better, scanned in ascending g): status 0,
//     len 2, which = that g, cost = 0.0 + that distance.
//     iters_used is 0 and the trees are empty (nodes 0) in all of these cases.
//  1. - 4. rrt_measure.hpp's, unchanged: nearest, steer, extend, connect and the back-extension (grow_reference; on
//     the device rrt_step_kernel itself).  Tree 1 starts with R nodes instead of one.  A tree holds at most M nodes and
//     the roots count towards M (M >= G is the caller's to give): a tree 1 that is full of roots never grows.
//  5. A found path: tree 0 from its root to its junction node, then tree 1 from its junction node up the parent links
//     to a root (route_reference); which = the goal slot g of that root; the cost is the forward sum from the start.
//     W <= Lmax: status 0, len W; W > Lmax: status 2 with the same cost and which = -1.
//  6. After I iterations without a junction: status 1, cost +inf, iters_used = I.
//  7. The path [Lmax][n]: for status 0 the waypoints padded with goal `which`; otherwise the start, then goal 0
//     repeated (the start repeated for count == 0), len 2, which = -1 (what roadmap_query_goals writes).
//
// With G = 1 and count = 1 every output equals rrt_measure.hpp's plan_reference (optik_hip_rrt_plan on the device) bit
// for bit -- path, len, cost, status, iters_used, nodes --, and which is 0 where the status is 0 and -1 elsewhere.
//
// A query's result is a function of its own start and goal set and of the call's arguments: not of the other queries,
// of how many there are, of the chunking, of `poll` or of a launch shape.
//
// Plain host C++ compiles this header too: tests/rrt_goals_util.py drives the serial reference at its end
// (plan_goals_reference) with g++, and the device is compared with it bit for bit.
#pragma once

#include "rrt_measure.hpp"

#ifndef OPTIK_HIP_RRT_MAX_GOALS
#define OPTIK_HIP_RRT_MAX_GOALS 16  // (include/optik_hip.h; OPTIK_HIP_ROADMAP_MAX_GOALS's value)
#endif

namespace optik {
namespace rrt {

constexpr int MAX_GOALS = OPTIK_HIP_RRT_MAX_GOALS;

OPTIK_CM_HD inline int clamp_count(int count, int G) { return count < 0 ? 0 : (count > G ? G : count); }

// the smallest tree size a call with G goal slots may ask for: every counted goal may be a root
OPTIK_CM_HD inline int min_nodes(int G) { return G > MIN_NODES ? G : MIN_NODES; }

// Rule 0's choice among the direct motions that are free, scanned in ascending g: does the distance d replace the best
// so far (bd of goal bg; bg < 0: none yet)?  Strict, so a tie stays with the lower g.
OPTIK_CM_HD inline bool direct_better(double d, double bd, int bg) { return bg < 0 || d < bd; }

// Rule 0: ends_finite = no NaN or infinite joint in the start and the counted goals; count clamped; roots = R; direct =
// the goal of the chosen free direct motion or -1.  RUNNING: the iterations begin.
OPTIK_CM_HD inline int begin_goals(bool ends_finite, int count, bool start_free, int roots, int direct) {
    if (!ends_finite) return QUERY_NAN;
    if (count == 0 || !start_free || roots == 0) return NO_ROUTE;
    return direct >= 0 ? FOUND : RUNNING;
}

// ---- the serial reference (the tests' g++ driver; the device is compared with it bit for bit) --------------------

struct GoalsResult {
    Result r;
    int which, roots;
};

// plan_reference with goals [G][n] and their count; config_free and motions_free as there -- neither is ever called
// on a goal g >= count.  M >= min_nodes(G).  conf [2][M][n] and parent [2][M] receive the trees, root_goal [G] the
// goal slot of every root of tree 1 (-1 past the roots); path_out [Lmax][n].
template <class ConfigFree, class MotionsFree>
inline GoalsResult plan_goals_reference(int n, const double *lo, const double *hi, const double *start,
                                        const double *goals, int G, int count, const double *samples, int I, double eta,
                                        int M, int Lmax, ConfigFree &&config_free, MotionsFree &&motions_free,
                                        double *conf, int32_t *parent, int32_t *root_goal, double *path_out) {
    Tree tree[2] = {{n, M, 0, conf, parent}, {n, M, 0, conf + (size_t)M * n, parent + M}};
    GoalsResult out{{RUNNING, 2, 0, {0, 0}, {-1, -1}, roadmap::inf()}, -1, 0};
    Result &res = out.r;
    const int gc = clamp_count(count, G);
    for (int g = 0; g < G; ++g) root_goal[g] = -1;
    bool ends_finite = true;
    for (int i = 0; i < n; ++i) ends_finite = ends_finite && finite(start[i]);
    for (int g = 0; g < gc; ++g)
        for (int i = 0; i < n; ++i) ends_finite = ends_finite && finite(goals[(size_t)g * n + i]);
    int R = 0, direct = -1;
    const bool start_free = ends_finite && gc > 0 && config_free(start);
    if (start_free) {
        for (int g = 0; g < gc; ++g)
            if (config_free(goals + (size_t)g * n)) root_goal[R++] = g;
        double bd = roadmap::inf();
        for (int r = 0; r < R; ++r) {
            const double *goal = goals + (size_t)root_goal[r] * n;
            unsigned char ok = 0;
            motions_free(1, start, goal, &ok);
            if (!ok) continue;
            const double d = motion::motion_distance(n, start, 1, goal, 1);
            if (direct_better(d, bd, direct)) { bd = d; direct = root_goal[r]; }
        }
    }
    out.roots = R;
    res.status = begin_goals(ends_finite, gc, start_free, R, direct);
    if (res.status == RUNNING) {
        tree[0].append(start, -1);
        for (int r = 0; r < R; ++r) tree[1].append(goals + (size_t)root_goal[r] * n, -1);
        grow_reference(tree, n, lo, hi, samples, I, eta, M, motions_free, res);
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
