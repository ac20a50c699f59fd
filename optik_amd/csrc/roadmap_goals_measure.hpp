// roadmap_goals_measure.hpp -- the rules of goal-set planning, one source for the host and the device
// (optik_hip_roadmap_query_goals, optik_hip.h; ik_roadmap_goals.hip).
//
// A goal-set query is a query of roadmap_measure.hpp with G goal slots, 1 <= G <= MAX_GOALS, in place of its one goal:
// one start with its start links, and per goal g its kg goal links gidx, gw [G][kg] (checked node -> goal) and its
// direct weight direct [G] (start -> goal g).  Only the goals g < gcount exist (gcount in 0 .. G; a count outside is
// clamped to that range): NOTHING of a goal g >= gcount is read -- not its joints, not its links, not its direct
// weight --, so the NaN rows that optik_hip_ik_solutions leaves past its count do not poison the query.  The plan is
// the cheapest route from the start to ANY counted goal, and `which` names the goal it ends in.  The exact operation
// order (the tests depend on it; -ffp-contract=off on both sides; nothing but roadmap_measure.hpp's relax -- one
// addition and one comparison -- and comparisons):
//
//  1. Distances.  d_u starts as the minimum of gw[g][s] over g < gcount and the slots s with gidx[g][s] == u, taken by
//     relax(., gw[g][s], 0.0) from +inf, g ascending then s ascending (goals_weight); +inf if no counted slot names
//     u.  Step 4 of roadmap_measure.hpp follows unchanged: every node pulls over its own out-list (pull) until a
//     sweep changes nothing.  relax takes a minimum and f64 addition is monotone, so d_u = min over the counted goals
//     of that goal's single-goal d_u, bit for bit.
//  2. The first hop (first_hop_goals).  best = +inf, which = -1.  For g ascending over the counted goals, direct[g] <
//     best strictly replaces best and sets which = g.  Then start slot s ascending replaces best only if sw_s +
//     d[sidx_s] < best strictly, and the first hop is then "by the graph".  Ties go to the direct edge of the lowest
//     goal, then to the lowest start slot.  best is the cost.
//  3. The successor of v (goal_of, then next_node).  Goal g for the LOWEST g < gcount whose own goal-link weight of v
//     (own_goal_weight: roadmap_measure.hpp's goal_weight restricted to goal g's kg slots) equals d_v; otherwise the
//     lowest node INDEX u of v's out-list with w(v, u) + d_u == d_v exactly.  At the fixed point one of the two holds
//     for a finite d_v.
//  4. The walk, the Lmax cap and the statuses are step 7 of roadmap_measure.hpp: start, the first hop's node,
//     successors until a goal, that goal; len = 2 + nodes; the walk stops as soon as len would exceed Lmax (TOO_LONG,
//     the true cost).  QUERY_NAN (cost NaN) if the start, a goal g < gcount, one of its direct or link weights, or a
//     start link weight is NaN -- looked at first, as there.  Else NO_ROUTE if the cost is +inf, which gcount == 0
//     always gives (no distance and no direct weight is finite).
//  5. Outputs.  path, len, cost and status as roadmap_measure.hpp's plan_reference; which = the goal reached when
//     FOUND, -1 otherwise.  A FOUND path ends in goal `which` and is padded with it; any other path is the start, then
//     goal 0 repeated, or the start repeated if gcount == 0 (goal 0 does not exist then).  route and hop are those of
//     roadmap_lazy_measure.hpp's rule 3: the node of waypoint t and the slot of the graph hop that leaves it.
//     With G = 1 and gcount = 1 every output equals the single-goal query's, bit for bit: the rules collapse to
//     steps 4 to 7 there (best starts at +inf instead of at the direct weight, which changes no comparison's outcome
//     for weights >= 0 or +inf).
//
// Theorem.  Let P_g be the single-goal plan (roadmap_measure.hpp) to goal g over the same graph and links.
//   (a) The goal-set cost equals min over g < gcount of cost(P_g), bit for bit.  Every route ends in exactly one goal
//       and is summed from that goal backwards, so the set of route sums is the union of the goals' sets; d, and with
//       it the first-hop minimum, is the minimum over that union.  (A NaN anywhere in the counted part makes both
//       sides QUERY_NAN for the goal-set plan and at least one P_g.)
//   (b) NO_ROUTE holds iff every P_g, g < gcount, is NO_ROUTE (or gcount == 0): the minimum of costs is +inf iff all
//       are.
//   (c) If exactly one goal g* attains a finite minimum, then status and len equal P_g*'s, and where that status is
//       FOUND which == g* and the path equals P_g*'s bit for bit.  (A TOO_LONG plan has which = -1 and, by rule 5,
//       the start and then goal 0, where P_g*'s holds goal g*.)  Let d^g be goal g's single-goal distances.  If the direct edge
//       of g* is the minimum it is strictly below every other direct weight and every sw_s + d[sidx_s]: both plans
//       take it.  Otherwise the walk's nodes v all have d_v = d^{g*}_v, and d_v < d^g_v for g != g*: were d_v
//       attained by another goal as well, the route start -> .. -> v continued by that goal's route would cost the
//       minimum too (d^g_v = d_v gives d^g <= d at the node before, by the same addition, and so on back to the
//       start link), a tie.  So on the walk own_goal_weight(g, v) == d_v can hold for g* only, and w(v, u) + d_u ==
//       d_v holds for exactly the u with w(v, u) + d^{g*}_u == d^{g*}_v (d_u <= d^{g*}_u; a u whose d_u is another
//       goal's alone would make d_v that goal's value too): the successors, the first hop and the Lmax cut are
//       P_g*'s.
//   With a cost tie between goals only (a), rules 2 and 3 and the serial reference below hold.
//
// Plain host C++ compiles this header too (no HIP runtime): tests/roadmap_goals_util.py drives it with g++, and the
// serial reference at its end (plan_goals_reference) is what the tests compare the device with.
#pragma once

#include "roadmap_lazy_measure.hpp"  // (roadmap_measure.hpp, and hop_slot for the route's slots)

#ifndef OPTIK_HIP_ROADMAP_MAX_GOALS
#define OPTIK_HIP_ROADMAP_MAX_GOALS 16  // (include/optik_hip.h)
#endif

namespace optik {
namespace roadmap {

constexpr int MAX_GOALS = OPTIK_HIP_ROADMAP_MAX_GOALS;
constexpr int BY_GRAPH = -2;  // first_hop_goals' `which` when the first hop is a start link

// One goal-set query against one graph.  y holds the graph, the start links (slot s at s * y.qs), kg and Lmax; its
// own gidx, gw and direct are not read.  Goal g's link slot s is at g * gs + s * gq, its direct weight at g * ds.
struct GoalsQuery {
    Query y;
    int G, gcount;  // gcount already clamped to 0 .. G (clamp_count)
    const int32_t *gidx;
    const double *gw;
    long long gq, gs;
    const double *direct;
    long long ds;
};

OPTIK_CM_HD inline int clamp_count(int gcount, int G) { return gcount < 0 ? 0 : (gcount > G ? G : gcount); }

// Rule 3: goal g's own goal-link weight of node u.
OPTIK_CM_HD inline double own_goal_weight(const GoalsQuery &z, int g, int u) {
    double m = inf();
    for (int s = 0; s < z.y.kg; ++s)
        if (z.gidx[g * z.gs + s * z.gq] == u) m = relax(m, z.gw[g * z.gs + s * z.gq], 0.0);
    return m;
}

// Rule 1: where d_u starts.
OPTIK_CM_HD inline double goals_weight(const GoalsQuery &z, int u) {
    double m = inf();
    for (int g = 0; g < z.gcount; ++g)
        for (int s = 0; s < z.y.kg; ++s)
            if (z.gidx[g * z.gs + s * z.gq] == u) m = relax(m, z.gw[g * z.gs + s * z.gq], 0.0);
    return m;
}

// Rule 3: the lowest counted goal whose own goal-link weight of v equals d_v, -1 if none.
OPTIK_CM_HD inline int goal_of(const GoalsQuery &z, double d_v, int v) {
    for (int g = 0; g < z.gcount; ++g)
        if (own_goal_weight(z, g, v) == d_v) return g;
    return -1;
}

// Rule 3: the lowest node index u of v's out-list with w(v, u) + d_u == d_v, -2 if none (roadmap_measure.hpp's
// next_hop without its goal test).
OPTIK_CM_HD inline int next_node(const Query &y, const double *d, int v) {
    int best = -2;
    for (int s = 0; s < y.k; ++s) {
        const int u = y.nbr[(long long)s * y.N + v];
        if (node_ok(y, u) && y.w[(long long)s * y.N + v] + d[u] == d[v] && (best < 0 || u < best)) best = u;
    }
    return best;
}

// Rule 2: the start slot of the first hop, -1 for a direct edge; *cost = best; *which = the direct edge's goal, BY_GRAPH
// for a start slot, -1 if best stayed +inf.
OPTIK_CM_HD inline int first_hop_goals(const GoalsQuery &z, const double *d, double *cost, int *which) {
    double best = inf();
    int hop = -1, wh = -1;
    for (int g = 0; g < z.gcount; ++g) {
        const double c = z.direct[g * z.ds];
        if (c < best) { best = c; wh = g; }
    }
    for (int s = 0; s < z.y.ks; ++s) {
        const int u = z.y.sidx[s * z.y.qs];
        if (!node_ok(z.y, u)) continue;
        const double c = z.y.sw[s * z.y.qs] + d[u];
        if (c < best) { best = c; hop = s; wh = BY_GRAPH; }
    }
    *cost = best;
    *which = wh;
    return hop;
}

// Rule 4: is a number of the counted part NaN?  start_i = start[i * ss], goal g's joint i = goals[g * sg + i * si].
OPTIK_CM_HD inline bool goals_query_has_nan(const GoalsQuery &z, int n, const double *start, long long ss,
                                            const double *goals, long long si, long long sg) {
    bool bad = false;
    for (int i = 0; i < n; ++i) bad = bad || start[i * ss] != start[i * ss];
    for (int s = 0; s < z.y.ks; ++s) bad = bad || z.y.sw[s * z.y.qs] != z.y.sw[s * z.y.qs];
    for (int g = 0; g < z.gcount; ++g) {
        bad = bad || z.direct[g * z.ds] != z.direct[g * z.ds];
        for (int i = 0; i < n; ++i) bad = bad || goals[g * sg + i * si] != goals[g * sg + i * si];
        for (int s = 0; s < z.y.kg; ++s) bad = bad || z.gw[g * z.gs + s * z.gq] != z.gw[g * z.gs + s * z.gq];
    }
    return bad;
}

struct GoalsPlan {
    Plan p;
    int which;
};

// Rules 2 to 4 from the converged d: the nodes walked go to nodes[0 .. len - 3] (room for MAX_WAYPOINTS - 2).
// goal_at(v) is rule 3's goal test of node v -- goal_of(z, d[v], v), or a table of it (the device keeps one in LDS).
template <class GoalAt>
OPTIK_CM_HD inline GoalsPlan plan_goals(const GoalsQuery &z, const double *d, bool has_nan, int *nodes,
                                        GoalAt goal_at) {
    if (has_nan) return GoalsPlan{Plan{QUERY_NAN, 2, nan_value()}, -1};
    double cost;
    int which;
    const int hop = first_hop_goals(z, d, &cost, &which);
    if (!(cost < inf())) return GoalsPlan{Plan{NO_ROUTE, 2, inf()}, -1};
    int count = 0;
    if (hop >= 0) {
        int v = z.y.sidx[hop * z.y.qs];
        for (;;) {
            if (count + 3 > z.y.Lmax) return GoalsPlan{Plan{TOO_LONG, 2, cost}, -1};
            nodes[count++] = v;
            which = goal_at(v);
            if (which >= 0) break;
            v = next_node(z.y, d, v);
            // (not at a fixed point: cannot happen after convergence)
            if (v < 0) return GoalsPlan{Plan{NO_ROUTE, 2, inf()}, -1};
        }
    }
    return GoalsPlan{Plan{FOUND, 2 + count, cost}, which};
}

// Rule 5: waypoint t's joint i.  A FOUND plan ends in and is padded with goal `which`; any other is the start, then
// goal 0 repeated -- the start where no goal is counted.  goals as in goals_query_has_nan; node j's joint i =
// nodes[i * N + j].
OPTIK_CM_HD inline double waypoint_value(const GoalsQuery &z, const GoalsPlan &r, const int *walked, int t, int i,
                                         const double *nodes, const double *start, long long ss, const double *goals,
                                         long long si, long long sg) {
    if (t == 0 || z.gcount == 0) return start[i * ss];
    if (t < r.p.len - 1) return nodes[(long long)i * z.y.N + walked[t - 1]];
    return goals[(r.which >= 0 ? r.which : 0) * sg + i * si];
}

// ---- the serial reference (the tests' g++ driver; the device is compared with it bit for bit) ----------------------

// Rule 1 with Jacobi sweeps (roadmap_measure.hpp's distances_reference from goals_weight): d and tmp hold N doubles.
inline int goals_distances_reference(const GoalsQuery &z, double *d, double *tmp) {
    const Query &y = z.y;
    for (int u = 0; u < y.N; ++u) d[u] = goals_weight(z, u);
    int sweeps = 0;
    for (; sweeps < y.N; ++sweeps) {
        bool changed = false;
        for (int v = 0; v < y.N; ++v) {
            tmp[v] = pull(y, d, v);
            changed = changed || tmp[v] < d[v];
        }
        if (!changed) break;
        for (int v = 0; v < y.N; ++v) d[v] = tmp[v];
    }
    return sweeps;
}

// The whole query: start [n], goals [G][n]; path_out [Lmax][n], route_out and hop_out [Lmax] (rule 5; may be null),
// d_out [N] the distances to the goal set (may be null).
inline GoalsPlan plan_goals_reference(const GoalsQuery &z, int n, const double *nodes, const double *start,
                                      const double *goals, double *path_out, int32_t *route_out, int32_t *hop_out,
                                      double *d_out) {
    const Query &y = z.y;
    double *d = new double[2 * (size_t)y.N];
    goals_distances_reference(z, d, d + y.N);
    int walked[MAX_WAYPOINTS];
    const GoalsPlan r = plan_goals(z, d, goals_query_has_nan(z, n, start, 1, goals, 1, n), walked,
                                   [&](int v) { return goal_of(z, d[v], v); });
    for (int t = 0; t < y.Lmax; ++t) {
        for (int i = 0; i < n; ++i)
            path_out[t * n + i] = waypoint_value(z, r, walked, t, i, nodes, start, 1, goals, 1, n);
        const bool node = t >= 1 && t < r.p.len - 1;
        if (route_out) route_out[t] = node ? walked[t - 1] : -1;
        if (hop_out) hop_out[t] = node && t < r.p.len - 2 ? hop_slot(y, d, walked[t - 1], walked[t]) : -1;
    }
    if (d_out)
        for (int u = 0; u < y.N; ++u) d_out[u] = d[u];
    delete[] d;
    return r;
}

}  // namespace roadmap
}  // namespace optik
