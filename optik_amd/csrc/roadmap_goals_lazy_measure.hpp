// roadmap_goals_lazy_measure.hpp -- the rules of goal-set planning on lazy roadmaps, one source for the host and the
// device (optik_hip_roadmap_lazy_plan_goals / _from_flags, optik_hip.h; ik_roadmap_goals_lazy.hip; DESIGN.md section
// 5.34).  The loop of roadmap_lazy_measure.hpp with the pass of roadmap_goals_measure.hpp in the place of the
// single-goal pass, and a rule that says which queries a later pass may leave out.  The exact rules (the tests depend
// on them; no arithmetic beyond roadmap_measure.hpp's: one addition and comparisons):
//
//  1. The state is the lazy roadmap's, unchanged: nodes [n][N], nbr, w0, verdict, w [k][N] (roadmap_lazy_measure.hpp,
//     rules 1 and 2).  Reset is lazy_reset_reference / optik_hip_roadmap_lazy_reset as it is.
//  2. A pass is rules 1 to 5 of roadmap_goals_measure.hpp for every query on w, unchanged.
//  3. Hop slots are rule 3 of roadmap_lazy_measure.hpp: the hop v -> u of a FOUND route uses the LOWEST slot s with
//     nbr[s][v] == u and w[s][v] + d[u] == d[v] exactly -- the `hop` that rule 5 of roadmap_goals_measure.hpp writes.
//     The start links, the G x kg goal links and the G direct motions are no slots: they are checked eagerly with the
//     call.
//  4. C, `rounds`, mark, rounds_used and checked are rule 4 of roadmap_lazy_measure.hpp: C is the set of UNKNOWN hop
//     slots over all FOUND routes of the pass, each slot once; the loop ends if C is empty or `rounds` checks have
//     been made; otherwise every slot of C is checked and marked, rounds_used += 1, checked += |C|, and the next pass
//     follows.
//  5. After the last pass a FOUND query whose route still holds an UNKNOWN slot becomes UNSETTLED (status 4): len 2,
//     the path is the start, then goal 0 repeated (a FOUND query has a counted goal), which = -1, and the cost is kept
//     -- the cost of a route through the partly unchecked graph, a lower bound.  TOO_LONG routes are not walked, so
//     none of their edges is checked; their cost is a lower bound too.
//  6. gcount == 0 is NO_ROUTE with the start repeated, as in roadmap_goals_measure.hpp.
//
// THE SPECIFICATION RECOMPUTES EVERY QUERY IN EVERY PASS (lazy_plan_goals_reference with freeze = false).
//
// Theorem (roadmap_lazy_measure.hpp's, carried over).  The eager graph -- every slot checked -- is a subgraph of every
// lazy graph: blocked marks come only from the reset and from failed checks, which the eager build blocks as well.  A
// FOUND route without an UNKNOWN slot lies in the eager graph; the lazy distances are lower bounds of the eager ones
// and are attained along that route, so its cost, its distances and its ties are the eager ones.  For final status 0,
// 1 and 3 the status, len, cost, path and which therefore equal those of plan_goals_reference
// (optik_hip_roadmap_query_goals) over the eagerly checked graph, bit for bit; for status 2 and 4 the cost is a lower
// bound.
//
// The freezing rule (what the device may do; lazy_plan_goals_reference with freeze = true).  After a pass a query is
// FROZEN if its status is NO_ROUTE, if its status is QUERY_NAN, or if its status is FOUND and no slot of its route is
// UNKNOWN or CLAIMED (frozen_after_pass).  A frozen query's outputs equal what every later pass of the specification
// would write, bit for bit, so later passes may leave it out.  Proof.  Write w for the weights of the pass that froze
// the query and w' for those of any later pass; d, d' for the converged distances.  The loop only replaces weights by
// +inf, so w' >= w slot by slot; relax takes a minimum and f64 addition is monotone, so d' >= d node by node.
//   QUERY_NAN reads no graph: the counted numbers of the query decide it, and its outputs are a function of them.
//   NO_ROUTE: every counted direct weight and every sw_s + d[sidx_s] is +inf.  d' >= d keeps each sum at +inf, the
//   direct weights do not change, and the outputs of NO_ROUTE are a function of the query alone.
//   FOUND by a direct edge has no slot.  best = direct[g] was taken before the start slots were looked at, and no
//   sw_s + d[sidx_s] was strictly below it; the sums only grow, so none is below it later.
//   FOUND by the graph, route r_0 .. r_{c-1}, goal `which`, every hop slot FREE.  A FREE verdict is never changed, so
//   w' = w on the route's slots; the links are not part of the graph.  (i) d' = d on the route: d_{r_{c-1}} equals
//   goal `which`'s own link weight of r_{c-1}, and w[s][r_i] + d[r_{i+1}] == d[r_i] exactly on each hop slot s, so
//   relaxing along the same slots from the same goal link gives d'_{r_i} <= d_{r_i}; with d' >= d they are equal --
//   along the route d can neither fall nor rise.  (ii) The first hop: the pass took start slot s* as the first slot
//   that attains the minimum, strictly below every counted direct weight and every slot before it.  Its sum is
//   unchanged by (i); every other sum is >= what it was, so a slot before s* stays strictly above and a slot behind
//   it stays at or above; the direct weights do not change.  (iii) The goal test of a route node compares the goals'
//   own link weights with d_v: both unchanged.  (iv) The successor of r_i is the lowest node index u of its out-list
//   with w(r_i, u) + d_u == d_{r_i}.  At the fixed point d_v <= w(v, u) + d_u for every slot, so a u below r_{i+1}
//   that was not equal was strictly above, and w' + d'_u >= w + d_u keeps it there; r_{i+1} keeps its equality by
//   (i).  (v) The hop slot is the lowest slot of r_i that names r_{i+1} with equality: a lower slot naming it was
//   strictly above and stays so.  Hence the walk, len (the same Lmax), the cost, the path, which, route and hop are
//   those of the freezing pass, and the route has no UNKNOWN slot in any later pass: it adds nothing to a later C.
// TOO_LONG and FOUND with an UNKNOWN or CLAIMED slot stay LIVE: a TOO_LONG route is not walked, and what the
// specification finally says of it depends on the final graph (it may become FOUND by a longer-in-cost, shorter-in-hops
// route once another query's checks block an edge).  C holds slots of live FOUND routes only, so C, rounds_used and
// checked are the specification's too, and a frozen query is never UNSETTLED.
//
// Plain host C++ compiles this header too (no HIP runtime): tests/roadmap_goals_lazy_util.py drives it with g++, and
// the serial reference at its end is what the tests compare the device with.
#pragma once

#include "roadmap_goals_measure.hpp"  // (roadmap_lazy_measure.hpp and roadmap_measure.hpp with it)

namespace optik {
namespace roadmap {

// The freezing rule: `unknown` = the query's route holds an UNKNOWN or CLAIMED slot (looked at only for FOUND).
OPTIK_CM_HD inline bool frozen_after_pass(int status, bool unknown) {
    return status == NO_ROUTE || status == QUERY_NAN || (status == FOUND && !unknown);
}

// ---- the serial reference (the tests' g++ driver; the device is compared with it bit for bit) ----------------------

// The loop of rules 2 to 6 over Q queries: w and verdict [k][N] are the state (read and updated), edge_free [k][N]
// stands for the motion check.  The queries: start [Q][n], goals [Q][G][n], gcount [Q]; the links and the direct
// weights in the layouts of the device call ([ks][Q], [G][kg][Q], [G][Q]).  path_out [Q][Lmax][n]; status, len, cost,
// which [Q]; frozen_after [Q] (may be null): the number of passes after which the query was first frozen, 0 if it
// stayed live to the end.  freeze = false recomputes every query in every pass (the specification); freeze = true
// leaves the frozen ones out of every pass after the one that froze them.
inline LazyCounts lazy_plan_goals_reference(int n, int N, int k, const double *nodes, const int32_t *nbr, double *w,
                                            int32_t *verdict, const uint8_t *edge_free, int Q, int G,
                                            const double *start, const double *goals, const int32_t *gcount,
                                            const int32_t *sidx, const double *sw, int ks, const int32_t *gidx,
                                            const double *gw, int kg, const double *direct, int Lmax, int rounds,
                                            bool freeze, double *path_out, int32_t *status, int32_t *len, double *cost,
                                            int32_t *which, int32_t *frozen_after) {
    const size_t uQ = Q > 0 ? (size_t)Q : 1;
    long long *claimed = new long long[(size_t)k * N];
    bool *unknown = new bool[uQ], *frozen = new bool[uQ];
    int32_t *first_frozen = new int32_t[uQ];
    int32_t route[MAX_WAYPOINTS], hop[MAX_WAYPOINTS];
    for (int j = 0; j < Q; ++j) { unknown[j] = frozen[j] = false; first_frozen[j] = 0; }
    LazyCounts counts{0, 0};
    for (int pass = 1;; ++pass) {
        long long count = 0;
        for (int j = 0; j < Q; ++j) {
            if (freeze && frozen[j]) continue;
            GoalsQuery z;
            z.y.N = N; z.y.k = k; z.y.nbr = nbr; z.y.w = w;
            z.y.ks = ks; z.y.kg = kg;
            z.y.sidx = sidx + j; z.y.sw = sw + j; z.y.gidx = nullptr; z.y.gw = nullptr;
            z.y.qs = Q;
            z.y.direct = 0.0;
            z.y.Lmax = Lmax;
            z.G = G; z.gcount = clamp_count(gcount[j], G);
            z.gidx = gidx + j; z.gw = gw + j; z.gq = Q; z.gs = (long long)kg * Q;
            z.direct = direct + j; z.ds = Q;
            const GoalsPlan r = plan_goals_reference(z, n, nodes, start + (size_t)j * n, goals + (size_t)j * G * n,
                                                     path_out + (size_t)j * Lmax * n, route, hop, nullptr);
            status[j] = r.p.status; len[j] = r.p.len; cost[j] = r.p.cost; which[j] = r.which;
            unknown[j] = false;
            // (rule 3: waypoint t, 1 <= t < len - 2, leaves by a graph hop; only a FOUND plan has any)
            for (int t = 1; t < Lmax - 1; ++t) {
                if (route[t] < 0) break;
                if (hop[t] < 0) continue;
                const long long e = (long long)hop[t] * N + route[t];
                if (verdict[e] == UNKNOWN) { verdict[e] = CLAIMED; claimed[count++] = e; }
                unknown[j] = unknown[j] || verdict[e] == CLAIMED;
            }
            const bool now = frozen_after_pass(r.p.status, unknown[j]);
            if (now && first_frozen[j] == 0) first_frozen[j] = pass;
            frozen[j] = frozen[j] || now;
        }
        const bool last = count == 0 || counts.rounds_used >= rounds;
        for (long long b = 0; b < count; ++b) {
            const long long e = claimed[b];
            verdict[e] = last ? UNKNOWN : mark(edge_free[e] != 0);
            if (verdict[e] == BLOCKED) w[e] = inf();
        }
        if (last) break;
        counts.rounds_used += 1;
        counts.checked += count;
    }
    for (int j = 0; j < Q; ++j) {
        if (frozen_after) frozen_after[j] = first_frozen[j];
        if (!(status[j] == FOUND && unknown[j])) continue;
        status[j] = UNSETTLED; len[j] = 2; which[j] = -1;
        for (int t = 1; t < Lmax; ++t)
            for (int i = 0; i < n; ++i)
                path_out[((size_t)j * Lmax + t) * n + i] = goals[(size_t)j * G * n + i];
    }
    delete[] claimed;
    delete[] unknown;
    delete[] frozen;
    delete[] first_frozen;
    return counts;
}

}  // namespace roadmap
}  // namespace optik
