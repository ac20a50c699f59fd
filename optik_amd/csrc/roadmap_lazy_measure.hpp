// roadmap_lazy_measure.hpp -- the rules of lazy roadmaps, one source for the host and the device
// (optik_hip_roadmap_query_route / _lazy_reset / _lazy_plan, optik_hip.h; ik_roadmap_lazy.hip).
//
// A lazy roadmap is the graph of roadmap_measure.hpp with its edges presumed free: nodes [n][N], nbr [k][N], the
// unchecked weights w0 [k][N], one int32 verdict per edge slot (UNKNOWN, FREE, BLOCKED) and the working weights
// w [k][N] = w0 with +inf at the BLOCKED slots.  An edge is checked by the motion check, in the direction v -> nbr,
// only when a shortest route uses it; a verdict holds until the world changes.  The exact rules (the tests depend on
// them; no arithmetic beyond roadmap_measure.hpp's: one addition and comparisons):
//
//  1. The unchecked weight of slot (s, v) is roadmap_measure.hpp's step 1 for v -> nbr[s][v], and +inf where the slot
//     is empty (an index outside 0 .. N - 1) or that weight is NaN or infinite (unchecked_weight).
//  2. Reset (reset_verdict): a slot is BLOCKED if it is empty, if w0 is +inf, if v is not free or if nbr[s][v] is not
//     free -- node_free is the classification of optik_hip_collision_batch --; every other slot is UNKNOWN.  w = w0,
//     +inf where BLOCKED.  The motion check copies its first and last sample from the ends of the motion
//     (motion_measure.hpp step 3), so it blocks exactly these edges too, and no other edge is prejudged.
//  3. A pass is steps 4 to 7 of roadmap_measure.hpp for every query on w, unchanged.  A FOUND route start, r_0 ..
//     r_{c-1}, goal has the graph hops r_i -> r_{i+1}; the hop v -> u uses the LOWEST slot s with nbr[s][v] == u and
//     w[s][v] + d[u] == d[v] exactly (hop_slot).  At the fixed point one exists.  The links start -> r_0 and r_{c-1} ->
//     goal are no slots: they are checked eagerly with the query.
//  4. C is the set of UNKNOWN hop slots over all FOUND routes of the pass, each slot once.  If C is empty, or if
//     `rounds` checks have been made, the loop ends.  Otherwise every slot of C is checked: a free motion makes it
//     FREE, anything else BLOCKED with w = +inf (mark); rounds_used += 1, checked += |C|; the next pass follows.
//  5. After the last pass a FOUND query whose route still holds an UNKNOWN slot becomes UNSETTLED (status 4): len 2,
//     the start, then the goal repeated, the cost kept -- the cost of a route through the partly unchecked graph, a
//     lower bound.  TOO_LONG routes are not walked, so none of their edges is checked; their cost is a lower bound too.
//
// Nothing above depends on the order in which slots are claimed or listed: C is a set, and a verdict is a function of
// the slot.  Blocked marks come only from 2 and from failed checks, which the eager build (optik_hip_roadmap_edges on
// every slot) blocks as well: the eager graph is a subgraph of every lazy graph.  A settled FOUND route lies in the
// eager graph, so its cost, its distances and its ties are the eager ones (DESIGN.md section 5.24 has the argument).
//
// Plain host C++ compiles this header too; the serial reference of the whole loop at its end (lazy_reset_reference,
// lazy_plan_reference) is what the tests compare the device with.
#pragma once

#include "roadmap_measure.hpp"

#ifndef OPTIK_HIP_ROADMAP_LAZY_MAX_ROUNDS
#define OPTIK_HIP_ROADMAP_LAZY_MAX_ROUNDS 4096  // (include/optik_hip.h)
#endif

namespace optik {
namespace roadmap {

constexpr int UNKNOWN = 0, FREE = 1, BLOCKED = 2;
constexpr int CLAIMED = 3;    // within one round only: an UNKNOWN slot that the round's check has taken
constexpr int UNSETTLED = 4;  // the status beside FOUND .. QUERY_NAN
constexpr int MAX_ROUNDS = OPTIK_HIP_ROADMAP_LAZY_MAX_ROUNDS;

// Rule 1: `weight` = edge_weight(v -> u).
OPTIK_CM_HD inline double unchecked_weight(double weight, int u, int N) {
    return (u >= 0 && u < N && weight < inf()) ? weight : inf();
}

// Rule 2.
OPTIK_CM_HD inline int reset_verdict(int u, int N, double w0, bool v_free, bool u_free) {
    return (u >= 0 && u < N && w0 < inf() && v_free && u_free) ? UNKNOWN : BLOCKED;
}

// Rule 3: the slot of the hop v -> u, -1 if none (not at a fixed point).
OPTIK_CM_HD inline int hop_slot(const Query &y, const double *d, int v, int u) {
    for (int s = 0; s < y.k; ++s)
        if (y.nbr[(long long)s * y.N + v] == u && y.w[(long long)s * y.N + v] + d[u] == d[v]) return s;
    return -1;
}

// Rule 4: a checked slot.
OPTIK_CM_HD inline int mark(bool motion_free) { return motion_free ? FREE : BLOCKED; }

// ---- the serial reference (the tests' g++ driver; the device is compared with it bit for bit) ----------------------

inline void lazy_reset_reference(int N, int k, const int32_t *nbr, const double *w0, const uint8_t *node_free,
                                 int32_t *verdict, double *w) {
    for (int s = 0; s < k; ++s)
        for (int v = 0; v < N; ++v) {
            const long long e = (long long)s * N + v;
            const int u = nbr[e];
            const bool u_free = u >= 0 && u < N && node_free[u] != 0;
            verdict[e] = reset_verdict(u, N, w0[e], node_free[v] != 0, u_free);
            w[e] = verdict[e] == BLOCKED ? inf() : w0[e];
        }
}

struct LazyCounts {
    int rounds_used;
    long long checked;
};

// The loop of rules 3 to 5 over Q queries: w and verdict [k][N] are the state (read and updated), edge_free [k][N]
// stands for the motion check.  The queries: start, goal [Q][n]; the links and the direct weights in the layouts of
// the device call ([ks][Q], [kg][Q], [Q]).  path_out [Q][Lmax][n], status, len, cost [Q].
inline LazyCounts lazy_plan_reference(int n, int N, int k, const double *nodes, const int32_t *nbr, double *w,
                                      int32_t *verdict, const uint8_t *edge_free, int Q, const double *start,
                                      const double *goal, const int32_t *sidx, const double *sw, int ks,
                                      const int32_t *gidx, const double *gw, int kg, const double *direct, int Lmax,
                                      int rounds, double *path_out, int32_t *status, int32_t *len, double *cost) {
    double *d = new double[2 * (size_t)N];
    long long *claimed = new long long[(size_t)k * N];
    bool *unknown = new bool[Q > 0 ? Q : 1];
    LazyCounts counts{0, 0};
    for (;;) {
        long long count = 0;
        for (int j = 0; j < Q; ++j) {
            Query y;
            y.N = N; y.k = k; y.nbr = nbr; y.w = w;
            y.ks = ks; y.kg = kg;
            y.sidx = sidx + j; y.sw = sw + j; y.gidx = gidx + j; y.gw = gw + j;
            y.qs = Q;
            y.direct = direct[j];
            y.Lmax = Lmax;
            const double *st = start + (size_t)j * n, *gl = goal + (size_t)j * n;
            distances_reference(y, d, d + N);
            int walked[MAX_WAYPOINTS];
            const Plan p = plan(y, d, query_has_nan(y, n, st, 1, gl, 1), walked);
            status[j] = p.status; len[j] = p.len; cost[j] = p.cost;
            for (int t = 0; t < Lmax; ++t)
                for (int i = 0; i < n; ++i) {
                    double x = gl[i];
                    if (t == 0) x = st[i];
                    else if (t < p.len - 1) x = nodes[(long long)i * N + walked[t - 1]];
                    path_out[((size_t)j * Lmax + t) * n + i] = x;
                }
            unknown[j] = false;
            if (p.status != FOUND) continue;
            for (int t = 0; t + 1 < p.len - 2; ++t) {
                const int s = hop_slot(y, d, walked[t], walked[t + 1]);
                if (s < 0) continue;
                const long long e = (long long)s * N + walked[t];
                if (verdict[e] == UNKNOWN) { verdict[e] = CLAIMED; claimed[count++] = e; }
                unknown[j] = unknown[j] || verdict[e] == CLAIMED;
            }
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
        if (!unknown[j]) continue;
        status[j] = UNSETTLED; len[j] = 2;
        for (int t = 1; t < Lmax; ++t)
            for (int i = 0; i < n; ++i) path_out[((size_t)j * Lmax + t) * n + i] = goal[(size_t)j * n + i];
    }
    delete[] d;
    delete[] claimed;
    delete[] unknown;
    return counts;
}

}  // namespace roadmap
}  // namespace optik
