// roadmap_measure.hpp -- the arithmetic of roadmap planning, one source for the host and the device
// (optik_hip_roadmap_knn / _edges / _query, optik_hip.h; ik_roadmap.hip).
//
// A roadmap is a directed graph over N joint-space nodes: node v has k out-edge slots nbr[s][v], w[s][v] (slot-major,
// [k][N]), each edge checked by the motion check (motion_measure.hpp) in the direction v -> nbr.  The metric is
// L-infinity in radians.  The exact operation order (the tests depend on it; -ffp-contract=off on both sides, only the
// correctly rounded - and +, fabs and comparisons -- no sqrt, no division):
//
//  1. The weight of an edge a -> b is motion_measure.hpp's step 1, unchanged: d = max_i fabs(b_i - a_i), i ascending
//     from d = 0, a NaN term taken and then kept (edge_weight).  It is the distance the motion check sampled.  An edge
//     whose motion is not free, or is not sampled (a NaN or infinite d among the reasons), or whose slot is empty
//     (index -1) has weight +inf (checked_weight).
//  2. Neighbours are ranked by the total order on (distance, index): a number before a NaN, then the smaller distance,
//     then the smaller index; -0 and +0 are equal distances.  An empty slot (index < 0) ranks after everything
//     (ranks_before).  The k best of a query are the first k of that order, so they do not depend on the order in
//     which candidates are visited (Best::insert: a fixed network over K_MAX slots, no dynamic indexing).
//  3. One relaxation is c = w + d_u, then d_v = c < d_v ? c : d_v (relax): a NaN c never wins, so a NaN weight is no
//     edge.  Slots with an index outside 0 .. N - 1 are skipped.  Weights are >= 0.
//  4. The distance to the goal: d_u starts as the goal-link weight of u (the minimum, by relax from +inf, over the
//     goal slots that name u; +inf if none), then every node pulls over its own out-list, d_v = relax(d_v, w(v, u),
//     d_u), until a sweep changes nothing, at most N sweeps.  f64 addition is monotone, so every fair sweep order
//     (Jacobi here and on the device) ends at the same values: min over routes of the route's weights added from the
//     goal backwards, ((w_last + 0...) ...): Dijkstra's values.
//  5. The successor of v (next_hop): the goal itself if v's goal-link weight == d_v; otherwise the lowest node INDEX u
//     of its out-list with w(v, u) + d_u == d_v exactly.  At the fixed point one of the two holds for a finite d_v.
//  6. The first hop (first_hop): best = the direct weight start -> goal; start slot s ascending replaces it only if
//     sw_s + d[sidx_s] < best strictly: ties go to the direct edge, then to the lowest slot.  best is the cost.
//  7. The walk (plan): start, the first hop's node, successors until the goal, goal.  It needs len = 2 + nodes
//     waypoints; it stops as soon as len would exceed Lmax (status 2), whatever the successors say -- that also ends a
//     zero-weight cycle between duplicate nodes.  Status: 3 if the start, the goal, the direct weight or a link weight
//     of the query is NaN (cost NaN), else 1 if the cost is +inf, else 2 or 0.
//
// Plain host C++ compiles this header too (no HIP runtime): tests/roadmap_util.py drives it with g++, and the serial
// reference of the whole of 2 to 7 at its end (knn_reference, plan_reference) is what the tests compare the device with.
#pragma once

#include "motion_measure.hpp"

#ifndef OPTIK_HIP_ROADMAP_MAX_NODES
#define OPTIK_HIP_ROADMAP_MAX_NODES 8192  // (include/optik_hip.h)
#endif

// (g++ does not know the pragma; clang needs it to keep Best in registers)
#if defined(__HIP__) || defined(__HIPCC__)
#define OPTIK_RM_UNROLL _Pragma("unroll")
#else
#define OPTIK_RM_UNROLL
#endif

namespace optik {
namespace roadmap {

constexpr int K_MAX = 16;                               // neighbours per node or query
constexpr int MAX_NODES = OPTIK_HIP_ROADMAP_MAX_NODES;  // two [N] f64 buffers in the 160 KiB of a CU's LDS
constexpr int MIN_WAYPOINTS = 2, MAX_WAYPOINTS = 64;    // Lmax (path_optimize.hpp's cap)
constexpr int FOUND = 0, NO_ROUTE = 1, TOO_LONG = 2, QUERY_NAN = 3;

OPTIK_CM_HD inline double inf() {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_huge_val();
#else
    return INFINITY;
#endif
}
OPTIK_CM_HD inline double nan_value() {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_nan("");
#else
    return NAN;
#endif
}

// Step 1: a_i = a[i * sa], b_i = b[i * sb].
OPTIK_CM_HD inline double edge_weight(int n, const double *a, long long sa, const double *b, long long sb) {
    return motion::motion_distance(n, a, sa, b, sb);
}
OPTIK_CM_HD inline double checked_weight(double weight, int index, bool motion_free) {
    return (index >= 0 && motion_free) ? weight : inf();
}

// Step 2: does (da, ia) come before (db, ib)?  ia >= 0; ib < 0 is an empty slot.
OPTIK_CM_HD inline bool ranks_before(double da, int ia, double db, int ib) {
    if (ib < 0) return true;
    const bool na = da != da, nb = db != db;
    if (na || nb) return na == nb ? ia < ib : nb;
    return da < db || (da == db && ia < ib);
}

// Step 2: the K_MAX best candidates so far, best first.
struct Best {
    double d[K_MAX];
    int i[K_MAX];
    OPTIK_CM_HD inline void clear() {
        OPTIK_RM_UNROLL
        for (int s = 0; s < K_MAX; ++s) { d[s] = inf(); i[s] = -1; }
    }
    OPTIK_CM_HD inline void insert(double dist, int index) {
        if (!ranks_before(dist, index, d[K_MAX - 1], i[K_MAX - 1])) return;
        OPTIK_RM_UNROLL
        for (int s = K_MAX - 1; s >= 0; --s) {
            // (slot s takes the slot above it while the candidate also comes before that one)
            const bool shift = s > 0 && ranks_before(dist, index, d[s > 0 ? s - 1 : 0], i[s > 0 ? s - 1 : 0]);
            const bool here = !shift && ranks_before(dist, index, d[s], i[s]);
            const double nd = shift ? d[s > 0 ? s - 1 : 0] : (here ? dist : d[s]);
            const int ni = shift ? i[s > 0 ? s - 1 : 0] : (here ? index : i[s]);
            d[s] = nd;
            i[s] = ni;
        }
    }
};

// Step 3.
OPTIK_CM_HD inline double relax(double d_v, double w, double d_u) {
    const double c = w + d_u;
    return c < d_v ? c : d_v;
}

// One query against one graph.  The slot arrays of the query are already offset to it: slot s is at s * qs.
struct Query {
    int N, k;             // the graph: nbr, w [k][N]
    const int32_t *nbr;
    const double *w;
    int ks, kg;           // start links start -> sidx, goal links gidx -> goal
    const int32_t *sidx, *gidx;
    const double *sw, *gw;
    long long qs;
    double direct;        // start -> goal
    int Lmax;
};

OPTIK_CM_HD inline bool node_ok(const Query &y, int u) { return u >= 0 && u < y.N; }

// Step 4: where d_u starts.
OPTIK_CM_HD inline double goal_weight(const Query &y, int u) {
    double g = inf();
    for (int s = 0; s < y.kg; ++s)
        if (y.gidx[s * y.qs] == u) g = relax(g, y.gw[s * y.qs], 0.0);
    return g;
}

// Step 4: node v's pull over its out-list, from the values d.
OPTIK_CM_HD inline double pull(const Query &y, const double *d, int v) {
    double dv = d[v];
    for (int s = 0; s < y.k; ++s) {
        const int u = y.nbr[(long long)s * y.N + v];
        if (node_ok(y, u)) dv = relax(dv, y.w[(long long)s * y.N + v], d[u]);
    }
    return dv;
}

// Step 5: -1 for the goal, the node index, or -2 when neither rule holds (d_v infinite or not a fixed point).
OPTIK_CM_HD inline int next_hop(const Query &y, const double *d, int v) {
    if (goal_weight(y, v) == d[v]) return -1;
    int best = -2;
    for (int s = 0; s < y.k; ++s) {
        const int u = y.nbr[(long long)s * y.N + v];
        if (node_ok(y, u) && y.w[(long long)s * y.N + v] + d[u] == d[v] && (best < 0 || u < best)) best = u;
    }
    return best;
}

// Step 6: the start slot of the first hop, -1 for the direct edge; *cost = best.
OPTIK_CM_HD inline int first_hop(const Query &y, const double *d, double *cost) {
    double best = y.direct;
    int hop = -1;
    for (int s = 0; s < y.ks; ++s) {
        const int u = y.sidx[s * y.qs];
        if (!node_ok(y, u)) continue;
        const double c = y.sw[s * y.qs] + d[u];
        if (c < best) { best = c; hop = s; }
    }
    *cost = best;
    return hop;
}

// Step 7: is a number of the query NaN?  start_i = start[i * ss], goal_i = goal[i * sg].
OPTIK_CM_HD inline bool query_has_nan(const Query &y, int n, const double *start, long long ss, const double *goal,
                                      long long sg) {
    bool bad = y.direct != y.direct;
    for (int i = 0; i < n; ++i) bad = bad || start[i * ss] != start[i * ss] || goal[i * sg] != goal[i * sg];
    for (int s = 0; s < y.ks; ++s) bad = bad || y.sw[s * y.qs] != y.sw[s * y.qs];
    for (int s = 0; s < y.kg; ++s) bad = bad || y.gw[s * y.qs] != y.gw[s * y.qs];
    return bad;
}

struct Plan {
    int status, len;  // len: the waypoints before padding
    double cost;
};

// Steps 6 and 7 from the converged d: the nodes walked go to nodes[0 .. len - 3] (room for MAX_WAYPOINTS - 2).
OPTIK_CM_HD inline Plan plan(const Query &y, const double *d, bool has_nan, int *nodes) {
    if (has_nan) return Plan{QUERY_NAN, 2, nan_value()};
    double cost;
    const int hop = first_hop(y, d, &cost);
    if (!(cost < inf())) return Plan{NO_ROUTE, 2, inf()};
    int count = 0;
    if (hop >= 0) {
        int v = y.sidx[hop * y.qs];
        for (;;) {
            if (count + 3 > y.Lmax) return Plan{TOO_LONG, 2, cost};
            nodes[count++] = v;
            v = next_hop(y, d, v);
            if (v == -1) break;
            if (v < 0) return Plan{NO_ROUTE, 2, inf()};  // (not at a fixed point: cannot happen after convergence)
        }
    }
    return Plan{FOUND, 2 + count, cost};
}

// ---- the serial reference of steps 2 to 7 (the tests' g++ driver; the device is compared with it bit for bit) ----

// The k best nodes of one query q (q_i = q[i * sq], node j's joint i = nodes[i * N + j]); self >= 0 skips that node.
inline void knn_reference(int n, const double *q, long long sq, const double *nodes, int N, int k, int self,
                          int32_t *idx_out, double *dist_out) {
    Best b;
    b.clear();
    for (int j = 0; j < N; ++j)
        if (j != self) b.insert(edge_weight(n, q, sq, nodes + j, N), j);
    for (int s = 0; s < k; ++s) { idx_out[s] = b.i[s]; dist_out[s] = b.d[s]; }
}

// Step 4 with Jacobi sweeps: d and tmp hold N doubles each; returns the sweeps that changed something.
inline int distances_reference(const Query &y, double *d, double *tmp) {
    for (int u = 0; u < y.N; ++u) d[u] = goal_weight(y, u);
    int sweeps = 0;
    for (; sweeps < y.N; ++sweeps) {
        bool changed = false;
        for (int v = 0; v < y.N; ++v) {
            tmp[v] = pull(y, d, v);
            // (values only fall, and never to a NaN)
            changed = changed || tmp[v] < d[v];
        }
        if (!changed) break;
        for (int v = 0; v < y.N; ++v) d[v] = tmp[v];
    }
    return sweeps;
}

// The whole query: path_out [Lmax][n] (start, the nodes, the goal, padded with the goal; start then the goal repeated
// unless the status is FOUND), d_out [N] the distances to the goal (may be null).
inline Plan plan_reference(const Query &y, int n, const double *nodes, const double *start, const double *goal,
                           double *path_out, double *d_out) {
    double *d = new double[2 * (size_t)y.N];
    distances_reference(y, d, d + y.N);
    int walked[MAX_WAYPOINTS];
    const Plan p = plan(y, d, query_has_nan(y, n, start, 1, goal, 1), walked);
    for (int t = 0; t < y.Lmax; ++t)
        for (int i = 0; i < n; ++i) {
            double v = goal[i];
            if (t == 0) v = start[i];
            else if (t < p.len - 1) v = nodes[(long long)i * y.N + walked[t - 1]];
            path_out[t * n + i] = v;
        }
    if (d_out)
        for (int u = 0; u < y.N; ++u) d_out[u] = d[u];
    delete[] d;
    return p;
}

}  // namespace roadmap
}  // namespace optik
