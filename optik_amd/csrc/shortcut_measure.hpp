// shortcut_measure.hpp -- the arithmetic of path shortcutting and of equal-spacing resampling, one source for the host
// and the device (optik_hip_path_shortcut / _path_resample, optik_hip.h; ik_shortcut.hip).
//
// A path is a polyline of `len` joint-space waypoints, 2 <= len <= Lin <= 64, joint i of waypoint t at
// path[t * st + i].  The metric is L-infinity in radians: the distances are motion::motion_distance, the interpolation
// is motion::motion_sample and the step count is motion::motion_steps (motion_measure.hpp), called and not restated.
// The exact operation order (the tests depend on it; -ffp-contract=off on both sides, only the correctly rounded
// + - * /, fabs, ceil and comparisons):
//
//  1. The length that is read: le = len clamped into 2 .. Lin.  Segment s = 0 .. le - 2 joins waypoint s to s + 1 and
//     weighs w_s = motion_distance.  A waypoint is finite when x - x == 0 for each of its joints (is_finite).
//  2. Subdivision into at most V vertices, 2 <= V <= 64 (pieces): T = ((0 + w_0) + w_1) + ..., s ascending.  With
//     V > le and 0 < T < +inf the target spacing is sp = T / (double)(V - le) and segment s is cut into
//     m_s = max(1, ceil(w_s / sp)) pieces (a NaN quotient gives 1), clamped, walking s upwards, to what the budget of
//     V - 1 pieces has left once every later segment keeps one.  Otherwise every m_s = 1.  Vertex off_s = m_0 + ... +
//     m_(s-1) is waypoint s, copied bit for bit; vertex off_s + k, 0 < k < m_s, is motion_sample(qa_i, qb_i, k, m_s)
//     per joint (vertex_joint).  There are nv = 1 + sum m_s <= V vertices.
//  3. Visibility: every pair i < j < nv is the motion vertex i -> vertex j, checked in that direction only at the
//     call's resolution by the motion check.  Pair (i, j) has the index pair_index(V, i, j) -- of the budget V, not of
//     nv -- in the path's flag array.  Its weight is motion_distance where the flag is set and +inf where it is not
//     (pair_weight).
//  4. The route: d[nv - 1] = 0; for i = nv - 2 down to 0 the candidates are c_j = (w(i, j) + hop_penalty) + d[j],
//     j = i + 1 .. nv - 1; only a c_j < +inf is a candidate (so neither +inf nor a NaN ever wins), the least wins and
//     exact ties go to the HIGHEST j (beats): d[i] = c_j, succ[i] = j; without a candidate d[i] = +inf.  (value, -j) is
//     a total order on the candidates, so the minimum does not depend on the order they are visited in.
//  5. The walk (finish): 0, succ[0], succ[succ[0]], ... to nv - 1 -- strictly ascending, at most nv vertices.  The cost
//     is the pure length of the walked route, without the penalties, added from the goal backwards:
//     (w_first + (... + (w_last + 0))).  cost_in is the same over the w_s of the input.
//  6. Status, in this order: BAD_LENGTH (2) when len is outside 2 .. min(Lin, V); PATH_NAN (3) when one of the le
//     waypoints is not finite; NO_ROUTE (1) when d[0] < +inf is false; BAD_LENGTH (2) when the route has more than Lout
//     vertices; else FOUND (0).  FOUND writes the route's vertices, padded with the goal (waypoint le - 1), and
//     len_out = their count.  Every other status returns the input: its le waypoints padded with the goal and
//     len_out = le when le <= Lout, else the start, then the goal repeated, and len_out = 2.  cost is cost_in then,
//     except for a route that does not fit Lout, which reports its true cost.
//  7. Resampling to Lout waypoints, 2 <= Lout <= 64 (resample_waypoint): c_0 = 0, c_(s+1) = c_s + w_s, T = c_(le-1).
//     Waypoint 0 is the start and waypoint Lout - 1 the goal, copied.  Waypoint j between them sits at
//     a = T * ((double)j / (double)(Lout - 1)) in the LAST segment s <= le - 2 with c_s <= a; t = (a - c_s) / w_s, 0
//     for w_s = 0, and 1 where the quotient exceeds 1 (c_(s+1) - c_s may exceed w_s by a rounding);
//     q_i = qa_i + t * (qb_i - qa_i).  T = 0 copies the start.  T NaN or infinite: status PATH_NAN, the start, then
//     the goal repeated.  Status BAD_LENGTH when len is outside 2 .. Lin (le is resampled all the same), else 0.
//
// Plain host C++ compiles this header too (no HIP runtime): tests/shortcut_util.py drives it with g++, and the serial
// reference of the whole of 1 to 7 at its end (shortcut_reference, resample_reference) is what the tests compare the
// device with.
#pragma once

#include "motion_measure.hpp"

#ifndef OPTIK_HIP_PATH_SHORTCUT_MAX_VERTICES
#define OPTIK_HIP_PATH_SHORTCUT_MAX_VERTICES 64  // (include/optik_hip.h)
#endif

namespace optik {
namespace shortcut {

constexpr int MIN_POINTS = 2, MAX_POINTS = OPTIK_HIP_PATH_SHORTCUT_MAX_VERTICES;  // len, Lin, V and Lout alike
constexpr int MAX_JOINTS = 16;  // joint positions of a chain (ik_wide.hpp: WIDE_MAX_DOF)
constexpr int FOUND = 0, NO_ROUTE = 1, BAD_LENGTH = 2, PATH_NAN = 3;
constexpr int GO_ON = -1;  // prepare: no status yet

OPTIK_CM_HD inline double inf() {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_huge_val();
#else
    return INFINITY;
#endif
}

OPTIK_CM_HD inline bool is_finite(double x) { return x - x == 0.0; }

// Step 1.
OPTIK_CM_HD inline int read_length(int len, int Lin) { return len < MIN_POINTS ? MIN_POINTS : (len > Lin ? Lin : len); }
OPTIK_CM_HD inline double segment_weight(int n, const double *path, long long st, int s) {
    return motion::motion_distance(n, path + s * st, 1, path + (s + 1) * st, 1);
}
OPTIK_CM_HD inline bool waypoint_finite(int n, const double *path, long long st, int t) {
    bool ok = true;
    for (int i = 0; i < n; ++i) ok = ok && is_finite(path[t * st + i]);
    return ok;
}

// Step 2: m [le - 1], off [le] from w [le - 1]; returns nv.
OPTIK_CM_HD inline int pieces(int le, int V, const double *w, int *m, int *off) {
    double T = 0.0;
    for (int s = 0; s < le - 1; ++s) T = T + w[s];
    const bool cut = V > le && T > 0.0 && T < inf();
    const double sp = cut ? T / (double)(V - le) : 0.0;
    int left = V - 1, o = 0;
    for (int s = 0; s < le - 1; ++s) {
        int ms = 1;
        if (cut) {
            const int cap = left - (le - 2 - s);  // (>= 1: left >= le - 1 - s holds on the way)
            const double r = ceil(w[s] / sp);
            ms = !(r >= 1.0) ? 1 : (r > (double)cap ? cap : (int)r);
        }
        m[s] = ms;
        off[s] = o;
        o += ms;
        left -= ms;
    }
    off[le - 1] = o;
    return o + 1;
}

// Step 2: the last s <= le - 1 with off[s] <= v.
OPTIK_CM_HD inline int vertex_segment(int le, const int *off, int v) {
    int s = 0;
    while (s + 1 < le && off[s + 1] <= v) ++s;
    return s;
}
OPTIK_CM_HD inline double vertex_joint(const double *path, long long st, const int *m, const int *off, int s, int v,
                                       int i) {
    const double qa = path[s * st + i];
    if (v == off[s]) return qa;  // (a waypoint; s = le - 1 has no segment behind it)
    return motion::motion_sample(qa, path[(s + 1) * st + i], v - off[s], m[s]);
}

// Steps 1 and 6, what comes before the vertices: the status so far and nv (0 unless GO_ON).
struct Prepared {
    int status, le, nv;
};
OPTIK_CM_HD inline Prepared prepare(int len, int Lin, int V, bool all_finite, const double *w, int *m, int *off) {
    const int le = read_length(len, Lin);
    if (len != le || len > V) return Prepared{BAD_LENGTH, le, 0};
    if (!all_finite) return Prepared{PATH_NAN, le, 0};
    return Prepared{GO_ON, le, pieces(le, V, w, m, off)};
}

// Step 3.  Vertex v's joint i is at verts[i * sv + v].
OPTIK_CM_HD inline int pair_count(int V) { return V * (V - 1) / 2; }
OPTIK_CM_HD inline int pair_index(int V, int i, int j) { return i * (2 * V - i - 1) / 2 + (j - i - 1); }
OPTIK_CM_HD inline double pair_weight(int n, const double *verts, long long sv, int i, int j, bool motion_free) {
    return motion_free ? motion::motion_distance(n, verts + i, sv, verts + j, sv) : inf();
}

// Step 4.
OPTIK_CM_HD inline double hop_cost(double w, double hop_penalty, double d_j) { return (w + hop_penalty) + d_j; }
// Does the candidate (c, j) come before the best so far (bc, bj)?  bj < 0: there is none yet.
OPTIK_CM_HD inline bool beats(double c, int j, double bc, int bj) {
    return c < inf() && (bj < 0 || c < bc || (c == bc && j > bj));
}

struct Result {
    int status, len;  // len: the waypoints before the padding
    double cost, cost_in;
};

// Step 5, cost_in: the w_s of the input from the goal backwards.
OPTIK_CM_HD inline double input_cost(int le, const double *w) {
    double c = 0.0;
    for (int s = le - 2; s >= 0; --s) c = w[s] + c;
    return c;
}

// Steps 5 and 6 from d[0] and succ: route [MAX_POINTS] receives the walked vertices; *count their number (0 unless
// the status is FOUND).
OPTIK_CM_HD inline Result finish(const Prepared &p, int n, const double *verts, long long sv, double d0,
                                 const int *succ, int Lout, double cost_in, int *route, int *count) {
    const int kept = p.le <= Lout ? p.le : 2;
    *count = 0;
    if (p.status != GO_ON) return Result{p.status, kept, cost_in, cost_in};
    if (!(d0 < inf())) return Result{NO_ROUTE, kept, cost_in, cost_in};
    int c = 0;
    for (int v = 0; v != p.nv - 1 && c < MAX_POINTS - 1; v = succ[v]) route[c++] = v;
    route[c++] = p.nv - 1;
    double cost = 0.0;
    for (int k = c - 2; k >= 0; --k) cost = motion::motion_distance(n, verts + route[k], sv, verts + route[k + 1], sv) + cost;
    if (c > Lout) return Result{BAD_LENGTH, kept, cost, cost_in};
    *count = c;
    return Result{FOUND, c, cost, cost_in};
}

// Step 6: joint i of output waypoint t.
OPTIK_CM_HD inline double output_joint(const Result &r, int le, const double *path, long long st, const double *verts,
                                       long long sv, const int *route, int t, int i) {
    if (r.status == FOUND) return t < r.len ? verts[i * sv + route[t]] : path[(le - 1) * st + i];
    if (r.len == le) return path[(t < le ? t : le - 1) * st + i];
    return path[(t == 0 ? 0 : le - 1) * st + i];
}

// Step 7: joint values of output waypoint j go to out[i * so]; returns the path's status.
OPTIK_CM_HD inline int resample_waypoint(int n, const double *path, long long st, int len, int Lin, int Lout, int j,
                                         double *out, long long so) {
    const int le = read_length(len, Lin);
    double T = 0.0;
    for (int s = 0; s < le - 1; ++s) T = T + segment_weight(n, path, st, s);
    const bool bad = !is_finite(T);
    int from = -1;  // the waypoint that is copied, if one is
    if (j == 0) from = 0;
    else if (j == Lout - 1 || bad) from = le - 1;
    else if (!(T > 0.0)) from = 0;
    if (from >= 0) {
        for (int i = 0; i < n; ++i) out[i * so] = path[from * st + i];
    } else {
        const double a = T * ((double)j / (double)(Lout - 1));
        int s = 0;
        double cs = 0.0, ws = 0.0, c = 0.0;
        for (int u = 0; u < le - 1; ++u) {
            const double wu = segment_weight(n, path, st, u);
            if (c <= a) { s = u; cs = c; ws = wu; }
            c = c + wu;
        }
        double t = ws > 0.0 ? (a - cs) / ws : 0.0;
        if (t > 1.0) t = 1.0;
        for (int i = 0; i < n; ++i) {
            const double qa = path[s * st + i], qb = path[(s + 1) * st + i];
            out[i * so] = qa + t * (qb - qa);
        }
    }
    return bad ? PATH_NAN : (len != le ? BAD_LENGTH : 0);
}

// ---- the serial reference of steps 1 to 7 (the tests' g++ driver; the device is compared with it bit for bit) ----

// The vertices of one path ([Lin][n]) -> verts [n][MAX_POINTS]; w [MAX_POINTS]; returns prepare's answer.
inline Prepared vertices_reference(int n, const double *path, int len, int Lin, int V, double *verts, double *w) {
    int m[MAX_POINTS], off[MAX_POINTS];
    const int le = read_length(len, Lin);
    bool fin = true;
    for (int t = 0; t < le; ++t) fin = fin && waypoint_finite(n, path, n, t);
    for (int s = 0; s < le - 1; ++s) w[s] = segment_weight(n, path, n, s);
    const Prepared p = prepare(len, Lin, V, fin, w, m, off);
    for (int v = 0; v < p.nv; ++v) {
        const int s = vertex_segment(p.le, off, v);
        for (int i = 0; i < n; ++i) verts[i * MAX_POINTS + v] = vertex_joint(path, n, m, off, s, v, i);
    }
    return p;
}

// The whole of one path: free_flag [pair_count(V)] the motion check's answers; path_out [Lout][n]; d_out [MAX_POINTS]
// (may be null) the objective of every vertex.
inline Result shortcut_reference(int n, const double *path, int len, int Lin, int V, const unsigned char *free_flag,
                                 double hop_penalty, int Lout, double *path_out, double *d_out) {
    double verts[MAX_JOINTS * MAX_POINTS], w[MAX_POINTS], d[MAX_POINTS];
    int succ[MAX_POINTS], route[MAX_POINTS], count;
    const Prepared p = vertices_reference(n, path, len, Lin, V, verts, w);
    for (int v = 0; v < MAX_POINTS; ++v) { d[v] = inf(); succ[v] = -1; }
    if (p.status == GO_ON) {
        d[p.nv - 1] = 0.0;
        for (int i = p.nv - 2; i >= 0; --i) {
            double bc = inf();
            int bj = -1;
            for (int j = i + 1; j < p.nv; ++j) {
                const double c = hop_cost(pair_weight(n, verts, MAX_POINTS, i, j, free_flag[pair_index(V, i, j)] != 0),
                                          hop_penalty, d[j]);
                if (beats(c, j, bc, bj)) { bc = c; bj = j; }
            }
            d[i] = bc;
            succ[i] = bj;
        }
    }
    const Result r = finish(p, n, verts, MAX_POINTS, d[0], succ, Lout, input_cost(p.le, w), route, &count);
    for (int t = 0; t < Lout; ++t)
        for (int i = 0; i < n; ++i) path_out[t * n + i] = output_joint(r, p.le, path, n, verts, MAX_POINTS, route, t, i);
    if (d_out)
        for (int v = 0; v < MAX_POINTS; ++v) d_out[v] = d[v];
    return r;
}

// path_out [Lout][n]; returns the status.
inline int resample_reference(int n, const double *path, int len, int Lin, int Lout, double *path_out) {
    int status = 0;
    for (int j = 0; j < Lout; ++j) status = resample_waypoint(n, path, n, len, Lin, Lout, j, path_out + j * n, 1);
    return status;
}

}  // namespace shortcut
}  // namespace optik
