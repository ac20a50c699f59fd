// shortcut_constrained_measure.hpp -- the rules of path shortcutting and of equal-spacing resampling under a pose
// constraint, one source for the host and the device (optik_hip_path_shortcut_constrained /
// _path_resample_constrained, optik_hip.h; ik_shortcut.hip).
//
// shortcut_measure.hpp's shortcutting with every subdivision vertex projected onto a pose constraint
// (constraint_measure.hpp: a box on the pose error against a reference) and every vertex pair judged by the collision
// motion check AND by constraint::motion at tol; its resampling with every interior waypoint projected.  Its rules are
// shortcut_measure.hpp's with these changes and no others (the exact operation order; the tests depend on it;
// -ffp-contract=off on both sides).  Everything that is not named here -- the subdivision counts, the pair indexing,
// the route recurrence and its tie rule, the walk, the status order, the padding -- is shortcut_measure.hpp's, called
// and not restated.
//
//  2'. Vertices.  The input's own waypoints are vertices, copied bit for bit and never projected: the start and the
//      goal never move.  Every other vertex is vertex_joint's value per joint, x, and then
//      constraint::project(x, ptol, piters, damping, max_step) is applied to it: one projection attempted.  Status
//      PROJECTED: the vertex is the projected configuration.  Any other status: the vertex is dead, all its joints
//      NaN (vertex_after).  Neither motion check samples a NaN endpoint, so every pair with a dead vertex is blocked
//      and no route passes through it.
//  3'. Visibility.  Pair i < j is open iff the motion vertex i -> vertex j is free by the collision motion check at
//      `resolution` AND ok by constraint::motion at `resolution`, tol, in that direction (the second check need not be
//      made where the first has said no: the verdict is the AND).  The weights and the cost are taken over the
//      vertices of rule 2'; cost_in stays the input's.
//  7'. Resampling.  Waypoint j is resample_waypoint's value; for 0 < j < Lout - 1, on a path whose status is not
//      PATH_NAN, it is then projected as in 2' (projects).  A projection that is not PROJECTED leaves the interpolated
//      value and gives the path the status UNPROJECTED (4), which ranks below PATH_NAN and BAD_LENGTH: they keep their
//      meaning and their precedence (resample_status).  On a row of status PATH_NAN nothing is projected.
//  8.  projected[0] = the projections attempted, projected[1] = those that ended PROJECTED, per path; both 0 where
//      prepare already gave a status (there are no vertices then).
//
// Consequences.  Every vertex of a FOUND route that is not an input waypoint has violation <= ptol and lies inside the
// joint limits (constraint_measure.hpp step 6).  What holds BETWEEN the vertices is what constraint::motion found at
// its samples with tol: edge interiors are not projected.  The cost of a found route can exceed cost_in, because
// projected vertices leave the polyline; the caller compares the two.  After resampling the spacing is equal before
// the projection and only approximately equal after it.
//
// With a box that is free on all six axes (lo = -inf, hi = +inf) a projection returns its input after 0 iterations,
// once clamped into the joint limits: on a path whose vertices lie within the limits the vertices are the
// unconstrained vertices bit for bit, every constraint verdict is ok wherever the motion is sampled -- and the
// collision motion check blocks every pair it does not sample --, so every shared output equals
// optik_hip_path_shortcut's and optik_hip_path_resample's bit for bit.
//
// This header does not include constraint_measure.hpp: the references at its end take the projection as a callback,
// as they take the verdicts, so plain g++ compiles it (tests/shortcut_constrained_util.py) and the device is compared
// with it bit for bit on the host header's projections and the device's own verdicts.
#pragma once

#include "shortcut_measure.hpp"

namespace optik {
namespace shortcut {

constexpr int UNPROJECTED = 4;    // rule 7': an interior waypoint kept its interpolated value
constexpr int PROJECTION_OK = 0;  // constraint::PROJECTED (ik_shortcut.hip asserts the two are one)

// Rule 2': is vertex v, of segment s = vertex_segment(v), one of the input's own waypoints?
OPTIK_CM_HD inline bool is_waypoint(const int *off, int s, int v) { return v == off[s]; }
// Rule 2': a joint of a vertex after its projection ended with `status`.
OPTIK_CM_HD inline double vertex_after(int status, double projected) {
    return status == PROJECTION_OK ? projected : __builtin_nan("");
}
// Rule 7': is output waypoint j of a path with resample_waypoint's status `status` projected?
OPTIK_CM_HD inline bool projects(int status, int Lout, int j) { return status != PATH_NAN && j > 0 && j < Lout - 1; }
OPTIK_CM_HD inline int resample_status(int status, bool unprojected) {
    return status != 0 ? status : (unprojected ? UNPROJECTED : 0);
}

// ---- the serial references (the tests' g++ driver; the device is compared with them bit for bit) ------------------

// Rule 2' for one path ([Lin][n]) -> verts [n][MAX_POINTS], w [MAX_POINTS]; returns prepare's answer.  project(x [n]
// in and out, &iterations) -> status.  iterations [MAX_POINTS] (may be null): what each vertex's projection took, -1
// for an input waypoint.
template <class Project>
inline Prepared vertices_constrained_reference(int n, const double *path, int len, int Lin, int V, Project &&project,
                                               double *verts, double *w, int *projected, int *iterations) {
    int m[MAX_POINTS], off[MAX_POINTS];
    const int le = read_length(len, Lin);
    bool fin = true;
    for (int t = 0; t < le; ++t) fin = fin && waypoint_finite(n, path, n, t);
    for (int s = 0; s < le - 1; ++s) w[s] = segment_weight(n, path, n, s);
    const Prepared p = prepare(len, Lin, V, fin, w, m, off);
    projected[0] = projected[1] = 0;
    for (int v = 0; v < p.nv; ++v) {
        const int s = vertex_segment(p.le, off, v);
        double x[MAX_JOINTS];
        for (int i = 0; i < n; ++i) x[i] = vertex_joint(path, n, m, off, s, v, i);
        int its = -1;
        if (!is_waypoint(off, s, v)) {
            its = 0;
            const int st = project(x, &its);
            projected[0] += 1;
            if (st == PROJECTION_OK) projected[1] += 1;
            for (int i = 0; i < n; ++i) x[i] = vertex_after(st, x[i]);
        }
        if (iterations) iterations[v] = its;
        for (int i = 0; i < n; ++i) verts[i * MAX_POINTS + v] = x[i];
    }
    return p;
}

// The whole of one path.  pair_open(i, j, qa [n], qb [n]) -> bool: rule 3' for the motion vertex i -> vertex j = qa ->
// qb, asked once for every i < j < nv.  path_out [Lout][n]; d_out [MAX_POINTS] and verts_out [n][MAX_POINTS] may be
// null; projected [2].
template <class Project, class PairOpen>
inline Result shortcut_constrained_reference(int n, const double *path, int len, int Lin, int V, Project &&project,
                                             PairOpen &&pair_open, double hop_penalty, int Lout, double *path_out,
                                             double *d_out, double *verts_out, int *projected) {
    double verts[MAX_JOINTS * MAX_POINTS], w[MAX_POINTS], d[MAX_POINTS], qa[MAX_JOINTS], qb[MAX_JOINTS];
    int succ[MAX_POINTS], route[MAX_POINTS], count;
    for (int e = 0; e < MAX_JOINTS * MAX_POINTS; ++e) verts[e] = __builtin_nan("");
    const Prepared p = vertices_constrained_reference(n, path, len, Lin, V, project, verts, w, projected, nullptr);
    for (int v = 0; v < MAX_POINTS; ++v) { d[v] = inf(); succ[v] = -1; }
    if (p.status == GO_ON) {
        d[p.nv - 1] = 0.0;
        for (int i = p.nv - 2; i >= 0; --i) {
            double bc = inf();
            int bj = -1;
            for (int j = i + 1; j < p.nv; ++j) {
                for (int k = 0; k < n; ++k) { qa[k] = verts[k * MAX_POINTS + i]; qb[k] = verts[k * MAX_POINTS + j]; }
                const double c = hop_cost(pair_weight(n, verts, MAX_POINTS, i, j, pair_open(i, j, qa, qb)),
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
    if (verts_out)
        for (int e = 0; e < MAX_JOINTS * MAX_POINTS; ++e) verts_out[e] = verts[e];
    return r;
}

// Rule 7' for one path: path_out [Lout][n]; projected [2]; returns the status.
template <class Project>
inline int resample_constrained_reference(int n, const double *path, int len, int Lin, int Lout, Project &&project,
                                          double *path_out, int *projected) {
    int status = 0;
    bool unprojected = false;
    projected[0] = projected[1] = 0;
    for (int j = 0; j < Lout; ++j) {
        double *out = path_out + j * n;
        status = resample_waypoint(n, path, n, len, Lin, Lout, j, out, 1);
        if (!projects(status, Lout, j)) continue;
        double x[MAX_JOINTS];
        for (int i = 0; i < n; ++i) x[i] = out[i];
        int its = 0;
        const int st = project(x, &its);
        projected[0] += 1;
        if (st == PROJECTION_OK) {
            projected[1] += 1;
            for (int i = 0; i < n; ++i) out[i] = x[i];
        } else {
            unprojected = true;
        }
    }
    return resample_status(status, unprojected);
}

}  // namespace shortcut
}  // namespace optik
