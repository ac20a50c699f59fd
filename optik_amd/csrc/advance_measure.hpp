// advance_measure.hpp -- the certified motion check (conservative advancement), one source for the host and the device
// (optik_hip_collision_motion_certify_batch, optik_hip.h).  The distances and the clearance of
// a configuration are collision_measure.hpp's, unchanged; the frames are section 5.12's: 0 the base, f = 1 .. n the
// pose after joint f, n + 1 the end effector with the call's ee_offset.
//
// The sampled check (motion_measure.hpp) says "free at the samples".  This one walks the straight joint-space segment
// q(t) = qa + t (qb - qa), t in [0, 1], in steps whose length comes from the clearance at the last sample and from
// bounds on how fast every distance term can shrink, and so says something about the whole segment.
//
// The exact operation order (the tests depend on it; -ffp-contract=off on both sides, only the correctly rounded
// + - * / sqrt, fabs, fmin / fmax and comparisons):
//
//  1. The reach table, built on the host per call (build_reach).  |v| = sqrt((x * x + y * y) + z * z) (norm3).  For
//     1 <= j <= f <= n + 1, reach(j, f) is the sum of the norms of the fixed translations between joint j's origin and
//     frame f's origin: starting from r = 0.0, r = r + |origin[i].t| for the joints i = j + 1 .. min(f, n) ascending
//     (reach(j, j) = 0.0), and for f = n + 1 then r = r + |t| of the trailing fixed joint, if the chain has one, and
//     r = r + |ee_offset.t| (0.0 without an ee_offset: the sum is unchanged).
//  2. Speeds.  a_j = fabs(qb_j - qa_j).  A robot sphere s on frame f with local centre c_s, |c_s| = norm3(c_s):
//         lam(s) = l, from l = 0.0:  l = l + a_j * (reach(j, f) + |c_s|)   for j = 1 .. min(f, n) ascending
//     (frame 0: 0.0; lam_sphere).  A self pair with the lower frame fa and the higher frame fb, b the sphere on fb:
//         lam(a, b) = l, from l = 0.0:  l = l + a_j * (reach(j, fb) + |c_b|)   for j = fa + 1 .. min(fb, n) ascending
//     (fa == fb: 0.0; lam_pair).  A pair stored with the frames the other way round is the same pair: the rule is
//     applied with the lower frame as fa (pair_lam); with equal frames no joint is summed, whichever sphere is b.
//     Why these bound the motion: joint j turns everything behind it about its axis through its origin o_j, so a
//     point p there moves at |v| <= |qdot_j| * dist(p, axis_j) <= |qdot_j| * |p - o_j|, and by the triangle inequality
//     along the chain |p - o_j| <= reach(j, f) + |c_s| in every configuration.  qdot_j = qb_j - qa_j per unit of t.
//     The joints up to fa move both spheres of a pair as one rigid body and the joints behind fb move neither, so only
//     fa + 1 .. fb change their distance, by the speed of b as seen from frame fa.
//  3. The sample at t (sample): t == 0.0 copies qa_i, t == 1.0 copies qb_i, otherwise qa_i + t * (qb_i - qa_i) (the
//     difference, the product, then the sum: motion_sample's arithmetic).
//  4. Terms.  m = the chain's margin, m' = m - tol.  Every term of the clearance has a distance d and an advance:
//         robot sphere vs world sphere / box:  d as collision_measure.hpp step 2 / 3;  advance (d - m') / lam(s)
//         self pair:                            d as step 2;                             advance (d - m') / lam(a, b)
//         grid term, centre inside the grid:    d = grid_distance (step 5);     advance (d - m') / (G * lam(s))
//         grid term, centre outside the grid:   d = +inf (it contributes nothing to the clearance, as in step 5);
//                                               advance fmax(dbox, ((g - r) - m') / G) / lam(s)
//     (term_advance, grid_term).  G is the call's grid_lipschitz, finite and > 0.  A divisor of 0.0 gives +inf; a
//     term with d < m is never divided (its advance is 0.0: it blocks the sample, and the walk stops there).
//     Outside the grid, with u_a = (p_a - origin_a) * inv as in step 5: uc_a = fmin(fmax(u_a, 0.0), (double)(n_a - 1)),
//     g = the trilinear value at uc (the cell and lerp rule of step 5: i_a = min((int)floor(uc_a), n_a - 2),
//     f_a = uc_a - (double)i_a, along z, then y, then x), e_a = fmax(fmax(0.0 - u_a, u_a - (double)(n_a - 1)), 0.0) and
//     dbox = sqrt((e_x * e_x + e_y * e_y) + e_z * e_z) / inv, the distance from the centre to the grid's box.
//     Why the outside rule is sound: ignoring the term would be wrong, because the sphere may enter the grid.  It
//     cannot enter before its centre has moved dbox, which gives dbox / lam.  And the clamped point is the point of
//     the box nearest the centre; clamping is 1-Lipschitz, so x -> trilinear(clamp(x)) is G-Lipschitz wherever the
//     field is, and where the centre is inside it equals the field.  So after t has moved by dt the grid term, should
//     the centre be inside by then, is >= g - r - G * lam * dt, which stays >= m' while dt <= ((g - r) - m') / (G *
//     lam).  Either bound is enough on its own: the larger one is taken.
//  5. The sample's clearance c is the minimum of the d (+inf when there is nothing to check), the bits
//     optik_hip_collision_batch gives that configuration; the sample's advance A is the minimum of the advances (+inf
//     when there are none).  Both minima are exact in any order, so neither depends on how the terms are spread over
//     lanes.
//  6. The walk (walk_begin, walk_take): k = 0, t_0 = 0.  At sample k:
//       a. a NaN frame: status NAN (3), t_stop = t_k, clearance NaN, stop
//       b. !(c >= m): status BLOCKED (1), t_stop = t_k, stop
//       c. t_k == 1.0: status FREE (0), t_stop = 1, stop
//       d. k + 1 == max_steps: status LIMIT (2), t_stop = t_k, stop
//       e. t_{k+1} = t_k + A, set to 1.0 when it is >= 1.0 (A = +inf included); k = k + 1
//     steps = the samples evaluated; clearance = the minimum c over them (fmin, from +inf).  A segment with a NaN or
//     infinite joint in qa or qb is not walked: status 3, steps 0, t_stop NaN, clearance NaN (segment_finite).
//     Without a model every finite segment is FREE with steps 2 (A = +inf: the samples are t = 0 and t = 1) and
//     clearance +inf; so is a free qa == qb (every lam is 0.0), which is BLOCKED at sample 0 otherwise.
//     At a free sample every term has d >= m, so A >= tol / (max(1, G) * lam_max) > 0 and a segment that stays free
//     ends within ceil(max(1, G) * lam_max / tol) + 2 samples -- except that with a grid installed and a centre
//     outside it the lower bound does not hold (dbox may be tiny while the field behind the boundary is low).
//
// What it certifies.  FREE: for every t in [0, 1] the clearance function of section 5.12 is >= margin - tol, and at the
// visited samples it is >= margin.  BLOCKED exhibits q(t_stop), a configuration that is not free.  A motion whose true
// minimum clearance is below margin - tol can never come back FREE; one whose minimum is >= margin can never come back
// BLOCKED; in between either answer is right.  LIMIT says nothing: a long grazing motion with a small tol, or a sphere
// creeping up to the boundary of a grid behind which the field is low.  The statement is about the library's clearance
// function: with a grid world it inherits section 5.14's sqrt(3) * voxel, it is only as true as grid_lipschitz
// (sqrt(3) holds for every grid whose neighbouring nodes differ by at most one voxel, as those of a true distance
// field do), and the floating-point rounding of the bounds is not accounted for: tol is meant to be many orders above
// 1e-16.
//
// Plain host C++ compiles this header too (no HIP runtime): tests/test_advance_host.py drives it with g++.
#pragma once

#include "collision_measure.hpp"

namespace optik {
namespace advance {

constexpr int MAX_JOINTS = 16;             // joint positions of a chain (WIDE_MAX_DOF)
constexpr int MAX_FRAMES = MAX_JOINTS + 2;
enum : int { FREE = 0, BLOCKED = 1, LIMIT = 2, NOT_A_NUMBER = 3 };  // OPTIK_HIP_CERTIFY_*

OPTIK_CM_HD inline double inf() { return __builtin_huge_val(); }
OPTIK_CM_HD inline double qnan() { return __builtin_nan(""); }

OPTIK_CM_HD inline double norm3(const double *v) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

// Step 1.  r[j - 1][f] = reach(j, f) for 1 <= j <= f <= n + 1; everything else 0.0.
struct Reach {
    double r[MAX_JOINTS][MAX_FRAMES];
};

// origin: the chain table's fixed transforms, 7 doubles each (t first): joint i's is origin[i - 1], the trailing fixed
// joint's origin[n] (read only with has_tip).  ee_offset7 may be null.
inline void build_reach(int n, const double (*origin)[7], bool has_tip, const double *ee_offset7, Reach &R) {
    for (int j = 0; j < MAX_JOINTS; ++j)
        for (int f = 0; f < MAX_FRAMES; ++f) R.r[j][f] = 0.0;
    for (int j = 1; j <= n; ++j) {
        double r = 0.0;
        for (int f = j + 1; f <= n; ++f) {
            r = r + norm3(origin[f - 1]);
            R.r[j - 1][f] = r;
        }
        if (has_tip) r = r + norm3(origin[n]);
        if (ee_offset7) r = r + norm3(ee_offset7);
        R.r[j - 1][n + 1] = r;
    }
}

// Step 2.  a: a_j = a[j - 1]; reach: a Reach's r, flat (Reach::r[0] or a copy of it).
OPTIK_CM_HD inline double lam_sphere(int n, int f, const double *a, const double *reach, double cnorm) {
    double l = 0.0;
    const int top = f < n ? f : n;
    for (int j = 1; j <= top; ++j) l = l + a[j - 1] * (reach[(j - 1) * MAX_FRAMES + f] + cnorm);
    return l;
}

// fa <= fb; cnorm_b: |c| of the sphere on fb.
OPTIK_CM_HD inline double lam_pair(int n, int fa, int fb, const double *a, const double *reach, double cnorm_b) {
    double l = 0.0;
    const int top = fb < n ? fb : n;
    for (int j = fa + 1; j <= top; ++j) l = l + a[j - 1] * (reach[(j - 1) * MAX_FRAMES + fb] + cnorm_b);
    return l;
}

// The pair as it is stored: sphere x on frame fx, sphere y on frame fy, in either order.
OPTIK_CM_HD inline double pair_lam(int n, int fx, double cnorm_x, int fy, double cnorm_y, const double *a,
                                   const double *reach) {
    return fx <= fy ? lam_pair(n, fx, fy, a, reach, cnorm_y) : lam_pair(n, fy, fx, a, reach, cnorm_x);
}

// Step 3, one joint.
OPTIK_CM_HD inline double sample(double qa, double qb, double t) {
    if (t == 0.0) return qa;
    if (t == 1.0) return qb;
    return qa + t * (qb - qa);
}

OPTIK_CM_HD inline bool finite(double x) { return x == x && fabs(x) != inf(); }

// Step 6: is every joint of qa and qb finite?  qa_i = qa[i * sa], qb_i = qb[i * sb].
OPTIK_CM_HD inline bool segment_finite(int n, const double *qa, long long sa, const double *qb, long long sb) {
    bool ok = true;
    for (int i = 0; i < n; ++i) ok = ok && finite(qa[i * sa]) && finite(qb[i * sb]);
    return ok;
}

// Step 4: the advance of a term at distance d whose distance shrinks by at most `den` per unit of t.
OPTIK_CM_HD inline double term_advance(double d, double m, double mp, double den) {
    if (d < m) return 0.0;
    if (den == 0.0) return inf();
    return (d - mp) / den;
}

// Step 4, outside the grid: the trilinear value at uc (every uc_a in [0, n_a - 1]).
OPTIK_CM_HD inline double grid_value(double ux, double uy, double uz, const coll::Grid &g) {
    int ix = (int)floor(ux), iy = (int)floor(uy), iz = (int)floor(uz);
    if (ix > g.n[0] - 2) ix = g.n[0] - 2;
    if (iy > g.n[1] - 2) iy = g.n[1] - 2;
    if (iz > g.n[2] - 2) iz = g.n[2] - 2;
    const double fx = ux - (double)ix, fy = uy - (double)iy, fz = uz - (double)iz;
    const int sy = g.n[2], sx = g.n[1] * g.n[2];
    const float *v = g.values + ((ix * g.n[1] + iy) * g.n[2] + iz);
    const double v000 = (double)v[0], v001 = (double)v[1];
    const double v010 = (double)v[sy], v011 = (double)v[sy + 1];
    const double v100 = (double)v[sx], v101 = (double)v[sx + 1];
    const double v110 = (double)v[sx + sy], v111 = (double)v[sx + sy + 1];
    const double c00 = v000 + fz * (v001 - v000);
    const double c01 = v010 + fz * (v011 - v010);
    const double c10 = v100 + fz * (v101 - v100);
    const double c11 = v110 + fz * (v111 - v110);
    const double c0 = c00 + fy * (c01 - c00);
    const double c1 = c10 + fy * (c11 - c10);
    return c0 + fx * (c1 - c0);
}

// Step 4, the grid term of a robot sphere (centre p, radius r, speed lam): its distance d (+inf outside) and advance.
OPTIK_CM_HD inline void grid_term(const double *p, double r, const coll::Grid &g, double m, double mp, double G,
                                  double lam, double &d, double &adv) {
    const double ux = (p[0] - g.origin[0]) * g.inv;
    const double uy = (p[1] - g.origin[1]) * g.inv;
    const double uz = (p[2] - g.origin[2]) * g.inv;
    const double hx = (double)(g.n[0] - 1), hy = (double)(g.n[1] - 1), hz = (double)(g.n[2] - 1);
    const bool inside = ux >= 0.0 && ux <= hx && uy >= 0.0 && uy <= hy && uz >= 0.0 && uz <= hz;
    if (inside) {
        d = coll::grid_distance(p, r, g);
        adv = term_advance(d, m, mp, G * lam);
        return;
    }
    d = inf();
    const double gv = grid_value(fmin(fmax(ux, 0.0), hx), fmin(fmax(uy, 0.0), hy), fmin(fmax(uz, 0.0), hz), g);
    const double ex = fmax(fmax(0.0 - ux, ux - hx), 0.0);
    const double ey = fmax(fmax(0.0 - uy, uy - hy), 0.0);
    const double ez = fmax(fmax(0.0 - uz, uz - hz), 0.0);
    const double dbox = sqrt((ex * ex + ey * ey) + ez * ez) / g.inv;
    const double num = fmax(dbox, ((gv - r) - mp) / G);
    adv = lam == 0.0 ? inf() : num / lam;
}

// Step 6.
struct Walk {
    double t;          // the t of the sample to evaluate next
    double clearance;  // the minimum c so far
    double t_stop;
    int32_t steps;     // samples evaluated
    int32_t status;    // -1 while walking
};

OPTIK_CM_HD inline void walk_begin(Walk &w) {
    w.t = 0.0;
    w.clearance = inf();
    w.t_stop = 0.0;
    w.steps = 0;
    w.status = -1;
}

// A segment that is not walked (a NaN or infinite joint).
OPTIK_CM_HD inline void walk_refuse(Walk &w) {
    w.t = qnan();
    w.clearance = qnan();
    w.t_stop = qnan();
    w.steps = 0;
    w.status = NOT_A_NUMBER;
}

// The sample at w.t has been evaluated: nan (a NaN frame), otherwise its clearance c and advance A.  Returns whether
// the walk goes on; then w.t is the next sample's t.
OPTIK_CM_HD inline bool walk_take(Walk &w, bool nan, double c, double A, double m, int max_steps) {
    w.steps += 1;
    w.t_stop = w.t;
    if (nan) { w.status = NOT_A_NUMBER; w.clearance = qnan(); return false; }
    w.clearance = fmin(w.clearance, c);
    if (!(c >= m)) { w.status = BLOCKED; return false; }
    if (w.t == 1.0) { w.status = FREE; return false; }
    if (w.steps == max_steps) { w.status = LIMIT; return false; }
    double tn = w.t + A;
    if (tn >= 1.0) tn = 1.0;
    w.t = tn;
    return true;
}

// Steps 4 and 5, the reference form (the tests' g++ driver): the sample's clearance c and advance A from its frames
// [nf][7], in the caller's numbering of spheres and pairs (terms in collision_measure.hpp's clearance() order, then the
// grid terms).  Returns false, and leaves c and A alone, when a frame holds a NaN.  a [n]; reach: Reach::r, flat.
inline bool sample_terms(int n, const double *frames, int S, const int32_t *frame, const double *centers,
                         const double *radii, int P, const int32_t *pairs, int Ms, const double *wspheres, int Mb,
                         const double *wboxes, const coll::Grid &grid, const double *a, const double *reach,
                         double m, double tol, double G, double &c_out, double &A_out) {
    const int nf = n + 2;
    for (int f = 0; f < nf; ++f)
        if (coll::pose_has_nan(frames + 7 * f)) return false;
    const double mp = m - tol;
    double c = inf(), A = inf();
    for (int s = 0; s < S; ++s) {
        double p[3];
        coll::sphere_centre(frames + 7 * frame[s], centers + 3 * s, p);
        const double lam = lam_sphere(n, frame[s], a, reach, norm3(centers + 3 * s));
        for (int k = 0; k < Ms; ++k) {
            const double d = coll::sphere_sphere(p, radii[s], wspheres + 4 * k, wspheres[4 * k + 3]);
            c = fmin(c, d);
            A = fmin(A, term_advance(d, m, mp, lam));
        }
        for (int k = 0; k < Mb; ++k) {
            const double d = coll::sphere_box(p, radii[s], wboxes + 10 * k);
            c = fmin(c, d);
            A = fmin(A, term_advance(d, m, mp, lam));
        }
    }
    for (int k = 0; k < P; ++k) {
        const int x = pairs[2 * k], y = pairs[2 * k + 1];
        double px[3], py[3];
        coll::sphere_centre(frames + 7 * frame[x], centers + 3 * x, px);
        coll::sphere_centre(frames + 7 * frame[y], centers + 3 * y, py);
        const double d = coll::sphere_sphere(px, radii[x], py, radii[y]);
        const double lam = pair_lam(n, frame[x], norm3(centers + 3 * x), frame[y], norm3(centers + 3 * y), a, reach);
        c = fmin(c, d);
        A = fmin(A, term_advance(d, m, mp, lam));
    }
    if (grid.values)
        for (int s = 0; s < S; ++s) {
            double p[3], d, adv;
            coll::sphere_centre(frames + 7 * frame[s], centers + 3 * s, p);
            grid_term(p, radii[s], grid, m, mp, G, lam_sphere(n, frame[s], a, reach, norm3(centers + 3 * s)), d, adv);
            c = fmin(c, d);
            A = fmin(A, adv);
        }
    c_out = c;
    A_out = A;
    return true;
}

}  // namespace advance
}  // namespace optik
