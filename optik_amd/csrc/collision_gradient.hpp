// collision_gradient.hpp -- which term produced a clearance, and its derivative with respect to the joint positions:
// one source for the host and the device (optik_hip_collision_witness_batch, optik_hip_diff_ik_avoid_batch,
// optik_hip.h).  collision_measure.hpp answers "how far"; this header answers "from what, and
// which way is out".
//
// A configuration of an n-joint revolute chain has F = n + 2 frames (collision_measure.hpp).  Its witness table has
// one row per frame f: the smallest term among
//     every (robot sphere on frame f, world sphere), every (robot sphere on frame f, world box), the grid term of
//     every robot sphere on frame f, and every self pair (a, b) with max(frame[a], frame[b]) == f.
// Ties go to the first term in this enumeration: spheres ascending, for each sphere the world spheres, the boxes, the
// grid; then the pairs in stored order.  "Smaller" is d < best, so +inf terms (a sphere outside the grid) never win.
// Every distance is the value collision_measure.hpp computes for the term (its functions are called, not restated),
// so the minimum over the rows is clearance / clearance_grid bit for bit.
//
// A row holds dist, the witness (robot sphere, kind, index) -- kind 0 world sphere, 1 box, 2 grid (index 0), 3 self
// pair (robot sphere = a, index = the pair's index) -- and grad[n] = d dist / d q.  A row without a term: dist +inf,
// grad 0, witness (-1, -1, -1).  Any NaN frame: every row dist NaN, grad NaN, witness -1.
//
// The exact operation order (both sides: -ffp-contract=off, only + - * / sqrt fabs fmin fmax floor):
//
//  1. The point: p = sphere_centre(frame f, c) (collision_measure.hpp, step 1).
//  2. The normal nrm, the derivative of the distance with respect to p:
//       sphere (and pair, with c = the other centre):  dx = p.x - c.x (dy, dz alike);
//           l = sqrt((dx * dx + dy * dy) + dz * dz);  nrm = (dx / l, dy / l, dz / l), or 0 when l == 0
//       box: l, e_i, o_i = fmax(e_i, 0), outside as in step 3 of collision_measure.hpp; sign(x) = x < 0 ? -1 : 1
//           outside > 0:  m_i = (sign(l_i) * o_i) / outside
//           otherwise:    m = sign(l_k) on the first axis k with the largest e_k, 0 on the other two
//           nrm = qrot(q_b, m)
//       grid: the cell, f_a and the eight v_xyz of step 5 of collision_measure.hpp (only called when that term is
//           finite), then
//           gx = c_1 - c_0
//           gy = y_0 + f_x * (y_1 - y_0),   y_x = c_x1 - c_x0
//           gz = z_0 + f_x * (z_1 - z_0),   z_x = z_x0 + f_y * (z_x1 - z_x0),   z_xy = v_xy1 - v_xy0
//           nrm = (gx * inv, gy * inv, gz * inv)      (the field's own slope: not a unit vector)
//  3. Joint j (1 <= j <= n) turns about a_j = qrot(quaternion of frame j, local axis of joint j) through
//     o_j = the translation of frame j (ik_eval.hpp: a joint's frame is its origin, then its rotation; the rotation is
//     about the local axis, so the axis is the same before and after it).  A point p on frame f moves by
//         dp/dq_j = a_j x (p - o_j)   for j <= f,   0 for j > f
//     with r = p - o_j component by component and a x r = (a.y * r.z - a.z * r.y, a.z * r.x - a.x * r.z,
//     a.x * r.y - a.y * r.x).
//  4. grad_j = (nrm.x * w.x + nrm.y * w.y) + nrm.z * w.z with w = dp/dq_j; for a pair w = dpa/dq_j - dpb/dq_j
//     component by component (each side 0 beyond its own frame).  A j beyond the row's frame gives exactly 0.
//
// Plain host C++ compiles this header too (no HIP runtime): tests/avoid_util.py drives witness_rows with g++.
#pragma once

#include "collision_measure.hpp"

namespace optik {
namespace coll {

enum : int { WIT_SPHERE = 0, WIT_BOX = 1, WIT_GRID = 2, WIT_PAIR = 3 };

OPTIK_CM_HD inline double sign1(double x) { return x < 0.0 ? -1.0 : 1.0; }

// Step 2, sphere and pair.
OPTIK_CM_HD inline void sphere_normal(const double *p, const double *c, double *nrm) {
    const double dx = p[0] - c[0], dy = p[1] - c[1], dz = p[2] - c[2];
    const double l = sqrt((dx * dx + dy * dy) + dz * dz);
    if (l == 0.0) {
        nrm[0] = 0.0; nrm[1] = 0.0; nrm[2] = 0.0;
    } else {
        nrm[0] = dx / l; nrm[1] = dy / l; nrm[2] = dz / l;
    }
}

// Step 2, box.
OPTIK_CM_HD inline void box_normal(const double *p, const double *box10, double *nrm) {
    const double d[3] = {p[0] - box10[0], p[1] - box10[1], p[2] - box10[2]};
    const double qc[4] = {-box10[3], -box10[4], -box10[5], box10[6]};
    double l[3];
    qrot3(qc, d, l);
    const double e0 = fabs(l[0]) - box10[7], e1 = fabs(l[1]) - box10[8], e2 = fabs(l[2]) - box10[9];
    const double o0 = fmax(e0, 0.0), o1 = fmax(e1, 0.0), o2 = fmax(e2, 0.0);
    const double outside = sqrt((o0 * o0 + o1 * o1) + o2 * o2);
    double m[3];
    if (outside > 0.0) {
        m[0] = (sign1(l[0]) * o0) / outside;
        m[1] = (sign1(l[1]) * o1) / outside;
        m[2] = (sign1(l[2]) * o2) / outside;
    } else {
        m[0] = 0.0; m[1] = 0.0; m[2] = 0.0;
        if (e0 >= e1 && e0 >= e2) m[0] = sign1(l[0]);
        else if (e1 >= e2) m[1] = sign1(l[1]);
        else m[2] = sign1(l[2]);
    }
    qrot3(box10 + 3, m, nrm);
}

// Step 2, grid: only for a p whose grid term is finite (inside the grid).
OPTIK_CM_HD inline void grid_normal(const double *p, const Grid &g, double *nrm) {
    const double ux = (p[0] - g.origin[0]) * g.inv;
    const double uy = (p[1] - g.origin[1]) * g.inv;
    const double uz = (p[2] - g.origin[2]) * g.inv;
    int ix = (int)floor(ux), iy = (int)floor(uy), iz = (int)floor(uz);
    if (ix > g.n[0] - 2) ix = g.n[0] - 2;
    if (iy > g.n[1] - 2) iy = g.n[1] - 2;
    if (iz > g.n[2] - 2) iz = g.n[2] - 2;
    if (ix < 0) ix = 0;  // (never taken for a finite term: keeps a misuse inside the array)
    if (iy < 0) iy = 0;
    if (iz < 0) iz = 0;
    const double fx = ux - (double)ix, fy = uy - (double)iy, fz = uz - (double)iz;
    const int sy = g.n[2], sx = g.n[1] * g.n[2];
    const float *v = g.values + ((ix * g.n[1] + iy) * g.n[2] + iz);
    const double v000 = (double)v[0], v001 = (double)v[1];
    const double v010 = (double)v[sy], v011 = (double)v[sy + 1];
    const double v100 = (double)v[sx], v101 = (double)v[sx + 1];
    const double v110 = (double)v[sx + sy], v111 = (double)v[sx + sy + 1];
    const double z00 = v001 - v000, z01 = v011 - v010, z10 = v101 - v100, z11 = v111 - v110;
    const double c00 = v000 + fz * z00;
    const double c01 = v010 + fz * z01;
    const double c10 = v100 + fz * z10;
    const double c11 = v110 + fz * z11;
    const double y0 = c01 - c00, y1 = c11 - c10;
    const double c0 = c00 + fy * y0;
    const double c1 = c10 + fy * y1;
    const double gx = c1 - c0;
    const double gy = y0 + fx * (y1 - y0);
    const double z0 = z00 + fy * (z01 - z00);
    const double z1 = z10 + fy * (z11 - z10);
    const double gz = z0 + fx * (z1 - z0);
    nrm[0] = gx * g.inv; nrm[1] = gy * g.inv; nrm[2] = gz * g.inv;
}

// Step 3: w = a x (p - o).
OPTIK_CM_HD inline void point_velocity(const double *a, const double *o, const double *p, double *w) {
    const double rx = p[0] - o[0], ry = p[1] - o[1], rz = p[2] - o[2];
    w[0] = a[1] * rz - a[2] * ry;
    w[1] = a[2] * rx - a[0] * rz;
    w[2] = a[0] * ry - a[1] * rx;
}

OPTIK_CM_HD inline double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// One (robot sphere, obstacle) witness.  What the caller resolved: the sphere's frame f and its pose fp, its centre c
// in that frame, the kind and the obstacle (a world sphere's 4 doubles, a box's 10; ignored for the grid).
// joint_of(j, a, o) gives a_j and o_j of step 3 for j = 1 .. n; gsink(j - 1, grad_j) takes the n components.
template <class JointFn, class GSink>
OPTIK_CM_HD inline void world_term_gradient(int n, int f, const double *fp, const double *c, int kind,
                                            const double *obstacle, const Grid &grid, JointFn &&joint_of,
                                            GSink &&gsink) {
    double p[3], nrm[3];
    sphere_centre(fp, c, p);
    if (kind == WIT_SPHERE) sphere_normal(p, obstacle, nrm);
    else if (kind == WIT_BOX) box_normal(p, obstacle, nrm);
    else grid_normal(p, grid, nrm);
    for (int j = 1; j <= n; ++j) {
        double g = 0.0;
        if (j <= f) {
            double a[3], o[3], w[3];
            joint_of(j, a, o);
            point_velocity(a, o, p, w);
            g = dot3(nrm, w);
        }
        gsink(j - 1, g);
    }
}

// One self-pair witness: sphere a (frame fa, pose fpa, centre ca) against sphere b.
template <class JointFn, class GSink>
OPTIK_CM_HD inline void pair_term_gradient(int n, int fa, const double *fpa, const double *ca, int fb,
                                           const double *fpb, const double *cb, JointFn &&joint_of, GSink &&gsink) {
    double pa[3], pb[3], nrm[3];
    sphere_centre(fpa, ca, pa);
    sphere_centre(fpb, cb, pb);
    sphere_normal(pa, pb, nrm);
    for (int j = 1; j <= n; ++j) {
        double g = 0.0;
        if (j <= fa || j <= fb) {
            double a[3], o[3], wa[3] = {0.0, 0.0, 0.0}, wb[3] = {0.0, 0.0, 0.0}, w[3];
            joint_of(j, a, o);
            if (j <= fa) point_velocity(a, o, pa, wa);
            if (j <= fb) point_velocity(a, o, pb, wb);
            w[0] = wa[0] - wb[0]; w[1] = wa[1] - wb[1]; w[2] = wa[2] - wb[2];
            g = dot3(nrm, w);
        }
        gsink(j - 1, g);
    }
}

// The velocity-damper rows of collision-avoiding diff_ik (diff_ik_lp.hpp: diff_ik_lp_damped).  A row f is active when
// its dist is finite and < influence; at most 4 are kept, the smallest, ties to the lower frame, in ascending order of
// (dist, frame).  dist_of(f) gives row f's dist; sel[4] receives the frames (-1: unused).  Returns how many.
template <class DistFn>
OPTIK_CM_HD inline int select_damper_rows(int nf, double influence, DistFn &&dist_of, int (&sel)[4]) {
    double sd[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
    sel[0] = -1; sel[1] = -1; sel[2] = -1; sel[3] = -1;
    for (int f = 0; f < nf; ++f) {
        double cd = dist_of(f);
        if (!(cd < influence) || !(cd > -INFINITY)) continue;
        int cf = f;
        // insertion ordered by (dist, frame): an element pushed down by a closer one must still pass an equal one of a
        // higher frame below it.  (An empty slot holds +inf: a finite cd always drops into it)
        for (int k = 0; k < 4; ++k)
            if (cd < sd[k] || (cd == sd[k] && cf < sel[k])) {
                const double td = sd[k]; sd[k] = cd; cd = td;
                const int tf = sel[k]; sel[k] = cf; cf = tf;
            }
    }
    return (sel[0] >= 0) + (sel[1] >= 0) + (sel[2] >= 0) + (sel[3] >= 0);
}

// h of the damper row of a term at distance d:  ((-gain) * (d - safety)) / (influence - safety).
OPTIK_CM_HD inline double damper_rhs(double d, double influence, double safety, double gain) {
    return (-gain * (d - safety)) / (influence - safety);
}

// The reference form (the tests' g++ driver): frames [n + 2][7]; axes [n][3], the local axis of joint j at j - 1;
// the model and world as clearance() takes them, the grid as clearance_grid() does (values null: none).
// Out: dist [n + 2], witness [n + 2][3], grad [n + 2][n].
inline void witness_rows(int n, const double *frames, const double *axes, int S, const int32_t *frame,
                         const double *centers, const double *radii, int P, const int32_t *pairs, int Ms,
                         const double *wspheres, int Mb, const double *wboxes, const Grid &grid, double *dist,
                         int32_t *witness, double *grad) {
    const int nf = n + 2;
    bool nan = false;
    for (int f = 0; f < nf; ++f) nan = nan || pose_has_nan(frames + 7 * f);
    for (int f = 0; f < nf; ++f) {
        dist[f] = nan ? NAN : INFINITY;
        for (int k = 0; k < 3; ++k) witness[3 * f + k] = -1;
        for (int j = 0; j < n; ++j) grad[f * n + j] = nan ? NAN : 0.0;
    }
    if (nan) return;
    auto take = [&](int f, double d, int s, int kind, int idx) {
        if (d < dist[f]) {
            dist[f] = d;
            witness[3 * f] = s; witness[3 * f + 1] = kind; witness[3 * f + 2] = idx;
        }
    };
    for (int s = 0; s < S; ++s) {
        double p[3];
        sphere_centre(frames + 7 * frame[s], centers + 3 * s, p);
        for (int m = 0; m < Ms; ++m)
            take(frame[s], sphere_sphere(p, radii[s], wspheres + 4 * m, wspheres[4 * m + 3]), s, WIT_SPHERE, m);
        for (int m = 0; m < Mb; ++m) take(frame[s], sphere_box(p, radii[s], wboxes + 10 * m), s, WIT_BOX, m);
        if (grid.values) take(frame[s], grid_distance(p, radii[s], grid), s, WIT_GRID, 0);
    }
    for (int k = 0; k < P; ++k) {
        const int a = pairs[2 * k], b = pairs[2 * k + 1];
        double pa[3], pb[3];
        sphere_centre(frames + 7 * frame[a], centers + 3 * a, pa);
        sphere_centre(frames + 7 * frame[b], centers + 3 * b, pb);
        take(frame[a] > frame[b] ? frame[a] : frame[b], sphere_sphere(pa, radii[a], pb, radii[b]), a, WIT_PAIR, k);
    }
    auto joint_of = [&](int j, double *a, double *o) {
        qrot3(frames + 7 * j + 3, axes + 3 * (j - 1), a);
        o[0] = frames[7 * j]; o[1] = frames[7 * j + 1]; o[2] = frames[7 * j + 2];
    };
    for (int f = 0; f < nf; ++f) {
        const int s = witness[3 * f], kind = witness[3 * f + 1], idx = witness[3 * f + 2];
        if (s < 0) continue;
        auto gsink = [&](int j, double g) { grad[f * n + j] = g; };
        if (kind == WIT_PAIR) {
            const int b = pairs[2 * idx + 1];
            pair_term_gradient(n, frame[s], frames + 7 * frame[s], centers + 3 * s, frame[b], frames + 7 * frame[b],
                               centers + 3 * b, joint_of, gsink);
        } else {
            const double *obstacle =
                kind == WIT_SPHERE ? wspheres + 4 * idx : (kind == WIT_BOX ? wboxes + 10 * idx : nullptr);
            world_term_gradient(n, f, frames + 7 * f, centers + 3 * s, kind, obstacle, grid, joint_of, gsink);
        }
    }
}

}  // namespace coll
}  // namespace optik
