// collision_measure.hpp -- the signed distances of the collision filter, one source for the host and the device
// (optik_hip_collision_batch and the key pass of a chain with a collision model, optik_hip.h).
//
// The robot is a set of spheres, each fixed in one frame of the chain; the world is a set of spheres and oriented boxes
// in the base frame.  A pose is 7 doubles: t (3), then the unit quaternion i, j, k, w.  A chain of n joint positions
// has n + 2 frames: 0 the base (identity), k = 1 .. n the pose after joint k's motion, n + 1 the end effector (with the
// tip joint and the call's ee_offset: the pose fk_batch returns).
//
// The exact operation order (the tests depend on it; both sides are compiled with -ffp-contract=off and use only
// the correctly rounded + - * / sqrt, fabs and fmin / fmax, so one source gives one set of bits wherever it runs):
//
//  1. A robot sphere's centre in the base frame: p = t_f + qrot(q_f, c), component by component t_f.x + r.x, where
//     qrot is ik_math.hpp's (nalgebra's) order: u = 2 * (v x c) (the cross product first, then each component times
//     2.0), w = v x u, r = (u * q.w + w) + c, with v = (q.i, q.j, q.k).
//  2. Sphere to sphere, a = the robot sphere (or the first sphere of a self pair), b = the other:
//         dx = a.x - b.x (dy, dz alike);  d = ((sqrt((dx * dx + dy * dy) + dz * dz) - r_a) - r_b)
//  3. Sphere (centre p, radius r) to box (t_b, unit q_b, half extents h):
//         l = qrot(conj(q_b), p - t_b)  (p - t_b component by component; conj = (-i, -j, -k, w))
//         e_i = fabs(l_i) - h_i
//         outside = sqrt((fmax(e0, 0)^2 + fmax(e1, 0)^2) + fmax(e2, 0)^2)   (x^2 = x * x)
//         inside  = fmin(fmax(fmax(e0, e1), e2), 0)
//         d = (outside + inside) - r
//  4. The clearance of a configuration is the minimum of every (robot sphere, world sphere), every (robot sphere,
//     world box) and every self-pair distance; +inf when there is nothing to check; NaN when any frame holds a NaN
//     (every frame after a NaN joint position does).  The configuration is free iff clearance >= margin.
//
// The minimum is exact in any order: every term is computed on its own from the frames, so a pass that visits the
// terms in another order -- the device groups the spheres by frame and the pairs by frame pair -- gets the same
// value, and a pass that only classifies (the key pass) may stop at the first term below the margin: it decides
// "not free" exactly as the full clearance does.  Terms are never NaN once the frames are not (the inputs are
// refused unless centres are finite and radii / half extents are >= 0; +inf radii give -inf).
//
//
// The distance-field world: a third obstacle kind, a sampled signed distance field on an
// axis-aligned grid in the base frame.  Node (i, j, k) sits at origin_a + voxel * (double)i_a per axis; values are
// float32 [nx][ny][nz] in C order (z fastest), every one finite; each of nx, ny, nz is in 2 .. 1024 and nx * ny * nz
// <= 2^24; voxel > 0 and finite.  The host stores inv = 1.0 / voxel once and both sides multiply by it.  All
// arithmetic is f64 (f32 -> f64 is exact).
//
//  5. The grid term of a robot sphere (centre p, radius r), per axis a with n_a nodes:
//         u_a = (p_a - origin_a) * inv
//     unless 0.0 <= u_a <= (double)(n_a - 1) on all three axes the grid says nothing about the sphere: +inf (a NaN
//     u_a fails the test, so a NaN centre reads nothing).  Otherwise
//         i_a = min((int)floor(u_a), n_a - 2);  f_a = u_a - (double)i_a      (u_a = n_a - 1: cell n_a - 2, f_a = 1)
//         v_xyz = (double)values[i_x + x][i_y + y][i_z + z],  x, y, z in {0, 1}
//         along z:  c_xy = v_xy0 + f_z * (v_xy1 - v_xy0)
//         along y:  c_x  = c_x0 + f_y * (c_x1 - c_x0)
//         along x:  c    = c_0 + f_x * (c_1 - c_0)
//         d = c - r
//  6. With a grid the clearance of step 4 is the minimum of its terms and the S grid terms; NaN frames still give
//     NaN, free is still clearance >= margin.  clearance() below keeps its signature (steps 1 - 4);
//     clearance_grid() is the minimum of the grid terms alone, and the two are combined with fmin.
//  7. The bake: the world's signed distance at a point p, primitive_field, is the minimum over the world of
//     sphere_sphere(p, 0, c, r) and sphere_box(p, 0, box) (spheres first, then boxes); the baked value of a node is
//     (float)primitive_field(node) (round to nearest even), the node at origin_a + voxel * (double)i_a.
//
// The interpolated field approximates: for a 1-Lipschitz field it is a convex combination of corners within one cell
// diagonal of p, so within sqrt(3) * voxel of the true distance, plus the f32 rounding of the values.
//
//
// From sensor data to that grid: an occupancy grid is turned into a signed field by an
// exact Euclidean distance transform, and a point cloud is turned into an occupancy grid.  `occupied` is uint8
// [nx][ny][nz] on the nodes of a grid as above (z fastest), non-zero = occupied.
//
//  8. The signed field of an occupancy grid.  For a node p, D2_occ(p) is the minimum over the occupied nodes q of the
//     squared distance in voxel units, (i_p - i_q)^2 + (j_p - j_q)^2 + (k_p - k_q)^2, an exact integer of at most
//     3 * 1023^2; D2_free(p) is the same over the free nodes.  max_distance is finite and > 0.
//         free node:      s = voxel * (sqrt((double)D2_occ) - 0.5)
//         occupied node:  s = -(voxel * (sqrt((double)D2_free) - 0.5))
//         a free node of a grid without occupied nodes:  s = +max_distance  (assigned, no arithmetic on a sentinel)
//         an occupied node of a grid without free nodes: s = -max_distance  (likewise)
//         value = (float)fmax(fmin(s, max_distance), -max_distance)
//     The zero level lies midway between a free node and an occupied neighbour (+voxel/2 and -voxel/2), and every
//     value is finite.  D2 is computed separably and exactly in int32 (edt_scan below): three passes, along z, y and
//     x, each out[i] = min_j in[j] + (j - i)^2 along its lines, both fields at once.  The first pass reads
//     in = 0 at the nodes of the field's own set and EDT_NONE = 2^30 elsewhere.  The candidate j = i is always
//     taken, so no pass ever stores more than EDT_NONE, and the largest sum formed is 2^30 + 1023^2 < 2^31.  A node
//     still at EDT_NONE after the third pass has no node of that set anywhere in the grid.  D2 is neither capped
//     nor is the search bounded by a window of max_distance: every D2 is the exact one.
//  9. Voxelization of a point cloud.  A point p (base frame) has, per axis a,
//         u_a = (p_a - origin_a) * inv;  w_a = u_a + 0.5
//     and lies inside iff w_a >= 0.0 && w_a < (double)n_a on all three axes (a NaN fails and the point is skipped;
//     so is an infinite one).  Its node is i_a = (int)floor(w_a): the nearest node, halves up.  With E exclusion
//     spheres (c, r) in the base frame the point is dropped iff, for any of them, with dx = p_x - c_x (dy, dz alike),
//         ((dx * dx + dy * dy) + dz * dz) <= r * r          (a NaN sphere excludes nothing)
//     A kept point sets occupied[i_x][i_y][i_z] = 1.  Nothing is ever cleared: clouds accumulate in one buffer.
//
// What the field of step 8 is not: it takes an occupied voxel for its node, a point.  The true distance from p to the
// occupied voxel CUBES (side voxel, centred on their nodes) lies between dist_node - (sqrt(3)/2) * voxel and dist_node
// - voxel/2, where dist_node = voxel * sqrt(D2_occ); the field's voxel * (sqrt(D2_occ) - 0.5) is the upper end of that
// range, so it is optimistic by up to ((sqrt(3) - 1) / 2) * voxel = 0.366 * voxel.  The trilinear bound above comes on
// top: a caller who needs a conservative answer adds (sqrt(3) + (sqrt(3) - 1) / 2) * voxel = 2.098 * voxel to the
// margin (and whatever the sensor's own error is).  The arithmetic does not hide any of this.
//
// Plain host C++ compiles this header too (no HIP runtime): tests/test_collision_host.py,
// tests/test_world_grid_host.py and tests/test_world_occupancy_host.py drive it with g++.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OPTIK_CM_HD __host__ __device__
#else
#define OPTIK_CM_HD
#endif

namespace optik {
namespace coll {

// qrot of ik_math.hpp, restated for plain C++: r' = (u * w + (v x u)) + r with u = 2 (v x r).
OPTIK_CM_HD inline void qrot3(const double *q, const double *r, double *o) {
    const double vx = q[0], vy = q[1], vz = q[2], w = q[3];
    double ux = vy * r[2] - vz * r[1], uy = vz * r[0] - vx * r[2], uz = vx * r[1] - vy * r[0];
    ux *= 2.0; uy *= 2.0; uz *= 2.0;
    const double cx = vy * uz - vz * uy, cy = vz * ux - vx * uz, cz = vx * uy - vy * ux;
    o[0] = ux * w + cx + r[0];
    o[1] = uy * w + cy + r[1];
    o[2] = uz * w + cz + r[2];
}

// Step 1: the centre c (in the frame of pose7) in the base frame.
OPTIK_CM_HD inline void sphere_centre(const double *pose7, const double *c, double *p) {
    double r[3];
    qrot3(pose7 + 3, c, r);
    p[0] = pose7[0] + r[0];
    p[1] = pose7[1] + r[1];
    p[2] = pose7[2] + r[2];
}

// Step 2.
OPTIK_CM_HD inline double sphere_sphere(const double *a, double ra, const double *b, double rb) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrt((dx * dx + dy * dy) + dz * dz) - ra - rb;
}

// Step 3.  box10 = t (3), q (4: i, j, k, w), half extents (3).
OPTIK_CM_HD inline double sphere_box(const double *p, double r, const double *box10) {
    const double d[3] = {p[0] - box10[0], p[1] - box10[1], p[2] - box10[2]};
    const double qc[4] = {-box10[3], -box10[4], -box10[5], box10[6]};
    double l[3];
    qrot3(qc, d, l);
    const double e0 = fabs(l[0]) - box10[7], e1 = fabs(l[1]) - box10[8], e2 = fabs(l[2]) - box10[9];
    const double o0 = fmax(e0, 0.0), o1 = fmax(e1, 0.0), o2 = fmax(e2, 0.0);
    const double outside = sqrt((o0 * o0 + o1 * o1) + o2 * o2);
    const double inside = fmin(fmax(fmax(e0, e1), e2), 0.0);
    return (outside + inside) - r;
}

// The distance-field world as both sides see it (values: host memory for the host, device memory for the device).
struct Grid {
    const float *values;  // [n[0]][n[1]][n[2]], z fastest; null: no grid
    double origin[3];
    double inv;           // 1.0 / voxel
    int32_t n[3];
};

// Step 5.
OPTIK_CM_HD inline double grid_distance(const double *p, double r, const Grid &g) {
    const double ux = (p[0] - g.origin[0]) * g.inv;
    const double uy = (p[1] - g.origin[1]) * g.inv;
    const double uz = (p[2] - g.origin[2]) * g.inv;
    const bool inside = ux >= 0.0 && ux <= (double)(g.n[0] - 1) && uy >= 0.0 && uy <= (double)(g.n[1] - 1)
                        && uz >= 0.0 && uz <= (double)(g.n[2] - 1);
    if (!inside) return INFINITY;
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
    const double c = c0 + fx * (c1 - c0);
    return c - r;
}

// Step 7: the world's signed distance at p, and the position of node (i, j, k).
OPTIK_CM_HD inline double primitive_field(const double *p, const double *spheres, int Ms, const double *boxes,
                                          int Mb) {
    double c = INFINITY;
    for (int m = 0; m < Ms; ++m) c = fmin(c, sphere_sphere(p, 0.0, spheres + 4 * m, spheres[4 * m + 3]));
    for (int m = 0; m < Mb; ++m) c = fmin(c, sphere_box(p, 0.0, boxes + 10 * m));
    return c;
}

OPTIK_CM_HD inline void grid_node(const double *origin, double voxel, int i, int j, int k, double *p) {
    p[0] = origin[0] + voxel * (double)i;
    p[1] = origin[1] + voxel * (double)j;
    p[2] = origin[2] + voxel * (double)k;
}

// Step 8.  The squared distances of one node to both node sets, in voxel units.
struct alignas(8) EdtPair {
    int32_t occ;    // to the nearest occupied node
    int32_t free_;  // to the nearest free node
};
constexpr int32_t EDT_NONE = 1 << 30;  // no node of the set seen so far

// What the first pass reads at a node.
OPTIK_CM_HD inline EdtPair edt_source(uint8_t occupied) {
    return occupied ? EdtPair{0, EDT_NONE} : EdtPair{EDT_NONE, 0};
}

// One node of one pass: min_j in(j) + (j - i)^2 over the line's nodes j = 0 .. n - 1, for both fields.  in(j) >= 0,
// so a candidate at distance t is at least t^2: the scan walks outward from i and stops once t^2 reaches the larger
// of the two minima (or both ends of the line).  Exact; t <= 1023, in(j) <= 2^30.
template <class In>
OPTIK_CM_HD inline EdtPair edt_scan(const In &in, int i, int n) {
    EdtPair best = in(i);
    for (int t = 1; t < n; ++t) {
        const int32_t tt = t * t;
        if (tt >= (best.occ > best.free_ ? best.occ : best.free_)) break;
        const bool lo = i - t >= 0, hi = i + t < n;
        if (!lo && !hi) break;
        if (lo) {
            const EdtPair v = in(i - t);
            if (v.occ + tt < best.occ) best.occ = v.occ + tt;
            if (v.free_ + tt < best.free_) best.free_ = v.free_ + tt;
        }
        if (hi) {
            const EdtPair v = in(i + t);
            if (v.occ + tt < best.occ) best.occ = v.occ + tt;
            if (v.free_ + tt < best.free_) best.free_ = v.free_ + tt;
        }
    }
    return best;
}

// The value of a node from its two squared distances after the third pass.
OPTIK_CM_HD inline float occupancy_value(uint8_t occupied, EdtPair d2, double voxel, double max_distance) {
    double s;
    if (occupied) {
        if (d2.free_ >= EDT_NONE) s = -max_distance;
        else s = -(voxel * (sqrt((double)d2.free_) - 0.5));
    } else {
        if (d2.occ >= EDT_NONE) s = max_distance;
        else s = voxel * (sqrt((double)d2.occ) - 0.5);
    }
    return (float)fmax(fmin(s, max_distance), -max_distance);
}

// Step 9: the node of a point, or false (outside, NaN, infinite).
OPTIK_CM_HD inline bool point_node(const double *p, const double *origin, double inv, const int32_t *n, int *ijk) {
    const double wx = (p[0] - origin[0]) * inv + 0.5;
    const double wy = (p[1] - origin[1]) * inv + 0.5;
    const double wz = (p[2] - origin[2]) * inv + 0.5;
    const bool inside = wx >= 0.0 && wx < (double)n[0] && wy >= 0.0 && wy < (double)n[1]
                        && wz >= 0.0 && wz < (double)n[2];
    if (!inside) return false;
    ijk[0] = (int)floor(wx);
    ijk[1] = (int)floor(wy);
    ijk[2] = (int)floor(wz);
    return true;
}

// Step 9: does the exclusion sphere (c, r) = sphere4 drop the point?
OPTIK_CM_HD inline bool point_excluded(const double *p, const double *sphere4) {
    const double dx = p[0] - sphere4[0], dy = p[1] - sphere4[1], dz = p[2] - sphere4[2];
    return ((dx * dx + dy * dy) + dz * dz) <= sphere4[3] * sphere4[3];
}

OPTIK_CM_HD inline bool pose_has_nan(const double *pose7) {
    bool nan = false;
    for (int i = 0; i < 7; ++i) nan = nan || (pose7[i] != pose7[i]);
    return nan;
}

// Step 4, the reference form (the tests' g++ driver): frames [nf][7]; robot spheres: frame index, centre [S][3],
// radius [S]; self pairs [P][2]; world spheres [Ms][4] (centre, radius), boxes [Mb][10].  Terms in the order
// (sphere s, world spheres, world boxes) for s ascending, then the pairs.
inline double clearance(int nf, const double *frames, int S, const int32_t *frame, const double *centers,
                        const double *radii, int P, const int32_t *pairs, int Ms, const double *wspheres, int Mb,
                        const double *wboxes) {
    for (int f = 0; f < nf; ++f)
        if (pose_has_nan(frames + 7 * f)) return NAN;
    double c = INFINITY;
    for (int s = 0; s < S; ++s) {
        double p[3];
        sphere_centre(frames + 7 * frame[s], centers + 3 * s, p);
        for (int m = 0; m < Ms; ++m) c = fmin(c, sphere_sphere(p, radii[s], wspheres + 4 * m, wspheres[4 * m + 3]));
        for (int m = 0; m < Mb; ++m) c = fmin(c, sphere_box(p, radii[s], wboxes + 10 * m));
    }
    for (int k = 0; k < P; ++k) {
        const int a = pairs[2 * k], b = pairs[2 * k + 1];
        double pa[3], pb[3];
        sphere_centre(frames + 7 * frame[a], centers + 3 * a, pa);
        sphere_centre(frames + 7 * frame[b], centers + 3 * b, pb);
        c = fmin(c, sphere_sphere(pa, radii[a], pb, radii[b]));
    }
    return c;
}

// Step 6, the reference form: the minimum of the S grid terms (+inf without a grid or without spheres).
inline double clearance_grid(int nf, const double *frames, int S, const int32_t *frame, const double *centers,
                             const double *radii, const Grid &grid) {
    for (int f = 0; f < nf; ++f)
        if (pose_has_nan(frames + 7 * f)) return NAN;
    double c = INFINITY;
    if (!grid.values) return c;
    for (int s = 0; s < S; ++s) {
        double p[3];
        sphere_centre(frames + 7 * frame[s], centers + 3 * s, p);
        c = fmin(c, grid_distance(p, radii[s], grid));
    }
    return c;
}

// Step 8, the reference form: the three passes on the host.  a, b: workspace, nx * ny * nz pairs each.
inline void occupancy_field(const uint8_t *occupied, int nx, int ny, int nz, double voxel, double max_distance,
                            EdtPair *a, EdtPair *b, float *out) {
    const long long nodes = (long long)nx * ny * nz;
    const long long sy = nz, sx = (long long)ny * nz;
    for (long long p = 0; p < nodes; ++p) {
        const long long base = p - p % nz;
        a[p] = edt_scan([&](int j) { return edt_source(occupied[base + j]); }, (int)(p % nz), nz);
    }
    for (long long p = 0; p < nodes; ++p) {
        const int i = (int)(p / sy % ny);
        const long long base = p - i * sy;
        b[p] = edt_scan([&](int j) { return a[base + j * sy]; }, i, ny);
    }
    for (long long p = 0; p < nodes; ++p) {
        const int i = (int)(p / sx);
        const long long base = p - i * sx;
        a[p] = edt_scan([&](int j) { return b[base + j * sx]; }, i, nx);
    }
    for (long long p = 0; p < nodes; ++p) out[p] = occupancy_value(occupied[p], a[p], voxel, max_distance);
}

// Step 9, the reference form: marks and never clears.
inline void voxelize(const double *origin, double voxel, const int32_t *n, const double *points3, long long N,
                     const double *exclude4, int E, uint8_t *occupied) {
    const double inv = 1.0 / voxel;
    for (long long i = 0; i < N; ++i) {
        const double *p = points3 + 3 * i;
        int ijk[3];
        if (!point_node(p, origin, inv, n, ijk)) continue;
        bool drop = false;
        for (int e = 0; e < E && !drop; ++e) drop = point_excluded(p, exclude4 + 4 * e);
        if (!drop) occupied[((long long)ijk[0] * n[1] + ijk[1]) * n[2] + ijk[2]] = 1;
    }
}

}  // namespace coll
}  // namespace optik
