// mesh_measure.hpp -- the signed distance field of a triangle mesh, one source for the host and the device
// (optik_hip_world_grid_from_mesh, optik_hip.h).  A producer of the float32 [nx][ny][nz] values
// of the distance-field world of collision_measure.hpp (steps 5 - 7): it installs nothing.
//
// A mesh is a triangle soup, double [M][9]: the vertices a, b, c of each triangle in the base frame, every coordinate
// finite, 1 <= M <= MESH_MAX_TRIANGLES = 2^20.  No connectivity is used: vertices need not be welded, the surface may
// have holes, and zero-area triangles (real STL files hold them) are harmless.  The grid is collision_measure.hpp's:
// node (i, j, k) at p_a = origin_a + voxel * (double)i_a (step 7's grid_node).
//
// The exact operation order (the tests depend on it; both sides are compiled with -ffp-contract=off and use only the
// correctly rounded + - * / sqrt, fabs and fmin / fmax, comparisons and selects, so one source gives one set of bits
// wherever it runs).  dot(u, v) = (u.x * v.x + u.y * v.y) + u.z * v.z;  cross(u, v) = (u.y * v.z - u.z * v.y,
// u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x);  -u negates every component (exact).
//
//  1. Per (node p, triangle a b c), what distance and sign share:
//         A = a - p,  B = b - p,  C = c - p      (component by component; p - a = -A exactly)
//         e0 = b - a,  e1 = c - b,  e2 = a - c   (the edges in cyclic order, from the vertices themselves)
//  2. The squared distance to the segment from v along e (V = v - p), for (A, e0), (B, e1), (C, e2):
//         ee = dot(e, e);  t = -dot(V, e)
//         s = ee == 0.0 ? 0.0 : fmin(fmax(t / ee, 0.0), 1.0)
//         r = V + s * e  (r.x = V.x + s * e.x, ...);   seg = dot(r, r)
//     (this is |(p - v) - s * e|^2: r is its negative.)
//  3. The face:  n = cross(e0, -e2)  (= cross(b - a, c - a));  nn = dot(n, n).  It applies iff
//         nn > 0.0  and  dot(cross(A, e0), n) >= 0.0  and  dot(cross(B, e1), n) >= 0.0  and  dot(cross(C, e2), n) >= 0.0
//     (cross(V, e) = cross(e, p - v) exactly), and then  face = (h * h) / nn  with  h = dot(A, n).
//  4. The triangle's squared distance:  m = fmin(fmin(seg0, seg1), seg2), and  fmin(m, face)  where the face applies.
//     D2(p) = the fmin over all triangles, from +inf: exact in any order.  d = sqrt(D2).  No term can be NaN: a
//     zero-length edge takes s = 0 and a zero-area triangle has no face term.
//  5. The triangle's signed solid angle (Van Oosterom - Strackee), with la = sqrt(dot(A, A)), lb, lc alike:
//         num = dot(A, cross(B, C))
//         den = (((la * lb) * lc + dot(A, B) * lc) + dot(B, C) * la) + dot(C, A) * lb
//         Omega = 2.0 * atan2m(num, den)
//  6. atan2m(y, x), with q1 the fdlibm atan sequence of ik_math.hpp's atan2_q1 (y > 0, x >= 0), restated below so that
//     the solver's header stays as it is, and PI = 3.141592653589793:
//         y == 0.0:  x < 0.0 ? PI : 0.0            (num = den = 0 included: a vertex at the node adds nothing)
//         y > 0.0:   x >= 0.0 ? q1(y, x) : PI - q1(y, -x)
//         y < 0.0:   -(atan2m(-y, x))
//  7. W(p) = the sum of Omega over the triangles IN INDEX ORDER, serially from 0.0: W = W + Omega_t, t = 0 .. M - 1.
//     This order is part of the contract (the sum is not exact in another one): whoever computes a node walks all
//     triangles in order.  The generalized winding number is W / (4 pi); the node is inside iff
//         fabs(W) >= 6.283185307179586        (2 pi: |winding number| >= 1/2; fabs: inward-oriented files work too)
//  8. s = inside ? -d : d;   value = (float)fmax(fmin(s, max_distance), -max_distance),  max_distance finite and > 0.
//
// What this is: the true distance to the surface, so the only error left in the world is step 5's interpolation of
// collision_measure.hpp, sqrt(3) * voxel (plus the f32 rounding of the values).  What it is not: there is no culling
// and no hierarchy -- a field costs nodes * M evaluations of steps 1 - 5 -- and an open sheet has no inside: its
// winding number stays below 1/2 away from its rim, so it reads as an unsigned distance.
//
// Plain host C++ compiles this header too (no HIP runtime): tests/mesh_util.py drives it with g++.
#pragma once

#include <string>

#include "collision_measure.hpp"

namespace optik {
namespace coll {

constexpr int32_t MESH_MAX_TRIANGLES = 1 << 20;  // OPTIK_HIP_MAX_MESH_TRIANGLES
// The device's launch shape (ik_mesh.hip); neither changes a bit of the result.
constexpr int MESH_TILE = 256;  // triangles per LDS tile: 256 * 72 B = 18 KiB
// The most (node, triangle) pairs one kernel launch evaluates: the host splits the nodes into stream-ordered launches
// of at most this many, so that no launch holds a shared device for long.  Measured on an MI355X: 9.5e10 pairs/s
// (DESIGN.md section 5.21), so 2^32 pairs are 45 ms -- a factor of 20 below a second for meshes that diverge more than
// the one measured, while a bound of 2^28 already costs 30 % in launch tails.
constexpr long long MESH_PAIRS_PER_LAUNCH = 1LL << 32;

// Step 6: q1, y > 0 and x >= 0 (x = 0: y / x = +inf takes the last branch and gives pi / 2).
OPTIK_CM_HD inline double atan2m_q1(double y, double x) {
    const double aT0 = 3.33333333333329318027e-01, aT1 = -1.99999999998764832476e-01,
                 aT2 = 1.42857142725034663711e-01, aT3 = -1.11111104054623557880e-01,
                 aT4 = 9.09088713343650656196e-02, aT5 = -7.69187620504482999495e-02,
                 aT6 = 6.66107313738753120669e-02, aT7 = -5.83357013379057348645e-02,
                 aT8 = 4.97687799461593236017e-02, aT9 = -3.65315727442169155270e-02,
                 aT10 = 1.62858201153657823623e-02;
    const double t = y / x;
    double num, den, hi, lo;
    const bool direct = t < 0.4375;
    if (direct) { num = t; den = 1.0; hi = 0.0; lo = 0.0; }
    else if (t < 0.6875) { num = 2.0 * t - 1.0; den = 2.0 + t;
        hi = 4.63647609000806093515e-01; lo = 2.26987774529616870924e-17; }
    else if (t < 1.1875) { num = t - 1.0; den = t + 1.0;
        hi = 7.85398163397448278999e-01; lo = 3.06161699786838301793e-17; }
    else if (t < 2.4375) { num = t - 1.5; den = 1.0 + 1.5 * t;
        hi = 9.82793723247329054082e-01; lo = 1.39033110312309984516e-17; }
    else { num = -1.0; den = t;
        hi = 1.57079632679489655800e+00; lo = 6.12323399573676603587e-17; }
    const double u = num / den;
    const double z = u * u;
    const double w = z * z;
    const double s1 = z * (aT0 + w * (aT2 + w * (aT4 + w * (aT6 + w * (aT8 + w * aT10)))));
    const double s2 = w * (aT1 + w * (aT3 + w * (aT5 + w * (aT7 + w * aT9))));
    return direct ? (u - u * (s1 + s2)) : (hi - ((u * (s1 + s2) - lo) - u));
}

// Step 6.
OPTIK_CM_HD inline double atan2m(double y, double x) {
    const double PI = 3.141592653589793;
    if (y == 0.0) return x < 0.0 ? PI : 0.0;
    const double ay = fabs(y);
    const double q = atan2m_q1(ay, fabs(x));
    const double r = x >= 0.0 ? q : PI - q;
    return y > 0.0 ? r : -r;
}

OPTIK_CM_HD inline double mesh_dot(const double *u, const double *v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

OPTIK_CM_HD inline void mesh_cross(const double *u, const double *v, double *o) {
    o[0] = u[1] * v[2] - u[2] * v[1];
    o[1] = u[2] * v[0] - u[0] * v[2];
    o[2] = u[0] * v[1] - u[1] * v[0];
}

// Step 2.
OPTIK_CM_HD inline double mesh_segment_d2(const double *V, const double *e) {
    const double ee = mesh_dot(e, e);
    const double t = -mesh_dot(V, e);
    const double s = ee == 0.0 ? 0.0 : fmin(fmax(t / ee, 0.0), 1.0);
    const double r[3] = {V[0] + s * e[0], V[1] + s * e[1], V[2] + s * e[2]};
    return mesh_dot(r, r);
}

// What a node carries along the triangles: steps 4 and 7.
struct MeshAcc {
    double d2;  // fmin so far, from +inf
    double w;   // the sum of Omega so far, from 0.0
};

OPTIK_CM_HD inline MeshAcc mesh_acc_start() { return MeshAcc{INFINITY, 0.0}; }

// Steps 1 - 5 and 7 for one triangle (tri9 = a, b, c).
OPTIK_CM_HD inline void mesh_accumulate(const double *p, const double *tri9, MeshAcc &acc) {
    const double *a = tri9, *b = tri9 + 3, *c = tri9 + 6;
    const double A[3] = {a[0] - p[0], a[1] - p[1], a[2] - p[2]};
    const double B[3] = {b[0] - p[0], b[1] - p[1], b[2] - p[2]};
    const double C[3] = {c[0] - p[0], c[1] - p[1], c[2] - p[2]};
    const double e0[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const double e1[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]};
    const double e2[3] = {a[0] - c[0], a[1] - c[1], a[2] - c[2]};
    // steps 2 and 4
    double m = fmin(fmin(mesh_segment_d2(A, e0), mesh_segment_d2(B, e1)), mesh_segment_d2(C, e2));
    // step 3
    const double g[3] = {-e2[0], -e2[1], -e2[2]};
    double n[3], x0[3], x1[3], x2[3];
    mesh_cross(e0, g, n);
    const double nn = mesh_dot(n, n);
    mesh_cross(A, e0, x0);
    mesh_cross(B, e1, x1);
    mesh_cross(C, e2, x2);
    const bool face = nn > 0.0 && mesh_dot(x0, n) >= 0.0 && mesh_dot(x1, n) >= 0.0 && mesh_dot(x2, n) >= 0.0;
    const double h = mesh_dot(A, n);
    const double fd = (h * h) / nn;
    m = face ? fmin(m, fd) : m;
    acc.d2 = fmin(acc.d2, m);
    // step 5
    const double la = sqrt(mesh_dot(A, A)), lb = sqrt(mesh_dot(B, B)), lc = sqrt(mesh_dot(C, C));
    double bc[3];
    mesh_cross(B, C, bc);
    const double num = mesh_dot(A, bc);
    const double den = (((la * lb) * lc + mesh_dot(A, B) * lc) + mesh_dot(B, C) * la) + mesh_dot(C, A) * lb;
    acc.w = acc.w + 2.0 * atan2m(num, den);
}

// Steps 7 and 8.
OPTIK_CM_HD inline float mesh_value(const MeshAcc &acc, double max_distance) {
    const double d = sqrt(acc.d2);
    const bool inside = fabs(acc.w) >= 6.283185307179586;
    const double s = inside ? -d : d;
    return (float)fmax(fmin(s, max_distance), -max_distance);
}

// The reference form (the tests' g++ driver): every node in memory order, each walking the triangles from 0.
inline void mesh_field(const double *origin, double voxel, const int32_t *n, const double *tris9, int M,
                       double max_distance, float *out) {
    for (int i = 0; i < n[0]; ++i)
        for (int j = 0; j < n[1]; ++j)
            for (int k = 0; k < n[2]; ++k) {
                double p[3];
                grid_node(origin, voxel, i, j, k, p);
                MeshAcc acc = mesh_acc_start();
                for (int t = 0; t < M; ++t) mesh_accumulate(p, tris9 + 9 * (size_t)t, acc);
                out[((size_t)i * n[1] + j) * n[2] + k] = mesh_value(acc, max_distance);
            }
}

// The arguments beyond the grid's geometry, checked on the host: the triangle count and the clamp; the coordinates
// where they are host arrays (tris9 non-null).  Returns 0, or non-zero with the refusal in `err`.
inline int check_mesh(int64_t M, double max_distance, const double *tris9, std::string &err) {
    if (M < 1 || M > (int64_t)MESH_MAX_TRIANGLES) {
        err = "world grid from mesh: the triangle count must be in 1..2^20, got " + std::to_string(M);
        return 1;
    }
    if (!(max_distance > 0.0) || !std::isfinite(max_distance)) {
        err = "world grid from mesh: max_distance must be finite and > 0";
        return 1;
    }
    if (tris9)
        for (int64_t k = 0; k < 9 * M; ++k)
            if (!std::isfinite(tris9[k])) {
                err = "world grid from mesh: triangle " + std::to_string(k / 9) + " has a NaN or infinite coordinate";
                return 1;
            }
    return 0;
}

}  // namespace coll
}  // namespace optik
