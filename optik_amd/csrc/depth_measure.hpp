// depth_measure.hpp -- the evidence map of depth-image worlds, one source for the host and the device
// (optik_hip_depth_integrate and optik_hip_occupancy_from_map, optik_hip.h).
//
// The map is int16 [nx][ny][nz] (z fastest) on the node lattice of the distance-field world (collision_measure.hpp:
// node (i, j, k) at origin_a + voxel * (double)i_a).  MAP_UNKNOWN = -32768 is a node that was never observed; every
// other value is evidence in [e_min, e_max].  A depth image is float32 [H][W], the z-depth in metres along the optical
// axis; pixel (v, u) has its centre at integer coordinates.  A camera is its intrinsics fx, fy, cx, cy and its pose in
// the base frame, rotation R and translation t (x right, y down, z forward), taken from a column-major 4x4:
// R_ab = m[4 * b + a], t_a = m[12 + a].
//
// The exact operation order (the tests depend on it; both sides are compiled with -ffp-contract=off and use only the
// correctly rounded + - * /, fabs and floor, so one source gives one set of bits wherever it runs).  All geometry is
// f64 (f32 -> f64 is exact).
//
//  1. The pixel pass, once per frame: the cleaned image c [H][W], float32.  d = (double)depth[v][u].
//       d not finite, or !(d > z_near):  c = NaN      (invalid: says nothing)
//       d > z_far:                       c = +inf     (free out to z_far, no surface)
//       otherwise back-project:
//           xc = (((double)u - cx) / fx) * d;  yc = (((double)v - cy) / fy) * d;  zc = d
//           p_a = ((R_a0 * xc + R_a1 * yc) + R_a2 * zc) + t_a
//       the pixel is masked iff, for any of the E exclusion spheres (s, r), with dx = p_x - s_x (dy, dz alike),
//           ((dx * dx + dy * dy) + dz * dz) <= r * r         (collision_measure.hpp, step 9: point_excluded)
//       c = -d when masked (the pixel sees the robot: free in front of it, no obstacle), c = d otherwise; both are
//       exact in float32, d came from one.
//  2. The node pass, per node with position p and evidence e, per frame:
//           q_a = p_a - t_a
//           xc = (R_00 * q_0 + R_10 * q_1) + R_20 * q_2     (yc, zc with the second and third columns: R transposed)
//       no update unless zc > z_near && zc <= z_far;
//           wu = (fx * (xc / zc) + cx) + 0.5;  wv = (fy * (yc / zc) + cy) + 0.5
//       no update unless 0.0 <= wu < (double)W and 0.0 <= wv < (double)H (a NaN fails);
//           c = cleaned[(int)floor(wv)][(int)floor(wu)];  a = fabs((double)c)
//       c NaN: no update.
//       zc < a - band:                              a miss:  e = max((e == UNKNOWN ? 0 : e) - miss, e_min)
//       else c > 0, c finite and zc <= a + band:    a hit:   e = min((e == UNKNOWN ? 0 : e) + hit, e_max)
//       otherwise no update (occluded, or in the band of a masked pixel).  The integers are int32, stored as int16.
//  3. Several frames are applied to a node in order; a call with F frames leaves what F calls with one frame leave.
//  4. occupancy_from_map: occ = (e == UNKNOWN) ? unknown_occupied : (e >= threshold), as 0 / 1.
//
// Each node is written by one lane from one gathered pixel per frame: no ray marching, no atomics, one result.
//
// Plain host C++ compiles this header too (no HIP runtime): tests/depth_util.py drives it with g++.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "collision_measure.hpp"

namespace optik {
namespace depth {

constexpr int MAP_UNKNOWN = -32768;

struct Camera {
    double fx, fy, cx, cy;
    double R[9];  // row-major: R_ab = R[3 * a + b]
    double t[3];
};

struct Params {
    double z_near, z_far, band;
    int32_t hit, miss, e_min, e_max;
};

// intrinsics4 = (fx, fy, cx, cy); pose16 = a column-major 4x4 (what optik_robot_fk_ex writes)
OPTIK_CM_HD inline Camera camera_from(const double *intrinsics4, const double *pose16) {
    Camera c;
    c.fx = intrinsics4[0]; c.fy = intrinsics4[1]; c.cx = intrinsics4[2]; c.cy = intrinsics4[3];
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) c.R[3 * a + b] = pose16[4 * b + a];
        c.t[a] = pose16[12 + a];
    }
    return c;
}

OPTIK_CM_HD inline bool finite(double x) { return fabs(x) <= DBL_MAX; }  // (false for a NaN)

// Step 1 up to the mask: the cleaned value of an unmasked pixel, and for a valid surface pixel (the return value) its
// point in the base frame.
OPTIK_CM_HD inline bool pixel_point(float depth, int v, int u, const Camera &c, double z_near, double z_far, float *clean,
                                    double *p) {
    const double d = (double)depth;
    if (!finite(d) || !(d > z_near)) { *clean = __builtin_nanf(""); return false; }
    if (d > z_far) { *clean = __builtin_inff(); return false; }
    const double xc = (((double)u - c.cx) / c.fx) * d;
    const double yc = (((double)v - c.cy) / c.fy) * d;
    const double zc = d;
    p[0] = ((c.R[0] * xc + c.R[1] * yc) + c.R[2] * zc) + c.t[0];
    p[1] = ((c.R[3] * xc + c.R[4] * yc) + c.R[5] * zc) + c.t[1];
    p[2] = ((c.R[6] * xc + c.R[7] * yc) + c.R[8] * zc) + c.t[2];
    *clean = depth;
    return true;
}

// Step 2 for one node and one frame: the evidence afterwards.  cleaned: this frame's [H][W].
OPTIK_CM_HD inline int integrate_frame(int e, double px, double py, double pz, const Camera &c, const float *cleaned,
                                       int H, int W, const Params &P) {
    const double q0 = px - c.t[0], q1 = py - c.t[1], q2 = pz - c.t[2];
    const double xc = (c.R[0] * q0 + c.R[3] * q1) + c.R[6] * q2;
    const double yc = (c.R[1] * q0 + c.R[4] * q1) + c.R[7] * q2;
    const double zc = (c.R[2] * q0 + c.R[5] * q1) + c.R[8] * q2;
    if (!(zc > P.z_near && zc <= P.z_far)) return e;
    const double wu = (c.fx * (xc / zc) + c.cx) + 0.5;
    const double wv = (c.fy * (yc / zc) + c.cy) + 0.5;
    if (!(wu >= 0.0 && wu < (double)W && wv >= 0.0 && wv < (double)H)) return e;
    // (0 <= floor(wv) <= H - 1 and 0 <= floor(wu) <= W - 1: inside the H * W floats)
    const float cv = cleaned[(size_t)(int)floor(wv) * (size_t)W + (size_t)(int)floor(wu)];
    if (cv != cv) return e;
    const double a = fabs((double)cv);
    const int base = e == MAP_UNKNOWN ? 0 : e;
    if (zc < a - P.band) {
        const int m = base - P.miss;
        return m > P.e_min ? m : P.e_min;
    }
    if (cv > 0.0f && finite(a) && zc <= a + P.band) {
        const int h = base + P.hit;
        return h < P.e_max ? h : P.e_max;
    }
    return e;
}

// Step 4 for one node.
OPTIK_CM_HD inline uint8_t map_occupied(int e, int threshold, bool unknown_occupied) {
    return (uint8_t)(e == MAP_UNKNOWN ? (unknown_occupied ? 1 : 0) : (e >= threshold ? 1 : 0));
}

// ---- the serial reference (the tests' g++ driver) ------------------------------------------------------------------

// Step 1: one frame's cleaned image.
inline void clean_image(const float *depth, int H, int W, const Camera &c, double z_near, double z_far,
                        const double *exclude4, int E, float *cleaned) {
    for (int v = 0; v < H; ++v)
        for (int u = 0; u < W; ++u) {
            const size_t i = (size_t)v * (size_t)W + (size_t)u;
            double p[3];
            float cv;
            if (pixel_point(depth[i], v, u, c, z_near, z_far, &cv, p)) {
                bool masked = false;
                for (int s = 0; s < E && !masked; ++s) masked = coll::point_excluded(p, exclude4 + 4 * s);
                if (masked) cv = -cv;
            }
            cleaned[i] = cv;
        }
}

// Steps 1 - 3: F frames into the map, in place.  depth [F][H][W], intrinsics4 [F][4], poses16 [F][16]; cleaned: H * W
// floats of workspace.
inline void integrate(const double *origin, double voxel, const int32_t *n, int16_t *map, const float *depth, int F, int H,
                      int W, const double *intrinsics4, const double *poses16, const double *exclude4, int E,
                      const Params &P, float *cleaned) {
    for (int f = 0; f < F; ++f) {
        const Camera c = camera_from(intrinsics4 + 4 * f, poses16 + 16 * f);
        clean_image(depth + (size_t)f * (size_t)H * (size_t)W, H, W, c, P.z_near, P.z_far, exclude4, E, cleaned);
        for (int i = 0; i < n[0]; ++i)
            for (int j = 0; j < n[1]; ++j)
                for (int k = 0; k < n[2]; ++k) {
                    int16_t &e = map[((size_t)i * n[1] + j) * n[2] + k];
                    e = (int16_t)integrate_frame(e, origin[0] + voxel * (double)i, origin[1] + voxel * (double)j,
                                                 origin[2] + voxel * (double)k, c, cleaned, H, W, P);
                }
    }
}

// Step 4: `accumulate` ORs into what `occupied` holds, otherwise it is overwritten.
inline void occupancy_from_map(const int16_t *map, long long nodes, int threshold, bool unknown_occupied, bool accumulate,
                               uint8_t *occupied) {
    for (long long p = 0; p < nodes; ++p) {
        const uint8_t o = map_occupied(map[p], threshold, unknown_occupied);
        occupied[p] = accumulate ? (uint8_t)(occupied[p] | o) : o;
    }
}

}  // namespace depth
}  // namespace optik
