// spherefit_measure.hpp -- a greedy sphere cover of a solid, one source for the host and the device
// (optik_hip_sphere_fit, optik_hip.h).  From a signed distance grid of the solid and points
// sampled on its surface to at most K spheres that contain the points and stay within `pad` of the solid: the robot
// model of collision_measure.hpp (spheres fixed in a frame) from collision geometry.  It installs nothing.
//
// Inputs: the float32 values [nx][ny][nz] of a signed distance field (negative inside; what mesh_measure.hpp
// produces) on collision_measure.hpp's grid, node (i, j, k) at origin_a + voxel * (double)i_a (grid_node), node index
// c = (i * ny + j) * nz + k (memory order), C = nx * ny * nz nodes; P surface points, double [P][3]; pad > 0,
// 0 <= slack < pad; K >= 1.
//
// The exact operation order (the tests depend on it; both sides are compiled with -ffp-contract=off and use only the
// correctly rounded + - * / and comparisons, so one source gives one set of integers wherever it runs):
//
//  1. Every node c is a candidate slot.  Its centre is its position and its radius
//         r = pad - (double)value[c]
//     and it is a candidate iff  r > slack  and the value is finite ((double)value - (double)value == 0.0).
//     Since the field is 1-Lipschitz, the ball of radius r about c reaches at most `pad` beyond the solid, wherever c
//     is: a point q of it is at signed distance <= value[c] + |q - c| <= value[c] + r = pad.
//  2. Point p is covered by candidate c iff
//         dx = p.x - c.x,  dy = p.y - c.y,  dz = p.z - c.z
//         d2 = (dx * dx + dy * dy) + dz * dz
//         t = r - slack
//         d2 <= t * t
//     (every product and sum rounded, in that order): p lies at least `slack` inside the ball.  A NaN coordinate is
//     covered by nothing.
//  3. Rounds j = 0 .. K - 1.  gain[c] = the number of points not yet covered that c covers (0 for a slot that is no
//     candidate).  The round picks the slot with the largest gain, ties to the lower node index.  If that gain is 0
//     the round and all later ones choose nothing.  Otherwise chosen[j] = c, gains[j] = gain[c], and the points c
//     covers count as covered from here on.
//  4. Outputs: chosen int32 [K] (-1 past the count), centers [K][3] and radii [K] (the node position and r of step 1;
//     NaN past the count), gains int32 [K] (0 past the count), count = the number of rounds that chose, uncovered =
//     P - the sum of the gains.
//
// Everything decided is an integer, so the device (ik_spherefit.hip) must equal fit_reference below exactly, whatever
// its launch shape, and whether it recounts the gains every round or, as it does, subtracts from them the points a
// round newly covered: both give the integers of step 3.
//
// The guarantee.  Let the grid contain the points' bounding box and pad >= sqrt(3) * voxel + slack.  The node c
// nearest to a surface point p is within sqrt(3) / 2 * voxel of it, so value[c] <= sqrt(3) / 2 * voxel (the field is
// 1-Lipschitz and 0 at p), r - slack >= sqrt(3) / 2 * voxel >= |p - c|: c is a candidate that covers p.  Every point
// is therefore coverable, and with K large enough uncovered == 0.  At uncovered == 0 every sampled point lies at least
// `slack` inside some sphere -- with the samples no further than `slack` apart (optik_amd.collision.surface_points)
// the whole surface lies inside the union -- and no sphere reaches further than `pad` outside the solid.  Both hold up
// to the float32 rounding of the field (and the error of a field that is not the exact distance).
//
// What this is not: an optimiser.  The centres are grid nodes, the radii follow from the field, the choice is greedy;
// nothing moves a sphere after it was picked.
//
// Plain host C++ compiles this header too (no HIP runtime): tests/spherefit_util.py drives it with g++.
#pragma once

#include <string>
#include <vector>

#include "collision_measure.hpp"

namespace optik {
namespace coll {

constexpr int32_t FIT_MAX_SPHERES = 256;       // OPTIK_HIP_MAX_FIT_SPHERES: K
constexpr int32_t FIT_MAX_POINTS = 1 << 20;    // OPTIK_HIP_MAX_FIT_POINTS: P
// The device's launch shape (ik_spherefit.hip); neither changes an integer of the result.
constexpr int FIT_TILE = 512;  // points per LDS tile: 512 * 24 B = 12 KiB
// The most (candidate, point) pair tests one launch of the gain pass makes: the host cuts the candidates into
// stream-ordered launches of at most this many (the precedent: mesh_measure.hpp's MESH_PAIRS_PER_LAUNCH).
constexpr long long FIT_PAIRS_PER_LAUNCH = 1LL << 32;

// Step 1: a slot's sphere.  ok: it is a candidate.
struct FitSlot {
    double c[3];
    double r;
    bool ok;
};

OPTIK_CM_HD inline FitSlot fit_slot(const double *origin, double voxel, const int32_t *n, int32_t node, float value,
                                    double pad, double slack) {
    FitSlot s;
    const int32_t sx = n[1] * n[2];
    grid_node(origin, voxel, node / sx, node / n[2] % n[1], node % n[2], s.c);
    const double v = (double)value;
    s.r = pad - v;
    s.ok = (s.r > slack) && (v - v == 0.0);
    return s;
}

// Step 2.
OPTIK_CM_HD inline bool fit_covers(const FitSlot &s, double slack, const double *p) {
    const double dx = p[0] - s.c[0], dy = p[1] - s.c[1], dz = p[2] - s.c[2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    const double t = s.r - slack;
    return s.ok && d2 <= t * t;
}

// Step 3's order: does (ogain, onode) come before (gain, node)?
OPTIK_CM_HD inline bool fit_takes(int32_t gain, int32_t node, int32_t ogain, int32_t onode) {
    return ogain > gain || (ogain == gain && onode < node);
}

// The reference form (the tests' g++ driver): serial, the gains recounted every round over the points still uncovered.
// chosen [K], centers [K][3], radii [K], gains [K]; count_uncovered [2].
inline void fit_reference(const double *origin, double voxel, const int32_t *n, const float *values,
                          const double *points, int32_t P, double pad, double slack, int32_t K, int32_t *chosen,
                          double *centers, double *radii, int32_t *gains, int32_t *count_uncovered) {
    const int32_t C = n[0] * n[1] * n[2];
    std::vector<int32_t> open((size_t)P);  // the points not yet covered
    for (int32_t p = 0; p < P; ++p) open[(size_t)p] = p;
    for (int32_t j = 0; j < K; ++j) {
        chosen[j] = -1;
        gains[j] = 0;
        radii[j] = centers[3 * j] = centers[3 * j + 1] = centers[3 * j + 2] = NAN;
    }
    int32_t count = 0;
    for (int32_t j = 0; j < K; ++j) {
        int32_t best_gain = 0, best = -1;
        for (int32_t c = 0; c < C; ++c) {
            const FitSlot s = fit_slot(origin, voxel, n, c, values[c], pad, slack);
            if (!s.ok) continue;
            int32_t g = 0;
            for (size_t q = 0; q < open.size(); ++q) g += fit_covers(s, slack, points + 3 * (size_t)open[q]) ? 1 : 0;
            if (best < 0 ? g > 0 : fit_takes(best_gain, best, g, c)) { best_gain = g; best = c; }
        }
        if (best < 0) break;
        const FitSlot s = fit_slot(origin, voxel, n, best, values[best], pad, slack);
        chosen[j] = best;
        gains[j] = best_gain;
        radii[j] = s.r;
        for (int a = 0; a < 3; ++a) centers[3 * j + a] = s.c[a];
        ++count;
        size_t w = 0;
        for (size_t q = 0; q < open.size(); ++q)
            if (!fit_covers(s, slack, points + 3 * (size_t)open[q])) open[w++] = open[q];
        open.resize(w);
    }
    count_uncovered[0] = count;
    count_uncovered[1] = (int32_t)open.size();
}

// The arguments beyond the grid's geometry, checked on the host; the points where they are host arrays (points
// non-null).  Returns 0, or non-zero with the refusal in `err`.
inline int check_fit(int64_t P, double pad, double slack, int64_t K, const double *points, std::string &err) {
    if (K < 1 || K > (int64_t)FIT_MAX_SPHERES) {
        err = "sphere fit: K must be in 1..256, got " + std::to_string(K);
        return 1;
    }
    if (P < 1 || P > (int64_t)FIT_MAX_POINTS) {
        err = "sphere fit: the point count must be in 1..2^20, got " + std::to_string(P);
        return 1;
    }
    if (!(pad > 0.0) || !std::isfinite(pad)) {
        err = "sphere fit: pad must be finite and > 0";
        return 1;
    }
    if (!(slack >= 0.0) || !(slack < pad)) {
        err = "sphere fit: slack must be finite, >= 0 and < pad";
        return 1;
    }
    if (points)
        for (int64_t k = 0; k < 3 * P; ++k)
            if (!std::isfinite(points[k])) {
                err = "sphere fit: point " + std::to_string(k / 3) + " has a NaN or infinite coordinate";
                return 1;
            }
    return 0;
}

// The bytes of the workspace optik_hip_sphere_fit needs (device memory, the caller's): the gains int32 [C], the
// covered flags and the list of newly covered points int32 [P] each, the pick's per-block records, the round state.
constexpr int FIT_PICK_BLOCKS = 256;  // blocks of the pick's first stage, at most
inline size_t fit_workspace_bytes(int64_t nodes, int64_t P) {
    return sizeof(int32_t) * ((size_t)nodes + 2 * (size_t)P + 2 * (size_t)FIT_PICK_BLOCKS + 16);
}

}  // namespace coll
}  // namespace optik
