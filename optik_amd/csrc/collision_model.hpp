// collision_model.hpp -- the collision model and world of a chain on the host: the argument checks shared by the
// kernel layer (optik_hip_chain_set_collision_model / _set_world, ik_collision.hip) and the robot layer
// (optik_robot_set_collision_model / _set_world, robot_rows.cpp), and the device layout of the model.
//
// The device model keeps the robot spheres grouped by frame and the self pairs grouped by (frame of a, frame of b):
// the kernels look a frame up once per group, not once per sphere (collision_measure.hpp: the minimum is exact in
// any order, and every pair keeps the (a, b) orientation it was given, so its distance has the same bits).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/optik_hip.h"

namespace optik {
namespace coll {

constexpr int MAX_SPHERES = OPTIK_HIP_MAX_COLLISION_SPHERES;  // 256: a sphere index fits a byte
constexpr int MAX_PAIRS = OPTIK_HIP_MAX_COLLISION_PAIRS;      // 4096
constexpr int MAX_OBSTACLES = OPTIK_HIP_MAX_WORLD_OBSTACLES;  // 65 536 of each kind
constexpr int MAX_FRAMES = 16 + 2;                            // n + 2 frames, n <= 16
constexpr int MAX_GROUPS = MAX_FRAMES * MAX_FRAMES;
static_assert(MAX_SPHERES <= 256, "pairs hold sphere indices in a byte each");

// What the kernels stage in LDS (only the first S spheres, P pairs and n_groups groups are read).
struct ModelDev {
    double sph[MAX_SPHERES][4];            // centre in its frame, radius; grouped by frame
    uint16_t pair[MAX_PAIRS];              // a | b << 8 (indices into sph); grouped by (frame a, frame b)
    uint16_t frame_begin[MAX_FRAMES + 2];  // spheres of frame f: [frame_begin[f], frame_begin[f + 1])
    uint16_t group_begin[MAX_GROUPS + 4];  // pairs of group g: [group_begin[g], group_begin[g + 1])
    uint8_t group_fa[MAX_GROUPS], group_fb[MAX_GROUPS];
};
static_assert(sizeof(ModelDev) % 8 == 0, "staged as doubles");

inline bool finite3(const double *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }
inline bool nonneg(double v) { return v >= 0.0; }  // (false for NaN)

// 0, or OPTIK_HIP_EINVAL with the reason in err.  n: the chain's joint positions (frames 0 .. n + 1).
inline int check_model(int n, const int32_t *frames, const double *centers3, const double *radii, int32_t S,
                       const int32_t *pairs2, int32_t P, double margin, std::string &err) {
    if (S < 0 || S > MAX_SPHERES) { err = "collision model: sphere count must be in 0..256"; return OPTIK_HIP_EINVAL; }
    if (P < 0 || P > MAX_PAIRS) { err = "collision model: self pair count must be in 0..4096"; return OPTIK_HIP_EINVAL; }
    if (S > 0 && (!frames || !centers3 || !radii)) { err = "collision model: null sphere array"; return OPTIK_HIP_EINVAL; }
    if (P > 0 && !pairs2) { err = "collision model: null pair array"; return OPTIK_HIP_EINVAL; }
    if (!(margin >= 0.0) || !std::isfinite(margin)) {
        err = "collision model: margin must be finite and >= 0";
        return OPTIK_HIP_EINVAL;
    }
    for (int s = 0; s < S; ++s) {
        if (frames[s] < 0 || frames[s] > n + 1) {
            err = "collision model: sphere " + std::to_string(s) + " has frame " + std::to_string(frames[s])
                  + " outside 0.." + std::to_string(n + 1);
            return OPTIK_HIP_EINVAL;
        }
        if (!finite3(centers3 + 3 * s)) {
            err = "collision model: sphere " + std::to_string(s) + " has a non-finite centre";
            return OPTIK_HIP_EINVAL;
        }
        if (!nonneg(radii[s])) {
            err = "collision model: sphere " + std::to_string(s) + " has a NaN or negative radius";
            return OPTIK_HIP_EINVAL;
        }
    }
    for (int k = 0; k < P; ++k) {
        const int32_t a = pairs2[2 * k], b = pairs2[2 * k + 1];
        if (a < 0 || a >= S || b < 0 || b >= S) {
            err = "collision model: self pair " + std::to_string(k) + " has a sphere index out of range";
            return OPTIK_HIP_EINVAL;
        }
        if (a == b) {
            err = "collision model: self pair " + std::to_string(k) + " pairs a sphere with itself";
            return OPTIK_HIP_EINVAL;
        }
    }
    return 0;
}

inline int check_world(const double *spheres4, int32_t Ms, const double *boxes10, int32_t Mb, std::string &err) {
    if (Ms < 0 || Ms > MAX_OBSTACLES || Mb < 0 || Mb > MAX_OBSTACLES) {
        err = "world: at most 65536 spheres and 65536 boxes";
        return OPTIK_HIP_EINVAL;
    }
    if ((Ms > 0 && !spheres4) || (Mb > 0 && !boxes10)) { err = "world: null obstacle array"; return OPTIK_HIP_EINVAL; }
    for (int m = 0; m < Ms; ++m) {
        const double *s = spheres4 + 4 * m;
        if (!finite3(s)) { err = "world: sphere " + std::to_string(m) + " has a non-finite centre"; return OPTIK_HIP_EINVAL; }
        if (!nonneg(s[3])) {
            err = "world: sphere " + std::to_string(m) + " has a NaN or negative radius";
            return OPTIK_HIP_EINVAL;
        }
    }
    for (int m = 0; m < Mb; ++m) {
        const double *b = boxes10 + 10 * m;
        if (!finite3(b)) { err = "world: box " + std::to_string(m) + " has a non-finite centre"; return OPTIK_HIP_EINVAL; }
        const double q2 = b[3] * b[3] + b[4] * b[4] + b[5] * b[5] + b[6] * b[6];
        if (!(std::fabs(q2 - 1.0) <= 1e-9)) {
            err = "world: box " + std::to_string(m) + " needs a unit quaternion (|q|^2 within 1e-9 of 1)";
            return OPTIK_HIP_EINVAL;
        }
        if (!nonneg(b[7]) || !nonneg(b[8]) || !nonneg(b[9])) {
            err = "world: box " + std::to_string(m) + " has a NaN or negative half extent";
            return OPTIK_HIP_EINVAL;
        }
    }
    return 0;
}

// The distance-field world (collision_measure.hpp, steps 5 - 7): the geometry of a grid, and its values unless
// `values` is null (the bake checks the geometry alone).
inline int check_grid(const double *origin3, double voxel, int32_t nx, int32_t ny, int32_t nz, const float *values,
                      bool with_values, std::string &err) {
    if (!origin3 || (with_values && !values)) { err = "world grid: null origin or value array"; return OPTIK_HIP_EINVAL; }
    const int32_t dims[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a)
        if (dims[a] < 2 || dims[a] > OPTIK_HIP_MAX_GRID_DIM) {
            err = "world grid: each of nx, ny, nz must be in 2..1024, got " + std::to_string(nx) + " x "
                  + std::to_string(ny) + " x " + std::to_string(nz);
            return OPTIK_HIP_EINVAL;
        }
    const int64_t nodes = (int64_t)nx * ny * nz;
    if (nodes > (int64_t)OPTIK_HIP_MAX_GRID_NODES) {
        err = "world grid: " + std::to_string(nodes) + " nodes, more than 2^24";
        return OPTIK_HIP_EINVAL;
    }
    if (!(voxel > 0.0) || !std::isfinite(voxel) || !std::isfinite(1.0 / voxel)) {
        err = "world grid: voxel must be finite and > 0 (and so must 1 / voxel)";
        return OPTIK_HIP_EINVAL;
    }
    if (!finite3(origin3)) { err = "world grid: non-finite origin"; return OPTIK_HIP_EINVAL; }
    if (with_values)
        for (int64_t i = 0; i < nodes; ++i)
            if (!std::isfinite(values[i])) {
                err = "world grid: the value of node (" + std::to_string(i / ((int64_t)ny * nz)) + ", "
                      + std::to_string(i / nz % ny) + ", " + std::to_string(i % nz) + ") is NaN or infinite";
                return OPTIK_HIP_EINVAL;
            }
    return 0;
}

// The arguments of the distance transform and of the voxelization beyond the grid's geometry (collision_measure.hpp,
// steps 8 and 9).
inline int check_max_distance(double max_distance, std::string &err) {
    if (!(max_distance > 0.0) || !std::isfinite(max_distance)) {
        err = "world grid from occupancy: max_distance must be finite and > 0";
        return OPTIK_HIP_EINVAL;
    }
    return 0;
}

inline int check_cloud(int64_t N, int32_t E, std::string &err) {
    if (N < 0) { err = "occupancy from points: the point count is negative"; return OPTIK_HIP_EINVAL; }
    if (E < 0 || E > OPTIK_HIP_MAX_EXCLUDE_SPHERES) {
        err = "occupancy from points: the exclusion sphere count must be in 0..1024";
        return OPTIK_HIP_EINVAL;
    }
    return 0;
}

// The arguments of the evidence map beyond the grid's geometry (depth_measure.hpp): the image
// stack, the ranges and the update constants ...
inline int check_depth(int32_t F, int32_t H, int32_t W, int32_t E, double z_near, double z_far, double band, int32_t hit,
                       int32_t miss, int32_t e_min, int32_t e_max, std::string &err) {
    if (F < 1 || F > OPTIK_HIP_MAX_DEPTH_FRAMES) { err = "depth integrate: the frame count must be in 1..64"; return OPTIK_HIP_EINVAL; }
    if (H < 1 || H > OPTIK_HIP_MAX_DEPTH_DIM || W < 1 || W > OPTIK_HIP_MAX_DEPTH_DIM) {
        err = "depth integrate: the image height and width must be in 1..4096, got " + std::to_string(H) + " x "
              + std::to_string(W);
        return OPTIK_HIP_EINVAL;
    }
    if (E < 0 || E > OPTIK_HIP_MAX_EXCLUDE_SPHERES) {
        err = "depth integrate: the exclusion sphere count must be in 0..1024";
        return OPTIK_HIP_EINVAL;
    }
    if (!std::isfinite(z_near) || !std::isfinite(z_far) || !(z_near > 0.0) || !(z_far > z_near)) {
        err = "depth integrate: z_near and z_far must be finite with 0 < z_near < z_far";
        return OPTIK_HIP_EINVAL;
    }
    if (!std::isfinite(band) || !(band >= 0.0)) { err = "depth integrate: band must be finite and >= 0"; return OPTIK_HIP_EINVAL; }
    if (hit < 1 || hit > 1024 || miss < 1 || miss > 1024) {
        err = "depth integrate: hit and miss must be in 1..1024";
        return OPTIK_HIP_EINVAL;
    }
    if (e_min < -32767 || e_min > 0 || e_max < 0 || e_max > 32767) {
        err = "depth integrate: e_min must be in -32767..0 and e_max in 0..32767";
        return OPTIK_HIP_EINVAL;
    }
    return 0;
}

// ... and the cameras, host arrays [F][4] and [F][16]: fx, fy > 0, everything finite.
inline int check_cameras(int32_t F, const double *intrinsics4, const double *poses16, std::string &err) {
    if (!intrinsics4 || !poses16) { err = "depth integrate: null intrinsics or poses"; return OPTIK_HIP_EINVAL; }
    for (int32_t f = 0; f < F; ++f) {
        const double *k = intrinsics4 + 4 * f;
        if (!std::isfinite(k[0]) || !std::isfinite(k[1]) || !std::isfinite(k[2]) || !std::isfinite(k[3]) || !(k[0] > 0.0)
            || !(k[1] > 0.0)) {
            err = "depth integrate: the intrinsics of frame " + std::to_string(f) + " must be finite with fx, fy > 0";
            return OPTIK_HIP_EINVAL;
        }
        for (int i = 0; i < 16; ++i)
            if (!std::isfinite(poses16[16 * f + i])) {
                err = "depth integrate: the camera pose of frame " + std::to_string(f) + " is not finite";
                return OPTIK_HIP_EINVAL;
            }
    }
    return 0;
}

inline int check_map_threshold(int32_t threshold, std::string &err) {
    if (threshold < -32767 || threshold > 32767) {
        err = "occupancy from map: the threshold must be in -32767..32767";
        return OPTIK_HIP_EINVAL;
    }
    return 0;
}

inline const char *bake_empty_msg() { return "world grid bake: the world has no spheres and no boxes"; }

// The device layout of a checked model; returns the number of pair groups.  `orig` (optional) receives the way back
// from the layout to the caller's numbering, S + P entries: the caller's index of the sphere in slot i, then the
// caller's index of the pair at position i (the witnesses of optik_hip_collision_witness_batch speak the caller's).
inline int pack_model(int n, const int32_t *frames, const double *centers3, const double *radii, int32_t S,
                      const int32_t *pairs2, int32_t P, ModelDev &m, std::vector<uint16_t> *orig = nullptr) {
    std::memset(&m, 0, sizeof m);
    const int nf = n + 2;
    std::vector<int> order((size_t)S), slot((size_t)S);
    for (int s = 0; s < S; ++s) order[(size_t)s] = s;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return frames[x] < frames[y]; });
    for (int i = 0; i < S; ++i) {
        const int s = order[(size_t)i];
        slot[(size_t)s] = i;
        for (int k = 0; k < 3; ++k) m.sph[i][k] = centers3[3 * s + k];
        m.sph[i][3] = radii[s];
    }
    for (int f = 0, i = 0; f <= nf; ++f) {
        while (i < S && frames[order[(size_t)i]] < f) ++i;
        m.frame_begin[f] = (uint16_t)i;
    }
    std::vector<int> porder((size_t)P);
    for (int k = 0; k < P; ++k) porder[(size_t)k] = k;
    auto gkey = [&](int k) { return frames[pairs2[2 * k]] * nf + frames[pairs2[2 * k + 1]]; };
    std::stable_sort(porder.begin(), porder.end(), [&](int x, int y) { return gkey(x) < gkey(y); });
    int g = -1, last = -1;
    for (int i = 0; i < P; ++i) {
        const int k = porder[(size_t)i];
        const int a = pairs2[2 * k], b = pairs2[2 * k + 1];
        m.pair[i] = (uint16_t)(slot[(size_t)a] | (slot[(size_t)b] << 8));
        if (gkey(k) != last) {
            ++g;
            last = gkey(k);
            m.group_begin[g] = (uint16_t)i;
            m.group_fa[g] = (uint8_t)frames[a];
            m.group_fb[g] = (uint8_t)frames[b];
        }
    }
    const int groups = g + 1;
    m.group_begin[groups] = (uint16_t)P;
    if (orig) {
        orig->resize((size_t)S + (size_t)P);
        for (int i = 0; i < S; ++i) (*orig)[(size_t)i] = (uint16_t)order[(size_t)i];
        for (int i = 0; i < P; ++i) (*orig)[(size_t)S + (size_t)i] = (uint16_t)porder[(size_t)i];
    }
    return groups;
}

}  // namespace coll
}  // namespace optik
