// robot_rows.cpp -- the row batches of the host API (diff_ik, manipulability, link frames, clearance, witnesses,
// motion, roadmap plans), each one stage_rows over the robot's first device; the batches of paths (the optimiser's,
// shortcutting, resampling, timing, sampling), which stage through the same batch block with a transpose of their own; and what they are checked against: the collision model,
// the worlds and their builders; and IK into pose regions (optik_robot_ik_region), chunks of whole regions through the
// same batch block.  (robot_host.hpp: the robot object and the shared plumbing.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "collision_model.hpp"
#include "mesh_measure.hpp"
#include "pose_convert.hpp"
#include "robot_host.hpp"
#include "spherefit_measure.hpp"

using namespace optik::robot;
using optik::pose::mat16_from_pose7;
using optik::pose::pose7_from_mat16;

namespace {

constexpr int64_t kRowChunk = (int64_t)1 << 18;     // rows per launch
constexpr int64_t kMotionChunk = (int64_t)1 << 16;  // segments per launch (each is many samples)
constexpr int64_t kWitnessChunk = (int64_t)1 << 15;  // rows per launch of the witness table (840 B a row at n = 8: 28 MB)
constexpr int64_t kPathChunk = (int64_t)1 << 13;     // paths per launch of the path optimiser (8 KB a path at L = 64, n = 8)
constexpr size_t kSampleChunkDoubles = (size_t)1 << 25;  // doubles per chunk of optik_robot_trajectory_sample (256 MiB)
constexpr int64_t kPlanChunk = (int64_t)1 << 12;     // queries per launch of a plan (one workgroup each; 8 KB of path at Lmax = 64, n = 16)

// A chunk of paths [P][L][n] with their lengths through the batch block, waypoint-major on the device ([L][chunk][n],
// the transpose optik_robot_path_optimize makes), the int32 lengths behind them; `out_doubles` doubles per path come
// back.  launch(d_paths, d_lens or null, Lc, d_out) queues the device work, scatter(b0, Lc, h_out) takes the results.
// `extra` (extra_doubles of them, may be none) is uploaded with every chunk, at d_paths + paths_extra_offset(nl, n, Lc).
inline size_t paths_extra_offset(size_t nl, size_t n, size_t Lc) { return nl * n * Lc + (Lc + 1) / 2; }

template <class Launch, class Scatter>
int stage_paths(DeviceCtx *c, const double *paths, const int32_t *lens, int64_t P, size_t nl, size_t n,
                size_t out_doubles, Launch &&launch, Scatter &&scatter, const double *extra = nullptr,
                size_t extra_doubles = 0) {
    BatchGuard guard(c);
    if (!guard.ok()) return set_err(-1, kSetDeviceMsg);
    const size_t w = nl * n;
    const int64_t chunk = P < kPathChunk ? P : kPathChunk;
    if (!reserve_batch(c, (w + 1 + out_doubles) * (size_t)chunk + extra_doubles)) return set_err(-1, kBatchAllocMsg);
    for (int64_t b0 = 0; b0 < P; b0 += chunk) {
        const size_t Lc = (size_t)(P - b0 < chunk ? P - b0 : chunk),
                     in_doubles = paths_extra_offset(nl, n, Lc) + extra_doubles;
        double *h_in = c->h_batch.get(), *h_out = h_in + in_doubles;
        double *d_in = c->d_batch.get(), *d_out = d_in + in_doubles;
        parallel_ranges(Lc, [&](size_t k0, size_t k1) {
            for (size_t k = k0; k < k1; ++k)
                for (size_t t = 0; t < nl; ++t)
                    std::memcpy(h_in + (t * Lc + k) * n, paths + (((size_t)b0 + k) * nl + t) * n, sizeof(double) * n);
        });
        if (lens) std::memcpy(h_in + w * Lc, lens + b0, sizeof(int32_t) * Lc);
        if (extra_doubles) std::memcpy(h_in + paths_extra_offset(nl, n, Lc), extra, sizeof(double) * extra_doubles);
        if (hipMemcpyAsync(d_in, h_in, sizeof(double) * in_doubles, hipMemcpyHostToDevice, nullptr) != hipSuccess)
            return set_err(-1, "upload failed");
        if (launch(d_in, lens ? reinterpret_cast<const int32_t *>(d_in + w * Lc) : nullptr, (int64_t)Lc, d_out))
            return set_err(-1, optik_hip_last_error());
        if (hipMemcpyAsync(h_out, d_out, sizeof(double) * out_doubles * Lc, hipMemcpyDeviceToHost, nullptr) != hipSuccess
            || hipStreamSynchronize(nullptr) != hipSuccess)
            return set_err(-1, "download failed");
        scatter((size_t)b0, Lc, h_out);
    }
    return 0;
}

// waypoint-major [L][Lc][n] back to rows [P][L][n]
void scatter_paths(double *paths_out, const double *h_out, size_t b0, size_t Lc, size_t nl, size_t n) {
    parallel_ranges(Lc, [&](size_t k0, size_t k1) {
        for (size_t k = k0; k < k1; ++k)
            for (size_t t = 0; t < nl; ++t)
                std::memcpy(paths_out + ((b0 + k) * nl + t) * n, h_out + (t * Lc + k) * n, sizeof(double) * n);
    });
}

// What every plan wrapper downloads first per chunk -- the paths [Lmax][L][n], the costs [L], then len [L] and status
// [L] int32 -- to the caller's rows b0 .. b0 + L (any may be null).  Returns the int32 words behind the status.
const int32_t *scatter_plans(const double *h_out, size_t b0, size_t L, size_t Lmax, size_t n, double *paths_out,
                             int32_t *len_out, double *cost_out, int32_t *status_out) {
    const double *h_cost = h_out + Lmax * n * L;
    const int32_t *h_len = reinterpret_cast<const int32_t *>(h_cost + L), *h_status = h_len + L;
    if (paths_out) scatter_paths(paths_out, h_out, b0, L, Lmax, n);
    if (cost_out) std::memcpy(cost_out + b0, h_cost, sizeof(double) * L);
    if (len_out) std::memcpy(len_out + b0, h_len, sizeof(int32_t) * L);
    if (status_out) std::memcpy(status_out + b0, h_status, sizeof(int32_t) * L);
    return h_status + L;
}

}  // namespace

extern "C" {

// B diff_ik calls in one launch per chunk of rows (optik_hip_diff_ik_batch: the same FK, Jacobian and LP code as
// optik_robot_diff_ik_ex, on the device).  Rows are staged to struct-of-arrays through the robot's pinned batch block.
int optik_robot_diff_ik_batch(const optik_robot *r, int64_t B, const double *x0, const double *V_WE,
                              const double *v_max, const double *ee16, double *alpha_out, double *v_out,
                              int32_t *status_out) {
    if (!r || !x0 || !V_WE || !v_max) return set_err(-1, "null argument");
    if (B < 0) return set_err(-1, "bad argument");
    const int n = r->n;
    if (n > 8) return set_err(-1, kDiffIkMaxNMsg);
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    // (B = 0: the kernel layer's refusals of the chain alone -- prismatic joints -- before anything is staged)
    if (optik_hip_diff_ik_batch(c->chain, nullptr, nullptr, nullptr, 0, nullptr, 0, 0, nullptr, nullptr, nullptr,
                                nullptr))
        return set_err(-1, optik_hip_last_error());
    if (B == 0) return 0;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    // per row: q n | V 6 | v_max n doubles in; alpha 1 | v n doubles, then the int32 status words (half a double each) out
    const RowInput in[] = {{x0, (size_t)n}, {V_WE, 6}, {v_max, (size_t)n}};
    // (rows per launch: 2^18 bounds the block, ~66 MB for 8 joints, whatever B is)
    return stage_rows(
        c, B, in, sizeof(double) * (size_t)(n + 1) + sizeof(int32_t), kRowChunk,
        [&](optik_hip_chain *ch, const double *d_q, int64_t L, double *d_a) {
            const double *d_V = d_q + (size_t)n * L, *d_vm = d_V + 6 * L;
            double *d_v = d_a + L;
            return optik_hip_diff_ik_batch(ch, ee16 ? ee7 : nullptr, d_q, d_V, L, d_vm, L, L, d_a, d_v,
                                           reinterpret_cast<int32_t *>(d_v + (size_t)n * L), nullptr);
        },
        [&](size_t b0, size_t L, const double *h_a) {
            const double *h_v = h_a + L;
            const int32_t *h_st = reinterpret_cast<const int32_t *>(h_v + (size_t)n * L);
            parallel_ranges(L, [&](size_t k0, size_t k1) {
                for (size_t k = k0; k < k1; ++k) {
                    const size_t row = b0 + k;
                    if (alpha_out) alpha_out[row] = h_a[k];
                    if (v_out) for (int i = 0; i < n; ++i) v_out[row * n + i] = h_v[(size_t)i * L + k];
                    if (status_out) status_out[row] = h_st[k];
                }
            });
        });
}

// The measures of solution modes 3 and 4 for B configurations (optik_hip_manip_batch), staged as
// optik_robot_diff_ik_batch stages its rows.
int optik_robot_manipulability_batch(const optik_robot *r, int64_t B, const double *x, const double *ee16,
                                     double *w_out, double *c_out) {
    if (!r || !x) return set_err(-1, "null argument");
    if (B < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    // (B = 0: the kernel layer's refusals of the chain alone -- prismatic joints -- before anything is staged)
    if (optik_hip_manip_batch(c->chain, nullptr, nullptr, 0, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (B == 0 || (!w_out && !c_out)) return 0;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    // per row: q n doubles in; w 1 | c 1 doubles out
    const RowInput in[] = {{x, (size_t)r->n}};
    return stage_rows(
        c, B, in, 2 * sizeof(double), kRowChunk,
        [&](optik_hip_chain *ch, const double *d_q, int64_t L, double *d_w) {
            return optik_hip_manip_batch(ch, ee16 ? ee7 : nullptr, d_q, L, w_out ? d_w : nullptr,
                                         c_out ? d_w + L : nullptr, nullptr);
        },
        [&](size_t b0, size_t L, const double *h_w) {
            if (w_out) std::memcpy(w_out + b0, h_w, sizeof(double) * L);
            if (c_out) std::memcpy(c_out + b0, h_w + L, sizeof(double) * L);
        });
}

// The collision model and world (include/optik.h): checked on the host before any device work, kept with the robot
// and applied to every device chain it has (device_ctx applies them to the chains it creates later).
int optik_robot_set_collision_model(optik_robot *r, const int32_t *frames, const double *centers3, const double *radii,
                                    int32_t S, const int32_t *pairs2, int32_t P, double margin) {
    if (!r) return set_err(-1, "null argument");
    std::string err;
    if (optik::coll::check_model(r->n, frames, centers3, radii, S, pairs2, P, margin, err)) return set_err(-1, err);
    if (S > 0)
        for (int32_t t : r->types)
            if (t == optik_host::PRISMATIC)
                return set_err(-1, "collision: prismatic joints are not supported (IK refuses such chains)");
    std::lock_guard<std::mutex> lock(r->mu);
    r->world_epoch.fetch_add(1);  // (a roadmap checked against what is replaced here is stale)
    if (S > 0) {
        r->coll_frames.assign(frames, frames + S);
        r->coll_centers.assign(centers3, centers3 + 3 * (size_t)S);
        r->coll_radii.assign(radii, radii + S);
        if (P > 0) r->coll_pairs.assign(pairs2, pairs2 + 2 * (size_t)P);
        else r->coll_pairs.clear();
        r->coll_margin = margin;
    } else {
        r->coll_frames.clear(); r->coll_centers.clear(); r->coll_radii.clear(); r->coll_pairs.clear();
        r->coll_margin = 0.0;
    }
    return for_each_chain(r, [&](optik_hip_chain *ch) {
        return optik_hip_chain_set_collision_model(ch, frames, centers3, radii, S, pairs2, P, margin);
    });
}

int optik_robot_set_world(optik_robot *r, const double *spheres4, int32_t Ms, const double *boxes10, int32_t Mb) {
    if (!r) return set_err(-1, "null argument");
    std::string err;
    if (optik::coll::check_world(spheres4, Ms, boxes10, Mb, err)) return set_err(-1, err);
    std::lock_guard<std::mutex> lock(r->mu);
    r->world_epoch.fetch_add(1);  // (a roadmap checked against what is replaced here is stale)
    if (Ms > 0) r->world_spheres.assign(spheres4, spheres4 + 4 * (size_t)Ms);
    else r->world_spheres.clear();
    if (Mb > 0) r->world_boxes.assign(boxes10, boxes10 + 10 * (size_t)Mb);
    else r->world_boxes.clear();
    return for_each_chain(r, [&](optik_hip_chain *ch) {
        return optik_hip_chain_set_world(ch, spheres4, Ms, boxes10, Mb);
    });
}

int optik_robot_set_world_grid(optik_robot *r, const double *origin3, double voxel, int32_t nx, int32_t ny, int32_t nz,
                               const float *values) {
    if (!r) return set_err(-1, "null argument");
    const bool clear = !values && nx == 0 && ny == 0 && nz == 0;
    std::string err;
    if (!clear && optik::coll::check_grid(origin3, voxel, nx, ny, nz, values, true, err)) return set_err(-1, err);
    std::lock_guard<std::mutex> lock(r->mu);
    r->world_epoch.fetch_add(1);  // (a roadmap checked against what is replaced here is stale)
    if (clear) {
        r->grid_values.clear();
        r->grid_n[0] = r->grid_n[1] = r->grid_n[2] = 0;
    } else {
        r->grid_values.assign(values, values + (size_t)nx * (size_t)ny * (size_t)nz);
        for (int k = 0; k < 3; ++k) r->grid_origin[k] = origin3[k];
        r->grid_voxel = voxel;
        r->grid_n[0] = nx; r->grid_n[1] = ny; r->grid_n[2] = nz;
    }
    return for_each_chain(r, [&](optik_hip_chain *ch) {
        return optik_hip_chain_set_world_grid(ch, origin3, voxel, nx, ny, nz, values);
    });
}

int optik_robot_world_grid_bake(const optik_robot *r, const double *origin3, double voxel, int32_t nx, int32_t ny,
                                int32_t nz, float *values_out) {
    if (!r || !values_out) return set_err(-1, "null argument");
    std::string err;
    if (optik::coll::check_grid(origin3, voxel, nx, ny, nz, nullptr, false, err)) return set_err(-1, err);
    {
        std::lock_guard<std::mutex> lock(r->mu);
        if (r->world_spheres.empty() && r->world_boxes.empty()) return set_err(-1, optik::coll::bake_empty_msg());
    }
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    BatchGuard guard(c);
    if (!guard.ok()) return set_err(-1, kSetDeviceMsg);
    const size_t nodes = (size_t)nx * (size_t)ny * (size_t)nz;
    optik::DeviceBuf<float> d_out;  // (this call's own; freed on return, before the guard lets go)
    if (d_out.reserve(nodes) != hipSuccess) return set_err(-1, "bake buffer allocation failed");
    if (optik_hip_world_grid_bake(c->chain, origin3, voxel, nx, ny, nz, d_out.get(), nullptr))
        return set_err(-1, optik_hip_last_error());
    if (hipMemcpy(values_out, d_out.get(), sizeof(float) * nodes, hipMemcpyDeviceToHost) != hipSuccess)
        return set_err(-1, "download failed");
    return 0;
}

int optik_robot_world_grid_from_occupancy(const optik_robot *r, double voxel, int32_t nx, int32_t ny, int32_t nz,
                                          const uint8_t *occupied, double max_distance, float *values_out) {
    if (!r || !occupied || !values_out) return set_err(-1, "null argument");
    std::string err;
    const double zero3[3] = {0.0, 0.0, 0.0};
    if (optik::coll::check_grid(zero3, voxel, nx, ny, nz, nullptr, false, err)
        || optik::coll::check_max_distance(max_distance, err))
        return set_err(-1, err);
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    BatchGuard guard(c);
    if (!guard.ok()) return set_err(-1, kSetDeviceMsg);
    const size_t nodes = (size_t)nx * (size_t)ny * (size_t)nz;
    // one block: the values, then the occupancy bytes
    optik::DeviceBuf<uint8_t> block;
    if (block.reserve(5 * nodes) != hipSuccess) return set_err(-1, "occupancy buffer allocation failed");
    float *d_out = reinterpret_cast<float *>(block.get());
    uint8_t *d_occ = reinterpret_cast<uint8_t *>(d_out + nodes);
    if (hipMemcpy(d_occ, occupied, nodes, hipMemcpyHostToDevice) != hipSuccess) return set_err(-1, "upload failed");
    if (optik_hip_world_grid_from_occupancy(c->chain, voxel, nx, ny, nz, d_occ, max_distance, d_out, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (hipMemcpy(values_out, d_out, sizeof(float) * nodes, hipMemcpyDeviceToHost) != hipSuccess)
        return set_err(-1, "download failed");
    return 0;
}

int optik_robot_occupancy_from_points(const optik_robot *r, const double *origin3, double voxel, int32_t nx, int32_t ny,
                                      int32_t nz, const double *points3, int64_t N, const double *exclude4, int32_t E,
                                      uint8_t *occupied) {
    if (!r) return set_err(-1, "null argument");
    std::string err;
    if (optik::coll::check_grid(origin3, voxel, nx, ny, nz, nullptr, false, err) || optik::coll::check_cloud(N, E, err))
        return set_err(-1, err);
    if (N == 0) return 0;
    if (!points3 || !occupied || (E > 0 && !exclude4)) return set_err(-1, "null argument");
    for (int64_t k = 0; k < 4 * (int64_t)E; ++k)
        if (!std::isfinite(exclude4[k])) return set_err(-1, "occupancy from points: non-finite exclusion sphere");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    BatchGuard guard(c);
    if (!guard.ok()) return set_err(-1, kSetDeviceMsg);
    const size_t nodes = (size_t)nx * (size_t)ny * (size_t)nz;
    // one block: the points, the exclusion spheres, then the occupancy bytes
    const size_t doubles = 3 * (size_t)N + 4 * (size_t)E;
    optik::DeviceBuf<uint8_t> block;
    if (block.reserve(sizeof(double) * doubles + nodes) != hipSuccess)
        return set_err(-1, "point buffer allocation failed");
    double *d_pts = reinterpret_cast<double *>(block.get()), *d_exc = d_pts + 3 * (size_t)N;
    uint8_t *d_occ = reinterpret_cast<uint8_t *>(d_pts + doubles);
    if (hipMemcpy(d_pts, points3, sizeof(double) * 3 * (size_t)N, hipMemcpyHostToDevice) != hipSuccess
        || (E > 0 && hipMemcpy(d_exc, exclude4, sizeof(double) * 4 * (size_t)E, hipMemcpyHostToDevice) != hipSuccess)
        || hipMemcpy(d_occ, occupied, nodes, hipMemcpyHostToDevice) != hipSuccess)
        return set_err(-1, "upload failed");
    if (optik_hip_occupancy_from_points(c->chain, origin3, voxel, nx, ny, nz, d_pts, N, E > 0 ? d_exc : nullptr, E, d_occ,
                                        nullptr))
        return set_err(-1, optik_hip_last_error());
    if (hipMemcpy(occupied, d_occ, nodes, hipMemcpyDeviceToHost) != hipSuccess) return set_err(-1, "download failed");
    return 0;
}

int optik_robot_depth_integrate(const optik_robot *r, const double *origin3, double voxel, int32_t nx, int32_t ny,
                                int32_t nz, int16_t *map, const float *depth, int32_t F, int32_t H, int32_t W,
                                const double *intrinsics4, const double *poses16, const double *exclude4, int32_t E,
                                double z_near, double z_far, double band, int32_t hit, int32_t miss, int32_t e_min,
                                int32_t e_max) {
    if (!r) return set_err(-1, "null argument");
    std::string err;
    if (optik::coll::check_grid(origin3, voxel, nx, ny, nz, nullptr, false, err)
        || optik::coll::check_depth(F, H, W, E, z_near, z_far, band, hit, miss, e_min, e_max, err)
        || optik::coll::check_cameras(F, intrinsics4, poses16, err))
        return set_err(-1, err);
    if (!map || !depth || (E > 0 && !exclude4)) return set_err(-1, "null argument");
    for (int64_t k = 0; k < 4 * (int64_t)E; ++k)
        if (!std::isfinite(exclude4[k])) return set_err(-1, "depth integrate: non-finite exclusion sphere");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    BatchGuard guard(c);
    if (!guard.ok()) return set_err(-1, kSetDeviceMsg);
    const size_t nodes = (size_t)nx * (size_t)ny * (size_t)nz, pixels = (size_t)F * (size_t)H * (size_t)W;
    // one block: the exclusion spheres, the images, then the map
    optik::DeviceBuf<uint8_t> block;
    if (block.reserve(sizeof(double) * 4 * (size_t)E + sizeof(float) * pixels + sizeof(int16_t) * nodes) != hipSuccess)
        return set_err(-1, "depth buffer allocation failed");
    double *d_exc = reinterpret_cast<double *>(block.get());
    float *d_depth = reinterpret_cast<float *>(d_exc + 4 * (size_t)E);
    int16_t *d_map = reinterpret_cast<int16_t *>(d_depth + pixels);
    if ((E > 0 && hipMemcpy(d_exc, exclude4, sizeof(double) * 4 * (size_t)E, hipMemcpyHostToDevice) != hipSuccess)
        || hipMemcpy(d_depth, depth, sizeof(float) * pixels, hipMemcpyHostToDevice) != hipSuccess
        || hipMemcpy(d_map, map, sizeof(int16_t) * nodes, hipMemcpyHostToDevice) != hipSuccess)
        return set_err(-1, "upload failed");
    if (optik_hip_depth_integrate(c->chain, origin3, voxel, nx, ny, nz, d_map, d_depth, F, H, W, intrinsics4, poses16,
                                  E > 0 ? d_exc : nullptr, E, z_near, z_far, band, hit, miss, e_min, e_max, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (hipMemcpy(map, d_map, sizeof(int16_t) * nodes, hipMemcpyDeviceToHost) != hipSuccess)
        return set_err(-1, "download failed");
    return 0;
}

int optik_robot_occupancy_from_map(const optik_robot *r, int32_t nx, int32_t ny, int32_t nz, const int16_t *map,
                                   int32_t threshold, int32_t unknown_occupied, int32_t accumulate, uint8_t *occupied) {
    if (!r) return set_err(-1, "null argument");
    std::string err;
    const double zero3[3] = {0.0, 0.0, 0.0};
    if (optik::coll::check_grid(zero3, 1.0, nx, ny, nz, nullptr, false, err)
        || optik::coll::check_map_threshold(threshold, err))
        return set_err(-1, err);
    if (!map || !occupied) return set_err(-1, "null argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    BatchGuard guard(c);
    if (!guard.ok()) return set_err(-1, kSetDeviceMsg);
    const size_t nodes = (size_t)nx * (size_t)ny * (size_t)nz;
    // one block: the map, then the occupancy bytes
    optik::DeviceBuf<uint8_t> block;
    if (block.reserve(3 * nodes) != hipSuccess) return set_err(-1, "map buffer allocation failed");
    int16_t *d_map = reinterpret_cast<int16_t *>(block.get());
    uint8_t *d_occ = reinterpret_cast<uint8_t *>(d_map + nodes);
    if (hipMemcpy(d_map, map, sizeof(int16_t) * nodes, hipMemcpyHostToDevice) != hipSuccess
        || (accumulate && hipMemcpy(d_occ, occupied, nodes, hipMemcpyHostToDevice) != hipSuccess))
        return set_err(-1, "upload failed");
    if (optik_hip_occupancy_from_map(c->chain, nx, ny, nz, d_map, threshold, unknown_occupied, accumulate, d_occ, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (hipMemcpy(occupied, d_occ, nodes, hipMemcpyDeviceToHost) != hipSuccess) return set_err(-1, "download failed");
    return 0;
}

int optik_robot_world_grid_from_mesh(const optik_robot *r, const double *origin3, double voxel, int32_t nx, int32_t ny,
                                     int32_t nz, const double *tris9, int32_t M, double max_distance,
                                     float *values_out) {
    if (!r || !tris9 || !values_out) return set_err(-1, "null argument");
    std::string err;
    if (optik::coll::check_grid(origin3, voxel, nx, ny, nz, nullptr, false, err)
        || optik::coll::check_mesh(M, max_distance, tris9, err))
        return set_err(-1, err);
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    BatchGuard guard(c);
    if (!guard.ok()) return set_err(-1, kSetDeviceMsg);
    const size_t nodes = (size_t)nx * (size_t)ny * (size_t)nz;
    // one block: the triangles, then the values
    optik::DeviceBuf<uint8_t> block;
    if (block.reserve(sizeof(double) * 9 * (size_t)M + sizeof(float) * nodes) != hipSuccess)
        return set_err(-1, "mesh buffer allocation failed");
    double *d_tris = reinterpret_cast<double *>(block.get());
    float *d_out = reinterpret_cast<float *>(d_tris + 9 * (size_t)M);
    if (hipMemcpy(d_tris, tris9, sizeof(double) * 9 * (size_t)M, hipMemcpyHostToDevice) != hipSuccess)
        return set_err(-1, "upload failed");
    if (optik_hip_world_grid_from_mesh(c->chain, origin3, voxel, nx, ny, nz, d_tris, M, max_distance, d_out, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (hipMemcpy(values_out, d_out, sizeof(float) * nodes, hipMemcpyDeviceToHost) != hipSuccess)
        return set_err(-1, "download failed");
    return 0;
}

int optik_robot_sphere_fit(const optik_robot *r, const double *origin3, double voxel, int32_t nx, int32_t ny, int32_t nz,
                           const float *values, const double *points3, int64_t P, double pad, double slack, int32_t K,
                           int32_t *chosen_out, double *centers_out, double *radii_out, int32_t *gains_out,
                           int32_t *count_uncovered_out) {
    if (!r || !values || !points3 || !chosen_out || !centers_out || !radii_out || !gains_out || !count_uncovered_out)
        return set_err(-1, "null argument");
    std::string err;
    if (optik::coll::check_grid(origin3, voxel, nx, ny, nz, nullptr, false, err)
        || optik::coll::check_fit(P, pad, slack, K, points3, err))
        return set_err(-1, err);
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    BatchGuard guard(c);
    if (!guard.ok()) return set_err(-1, kSetDeviceMsg);
    const size_t nodes = (size_t)nx * (size_t)ny * (size_t)nz, k = (size_t)K;
    const size_t ws = optik::coll::fit_workspace_bytes((int64_t)nodes, P);
    // one block: the points, the centres and radii (doubles), then the values, the int32 outputs and the workspace
    optik::DeviceBuf<uint8_t> block;
    if (block.reserve(sizeof(double) * (3 * (size_t)P + 4 * k) + sizeof(float) * nodes + sizeof(int32_t) * (2 * k + 2) + ws)
        != hipSuccess)
        return set_err(-1, "sphere fit buffer allocation failed");
    double *d_pts = reinterpret_cast<double *>(block.get());
    double *d_cen = d_pts + 3 * (size_t)P, *d_rad = d_cen + 3 * k;
    float *d_val = reinterpret_cast<float *>(d_rad + k);
    int32_t *d_cho = reinterpret_cast<int32_t *>(d_val + nodes), *d_gai = d_cho + k, *d_cu = d_gai + k;
    void *d_ws = d_cu + 2;
    if (hipMemcpy(d_pts, points3, sizeof(double) * 3 * (size_t)P, hipMemcpyHostToDevice) != hipSuccess
        || hipMemcpy(d_val, values, sizeof(float) * nodes, hipMemcpyHostToDevice) != hipSuccess)
        return set_err(-1, "upload failed");
    if (optik_hip_sphere_fit(c->chain, origin3, voxel, nx, ny, nz, d_val, d_pts, P, pad, slack, K, d_cho, d_cen, d_rad,
                             d_gai, d_cu, d_ws, (int64_t)ws, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (hipMemcpy(centers_out, d_cen, sizeof(double) * 3 * k, hipMemcpyDeviceToHost) != hipSuccess
        || hipMemcpy(radii_out, d_rad, sizeof(double) * k, hipMemcpyDeviceToHost) != hipSuccess
        || hipMemcpy(chosen_out, d_cho, sizeof(int32_t) * k, hipMemcpyDeviceToHost) != hipSuccess
        || hipMemcpy(gains_out, d_gai, sizeof(int32_t) * k, hipMemcpyDeviceToHost) != hipSuccess
        || hipMemcpy(count_uncovered_out, d_cu, sizeof(int32_t) * 2, hipMemcpyDeviceToHost) != hipSuccess)
        return set_err(-1, "download failed");
    return 0;
}

int optik_robot_link_frames_batch(const optik_robot *r, int64_t B, const double *x, const double *ee16,
                                  double *frames16_out) {
    if (!r || !x || !frames16_out) return set_err(-1, "null argument");
    if (B < 0) return set_err(-1, "bad argument");
    DeviceCtx *c0 = device_ctx(r);
    if (!c0) return -1;
    // (B = 0: the kernel layer's refusals of the chain alone -- prismatic joints -- before anything is staged)
    if (optik_hip_link_frames_batch(c0->chain, nullptr, nullptr, 0, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (B == 0) return 0;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    const size_t nf = (size_t)r->n + 2;
    const RowInput in[] = {{x, (size_t)r->n}};
    return stage_rows(
        c0, B, in, sizeof(double) * 7 * nf, kRowChunk,
        [&](optik_hip_chain *ch, const double *d_q, int64_t L, double *d_out) {
            return optik_hip_link_frames_batch(ch, ee16 ? ee7 : nullptr, d_q, L, d_out, nullptr);
        },
        [&](size_t b0, size_t L, const double *h_out) {
            parallel_ranges(L * nf, [&](size_t k0, size_t k1) {
                for (size_t k = k0; k < k1; ++k) mat16_from_pose7(h_out + 7 * k, frames16_out + 16 * (b0 * nf + k));
            });
        });
}

int optik_robot_collision_batch(const optik_robot *r, int64_t B, const double *x, const double *ee16,
                                double *clearance_out, uint8_t *free_out) {
    if (!r || !x) return set_err(-1, "null argument");
    if (B < 0) return set_err(-1, "bad argument");
    DeviceCtx *c0 = device_ctx(r);
    if (!c0) return -1;
    if (optik_hip_collision_batch(c0->chain, nullptr, nullptr, 0, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (B == 0 || (!clearance_out && !free_out)) return 0;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    // per row: the clearance, then the free flag in the bytes of a second double
    const RowInput in[] = {{x, (size_t)r->n}};
    return stage_rows(
        c0, B, in, 2 * sizeof(double), kRowChunk,
        [&](optik_hip_chain *ch, const double *d_q, int64_t L, double *d_out) {
            return optik_hip_collision_batch(ch, ee16 ? ee7 : nullptr, d_q, L, d_out,
                                             reinterpret_cast<uint8_t *>(d_out + L), nullptr);
        },
        [&](size_t b0, size_t L, const double *h_out) {
            if (clearance_out) std::memcpy(clearance_out + b0, h_out, sizeof(double) * L);
            if (free_out) std::memcpy(free_out + b0, reinterpret_cast<const uint8_t *>(h_out + L), L);
        });
}

// The witness table of B configurations (optik_hip_collision_witness_batch), rows staged as the clearance's are.
int optik_robot_collision_witness_batch(const optik_robot *r, int64_t B, const double *x, const double *ee16,
                                        double *dist_out, double *grad_out, int32_t *witness_out) {
    if (!r || !x) return set_err(-1, "null argument");
    if (B < 0) return set_err(-1, "bad argument");
    DeviceCtx *c0 = device_ctx(r);
    if (!c0) return -1;
    if (optik_hip_collision_witness_batch(c0->chain, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (B == 0 || (!dist_out && !grad_out && !witness_out)) return 0;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    const size_t n = (size_t)r->n, nf = n + 2;
    // per row: dist F | grad F n doubles, then the witness words F 3 int32 out
    const RowInput in[] = {{x, n}};
    return stage_rows(
        c0, B, in, sizeof(double) * (nf + nf * n) + sizeof(int32_t) * 3 * nf, kWitnessChunk,
        [&](optik_hip_chain *ch, const double *d_q, int64_t L, double *d_out) {
            double *d_grad = d_out + nf * (size_t)L;
            return optik_hip_collision_witness_batch(ch, ee16 ? ee7 : nullptr, d_q, L, d_out, d_grad,
                                                     reinterpret_cast<int32_t *>(d_grad + nf * n * (size_t)L), nullptr);
        },
        [&](size_t b0, size_t L, const double *h_out) {
            const double *h_grad = h_out + nf * L;
            const int32_t *h_wit = reinterpret_cast<const int32_t *>(h_grad + nf * n * L);
            parallel_ranges(L, [&](size_t k0, size_t k1) {
                for (size_t k = k0; k < k1; ++k) {
                    const size_t row = b0 + k;
                    for (size_t f = 0; f < nf; ++f) {
                        if (dist_out) dist_out[row * nf + f] = h_out[f * L + k];
                        if (grad_out)
                            for (size_t j = 0; j < n; ++j)
                                grad_out[(row * nf + f) * n + j] = h_grad[(f * n + j) * L + k];
                        if (witness_out)
                            for (size_t i = 0; i < 3; ++i)
                                witness_out[(row * nf + f) * 3 + i] = h_wit[(f * 3 + i) * L + k];
                    }
                }
            });
        });
}

// B collision-avoiding diff_ik calls (optik_hip_diff_ik_avoid_batch), staged as optik_robot_diff_ik_batch stages its
// rows.  The single call is this with B = 1: one launch, the same kernel, so a row of a batch has its bits.
int optik_robot_diff_ik_avoid_batch(const optik_robot *r, int64_t B, const double *x0, const double *V_WE,
                                    const double *v_max, double influence, double safety, double gain,
                                    const double *ee16, double *alpha_out, double *v_out, int32_t *status_out) {
    if (!r || !x0 || !V_WE || !v_max) return set_err(-1, "null argument");
    if (B < 0) return set_err(-1, "bad argument");
    const int n = r->n;
    if (n > 8) return set_err(-1, kDiffIkMaxNMsg);
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    // (B = 0: the kernel layer's refusals of the chain and of influence / safety / gain, before anything is staged)
    if (optik_hip_diff_ik_avoid_batch(c->chain, nullptr, nullptr, nullptr, 0, nullptr, 0, 0, influence, safety, gain,
                                      nullptr, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (B == 0) return 0;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    const RowInput in[] = {{x0, (size_t)n}, {V_WE, 6}, {v_max, (size_t)n}};
    return stage_rows(
        c, B, in, sizeof(double) * (size_t)(n + 1) + sizeof(int32_t), kRowChunk,
        [&](optik_hip_chain *ch, const double *d_q, int64_t L, double *d_a) {
            const double *d_V = d_q + (size_t)n * L, *d_vm = d_V + 6 * L;
            double *d_v = d_a + L;
            return optik_hip_diff_ik_avoid_batch(ch, ee16 ? ee7 : nullptr, d_q, d_V, L, d_vm, L, L, influence, safety,
                                                 gain, d_a, d_v, reinterpret_cast<int32_t *>(d_v + (size_t)n * L),
                                                 nullptr);
        },
        [&](size_t b0, size_t L, const double *h_a) {
            const double *h_v = h_a + L;
            const int32_t *h_st = reinterpret_cast<const int32_t *>(h_v + (size_t)n * L);
            parallel_ranges(L, [&](size_t k0, size_t k1) {
                for (size_t k = k0; k < k1; ++k) {
                    const size_t row = b0 + k;
                    if (alpha_out) alpha_out[row] = h_a[k];
                    if (v_out) for (int i = 0; i < n; ++i) v_out[row * n + i] = h_v[(size_t)i * L + k];
                    if (status_out) status_out[row] = h_st[k];
                }
            });
        });
}

int optik_robot_diff_ik_avoid(const optik_robot *r, const double *x0, const double *V_WE, const double *v_max,
                              double influence, double safety, double gain, const double *ee16, double *alpha_out,
                              double *v_out) {
    int32_t status = 0;
    const int rc = optik_robot_diff_ik_avoid_batch(r, 1, x0, V_WE, v_max, influence, safety, gain, ee16, alpha_out,
                                                   v_out, &status);
    return rc < 0 ? rc : status;
}

// P paths through optik_hip_path_optimize.  The kernel layer takes the waypoints as optik_hip_ik_path writes them,
// [L][P][n], which is not the struct-of-arrays form stage_rows makes: the same steps here -- the batch block under
// its guard, one upload, one launch, one download per chunk of paths --, with the waypoint-major transpose.
int optik_robot_path_optimize(const optik_robot *r, int64_t P, int32_t L, const double *paths, int32_t iters,
                              double step, double w_smooth, double w_obs, double influence, double safety,
                              const double *ee16, double *paths_out, double *cost_first_out, double *cost_last_out,
                              double *clearance_out, int32_t *status_out) {
    if (!r || !paths) return set_err(-1, "null argument");
    if (P < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    // (P = 0: the kernel layer's refusals of the chain, of L, iters and the parameters, before anything is staged)
    if (optik_hip_path_optimize(c->chain, nullptr, nullptr, L, 0, iters, step, w_smooth, w_obs, influence, safety,
                                nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (P == 0 || (!paths_out && !cost_first_out && !cost_last_out && !clearance_out && !status_out)) return 0;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    BatchGuard guard(c);
    if (!guard.ok()) return set_err(-1, kSetDeviceMsg);
    const size_t n = (size_t)r->n, nl = (size_t)L, w = nl * n;
    const int64_t chunk = P < kPathChunk ? P : kPathChunk;
    // per path: the waypoints in; the waypoints, cost_first 3, cost_last 3, the clearance, and the status word in
    // the bytes of one more double out
    if (!reserve_batch(c, (2 * w + 8) * (size_t)chunk)) return set_err(-1, kBatchAllocMsg);
    for (int64_t b0 = 0; b0 < P; b0 += chunk) {
        const size_t Lc = (size_t)(P - b0 < chunk ? P - b0 : chunk);
        double *h_in = c->h_batch.get(), *h_out = h_in + w * Lc;
        double *d_in = c->d_batch.get(), *d_out = d_in + w * Lc;
        parallel_ranges(Lc, [&](size_t k0, size_t k1) {
            for (size_t k = k0; k < k1; ++k)
                for (size_t t = 0; t < nl; ++t)
                    std::memcpy(h_in + (t * Lc + k) * n, paths + (((size_t)b0 + k) * nl + t) * n, sizeof(double) * n);
        });
        if (hipMemcpyAsync(d_in, h_in, sizeof(double) * w * Lc, hipMemcpyHostToDevice, nullptr) != hipSuccess)
            return set_err(-1, "upload failed");
        double *d_cf = d_out + w * Lc, *d_cl = d_cf + 3 * Lc, *d_clr = d_cl + 3 * Lc;
        if (optik_hip_path_optimize(c->chain, ee16 ? ee7 : nullptr, d_in, L, (int64_t)Lc, iters, step, w_smooth, w_obs,
                                    influence, safety, d_out, d_cf, d_cl, d_clr, reinterpret_cast<int32_t *>(d_clr + Lc),
                                    nullptr))
            return set_err(-1, optik_hip_last_error());
        if (hipMemcpyAsync(h_out, d_out, sizeof(double) * (w + 8) * Lc, hipMemcpyDeviceToHost, nullptr) != hipSuccess
            || hipStreamSynchronize(nullptr) != hipSuccess)
            return set_err(-1, "download failed");
        const double *h_cf = h_out + w * Lc, *h_cl = h_cf + 3 * Lc, *h_clr = h_cl + 3 * Lc;
        const int32_t *h_st = reinterpret_cast<const int32_t *>(h_clr + Lc);
        parallel_ranges(Lc, [&](size_t k0, size_t k1) {
            for (size_t k = k0; k < k1; ++k) {
                const size_t row = (size_t)b0 + k;
                if (paths_out)
                    for (size_t t = 0; t < nl; ++t)
                        std::memcpy(paths_out + (row * nl + t) * n, h_out + (t * Lc + k) * n, sizeof(double) * n);
                if (cost_first_out) std::memcpy(cost_first_out + 3 * row, h_cf + 3 * k, 3 * sizeof(double));
                if (cost_last_out) std::memcpy(cost_last_out + 3 * row, h_cl + 3 * k, 3 * sizeof(double));
                if (clearance_out) clearance_out[row] = h_clr[k];
                if (status_out) status_out[row] = h_st[k];
            }
        });
    }
    return 0;
}

// P paths through optik_hip_path_optimize_constrained, staged as optik_robot_path_optimize stages its paths.
int optik_robot_path_optimize_constrained(const optik_robot *r, int64_t P, int32_t L, const double *paths,
                                          int32_t iters, double step, double w_smooth, double w_obs, double influence,
                                          double safety, const double *ref7, const double *lo6, const double *hi6,
                                          double ptol, int32_t piters, double damping, double max_step,
                                          const double *ee16, double *paths_out, double *cost_first_out,
                                          double *cost_last_out, double *clearance_out, int32_t *status_out,
                                          double *violation_out, int32_t *projected_out) {
    if (!r || !paths || !ref7 || !lo6 || !hi6) return set_err(-1, "null argument");
    if (P < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    // (P = 0: the kernel layer's refusals of the chain, of L, iters, the parameters and the constraint)
    if (optik_hip_path_optimize_constrained(c->chain, nullptr, nullptr, L, 0, iters, step, w_smooth, w_obs, influence,
                                            safety, ref7, lo6, hi6, ptol, piters, damping, max_step, nullptr, nullptr,
                                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (P == 0
        || (!paths_out && !cost_first_out && !cost_last_out && !clearance_out && !status_out && !violation_out
            && !projected_out))
        return 0;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    const size_t n = (size_t)r->n, w = (size_t)L * n;
    // per path out: the waypoints, cost_first 3, cost_last 3, the clearance, the violation, then the status word and
    // the two counters in the bytes of two more doubles
    return stage_paths(
        c, paths, nullptr, P, (size_t)L, n, w + 10,
        [&](const double *d_in, const int32_t *, int64_t Lc, double *d_out) {
            double *d_cf = d_out + w * (size_t)Lc, *d_cl = d_cf + 3 * Lc, *d_clr = d_cl + 3 * Lc, *d_v = d_clr + Lc;
            int32_t *d_st = reinterpret_cast<int32_t *>(d_v + Lc);
            return optik_hip_path_optimize_constrained(c->chain, ee16 ? ee7 : nullptr, d_in, L, Lc, iters, step, w_smooth,
                                                       w_obs, influence, safety, ref7, lo6, hi6, ptol, piters, damping,
                                                       max_step, d_out, d_cf, d_cl, d_clr, d_st, d_v, d_st + Lc, nullptr);
        },
        [&](size_t b0, size_t Lc, const double *h_out) {
            const double *h_cf = h_out + w * Lc, *h_cl = h_cf + 3 * Lc, *h_clr = h_cl + 3 * Lc, *h_v = h_clr + Lc;
            const int32_t *h_st = reinterpret_cast<const int32_t *>(h_v + Lc), *h_pr = h_st + Lc;
            if (paths_out) scatter_paths(paths_out, h_out, b0, Lc, (size_t)L, n);
            if (cost_first_out) std::memcpy(cost_first_out + 3 * b0, h_cf, sizeof(double) * 3 * Lc);
            if (cost_last_out) std::memcpy(cost_last_out + 3 * b0, h_cl, sizeof(double) * 3 * Lc);
            if (clearance_out) std::memcpy(clearance_out + b0, h_clr, sizeof(double) * Lc);
            if (violation_out) std::memcpy(violation_out + b0, h_v, sizeof(double) * Lc);
            if (status_out) std::memcpy(status_out + b0, h_st, sizeof(int32_t) * Lc);
            if (projected_out)
                for (size_t k = 0; k < Lc; ++k) {
                    projected_out[2 * (b0 + k)] = h_pr[k];
                    projected_out[2 * (b0 + k) + 1] = h_pr[Lc + k];
                }
        });
}

// B rows through optik_hip_collision_repair_batch.
int optik_robot_collision_repair_batch(const optik_robot *r, int64_t B, const double *x, double influence,
                                       double safety, double step, int32_t iters, double max_move, const double *ref7,
                                       const double *lo6, const double *hi6, double ptol, int32_t piters,
                                       double damping, double project_max_step, const double *ee16, double *x_out,
                                       double *clearance_out, double *violation_out, double *moved_out,
                                       int32_t *status_out, int32_t *iterations_out) {
    if (!r) return set_err(-1, "null argument");
    if (B < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    // (B = 0: the kernel layer's refusals of the chain, the parameters, the box and the missing model)
    if (optik_hip_collision_repair_batch(c->chain, nullptr, nullptr, 0, influence, safety, step, iters, max_move, ref7,
                                         lo6, hi6, ptol, piters, damping, project_max_step, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (B == 0 || (!x_out && !clearance_out && !violation_out && !moved_out && !status_out && !iterations_out)) return 0;
    if (!x) return set_err(-1, "null argument");
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    const size_t n = (size_t)r->n;
    // per row: x n doubles in; x n | clearance, violation, moved 3 doubles, then the status and iteration words in one
    // more double out
    const RowInput in[] = {{x, n}};
    return stage_rows(
        c, B, in, sizeof(double) * (n + 4), kRowChunk,
        [&](optik_hip_chain *ch, const double *d_q, int64_t L, double *d_x) {
            double *d_c = d_x + n * (size_t)L;
            int32_t *d_st = reinterpret_cast<int32_t *>(d_c + 3 * (size_t)L);
            const optik_hip_collision_repair_outputs o{d_x, d_c, d_c + L, d_c + 2 * (size_t)L, d_st, d_st + L};
            return optik_hip_collision_repair_batch(ch, ee16 ? ee7 : nullptr, d_q, L, influence, safety, step, iters,
                                                    max_move, ref7, lo6, hi6, ptol, piters, damping, project_max_step,
                                                    &o, nullptr);
        },
        [&](size_t b0, size_t L, const double *h_x) {
            const double *h_c = h_x + n * L;
            const int32_t *h_st = reinterpret_cast<const int32_t *>(h_c + 3 * L);
            if (x_out)
                parallel_ranges(L, [&](size_t k0, size_t k1) {
                    for (size_t k = k0; k < k1; ++k)
                        for (size_t i = 0; i < n; ++i) x_out[(b0 + k) * n + i] = h_x[i * L + k];
                });
            if (clearance_out) std::memcpy(clearance_out + b0, h_c, sizeof(double) * L);
            if (violation_out) std::memcpy(violation_out + b0, h_c + L, sizeof(double) * L);
            if (moved_out) std::memcpy(moved_out + b0, h_c + 2 * L, sizeof(double) * L);
            if (status_out) std::memcpy(status_out + b0, h_st, sizeof(int32_t) * L);
            if (iterations_out) std::memcpy(iterations_out + b0, h_st + L, sizeof(int32_t) * L);
        });
}

// P paths through optik_hip_path_shortcut, staged as optik_robot_path_optimize stages its paths.
int optik_robot_path_shortcut(const optik_robot *r, int64_t P, int32_t L, const double *paths, const int32_t *lens,
                              int32_t vertices, double resolution, double hop_penalty, int32_t Lout,
                              const double *ee16, double *paths_out, int32_t *len_out, double *cost_out,
                              double *cost_in_out, int32_t *status_out) {
    if (!r || !paths) return set_err(-1, "null argument");
    if (P < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    // (P = 0: the kernel layer's refusals of the chain, the sizes, the resolution and the penalty)
    if (optik_hip_path_shortcut(c->chain, nullptr, nullptr, nullptr, L, 0, vertices, resolution, hop_penalty, Lout,
                                nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (P == 0 || (!paths_out && !len_out && !cost_out && !cost_in_out && !status_out)) return 0;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    const size_t n = (size_t)r->n, wo = (size_t)Lout * n;
    // per path out: the waypoints, cost, cost_in, then len and status in one more double
    return stage_paths(
        c, paths, lens, P, (size_t)L, n, wo + 3,
        [&](const double *d_in, const int32_t *d_len, int64_t Lc, double *d_out) {
            double *d_cost = d_out + wo * (size_t)Lc, *d_cin = d_cost + Lc;
            int32_t *d_lo = reinterpret_cast<int32_t *>(d_cin + Lc);
            return optik_hip_path_shortcut(c->chain, ee16 ? ee7 : nullptr, d_in, d_len, L, Lc, vertices, resolution,
                                           hop_penalty, Lout, d_out, d_lo, d_cost, d_cin, d_lo + Lc, nullptr);
        },
        [&](size_t b0, size_t Lc, const double *h_out) {
            const double *h_cost = h_out + wo * Lc, *h_cin = h_cost + Lc;
            const int32_t *h_lo = reinterpret_cast<const int32_t *>(h_cin + Lc);
            if (paths_out) scatter_paths(paths_out, h_out, b0, Lc, (size_t)Lout, n);
            if (cost_out) std::memcpy(cost_out + b0, h_cost, sizeof(double) * Lc);
            if (cost_in_out) std::memcpy(cost_in_out + b0, h_cin, sizeof(double) * Lc);
            if (len_out) std::memcpy(len_out + b0, h_lo, sizeof(int32_t) * Lc);
            if (status_out) std::memcpy(status_out + b0, h_lo + Lc, sizeof(int32_t) * Lc);
        });
}

// P paths through optik_hip_path_resample.
int optik_robot_path_resample(const optik_robot *r, int64_t P, int32_t L, const double *paths, const int32_t *lens,
                              int32_t Lout, double *paths_out, int32_t *status_out) {
    if (!r || !paths) return set_err(-1, "null argument");
    if (P < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    if (optik_hip_path_resample(c->chain, nullptr, nullptr, L, 0, Lout, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (P == 0 || (!paths_out && !status_out)) return 0;
    const size_t n = (size_t)r->n, wo = (size_t)Lout * n;
    // per path out: the waypoints, then the status word in the bytes of one more double
    return stage_paths(
        c, paths, lens, P, (size_t)L, n, wo + 1,
        [&](const double *d_in, const int32_t *d_len, int64_t Lc, double *d_out) {
            return optik_hip_path_resample(c->chain, d_in, d_len, L, Lc, Lout, d_out,
                                           reinterpret_cast<int32_t *>(d_out + wo * (size_t)Lc), nullptr);
        },
        [&](size_t b0, size_t Lc, const double *h_out) {
            if (paths_out) scatter_paths(paths_out, h_out, b0, Lc, (size_t)Lout, n);
            if (status_out) std::memcpy(status_out + b0, h_out + wo * Lc, sizeof(int32_t) * Lc);
        });
}

// P paths through optik_hip_path_shortcut_constrained: optik_robot_path_shortcut's staging with one more double out per
// path, its two projection counters.
int optik_robot_path_shortcut_constrained(const optik_robot *r, int64_t P, int32_t L, const double *paths,
                                          const int32_t *lens, int32_t vertices, double resolution, double hop_penalty,
                                          int32_t Lout, const double *ref7, const double *lo6, const double *hi6,
                                          double tol, double ptol, int32_t piters, double damping, double max_step,
                                          const double *ee16, double *paths_out, int32_t *len_out, double *cost_out,
                                          double *cost_in_out, int32_t *status_out, int32_t *projected_out) {
    if (!r || !paths || !ref7 || !lo6 || !hi6) return set_err(-1, "null argument");
    if (P < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    // (P = 0: the kernel layer's refusals of the chain, the sizes, the resolution, the penalty and the constraint)
    if (optik_hip_path_shortcut_constrained(c->chain, nullptr, nullptr, nullptr, L, 0, vertices, resolution, hop_penalty,
                                            Lout, ref7, lo6, hi6, tol, ptol, piters, damping, max_step, nullptr, nullptr,
                                            nullptr, nullptr, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (P == 0 || (!paths_out && !len_out && !cost_out && !cost_in_out && !status_out && !projected_out)) return 0;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    const size_t n = (size_t)r->n, wo = (size_t)Lout * n;
    // per path out: the waypoints, cost, cost_in, then len and status in one more double, the counters in another
    return stage_paths(
        c, paths, lens, P, (size_t)L, n, wo + 4,
        [&](const double *d_in, const int32_t *d_len, int64_t Lc, double *d_out) {
            double *d_cost = d_out + wo * (size_t)Lc, *d_cin = d_cost + Lc;
            int32_t *d_lo = reinterpret_cast<int32_t *>(d_cin + Lc);
            return optik_hip_path_shortcut_constrained(c->chain, ee16 ? ee7 : nullptr, d_in, d_len, L, Lc, vertices,
                                                       resolution, hop_penalty, Lout, ref7, lo6, hi6, tol, ptol, piters,
                                                       damping, max_step, d_out, d_lo, d_cost, d_cin, d_lo + Lc,
                                                       d_lo + 2 * Lc, nullptr);
        },
        [&](size_t b0, size_t Lc, const double *h_out) {
            const double *h_cost = h_out + wo * Lc, *h_cin = h_cost + Lc;
            const int32_t *h_lo = reinterpret_cast<const int32_t *>(h_cin + Lc), *h_pr = h_lo + 2 * Lc;
            if (paths_out) scatter_paths(paths_out, h_out, b0, Lc, (size_t)Lout, n);
            if (cost_out) std::memcpy(cost_out + b0, h_cost, sizeof(double) * Lc);
            if (cost_in_out) std::memcpy(cost_in_out + b0, h_cin, sizeof(double) * Lc);
            if (len_out) std::memcpy(len_out + b0, h_lo, sizeof(int32_t) * Lc);
            if (status_out) std::memcpy(status_out + b0, h_lo + Lc, sizeof(int32_t) * Lc);
            if (projected_out)
                for (size_t k = 0; k < Lc; ++k) {
                    projected_out[2 * (b0 + k)] = h_pr[k];
                    projected_out[2 * (b0 + k) + 1] = h_pr[Lc + k];
                }
        });
}

// P paths through optik_hip_path_resample_constrained.
int optik_robot_path_resample_constrained(const optik_robot *r, int64_t P, int32_t L, const double *paths,
                                          const int32_t *lens, int32_t Lout, const double *ref7, const double *lo6,
                                          const double *hi6, double ptol, int32_t piters, double damping,
                                          double max_step, const double *ee16, double *paths_out, int32_t *status_out,
                                          int32_t *projected_out) {
    if (!r || !paths || !ref7 || !lo6 || !hi6) return set_err(-1, "null argument");
    if (P < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    if (optik_hip_path_resample_constrained(c->chain, nullptr, nullptr, nullptr, L, 0, Lout, ref7, lo6, hi6, ptol, piters,
                                            damping, max_step, nullptr, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (P == 0 || (!paths_out && !status_out && !projected_out)) return 0;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    const size_t n = (size_t)r->n, wo = (size_t)Lout * n;
    // per path out: the waypoints, then the status word and the two counters in the bytes of two more doubles
    return stage_paths(
        c, paths, lens, P, (size_t)L, n, wo + 2,
        [&](const double *d_in, const int32_t *d_len, int64_t Lc, double *d_out) {
            int32_t *d_st = reinterpret_cast<int32_t *>(d_out + wo * (size_t)Lc);
            return optik_hip_path_resample_constrained(c->chain, ee16 ? ee7 : nullptr, d_in, d_len, L, Lc, Lout, ref7,
                                                       lo6, hi6, ptol, piters, damping, max_step, d_out, d_st,
                                                       d_st + Lc, nullptr);
        },
        [&](size_t b0, size_t Lc, const double *h_out) {
            const int32_t *h_st = reinterpret_cast<const int32_t *>(h_out + wo * Lc), *h_pr = h_st + Lc;
            if (paths_out) scatter_paths(paths_out, h_out, b0, Lc, (size_t)Lout, n);
            if (status_out) std::memcpy(status_out + b0, h_st, sizeof(int32_t) * Lc);
            if (projected_out)
                for (size_t k = 0; k < Lc; ++k) {
                    projected_out[2 * (b0 + k)] = h_pr[k];
                    projected_out[2 * (b0 + k) + 1] = h_pr[Lc + k];
                }
        });
}

// P paths through optik_hip_path_time; the limits travel behind the lengths in the batch block.
int optik_robot_path_time(const optik_robot *r, int64_t P, int32_t L, const double *paths, const int32_t *lens,
                          const double *v_max, const double *a_max, double *times_out, double *vel_out,
                          double *acc_out, double *duration_out, int32_t *status_out) {
    if (!r || !paths || !v_max || !a_max) return set_err(-1, "null argument");
    if (P < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    // (P = 0: the kernel layer's refusals of the chain and the sizes)
    if (optik_hip_path_time(c->chain, nullptr, nullptr, L, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (P == 0 || (!times_out && !vel_out && !acc_out && !duration_out && !status_out)) return 0;
    const size_t n = (size_t)r->n, nl = (size_t)L, w = nl * n;
    std::vector<double> limits(v_max, v_max + n);
    limits.insert(limits.end(), a_max, a_max + n);
    // per path out: times [L], velocities [L][n], accelerations [L][n], the duration, then the status in one more double
    return stage_paths(
        c, paths, lens, P, nl, n, nl + 2 * w + 2,
        [&](const double *d_in, const int32_t *d_len, int64_t Lc, double *d_out) {
            const double *d_lim = d_in + paths_extra_offset(nl, n, (size_t)Lc);
            double *d_t = d_out, *d_qd = d_t + nl * (size_t)Lc, *d_qdd = d_qd + w * (size_t)Lc,
                   *d_dur = d_qdd + w * (size_t)Lc;
            return optik_hip_path_time(c->chain, d_in, d_len, L, Lc, d_lim, d_lim + n, d_t, d_qd, d_qdd, nullptr, d_dur,
                                       reinterpret_cast<int32_t *>(d_dur + Lc), nullptr);
        },
        [&](size_t b0, size_t Lc, const double *h_out) {
            const double *h_t = h_out, *h_qd = h_t + nl * Lc, *h_qdd = h_qd + w * Lc, *h_dur = h_qdd + w * Lc;
            if (times_out) scatter_paths(times_out, h_t, b0, Lc, nl, 1);
            if (vel_out) scatter_paths(vel_out, h_qd, b0, Lc, nl, n);
            if (acc_out) scatter_paths(acc_out, h_qdd, b0, Lc, nl, n);
            if (duration_out) std::memcpy(duration_out + b0, h_dur, sizeof(double) * Lc);
            if (status_out) std::memcpy(status_out + b0, h_dur + Lc, sizeof(int32_t) * Lc);
        },
        limits.data(), limits.size());
}

// P paths through optik_hip_path_time_tool, exactly as optik_robot_path_time goes; the tool's limits are host arguments.
int optik_robot_path_time_tool(const optik_robot *r, int64_t P, int32_t L, const double *paths, const int32_t *lens,
                               const double *v_max, const double *a_max, const double *tool_limits4,
                               const double *ee16, double *times_out, double *vel_out, double *acc_out,
                               double *duration_out, int32_t *status_out, double *tool_speed_out,
                               double *tool_accel_out, double *tool_wspeed_out) {
    if (!r || !paths || !v_max || !a_max || !tool_limits4) return set_err(-1, "null argument");
    if (P < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    // (P = 0: the kernel layer's refusals of the chain, the sizes and the tool limits)
    if (optik_hip_path_time_tool(c->chain, nullptr, nullptr, L, 0, nullptr, nullptr, tool_limits4, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (P == 0 || (!times_out && !vel_out && !acc_out && !duration_out && !status_out && !tool_speed_out
                   && !tool_accel_out && !tool_wspeed_out))
        return 0;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    const size_t n = (size_t)r->n, nl = (size_t)L, w = nl * n;
    std::vector<double> limits(v_max, v_max + n);
    limits.insert(limits.end(), a_max, a_max + n);
    // per path out: times [L], velocities [L][n], accelerations [L][n], tool speed [L], tool acceleration [L][2], tool
    // angular speed [L], the duration, then the status in one more double
    return stage_paths(
        c, paths, lens, P, nl, n, 5 * nl + 2 * w + 2,
        [&](const double *d_in, const int32_t *d_len, int64_t Lc, double *d_out) {
            const double *d_lim = d_in + paths_extra_offset(nl, n, (size_t)Lc);
            double *d_t = d_out, *d_qd = d_t + nl * (size_t)Lc, *d_qdd = d_qd + w * (size_t)Lc,
                   *d_ts = d_qdd + w * (size_t)Lc, *d_ta = d_ts + nl * (size_t)Lc, *d_tw = d_ta + 2 * nl * (size_t)Lc,
                   *d_dur = d_tw + nl * (size_t)Lc;
            return optik_hip_path_time_tool(c->chain, d_in, d_len, L, Lc, d_lim, d_lim + n, tool_limits4,
                                            ee16 ? ee7 : nullptr, d_t, d_qd, d_qdd, nullptr, d_dur,
                                            reinterpret_cast<int32_t *>(d_dur + Lc), d_ts, d_ta, d_tw, nullptr);
        },
        [&](size_t b0, size_t Lc, const double *h_out) {
            const double *h_t = h_out, *h_qd = h_t + nl * Lc, *h_qdd = h_qd + w * Lc, *h_ts = h_qdd + w * Lc,
                         *h_ta = h_ts + nl * Lc, *h_tw = h_ta + 2 * nl * Lc, *h_dur = h_tw + nl * Lc;
            if (times_out) scatter_paths(times_out, h_t, b0, Lc, nl, 1);
            if (vel_out) scatter_paths(vel_out, h_qd, b0, Lc, nl, n);
            if (acc_out) scatter_paths(acc_out, h_qdd, b0, Lc, nl, n);
            if (tool_speed_out) scatter_paths(tool_speed_out, h_ts, b0, Lc, nl, 1);
            if (tool_accel_out) scatter_paths(tool_accel_out, h_ta, b0, Lc, nl, 2);
            if (tool_wspeed_out) scatter_paths(tool_wspeed_out, h_tw, b0, Lc, nl, 1);
            if (duration_out) std::memcpy(duration_out + b0, h_dur, sizeof(double) * Lc);
            if (status_out) std::memcpy(status_out + b0, h_dur + Lc, sizeof(int32_t) * Lc);
        },
        limits.data(), limits.size());
}

// P timed paths through optik_hip_path_time_spline.  The times travel waypoint-major like the paths; the three limit
// vectors, the lengths and the input statuses behind them.
int optik_robot_path_time_spline(const optik_robot *r, int64_t P, int32_t L, const double *paths, const int32_t *lens,
                                 const double *times, const int32_t *status, const double *v_max, const double *a_max,
                                 const double *j_max, double *times_out, double *vel_out, double *acc_out,
                                 double *duration_out, double *factor_out, double *ratios_out, int32_t *status_out) {
    if (!r || !paths || !times || !v_max || !a_max || !j_max) return set_err(-1, "null argument");
    if (P < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    // (P = 0: the kernel layer's refusals of the chain and the sizes)
    if (optik_hip_path_time_spline(c->chain, nullptr, nullptr, L, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (P == 0 || (!times_out && !vel_out && !acc_out && !duration_out && !factor_out && !ratios_out && !status_out))
        return 0;
    BatchGuard guard(c);
    if (!guard.ok()) return set_err(-1, kSetDeviceMsg);
    const size_t n = (size_t)r->n, nl = (size_t)L, w = nl * n;
    // per path in: the path, its times, its length and status (two int32: one double); out: times [L], velocities and
    // accelerations [L][n], the duration, the factor, three ratios, then the status in one more double
    const size_t per_in = w + nl + 1, per_out = nl + 2 * w + 6;
    const int64_t chunk = P < kPathChunk ? P : kPathChunk;
    if (!reserve_batch(c, (per_in + per_out) * (size_t)chunk + 3 * n)) return set_err(-1, kBatchAllocMsg);
    for (int64_t b0 = 0; b0 < P; b0 += chunk) {
        const size_t Lc = (size_t)(P - b0 < chunk ? P - b0 : chunk);
        // in: paths [L][Lc][n] | times [L][Lc] | v_max, a_max, j_max [n] | lens [Lc], status [Lc] (int32)
        const size_t in_doubles = per_in * Lc + 3 * n;
        double *h_in = c->h_batch.get(), *h_out = h_in + in_doubles;
        double *d_in = c->d_batch.get(), *d_out = d_in + in_doubles;
        double *h_t = h_in + w * Lc, *h_lim = h_t + nl * Lc;
        int32_t *h_len = reinterpret_cast<int32_t *>(h_lim + 3 * n);
        parallel_ranges(Lc, [&](size_t k0, size_t k1) {
            for (size_t k = k0; k < k1; ++k)
                for (size_t t = 0; t < nl; ++t) {
                    const size_t src = ((size_t)b0 + k) * nl + t;
                    std::memcpy(h_in + (t * Lc + k) * n, paths + src * n, sizeof(double) * n);
                    h_t[t * Lc + k] = times[src];
                }
        });
        std::memcpy(h_lim, v_max, sizeof(double) * n);
        std::memcpy(h_lim + n, a_max, sizeof(double) * n);
        std::memcpy(h_lim + 2 * n, j_max, sizeof(double) * n);
        for (size_t k = 0; k < Lc; ++k) {
            h_len[k] = lens ? lens[(size_t)b0 + k] : L;
            h_len[Lc + k] = status ? status[(size_t)b0 + k] : 0;
        }
        if (hipMemcpyAsync(d_in, h_in, sizeof(double) * in_doubles, hipMemcpyHostToDevice, nullptr) != hipSuccess)
            return set_err(-1, "upload failed");
        const double *d_tin = d_in + w * Lc, *d_lim = d_tin + nl * Lc;
        const int32_t *d_len = reinterpret_cast<const int32_t *>(d_lim + 3 * n);
        double *d_t = d_out, *d_qd = d_t + nl * Lc, *d_qdd = d_qd + w * Lc, *d_dur = d_qdd + w * Lc, *d_fac = d_dur + Lc,
               *d_rat = d_fac + Lc;
        if (optik_hip_path_time_spline(c->chain, d_in, d_len, L, (int64_t)Lc, d_tin, d_len + Lc, d_lim, d_lim + n,
                                       d_lim + 2 * n, d_t, d_qd, d_qdd, d_dur, d_fac, d_rat,
                                       reinterpret_cast<int32_t *>(d_rat + 3 * Lc), nullptr))
            return set_err(-1, optik_hip_last_error());
        if (hipMemcpyAsync(h_out, d_out, sizeof(double) * per_out * Lc, hipMemcpyDeviceToHost, nullptr) != hipSuccess
            || hipStreamSynchronize(nullptr) != hipSuccess)
            return set_err(-1, "download failed");
        const double *o_t = h_out, *o_qd = o_t + nl * Lc, *o_qdd = o_qd + w * Lc, *o_dur = o_qdd + w * Lc,
                     *o_fac = o_dur + Lc, *o_rat = o_fac + Lc;
        if (times_out) scatter_paths(times_out, o_t, (size_t)b0, Lc, nl, 1);
        if (vel_out) scatter_paths(vel_out, o_qd, (size_t)b0, Lc, nl, n);
        if (acc_out) scatter_paths(acc_out, o_qdd, (size_t)b0, Lc, nl, n);
        if (duration_out) std::memcpy(duration_out + b0, o_dur, sizeof(double) * Lc);
        if (factor_out) std::memcpy(factor_out + b0, o_fac, sizeof(double) * Lc);
        if (ratios_out) std::memcpy(ratios_out + 3 * b0, o_rat, sizeof(double) * 3 * Lc);
        if (status_out) std::memcpy(status_out + b0, o_rat + 3 * Lc, sizeof(int32_t) * Lc);
    }
    return 0;
}

// P timed paths through optik_hip_trajectory_sample.  A path's samples are 2 T n doubles -- 7 MB at T = 65 536, n = 7 --
// so the chunk is sized by the bytes of its results (kSampleChunkDoubles), not by kPathChunk.
int optik_robot_trajectory_sample(const optik_robot *r, int64_t P, int32_t L, const double *paths, const int32_t *lens,
                                  const double *times, const double *velocities, const int32_t *status, double dt,
                                  int32_t T, double *q_out, double *qd_out) {
    if (!r || !paths || !times || !velocities || !status) return set_err(-1, "null argument");
    if (P < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    if (optik_hip_trajectory_sample(c->chain, nullptr, nullptr, L, 0, nullptr, nullptr, nullptr, dt, T, nullptr, nullptr,
                                    nullptr))
        return set_err(-1, optik_hip_last_error());
    if (P == 0 || (!q_out && !qd_out)) return 0;
    BatchGuard guard(c);
    if (!guard.ok()) return set_err(-1, kSetDeviceMsg);
    const size_t n = (size_t)r->n, nl = (size_t)L, w = nl * n, wo = (size_t)T * n;
    const size_t per_path = 2 * w + nl + 1 + 2 * wo;
    int64_t chunk = (int64_t)(kSampleChunkDoubles / per_path);
    chunk = chunk < 1 ? 1 : (chunk > kPathChunk ? kPathChunk : chunk);
    if (P < chunk) chunk = P;
    if (!reserve_batch(c, per_path * (size_t)chunk)) return set_err(-1, kBatchAllocMsg);
    for (int64_t b0 = 0; b0 < P; b0 += chunk) {
        const size_t Lc = (size_t)(P - b0 < chunk ? P - b0 : chunk);
        // in: paths [L][Lc][n] | velocities [L][Lc][n] | times [L][Lc] | lens [Lc], status [Lc] (int32)
        const size_t in_doubles = 2 * w * Lc + nl * Lc + Lc;
        double *h_in = c->h_batch.get(), *h_out = h_in + in_doubles;
        double *d_in = c->d_batch.get(), *d_out = d_in + in_doubles;
        double *h_qd = h_in + w * Lc, *h_t = h_qd + w * Lc;
        int32_t *h_len = reinterpret_cast<int32_t *>(h_t + nl * Lc);
        parallel_ranges(Lc, [&](size_t k0, size_t k1) {
            for (size_t k = k0; k < k1; ++k)
                for (size_t t = 0; t < nl; ++t) {
                    const size_t src = ((size_t)b0 + k) * nl + t;
                    std::memcpy(h_in + (t * Lc + k) * n, paths + src * n, sizeof(double) * n);
                    std::memcpy(h_qd + (t * Lc + k) * n, velocities + src * n, sizeof(double) * n);
                    h_t[t * Lc + k] = times[src];
                }
        });
        for (size_t k = 0; k < Lc; ++k) h_len[k] = lens ? lens[(size_t)b0 + k] : L;
        std::memcpy(h_len + Lc, status + b0, sizeof(int32_t) * Lc);
        if (hipMemcpyAsync(d_in, h_in, sizeof(double) * in_doubles, hipMemcpyHostToDevice, nullptr) != hipSuccess)
            return set_err(-1, "upload failed");
        const double *d_qd = d_in + w * Lc, *d_t = d_qd + w * Lc;
        const int32_t *d_len = reinterpret_cast<const int32_t *>(d_t + nl * Lc);
        if (optik_hip_trajectory_sample(c->chain, d_in, d_len, L, (int64_t)Lc, d_t, d_qd, d_len + Lc, dt, T, d_out,
                                        d_out + wo * Lc, nullptr))
            return set_err(-1, optik_hip_last_error());
        if (hipMemcpyAsync(h_out, d_out, sizeof(double) * 2 * wo * Lc, hipMemcpyDeviceToHost, nullptr) != hipSuccess
            || hipStreamSynchronize(nullptr) != hipSuccess)
            return set_err(-1, "download failed");
        if (q_out) scatter_paths(q_out, h_out, (size_t)b0, Lc, (size_t)T, n);
        if (qd_out) scatter_paths(qd_out, h_out + wo * Lc, (size_t)b0, Lc, (size_t)T, n);
    }
    return 0;
}

// The roadmap (include/optik.h): N seeds of the restart generator as nodes, their k nearest others and the checked
// motions to them, kept in the first device's context.  Everything stays on the device but the weights' count.
int64_t optik_robot_roadmap_build(optik_robot *r, int32_t N, int32_t k, double resolution, uint64_t first) {
    if (!r) return set_err(-1, "null argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    // (Q = 0: the kernel layer's refusals of N, k, the resolution and the chain, before anything is allocated)
    if (optik_hip_roadmap_knn(c->chain, nullptr, 0, nullptr, N, k, 1, nullptr, nullptr, nullptr)
        || optik_hip_roadmap_edges(c->chain, nullptr, nullptr, 0, nullptr, N, nullptr, 1, resolution, 0, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    BatchGuard guard(c);
    if (!guard.ok()) return set_err(-1, kSetDeviceMsg);
    const uint64_t epoch = r->world_epoch.load();
    const size_t n = (size_t)r->n, cells = (size_t)k * (size_t)N;
    c->rm_N = 0;
    if (c->rm_graph.reserve(n * (size_t)N + cells) != hipSuccess || c->rm_nbr.reserve(cells) != hipSuccess
        || !reserve_batch(c, cells))
        return set_err(-1, kBatchAllocMsg);
    double *d_nodes = c->rm_graph.get(), *d_w = d_nodes + n * (size_t)N;
    if (optik_hip_seed_batch(c->chain, first, N, d_nodes, nullptr)
        || optik_hip_roadmap_knn(c->chain, d_nodes, N, d_nodes, N, k, 1, c->rm_nbr.get(), nullptr, nullptr)
        || optik_hip_roadmap_edges(c->chain, nullptr, d_nodes, N, d_nodes, N, c->rm_nbr.get(), k, resolution, 0, d_w,
                                   nullptr))
        return set_err(-1, optik_hip_last_error());
    double *h_w = c->h_batch.get();
    if (hipMemcpyAsync(h_w, d_w, sizeof(double) * cells, hipMemcpyDeviceToHost, nullptr) != hipSuccess
        || hipStreamSynchronize(nullptr) != hipSuccess)
        return set_err(-1, "download failed");
    int64_t edges = 0;
    for (size_t e = 0; e < cells; ++e) edges += std::isfinite(h_w[e]) ? 1 : 0;
    c->rm_N = N; c->rm_k = k; c->rm_h = resolution; c->rm_epoch = epoch; c->rm_lazy = false;
    return edges;
}

// Q plans over the robot's roadmap: the rows are staged as every row batch stages them, and per chunk the two
// neighbour searches, the three edge checks and the query run back to back on the device.
int optik_robot_roadmap_plan(const optik_robot *r, const double *starts, const double *goals, int64_t Q, int32_t Lmax,
                             double *paths_out, int32_t *len_out, double *cost_out, int32_t *status_out) {
    if (!r || !starts || !goals) return set_err(-1, "null argument");
    if (Q < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    int32_t N, k;
    double h;
    {
        // (the setters bump the epoch before they take this mutex for the chain: a plan either sees the new count
        // here or has the chain to itself until it is done)
        std::lock_guard<std::mutex> lock(c->batch_mu);
        if (c->rm_N == 0) return set_err(-1, "roadmap_plan: no roadmap (call optik_robot_roadmap_build first)");
        if (c->rm_lazy)
            return set_err(-1, "roadmap_plan: the roadmap is a lazy one (call optik_robot_roadmap_plan_lazy)");
        if (c->rm_epoch != r->world_epoch.load())
            return set_err(-1, "roadmap_plan: the roadmap is stale: the collision model or the world changed since it "
                               "was built (build it again)");
        N = c->rm_N; k = c->rm_k; h = c->rm_h;
    }
    // (Q = 0: the kernel layer's refusal of Lmax)
    if (optik_hip_roadmap_query(c->chain, nullptr, N, nullptr, nullptr, k, nullptr, nullptr, 0, nullptr, nullptr, k,
                                nullptr, nullptr, k, nullptr, Lmax, nullptr, nullptr, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (Q == 0 || (!paths_out && !len_out && !cost_out && !status_out)) return 0;
    const size_t n = (size_t)r->n, w = (size_t)Lmax * n, uk = (size_t)k;
    bool stale = false;
    // per query out: the path, the cost, then len and status in one more double; behind them the scratch of the
    // chunk (downloaded with the rest, not looked at): direct 1 | sw k | gw k doubles, sidx k | gidx k int32
    const RowInput in[] = {{starts, n}, {goals, n}};
    const int rc = stage_rows(
        c, Q, in, sizeof(double) * (w + 3 + 3 * uk), kPlanChunk,
        [&](optik_hip_chain *ch, const double *d_s, int64_t L, double *d_out) -> int {
            // (under the batch guard now: the roadmap this chunk reads is still the one checked above?)
            if (c->rm_N != N || c->rm_k != k || c->rm_lazy || c->rm_epoch != r->world_epoch.load()) {
                stale = true;
                return 1;
            }
            const double *d_g = d_s + n * (size_t)L, *d_nodes = c->rm_graph.get(), *d_w = d_nodes + n * (size_t)N;
            double *d_cost = d_out + w * (size_t)L;
            int32_t *d_len = reinterpret_cast<int32_t *>(d_cost + L), *d_status = d_len + L;
            double *d_direct = d_cost + 2 * L, *d_sw = d_direct + L, *d_gw = d_sw + uk * (size_t)L;
            int32_t *d_sidx = reinterpret_cast<int32_t *>(d_gw + uk * (size_t)L), *d_gidx = d_sidx + uk * (size_t)L;
            return (optik_hip_roadmap_knn(ch, d_s, L, d_nodes, N, k, 0, d_sidx, nullptr, nullptr)
                   || optik_hip_roadmap_knn(ch, d_g, L, d_nodes, N, k, 0, d_gidx, nullptr, nullptr)
                   || optik_hip_roadmap_edges(ch, nullptr, d_s, L, d_nodes, N, d_sidx, k, h, 0, d_sw, nullptr)
                   || optik_hip_roadmap_edges(ch, nullptr, d_g, L, d_nodes, N, d_gidx, k, h, 1, d_gw, nullptr)
                   || optik_hip_roadmap_edges(ch, nullptr, d_s, L, d_g, (int32_t)L, nullptr, 1, h, 0, d_direct, nullptr)
                   || optik_hip_roadmap_query(ch, d_nodes, N, c->rm_nbr.get(), d_w, k, d_s, d_g, L, d_sidx, d_sw, k,
                                              d_gidx, d_gw, k, d_direct, Lmax, d_out, d_len, d_cost, d_status, nullptr))
                       ? 1 : 0;
        },
        [&](size_t b0, size_t L, const double *h_out) {
            scatter_plans(h_out, b0, L, (size_t)Lmax, n, paths_out, len_out, cost_out, status_out);
        });
    if (stale) return set_err(-1, "roadmap_plan: the roadmap changed or went stale during the call");
    return rc;
}

// Q goal-set plans over the robot's roadmap (include/optik.h): optik_robot_roadmap_plan's
// staging and refusals with G goal rows per query.  Per chunk the searches and the edge checks of the goals run goal
// slot by goal slot ([G][n][L] is how the rows are staged, and [G][k][L] is how the query takes the links), then
// optik_hip_roadmap_query_goals.
int optik_robot_roadmap_plan_goals(const optik_robot *r, const double *starts, const double *goals,
                                   const int32_t *counts, int32_t G, int64_t Q, int32_t Lmax, double *paths_out,
                                   int32_t *len_out, double *cost_out, int32_t *status_out, int32_t *goal_out) {
    if (!r || !starts || !goals) return set_err(-1, "null argument");
    if (Q < 0) return set_err(-1, "bad argument");
    if (G < 1 || G > OPTIK_HIP_ROADMAP_MAX_GOALS)
        return set_err(-1, "roadmap_plan_goals: G must be in 1 .. " + std::to_string(OPTIK_HIP_ROADMAP_MAX_GOALS)
                               + " goals per query");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    int32_t N, k;
    double h;
    {
        // (as optik_robot_roadmap_plan: the setters bump the epoch before they take this mutex for the chain)
        std::lock_guard<std::mutex> lock(c->batch_mu);
        if (c->rm_N == 0) return set_err(-1, "roadmap_plan_goals: no roadmap (call optik_robot_roadmap_build first)");
        if (c->rm_lazy)
            return set_err(-1, "roadmap_plan_goals: the roadmap is a lazy one; goal sets are planned over eager "
                               "roadmaps only (optik_robot_roadmap_plan_lazy plans single goals)");
        if (c->rm_epoch != r->world_epoch.load())
            return set_err(-1, "roadmap_plan_goals: the roadmap is stale: the collision model or the world changed "
                               "since it was built (build it again)");
        N = c->rm_N; k = c->rm_k; h = c->rm_h;
    }
    // (Q = 0: the kernel layer's refusals of Lmax and G)
    if (optik_hip_roadmap_query_goals(c->chain, nullptr, N, nullptr, nullptr, k, nullptr, nullptr, nullptr, G, 0,
                                      nullptr, nullptr, k, nullptr, nullptr, k, nullptr, Lmax, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (Q == 0 || (!paths_out && !len_out && !cost_out && !status_out && !goal_out)) return 0;
    const size_t n = (size_t)r->n, w = (size_t)Lmax * n, uk = (size_t)k, uG = (size_t)G;
    bool stale = false, upload_failed = false;
    int64_t done = 0;  // (the chunks come in order: the rows before this one)
    const std::vector<int32_t> all((size_t)(Q < kPlanChunk ? Q : kPlanChunk), G);  // counts NULL: every goal exists
    // per query out: the path, the cost, len and status in one more double, the goal reached and the goal count in
    // another; behind them the scratch of the chunk (downloaded with the rest, not looked at): direct G | sw k |
    // gw G k doubles, sidx k | gidx G k int32
    const RowInput in[] = {{starts, n}, {goals, uG * n}};
    const int rc = stage_rows(
        c, Q, in, sizeof(double) * (w + 3 + uG + uk + uG * uk) + sizeof(int32_t) * (uk + uG * uk), kPlanChunk,
        [&](optik_hip_chain *ch, const double *d_s, int64_t L, double *d_out) -> int {
            // (under the batch guard now: the roadmap this chunk reads is still the one checked above?)
            if (c->rm_N != N || c->rm_k != k || c->rm_lazy || c->rm_epoch != r->world_epoch.load()) {
                stale = true;
                return 1;
            }
            const size_t uL = (size_t)L;
            const double *d_g = d_s + n * uL, *d_nodes = c->rm_graph.get(), *d_w = d_nodes + n * (size_t)N;
            double *d_cost = d_out + w * uL;
            int32_t *d_len = reinterpret_cast<int32_t *>(d_cost + uL), *d_status = d_len + uL;
            int32_t *d_which = reinterpret_cast<int32_t *>(d_cost + 2 * uL), *d_gcount = d_which + uL;
            double *d_direct = d_cost + 3 * uL, *d_sw = d_direct + uG * uL, *d_gw = d_sw + uk * uL;
            int32_t *d_sidx = reinterpret_cast<int32_t *>(d_gw + uG * uk * uL), *d_gidx = d_sidx + uk * uL;
            if (hipMemcpyAsync(d_gcount, counts ? counts + done : all.data(), sizeof(int32_t) * uL,
                               hipMemcpyHostToDevice, nullptr) != hipSuccess) {
                upload_failed = true;
                return 1;
            }
            done += L;
            if (optik_hip_roadmap_knn(ch, d_s, L, d_nodes, N, k, 0, d_sidx, nullptr, nullptr)
                || optik_hip_roadmap_edges(ch, nullptr, d_s, L, d_nodes, N, d_sidx, k, h, 0, d_sw, nullptr))
                return 1;
            for (size_t g = 0; g < uG; ++g) {
                const double *d_goal = d_g + g * n * uL;
                int32_t *d_gi = d_gidx + g * uk * uL;
                if (optik_hip_roadmap_knn(ch, d_goal, L, d_nodes, N, k, 0, d_gi, nullptr, nullptr)
                    || optik_hip_roadmap_edges(ch, nullptr, d_goal, L, d_nodes, N, d_gi, k, h, 1, d_gw + g * uk * uL,
                                               nullptr)
                    || optik_hip_roadmap_edges(ch, nullptr, d_s, L, d_goal, (int32_t)L, nullptr, 1, h, 0,
                                               d_direct + g * uL, nullptr))
                    return 1;
            }
            return optik_hip_roadmap_query_goals(ch, d_nodes, N, c->rm_nbr.get(), d_w, k, d_s, d_g, d_gcount, G, L,
                                                 d_sidx, d_sw, k, d_gidx, d_gw, k, d_direct, Lmax, d_out, d_len, d_cost,
                                                 d_status, d_which, nullptr, nullptr, nullptr)
                       ? 1 : 0;
        },
        [&](size_t b0, size_t L, const double *h_out) {
            const int32_t *h_which =
                scatter_plans(h_out, b0, L, (size_t)Lmax, n, paths_out, len_out, cost_out, status_out);
            if (goal_out) std::memcpy(goal_out + b0, h_which, sizeof(int32_t) * L);
        });
    if (stale) return set_err(-1, "roadmap_plan_goals: the roadmap changed or went stale during the call");
    if (upload_failed) return set_err(-1, "upload failed");
    return rc;
}

namespace {

// The verdicts and working weights of the lazy roadmap of context c from the chain's model and world as they are
// (under the robot's mutex and the context's batch guard: no setter is half-way).  The count of slots left open
// goes to *open_out (may be null).
int lazy_reset(DeviceCtx *c, size_t n, bool lengths, int64_t *open_out) {
    const int32_t N = c->rm_N, k = c->rm_k;
    const size_t cells = (size_t)k * (size_t)N;
    double *d_nodes = c->rm_graph.get(), *d_w = d_nodes + n * (size_t)N, *d_w0 = d_w + cells;
    int32_t *d_verdict = c->rm_nbr.get() + cells;
    if (optik_hip_roadmap_lazy_reset(c->chain, nullptr, d_nodes, N, c->rm_nbr.get(), k, lengths ? 1 : 0, d_w0, nullptr,
                                     d_verdict, d_w, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (!open_out) return 0;
    if (!reserve_batch(c, (cells + 1) / 2)) return set_err(-1, kBatchAllocMsg);
    int32_t *h_verdict = reinterpret_cast<int32_t *>(c->h_batch.get());
    if (hipMemcpyAsync(h_verdict, d_verdict, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, nullptr) != hipSuccess
        || hipStreamSynchronize(nullptr) != hipSuccess)
        return set_err(-1, "download failed");
    int64_t open = 0;
    for (size_t e = 0; e < cells; ++e) open += h_verdict[e] != OPTIK_HIP_ROADMAP_BLOCKED ? 1 : 0;
    *open_out = open;
    return 0;
}

}  // namespace

// A lazy roadmap (include/optik.h): the nodes and neighbour lists of optik_robot_roadmap_build, the lengths of the
// motions in place of their check, and the reset of the verdicts against the world as it is.
int64_t optik_robot_roadmap_build_lazy(optik_robot *r, int32_t N, int32_t k, double resolution, uint64_t first) {
    if (!r) return set_err(-1, "null argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    // (Q = 0: the kernel layer's refusals of N, k, the resolution and the chain, before anything is allocated)
    if (optik_hip_roadmap_knn(c->chain, nullptr, 0, nullptr, N, k, 1, nullptr, nullptr, nullptr)
        || optik_hip_roadmap_edges(c->chain, nullptr, nullptr, 0, nullptr, N, nullptr, 1, resolution, 0, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    // (the setters hold the robot's mutex from the bump of the epoch to the last chain: under it the epoch read here
    // is the epoch of the world the chain has)
    std::lock_guard<std::mutex> world_lock(r->mu);
    BatchGuard guard(c);
    if (!guard.ok()) return set_err(-1, kSetDeviceMsg);
    const size_t n = (size_t)r->n, cells = (size_t)k * (size_t)N;
    c->rm_N = 0;
    if (c->rm_graph.reserve(n * (size_t)N + 2 * cells) != hipSuccess || c->rm_nbr.reserve(2 * cells) != hipSuccess)
        return set_err(-1, kBatchAllocMsg);
    double *d_nodes = c->rm_graph.get();
    if (optik_hip_seed_batch(c->chain, first, N, d_nodes, nullptr)
        || optik_hip_roadmap_knn(c->chain, d_nodes, N, d_nodes, N, k, 1, c->rm_nbr.get(), nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    c->rm_N = N; c->rm_k = k;
    int64_t open = 0;
    if (lazy_reset(c, n, true, &open)) {
        c->rm_N = 0;
        return -1;
    }
    c->rm_h = resolution; c->rm_epoch = r->world_epoch.load(); c->rm_lazy = true;
    return open;
}

// Q plans over the robot's lazy roadmap: optik_robot_roadmap_plan's staging, with the loop of
// optik_hip_roadmap_lazy_plan in place of the query; the verdicts are shared by the chunks and by later calls.
int optik_robot_roadmap_plan_lazy(const optik_robot *r, const double *starts, const double *goals, int64_t Q,
                                  int32_t Lmax, int32_t rounds, double *paths_out, int32_t *len_out, double *cost_out,
                                  int32_t *status_out, int32_t *rounds_used_out, int64_t *checked_out) {
    if (!r || !starts || !goals) return set_err(-1, "null argument");
    if (Q < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    if (rounds_used_out) *rounds_used_out = 0;
    if (checked_out) *checked_out = 0;
    const size_t n = (size_t)r->n;
    // (a world that changes between the reset and a chunk makes the call start again; each further attempt needs
    // another setter call, so the bound is never met by a caller that does not race its own setters)
    for (int attempt = 0; attempt < 8; ++attempt) {
        int32_t N, k;
        double h;
        uint64_t epoch;
        {
            // (under the robot's mutex no setter is half-way: the epoch and the chain's world belong together)
            std::lock_guard<std::mutex> world_lock(r->mu);
            BatchGuard guard(c);
            if (!guard.ok()) return set_err(-1, kSetDeviceMsg);
            if (c->rm_N == 0)
                return set_err(-1, "roadmap_plan_lazy: no roadmap (call optik_robot_roadmap_build_lazy first)");
            if (!c->rm_lazy)
                return set_err(-1, "roadmap_plan_lazy: the roadmap is an eager one (call optik_robot_roadmap_plan)");
            N = c->rm_N; k = c->rm_k; h = c->rm_h;
            // (Q = 0: the kernel layer's refusals of Lmax and rounds)
            if (optik_hip_roadmap_lazy_plan(c->chain, nullptr, nullptr, N, nullptr, nullptr, nullptr, k, h, nullptr,
                                            nullptr, 0, nullptr, nullptr, k, nullptr, nullptr, k, nullptr, Lmax, rounds,
                                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
                return set_err(-1, optik_hip_last_error());
            epoch = r->world_epoch.load();
            if (c->rm_epoch != epoch) {
                if (lazy_reset(c, n, false, nullptr)) return -1;
                c->rm_epoch = epoch;
            }
        }
        if (Q == 0) return 0;
        const size_t w = (size_t)Lmax * n, uk = (size_t)k, cells = uk * (size_t)N;
        bool changed = false;
        int64_t used = 0, checked = 0;
        // (per query out and the chunk's scratch behind it: as optik_robot_roadmap_plan)
        const RowInput in[] = {{starts, n}, {goals, n}};
        const int rc = stage_rows(
            c, Q, in, sizeof(double) * (w + 3 + 3 * uk), kPlanChunk,
            [&](optik_hip_chain *ch, const double *d_s, int64_t L, double *d_out) -> int {
                if (c->rm_N != N || c->rm_k != k || !c->rm_lazy || c->rm_epoch != epoch
                    || epoch != r->world_epoch.load()) {
                    changed = true;
                    return 1;
                }
                const double *d_g = d_s + n * (size_t)L, *d_nodes = c->rm_graph.get();
                double *d_w = c->rm_graph.get() + n * (size_t)N;
                int32_t *d_verdict = c->rm_nbr.get() + cells;
                double *d_cost = d_out + w * (size_t)L;
                int32_t *d_len = reinterpret_cast<int32_t *>(d_cost + L), *d_status = d_len + L;
                double *d_direct = d_cost + 2 * L, *d_sw = d_direct + L, *d_gw = d_sw + uk * (size_t)L;
                int32_t *d_sidx = reinterpret_cast<int32_t *>(d_gw + uk * (size_t)L), *d_gidx = d_sidx + uk * (size_t)L;
                int32_t chunk_used = 0;
                int64_t chunk_checked = 0;
                if (optik_hip_roadmap_knn(ch, d_s, L, d_nodes, N, k, 0, d_sidx, nullptr, nullptr)
                    || optik_hip_roadmap_knn(ch, d_g, L, d_nodes, N, k, 0, d_gidx, nullptr, nullptr)
                    || optik_hip_roadmap_edges(ch, nullptr, d_s, L, d_nodes, N, d_sidx, k, h, 0, d_sw, nullptr)
                    || optik_hip_roadmap_edges(ch, nullptr, d_g, L, d_nodes, N, d_gidx, k, h, 1, d_gw, nullptr)
                    || optik_hip_roadmap_edges(ch, nullptr, d_s, L, d_g, (int32_t)L, nullptr, 1, h, 0, d_direct, nullptr)
                    || optik_hip_roadmap_lazy_plan(ch, nullptr, d_nodes, N, c->rm_nbr.get(), d_w, d_verdict, k, h, d_s,
                                                   d_g, L, d_sidx, d_sw, k, d_gidx, d_gw, k, d_direct, Lmax, rounds,
                                                   d_out, d_len, d_cost, d_status, &chunk_used, &chunk_checked, nullptr))
                    return 1;
                used += chunk_used;
                checked += chunk_checked;
                return 0;
            },
            [&](size_t b0, size_t L, const double *h_out) {
                scatter_plans(h_out, b0, L, (size_t)Lmax, n, paths_out, len_out, cost_out, status_out);
            });
        if (changed) continue;
        if (rc) return rc;
        if (rounds_used_out) *rounds_used_out = (int32_t)(used > INT32_MAX ? INT32_MAX : used);
        if (checked_out) *checked_out = checked;
        return 0;
    }
    return set_err(-1, "roadmap_plan_lazy: the world or the roadmap kept changing during the call");
}

// Q goal-set plans over the robot's lazy roadmap (include/optik.h):
// optik_robot_roadmap_plan_goals' staging and links with optik_robot_roadmap_plan_lazy's state -- the epoch compared
// and the verdicts reset under the robot's mutex, the chunks against the shared verdicts, the call started again if
// the world changed under it -- and the loop of optik_hip_roadmap_lazy_plan_goals in place of the query.
int optik_robot_roadmap_plan_goals_lazy(const optik_robot *r, const double *starts, const double *goals,
                                        const int32_t *counts, int32_t G, int64_t Q, int32_t Lmax, int32_t rounds,
                                        double *paths_out, int32_t *len_out, double *cost_out, int32_t *status_out,
                                        int32_t *goal_out, int32_t *rounds_used_out, int64_t *checked_out) {
    if (!r || !starts || !goals) return set_err(-1, "null argument");
    if (Q < 0) return set_err(-1, "bad argument");
    if (G < 1 || G > OPTIK_HIP_ROADMAP_MAX_GOALS)
        return set_err(-1, "roadmap_plan_goals_lazy: G must be in 1 .. " + std::to_string(OPTIK_HIP_ROADMAP_MAX_GOALS)
                               + " goals per query");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    if (rounds_used_out) *rounds_used_out = 0;
    if (checked_out) *checked_out = 0;
    const size_t n = (size_t)r->n, uG = (size_t)G;
    const std::vector<int32_t> all((size_t)(Q < kPlanChunk ? Q : kPlanChunk), G);  // counts NULL: every goal exists
    for (int attempt = 0; attempt < 8; ++attempt) {
        int32_t N, k;
        double h;
        uint64_t epoch;
        {
            // (under the robot's mutex no setter is half-way: the epoch and the chain's world belong together)
            std::lock_guard<std::mutex> world_lock(r->mu);
            BatchGuard guard(c);
            if (!guard.ok()) return set_err(-1, kSetDeviceMsg);
            if (c->rm_N == 0)
                return set_err(-1, "roadmap_plan_goals_lazy: no roadmap (call optik_robot_roadmap_build_lazy first)");
            if (!c->rm_lazy)
                return set_err(-1, "roadmap_plan_goals_lazy: the roadmap is an eager one (call "
                                   "optik_robot_roadmap_plan_goals)");
            N = c->rm_N; k = c->rm_k; h = c->rm_h;
            // (Q = 0: the kernel layer's refusals of Lmax, G and rounds)
            if (optik_hip_roadmap_lazy_plan_goals(c->chain, nullptr, nullptr, N, nullptr, nullptr, nullptr, k, h, nullptr,
                                                  nullptr, nullptr, G, 0, nullptr, nullptr, k, nullptr, nullptr, k,
                                                  nullptr, Lmax, rounds, 1, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                  nullptr, nullptr, nullptr))
                return set_err(-1, optik_hip_last_error());
            epoch = r->world_epoch.load();
            if (c->rm_epoch != epoch) {
                if (lazy_reset(c, n, false, nullptr)) return -1;
                c->rm_epoch = epoch;
            }
        }
        if (Q == 0) return 0;
        const size_t w = (size_t)Lmax * n, uk = (size_t)k, cells = uk * (size_t)N;
        bool changed = false, upload_failed = false;
        int64_t used = 0, checked = 0, done = 0;  // (the chunks come in order: done = the rows before this one)
        // (per query out and the chunk's scratch behind it: as optik_robot_roadmap_plan_goals)
        const RowInput in[] = {{starts, n}, {goals, uG * n}};
        const int rc = stage_rows(
            c, Q, in, sizeof(double) * (w + 3 + uG + uk + uG * uk) + sizeof(int32_t) * (uk + uG * uk), kPlanChunk,
            [&](optik_hip_chain *ch, const double *d_s, int64_t L, double *d_out) -> int {
                if (c->rm_N != N || c->rm_k != k || !c->rm_lazy || c->rm_epoch != epoch
                    || epoch != r->world_epoch.load()) {
                    changed = true;
                    return 1;
                }
                const size_t uL = (size_t)L;
                const double *d_g = d_s + n * uL, *d_nodes = c->rm_graph.get();
                double *d_w = c->rm_graph.get() + n * (size_t)N;
                int32_t *d_verdict = c->rm_nbr.get() + cells;
                double *d_cost = d_out + w * uL;
                int32_t *d_len = reinterpret_cast<int32_t *>(d_cost + uL), *d_status = d_len + uL;
                int32_t *d_which = reinterpret_cast<int32_t *>(d_cost + 2 * uL), *d_gcount = d_which + uL;
                double *d_direct = d_cost + 3 * uL, *d_sw = d_direct + uG * uL, *d_gw = d_sw + uk * uL;
                int32_t *d_sidx = reinterpret_cast<int32_t *>(d_gw + uG * uk * uL), *d_gidx = d_sidx + uk * uL;
                if (hipMemcpyAsync(d_gcount, counts ? counts + done : all.data(), sizeof(int32_t) * uL,
                                   hipMemcpyHostToDevice, nullptr) != hipSuccess) {
                    upload_failed = true;
                    return 1;
                }
                done += L;
                if (optik_hip_roadmap_knn(ch, d_s, L, d_nodes, N, k, 0, d_sidx, nullptr, nullptr)
                    || optik_hip_roadmap_edges(ch, nullptr, d_s, L, d_nodes, N, d_sidx, k, h, 0, d_sw, nullptr))
                    return 1;
                for (size_t g = 0; g < uG; ++g) {
                    const double *d_goal = d_g + g * n * uL;
                    int32_t *d_gi = d_gidx + g * uk * uL;
                    if (optik_hip_roadmap_knn(ch, d_goal, L, d_nodes, N, k, 0, d_gi, nullptr, nullptr)
                        || optik_hip_roadmap_edges(ch, nullptr, d_goal, L, d_nodes, N, d_gi, k, h, 1,
                                                   d_gw + g * uk * uL, nullptr)
                        || optik_hip_roadmap_edges(ch, nullptr, d_s, L, d_goal, (int32_t)L, nullptr, 1, h, 0,
                                                   d_direct + g * uL, nullptr))
                        return 1;
                }
                int32_t chunk_used = 0;
                int64_t chunk_checked = 0;
                if (optik_hip_roadmap_lazy_plan_goals(ch, nullptr, d_nodes, N, c->rm_nbr.get(), d_w, d_verdict, k, h, d_s,
                                                      d_g, d_gcount, G, L, d_sidx, d_sw, k, d_gidx, d_gw, k, d_direct,
                                                      Lmax, rounds, 1, d_out, d_len, d_cost, d_status, d_which,
                                                      &chunk_used, &chunk_checked, nullptr))
                    return 1;
                used += chunk_used;
                checked += chunk_checked;
                return 0;
            },
            [&](size_t b0, size_t L, const double *h_out) {
                const int32_t *h_which =
                    scatter_plans(h_out, b0, L, (size_t)Lmax, n, paths_out, len_out, cost_out, status_out);
                if (goal_out) std::memcpy(goal_out + b0, h_which, sizeof(int32_t) * L);
            });
        if (changed) continue;
        if (upload_failed) return set_err(-1, "upload failed");
        if (rc) return rc;
        if (rounds_used_out) *rounds_used_out = (int32_t)(used > INT32_MAX ? INT32_MAX : used);
        if (checked_out) *checked_out = checked;
        return 0;
    }
    return set_err(-1, "roadmap_plan_goals_lazy: the world or the roadmap kept changing during the call");
}

namespace {

// The staging of both tree-planner wrappers, their arguments checked: G goal rows per query -- staged as [G][n][L],
// which is how optik_hip_rrt_plan_goals takes them -- and the counts (null: every goal exists, nothing is uploaded).
// No roadmap is read, so nothing can be stale.  With a constraint (con not null) the call is
// optik_hip_rrt_plan_constrained and every query has one more double out, its two projection counters.
struct RrtRowsConstraint {
    const double *ref7, *lo6, *hi6;
    double tol, ptol, damping, max_step;
    int32_t piters;
    int32_t *projected_out;  // [Q][2] or null
};

int rrt_plan_rows(const optik_robot *r, DeviceCtx *c, const RrtRowsConstraint *con, const double *starts,
                  const double *goals, const int32_t *counts,
                  int32_t G, int64_t Q, int32_t iters, double step, double resolution, uint64_t first,
                  int32_t max_nodes, int32_t Lmax, int32_t poll, const double *ee16, double *paths_out,
                  int32_t *len_out, double *cost_out, int32_t *status_out, int32_t *iters_out, int32_t *nodes_out,
                  int32_t *goal_out) {
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    const size_t n = (size_t)r->n, w = (size_t)Lmax * n, uG = (size_t)G;
    bool upload_failed = false;
    int64_t done = 0;  // (the chunks come in order: the rows before this one)
    // per query out: the path, the cost, then len and status in one more double, iters and the goal reached in
    // another, the two tree sizes in a third; with counts the goal count and a spare word in a last one
    const RowInput in[] = {{starts, n}, {goals, uG * n}};
    const int rc = stage_rows(
        c, Q, in, sizeof(double) * (w + (counts ? 5 : 4) + (con ? 1 : 0)), kPlanChunk,
        [&](optik_hip_chain *ch, const double *d_s, int64_t L, double *d_out) -> int {
            double *d_cost = d_out + w * (size_t)L;
            int32_t *d_len = reinterpret_cast<int32_t *>(d_cost + L), *d_status = d_len + L, *d_it = d_status + L,
                    *d_which = d_it + L, *d_nodes = d_which + L, *d_gcount = counts ? d_nodes + 2 * L : nullptr;
            if (counts
                && hipMemcpyAsync(d_gcount, counts + done, sizeof(int32_t) * (size_t)L, hipMemcpyHostToDevice, nullptr)
                       != hipSuccess) {
                upload_failed = true;
                return 1;
            }
            done += L;
            if (con)
                return optik_hip_rrt_plan_constrained(ch, ee16 ? ee7 : nullptr, con->ref7, con->lo6, con->hi6, con->tol,
                                                      con->ptol, con->piters, con->damping, con->max_step, d_s,
                                                      d_s + n * (size_t)L, d_gcount, L, G, iters, step, resolution, first,
                                                      max_nodes, Lmax, poll, d_out, d_len, d_cost, d_status, d_it,
                                                      d_nodes, d_which, d_nodes + (counts ? 4 : 2) * L, nullptr);
            return optik_hip_rrt_plan_goals(ch, ee16 ? ee7 : nullptr, d_s, d_s + n * (size_t)L, d_gcount, L, G, iters,
                                            step, resolution, first, max_nodes, Lmax, poll, d_out, d_len, d_cost,
                                            d_status, d_it, d_nodes, d_which, nullptr);
        },
        [&](size_t b0, size_t L, const double *h_out) {
            const int32_t *h_it = scatter_plans(h_out, b0, L, (size_t)Lmax, n, paths_out, len_out, cost_out, status_out),
                          *h_which = h_it + L, *h_nodes = h_which + L;
            if (iters_out) std::memcpy(iters_out + b0, h_it, sizeof(int32_t) * L);
            if (goal_out) std::memcpy(goal_out + b0, h_which, sizeof(int32_t) * L);
            if (nodes_out)
                for (size_t q = 0; q < L; ++q) {
                    nodes_out[2 * (b0 + q)] = h_nodes[q];
                    nodes_out[2 * (b0 + q) + 1] = h_nodes[L + q];
                }
            if (con && con->projected_out) {
                const int32_t *h_proj = h_nodes + (counts ? 4 : 2) * L;
                for (size_t q = 0; q < L; ++q) {
                    con->projected_out[2 * (b0 + q)] = h_proj[q];
                    con->projected_out[2 * (b0 + q) + 1] = h_proj[L + q];
                }
            }
        });
    if (upload_failed) return set_err(-1, "upload failed");
    return rc;
}

}  // namespace

// Q queries through the tree planner (include/optik.h): one goal row per query, every one
// counted.
int optik_robot_rrt_plan(const optik_robot *r, const double *starts, const double *goals, int64_t Q, int32_t iters,
                         double step, double resolution, uint64_t first, int32_t max_nodes, int32_t Lmax, int32_t poll,
                         const double *ee16, double *paths_out, int32_t *len_out, double *cost_out,
                         int32_t *status_out, int32_t *iters_out, int32_t *nodes_out) {
    if (!r || !starts || !goals) return set_err(-1, "null argument");
    if (Q < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    // (Q = 0: the kernel layer's refusals of the chain, the sizes, the step and the resolution)
    if (optik_hip_rrt_plan(c->chain, nullptr, nullptr, nullptr, 0, iters, step, resolution, first, max_nodes, Lmax, poll,
                           nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (Q == 0 || (!paths_out && !len_out && !cost_out && !status_out && !iters_out && !nodes_out)) return 0;
    return rrt_plan_rows(r, c, nullptr, starts, goals, nullptr, 1, Q, iters, step, resolution, first, max_nodes, Lmax, poll, ee16,
                         paths_out, len_out, cost_out, status_out, iters_out, nodes_out, nullptr);
}

// Q goal-set queries through optik_hip_rrt_plan_goals (include/optik.h).
int optik_robot_rrt_plan_goals(const optik_robot *r, const double *starts, const double *goals, const int32_t *counts,
                               int32_t G, int64_t Q, int32_t iters, double step, double resolution, uint64_t first,
                               int32_t max_nodes, int32_t Lmax, int32_t poll, const double *ee16, double *paths_out,
                               int32_t *len_out, double *cost_out, int32_t *status_out, int32_t *iters_out,
                               int32_t *nodes_out, int32_t *goal_out) {
    if (!r || !starts || !goals) return set_err(-1, "null argument");
    if (Q < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    // (Q = 0: the kernel layer's refusals of the chain, G, the sizes, the step and the resolution)
    if (optik_hip_rrt_plan_goals(c->chain, nullptr, nullptr, nullptr, nullptr, 0, G, iters, step, resolution, first,
                                 max_nodes, Lmax, poll, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 nullptr))
        return set_err(-1, optik_hip_last_error());
    if (Q == 0 || (!paths_out && !len_out && !cost_out && !status_out && !iters_out && !nodes_out && !goal_out))
        return 0;
    return rrt_plan_rows(r, c, nullptr, starts, goals, counts, G, Q, iters, step, resolution, first, max_nodes, Lmax, poll,
                         ee16, paths_out, len_out, cost_out, status_out, iters_out, nodes_out, goal_out);
}

// Q goal-set queries through optik_hip_rrt_plan_constrained (include/optik.h).
int optik_robot_rrt_plan_constrained(const optik_robot *r, const double *starts, const double *goals,
                                     const int32_t *counts, int32_t G, int64_t Q, const double *ref7, const double *lo6,
                                     const double *hi6, double tol, double ptol, int32_t piters, double damping,
                                     double max_step, int32_t iters, double step, double resolution, uint64_t first,
                                     int32_t max_nodes, int32_t Lmax, int32_t poll, const double *ee16,
                                     double *paths_out, int32_t *len_out, double *cost_out, int32_t *status_out,
                                     int32_t *iters_out, int32_t *nodes_out, int32_t *goal_out,
                                     int32_t *projected_out) {
    if (!r || !starts || !goals) return set_err(-1, "null argument");
    if (Q < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    // (Q = 0: the kernel layer's refusals of the chain, G, the sizes, the step, the resolution and the constraint)
    if (optik_hip_rrt_plan_constrained(c->chain, nullptr, ref7, lo6, hi6, tol, ptol, piters, damping, max_step, nullptr,
                                       nullptr, nullptr, 0, G, iters, step, resolution, first, max_nodes, Lmax, poll,
                                       nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (Q == 0
        || (!paths_out && !len_out && !cost_out && !status_out && !iters_out && !nodes_out && !goal_out
            && !projected_out))
        return 0;
    const RrtRowsConstraint con{ref7, lo6, hi6, tol, ptol, damping, max_step, piters, projected_out};
    return rrt_plan_rows(r, c, &con, starts, goals, counts, G, Q, iters, step, resolution, first, max_nodes, Lmax, poll,
                         ee16, paths_out, len_out, cost_out, status_out, iters_out, nodes_out, goal_out);
}

int optik_robot_set_motion_resolution(optik_robot *r, double h) {
    if (!r) return set_err(-1, "null argument");
    if (!(h >= 0.0) || !std::isfinite(h))
        return set_err(-1, "motion resolution must be finite and >= 0 (0: no motion check)");
    std::lock_guard<std::mutex> lock(r->mu);
    r->motion_h = h;
    return for_each_chain(r, [&](optik_hip_chain *ch) {
        return optik_hip_chain_set_motion_resolution(ch, h);
    });
}

int optik_robot_collision_motion_batch(const optik_robot *r, int64_t B, const double *xa, const double *xb,
                                       double resolution, const double *ee16, double *clearance_out,
                                       uint8_t *free_out, int32_t *first_out, int32_t *steps_out) {
    if (!r || !xa || !xb) return set_err(-1, "null argument");
    if (B < 0) return set_err(-1, "bad argument");
    // (refused on the host, before a device context exists)
    if (!(resolution > 0.0) || !std::isfinite(resolution))
        return set_err(-1, "motion resolution must be finite and > 0");
    for (int32_t t : r->types)
        if (t == optik_host::PRISMATIC)
            return set_err(-1, "collision: prismatic joints are not supported (IK refuses such chains)");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    // (B = 0: the kernel layer's own refusals of the chain, before anything is staged)
    if (optik_hip_collision_motion_batch(c->chain, nullptr, nullptr, nullptr, 0, resolution, nullptr, nullptr, nullptr,
                                         nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (B == 0 || (!clearance_out && !free_out && !first_out && !steps_out)) return 0;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    // per segment: qa and qb (2 n doubles) in; the clearance, then first and steps in a second double and the free
    // flag in the bytes of a third out
    const RowInput in[] = {{xa, (size_t)r->n}, {xb, (size_t)r->n}};
    return stage_rows(
        c, B, in, 3 * sizeof(double), kMotionChunk,
        [&](optik_hip_chain *ch, const double *d_q, int64_t L, double *d_out) {
            int32_t *d_first = reinterpret_cast<int32_t *>(d_out + L);
            return optik_hip_collision_motion_batch(ch, ee16 ? ee7 : nullptr, d_q, d_q + (size_t)r->n * L, L, resolution,
                                                    clearance_out ? d_out : nullptr,
                                                    reinterpret_cast<uint8_t *>(d_out + 2 * L), d_first, d_first + L,
                                                    nullptr);
        },
        [&](size_t b0, size_t L, const double *h_out) {
            const int32_t *h_first = reinterpret_cast<const int32_t *>(h_out + L);
            if (clearance_out) std::memcpy(clearance_out + b0, h_out, sizeof(double) * L);
            if (first_out) std::memcpy(first_out + b0, h_first, sizeof(int32_t) * L);
            if (steps_out) std::memcpy(steps_out + b0, h_first + L, sizeof(int32_t) * L);
            if (free_out) std::memcpy(free_out + b0, reinterpret_cast<const uint8_t *>(h_out + 2 * L), L);
        });
}

int optik_robot_collision_motion_certify_batch(const optik_robot *r, int64_t B, const double *xa, const double *xb,
                                               double tol, double grid_lipschitz, int32_t max_steps,
                                               const double *ee16, int32_t *status_out, int32_t *steps_out,
                                               double *t_stop_out, double *clearance_out) {
    if (!r || !xa || !xb) return set_err(-1, "null argument");
    if (B < 0) return set_err(-1, "bad argument");
    // (refused on the host, before a device context exists)
    if (!(tol > 0.0) || !std::isfinite(tol)) return set_err(-1, "motion certify: tol must be finite and > 0");
    if (!(grid_lipschitz > 0.0) || !std::isfinite(grid_lipschitz))
        return set_err(-1, "motion certify: grid_lipschitz must be finite and > 0");
    if (max_steps < 2 || max_steps > OPTIK_HIP_CERTIFY_MAX_STEPS)
        return set_err(-1, "motion certify: max_steps must be in 2 .. 65536");
    for (int32_t t : r->types)
        if (t == optik_host::PRISMATIC)
            return set_err(-1, "collision: prismatic joints are not supported (IK refuses such chains)");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    if (B == 0 || (!status_out && !steps_out && !t_stop_out && !clearance_out)) return 0;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    // per segment: qa and qb (2 n doubles) in; t_stop, the clearance, then status and steps in a third double out
    const RowInput in[] = {{xa, (size_t)r->n}, {xb, (size_t)r->n}};
    return stage_rows(
        c, B, in, 3 * sizeof(double), kMotionChunk,
        [&](optik_hip_chain *ch, const double *d_q, int64_t L, double *d_out) {
            int32_t *d_status = reinterpret_cast<int32_t *>(d_out + 2 * L);
            return optik_hip_collision_motion_certify_batch(ch, ee16 ? ee7 : nullptr, d_q, d_q + (size_t)r->n * L, L,
                                                            tol, grid_lipschitz, max_steps, d_status, d_status + L,
                                                            d_out, d_out + L, nullptr);
        },
        [&](size_t b0, size_t L, const double *h_out) {
            const int32_t *h_status = reinterpret_cast<const int32_t *>(h_out + 2 * L);
            if (t_stop_out) std::memcpy(t_stop_out + b0, h_out, sizeof(double) * L);
            if (clearance_out) std::memcpy(clearance_out + b0, h_out + L, sizeof(double) * L);
            if (status_out) std::memcpy(status_out + b0, h_status, sizeof(int32_t) * L);
            if (steps_out) std::memcpy(steps_out + b0, h_status + L, sizeof(int32_t) * L);
        });
}


// A region as ik_constraint.hip validates a constraint; the message names the row.
static int check_region_row(int64_t t, const double *reg) {
    const std::string row = "ik_region: region " + std::to_string(t) + ": ";
    double n2 = 0.0;
    for (int i = 0; i < 7; ++i) {
        if (!std::isfinite(reg[i])) return set_err(-1, row + "the reference pose must be finite");
        if (i >= 3) n2 += reg[i] * reg[i];
    }
    if (!(std::fabs(n2 - 1.0) <= 100.0 * 2.220446049250313e-16))
        return set_err(-1, row + "the reference quaternion must have unit norm");
    for (int i = 0; i < 6; ++i)
        if (!(reg[7 + i] <= reg[13 + i])) return set_err(-1, row + "needs lo <= hi on every axis, no NaN");
    return 0;
}

int optik_robot_ik_region(const optik_robot *r, int32_t T, const double *regions19, const double *x0,
                          uint64_t restarts, double tol, int32_t iters, double damping, double max_step, int32_t mode,
                          const double *keep_ref7, const double *keep_lo6, const double *keep_hi6, double keep_tol,
                          int32_t K, double min_dist, const double *ee16, int32_t *count_out, double *x_out,
                          double *violation_out, uint64_t *idx_out, double *key_out) {
    return optik_robot_ik_region_repair(r, T, regions19, x0, restarts, tol, iters, damping, max_step, mode, keep_ref7,
                                        keep_lo6, keep_hi6, keep_tol, K, min_dist, nullptr, ee16, count_out, x_out,
                                        violation_out, idx_out, key_out, nullptr);
}

// The one body of both: repair5 = influence, safety, step, iters, max_move (null: optik_robot_ik_region).
int optik_robot_ik_region_repair(const optik_robot *r, int32_t T, const double *regions19, const double *x0,
                                 uint64_t restarts, double tol, int32_t iters, double damping, double max_step,
                                 int32_t mode, const double *keep_ref7, const double *keep_lo6, const double *keep_hi6,
                                 double keep_tol, int32_t K, double min_dist, const double *repair5, const double *ee16,
                                 int32_t *count_out, double *x_out, double *violation_out, uint64_t *idx_out,
                                 double *key_out, int32_t *repaired_out) {
    if (!r || T < 0 || (T > 0 && (!regions19 || !x0))) return set_err(-1, "null argument");
    if (restarts < 1 || restarts > ((uint64_t)1 << 22))
        return set_err(-1, "ik_region: restarts must be in 1 .. 2^22 (every restart index in [0, restarts) runs)");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    optik_hip_ik_region_outputs o;
    std::memset(&o, 0, sizeof o);
    optik_hip_region_repair rep;
    std::memset(&rep, 0, sizeof rep);
    if (repair5) {
        if (!(repair5[3] >= 0.0 && repair5[3] <= 4096.0 && repair5[3] == (double)(int32_t)repair5[3]))
            return set_err(-1, "ik_region: repair iters must be an integer in 0 .. 4096");
        rep.influence = repair5[0]; rep.safety = repair5[1]; rep.step = repair5[2];
        rep.iters = (int32_t)repair5[3]; rep.max_move = repair5[4];
    }
    const optik_hip_region_repair *prep = repair5 ? &rep : nullptr;
    // (T = 0: the kernel layer's refusals, before anything is staged)
    if (optik_hip_ik_region_repair(c->chain, nullptr, nullptr, nullptr, 0, 0, restarts, tol, iters, damping, max_step,
                                   mode, keep_ref7, keep_lo6, keep_hi6, keep_tol, K, min_dist, prep, &o, nullptr))
        return set_err(-1, optik_hip_last_error());
    for (int64_t t = 0; t < T; ++t)
        if (int rc = check_region_row(t, regions19 + (size_t)t * OPTIK_HIP_REGION_DOUBLES)) return rc;
    if (T == 0) return 0;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    const size_t n = (size_t)r->n, W = OPTIK_HIP_REGION_DOUBLES;
    // chunks of whole regions, about 4 M (region, restart) items a launch at most (as optik_robot_ik_solutions).  The
    // robot's batch block: in = regions [C][19] | x0 [C][n]; out = x [C][K][n] | violation, key, idx [C][K] | count [C] |
    // repaired [C]
    const size_t chunk = (size_t)std::min<uint64_t>((uint64_t)T, std::max<uint64_t>(1, ((uint64_t)4 << 20) / restarts));
    BatchGuard guard(c);
    if (!guard.ok()) return set_err(-1, kSetDeviceMsg);
    if (!reserve_batch(c, (W + n) * chunk + (size_t)K * chunk * (n + 3) + 2 * chunk)) return set_err(-1, kBatchAllocMsg);
    for (size_t t0 = 0; t0 < (size_t)T; t0 += chunk) {
        const size_t L = std::min(chunk, (size_t)T - t0), KL = (size_t)K * L, n_in = (W + n) * L;
        double *h_in = c->h_batch.get(), *h_out = h_in + n_in;
        double *d_in = c->d_batch.get(), *d_x = d_in + n_in, *d_v = d_x + KL * n, *d_key = d_v + KL;
        uint64_t *d_idx = reinterpret_cast<uint64_t *>(d_key + KL);
        int32_t *d_count = reinterpret_cast<int32_t *>(d_idx + KL);
        std::memcpy(h_in, regions19 + t0 * W, sizeof(double) * W * L);
        std::memcpy(h_in + W * L, x0 + t0 * n, sizeof(double) * n * L);
        if (hipMemcpyAsync(d_in, h_in, sizeof(double) * n_in, hipMemcpyHostToDevice, nullptr) != hipSuccess)
            return set_err(-1, "upload failed");
        o.d_count = d_count; o.d_sol_x = d_x; o.d_sol_violation = d_v; o.d_sol_idx = d_idx; o.d_sol_key = d_key;
        rep.d_repaired = d_count + L;
        if (optik_hip_ik_region_repair(c->chain, ee16 ? ee7 : nullptr, d_in, d_in + W * L, (int32_t)L, 0, restarts, tol,
                                       iters, damping, max_step, mode, keep_ref7, keep_lo6, keep_hi6, keep_tol, K,
                                       min_dist, prep, &o, nullptr))
            return set_err(-1, optik_hip_last_error());
        if (hipMemcpyAsync(h_out, d_x, sizeof(double) * (KL * (n + 3) + (prep ? 2 * L : L)), hipMemcpyDeviceToHost, nullptr)
                != hipSuccess
            || hipStreamSynchronize(nullptr) != hipSuccess)
            return set_err(-1, "download failed");
        const double *hx = h_out, *hv = hx + KL * n, *hk = hv + KL;
        const uint64_t *hi = reinterpret_cast<const uint64_t *>(hk + KL);
        const int32_t *hc = reinterpret_cast<const int32_t *>(hi + KL);
        if (x_out) std::memcpy(x_out + t0 * (size_t)K * n, hx, sizeof(double) * KL * n);
        if (violation_out) std::memcpy(violation_out + t0 * (size_t)K, hv, sizeof(double) * KL);
        if (key_out) std::memcpy(key_out + t0 * (size_t)K, hk, sizeof(double) * KL);
        if (idx_out) std::memcpy(idx_out + t0 * (size_t)K, hi, sizeof(uint64_t) * KL);
        if (count_out) std::memcpy(count_out + t0, hc, sizeof(int32_t) * L);
        if (repaired_out) {
            if (prep) std::memcpy(repaired_out + t0, hc + L, sizeof(int32_t) * L);
            else std::memset(repaired_out + t0, 0, sizeof(int32_t) * L);
        }
    }
    return 0;
}

}  // extern "C"
