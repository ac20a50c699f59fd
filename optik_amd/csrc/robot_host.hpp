// robot_host.hpp -- what the translation units of the host API share: the robot object, its per-GPU contexts, error
// reporting and the plumbing every entry point is made of (the batch guard, the thread fan-out, the row staging).
//
//   robot_host.cpp   the robot object, devices, FK / Jacobian, ik / ik_batch / ik_solutions / ik_path and their scheduling
//   robot_rows.cpp   the row batches (diff_ik, manipulability, link frames, clearance, motion), the collision model /
//                    world / grid / motion-resolution setters, the world builders, the roadmap
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/optik.h"
#include "device_buf.hpp"
#include "device_scope.hpp"
#include "urdf_chain.hpp"

// What the robot keeps on one GPU: the uploaded chain and reusable staging for the host API.  Deleted with its device
// current (optik_robot_free, device_ctx): the chain goes first, then the blocks free themselves.
struct DeviceCtx {
    int device = 0;
    optik_hip_chain *chain = nullptr;
    optik::DeviceBuf<double> d_scratch;  // q[n] | pose[7] | jac[6n]
    optik::PinnedBuf<double> h_scratch;  // the same, pinned host memory the FK kernel reads and writes directly
    int num_cus = 0;
    // the batch workspace, grown on demand and kept across calls (optik_robot_ik_batch_ex:
    // device block = targets [T][7] | x0 [T][n] | win_x [T][n] | win_f [T] | win_key [T] | win_idx [T])
    optik::DeviceBuf<double> d_batch;
    optik::PinnedBuf<double> h_batch;  // pinned mirror
    std::mutex batch_mu;               // one batch at a time per device
    // the roadmap of optik_robot_roadmap_build (under batch_mu): nodes [n][N] | w [k][N], then nbr [k][N]; rm_N = 0:
    // none.  rm_epoch: the robot's world_epoch the edges were checked under
    optik::DeviceBuf<double> rm_graph;
    optik::DeviceBuf<int32_t> rm_nbr;
    int32_t rm_N = 0, rm_k = 0;
    double rm_h = 0.0;
    uint64_t rm_epoch = 0;
    // a lazy roadmap (optik_robot_roadmap_build_lazy): w is the working weights, w0 [k][N] follows it and the int32
    // verdicts [k][N] follow nbr; rm_epoch: the world_epoch the verdicts were reset under
    bool rm_lazy = false;
    ~DeviceCtx() { if (chain) optik_hip_chain_destroy(chain); }
};

struct optik_robot {
    optik_host::Chain chain;
    int n = 0;
    std::vector<double> lb, ub;
    std::vector<double> vel;  // the URDF's velocity limits of the n joint positions (+inf: none)
    std::vector<double> origins, axes;  // n_joints x 7, n_joints x 3
    std::vector<int32_t> types;
    // set_parallelism (lib.rs:66-72).  The rayon pool size has no counterpart, but its one
    // observable consequence has: with one thread SolutionMode::Speed returns the lowest
    // successful restart (deterministic; tests/test_ik.rs:45-89 sets 1 for exactly that), with more
    // it returns whichever success comes first (find_any, lib.rs:409-412; README.md:17, 96).
    // 0 = never set = the reference's default pool (ThreadPoolBuilder::default(): every core,
    // lib.rs:42-47) and n > 1 let a Speed call stop at the first success anywhere; 1 gives the
    // deterministic 1-thread answer.
    unsigned parallelism = 0;
    mutable std::mutex mu;     // guards the lazily created device contexts and the FK scratch
    // GPUs this robot spreads restart ranges / targets over (optik_robot_set_devices,
    // OPTIK_DEVICES); empty = the HIP device current at first use.  The same id may be listed
    // more than once (two contexts on one GPU: how the sharding is tested on a 1-GPU box).
    std::vector<int> device_ids;
    // one slot per listed GPU from the first GPU call on; null until that context is created
    mutable std::vector<std::unique_ptr<DeviceCtx>> devs;
    // over how many of them the widest round of the last ik / ik_batch call was actually cut (optik_robot_last_parts)
    mutable std::atomic<int32_t> last_parts{0};
    // the collision model and world (optik_robot_set_collision_model / _set_world), kept on the host and applied to
    // every device chain, also to those created later; the filter is active while coll_frames is not empty
    std::vector<int32_t> coll_frames, coll_pairs;
    std::vector<double> coll_centers, coll_radii;
    double coll_margin = 0.0;
    std::vector<double> world_spheres, world_boxes;
    // the distance-field world (optik_robot_set_world_grid); no grid while grid_values is empty
    std::vector<float> grid_values;
    double grid_origin[3] = {0.0, 0.0, 0.0}, grid_voxel = 0.0;
    int32_t grid_n[3] = {0, 0, 0};
    double motion_h = 0.0;  // optik_robot_set_motion_resolution (0: off)
    // counts the installs of a collision model, a world or a grid: a roadmap built under another count is stale
    // (optik_robot_roadmap_plan)
    std::atomic<uint64_t> world_epoch{0};
    bool collision_active() const {
        std::lock_guard<std::mutex> lock(mu);
        return !coll_frames.empty();
    }
};

namespace optik {
namespace robot {

extern thread_local std::string g_robot_err;  // optik_robot_last_error() of the calling thread (robot_host.cpp)

[[noreturn]] inline void panic(const std::string &msg) {
    // A Rust panic crossing `extern "C"` aborts the process; keep the message.
    std::fprintf(stderr, "optik: %s\n", msg.c_str());
    std::fflush(stderr);
    std::abort();
}

inline int set_err(int code, const std::string &msg) {
    g_robot_err = msg;
    return code;
}

// diff_ik and diff_ik_batch refuse the same chains with the same words
constexpr const char *kDiffIkMaxNMsg =
    "diff_ik: chains of more than 8 joint positions are not supported (the reference's own "
    "diff_ik only runs for n = 6: lib.rs:196-197 builds a 6-row block for n columns)";
constexpr const char *kSetDeviceMsg = "hipSetDevice failed";
constexpr const char *kBatchAllocMsg = "batch workspace allocation failed";

// Context k of the robot (its k-th listed GPU), created on first use.  Returns nullptr and sets
// the error string on failure.  (robot_host.cpp)
DeviceCtx *device_ctx(const optik_robot *r, size_t k = 0);

// fn(begin, end) over [0, count) on a few host threads when the range is long (the per-target
// host work of a batch -- validation, pose conversion, staging, gathering -- is ~50 ns a target:
// 13 of 60 ms at 262 144 targets on one thread)
template <class Fn>
void parallel_ranges(size_t count, Fn fn) {
    static const unsigned max_threads = [] {
        const char *e = std::getenv("OPTIK_HOST_THREADS");
        unsigned h = e ? (unsigned)std::atoi(e) : std::thread::hardware_concurrency() / 2;
        return h < 1 ? 1u : (h > 8 ? 8u : h);
    }();
    const size_t parts = count < 32768 ? 1 : std::min<size_t>(max_threads, count / 16384);
    if (parts <= 1) { fn((size_t)0, count); return; }
    std::vector<std::thread> th;
    for (size_t p = 1; p < parts; ++p) th.emplace_back(fn, count * p / parts, count * (p + 1) / parts);
    fn((size_t)0, count / parts);
    for (auto &t : th) t.join();
}

// One batch at a time per device: holds the context's batch mutex and makes its device current for the scope (the
// caller's device is current again afterwards).  Not ok(): the device could not be bound (kSetDeviceMsg).
class BatchGuard {
public:
    explicit BatchGuard(DeviceCtx *c) : lock_(c->batch_mu), dev_(c->device) {}
    bool ok() const { return dev_.ok(); }

private:
    std::lock_guard<std::mutex> lock_;
    optik::DeviceScope dev_;
};

// The context's batch block and its pinned mirror, at least `doubles` each (under a BatchGuard; kBatchAllocMsg).
inline bool reserve_batch(DeviceCtx *c, size_t doubles) {
    return c->d_batch.reserve(doubles) == hipSuccess && c->h_batch.reserve(doubles) == hipSuccess;
}

// run(part) for every part -- parts 1.. on a host thread each, part 0 on this one; a part reports through its `rc`
// and `err` members.  0, or -1 with the first failing part's message.
template <class Part, class Run>
int run_parts(std::vector<Part> &parts, Run run) {
    std::vector<std::thread> th;
    for (size_t g = 1; g < parts.size(); ++g) th.emplace_back([&run, &parts, g] { run(parts[g]); });
    run(parts[0]);
    for (auto &t : th) t.join();
    for (const Part &p : parts)
        if (p.rc) return set_err(-1, p.err);
    return 0;
}

// fn(chain) -> rc for the chain of every context the robot has created, each under its batch mutex (with r->mu held).
template <class Fn>
int for_each_chain(optik_robot *r, Fn fn) {
    for (auto &c : r->devs) {
        if (!c) continue;
        std::lock_guard<std::mutex> batch_lock(c->batch_mu);
        if (fn(c->chain)) return set_err(-1, optik_hip_last_error());
    }
    return 0;
}

// One input array of a row batch: [B][width] doubles, row-major.
struct RowInput {
    const double *rows;
    size_t width;
};

// B rows through one of the per-row kernels on context c, in chunks of at most `max_chunk` rows.  Per chunk of L rows:
// the inputs are transposed to struct-of-arrays (stride L) back to back into the pinned batch block, ONE upload, run(
// chain, d_in, L, d_out) -> rc launches the kernel -- d_out follows the inputs in the block and takes `out_bytes` per row
// --, ONE download, and take(b0, L, h_out) hands the chunk's outputs (rows b0 .. b0 + L) to the caller.
template <size_t N, class Run, class Take>
int stage_rows(DeviceCtx *c, int64_t B, const RowInput (&in)[N], size_t out_bytes, int64_t max_chunk, Run run,
               Take take) {
    BatchGuard guard(c);
    if (!guard.ok()) return set_err(-1, kSetDeviceMsg);
    size_t in_width = 0;
    for (const RowInput &a : in) in_width += a.width;
    const int64_t chunk = B < max_chunk ? B : max_chunk;
    if (!reserve_batch(c, in_width * (size_t)chunk + (out_bytes * (size_t)chunk + 7) / 8))
        return set_err(-1, kBatchAllocMsg);
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const size_t L = (size_t)(B - b0 < chunk ? B - b0 : chunk);
        double *h_in = c->h_batch.get(), *h_out = h_in + in_width * L;
        double *d_in = c->d_batch.get(), *d_out = d_in + in_width * L;
        parallel_ranges(L, [&](size_t k0, size_t k1) {
            double *h = h_in;
            for (const RowInput &a : in) {
                for (size_t k = k0; k < k1; ++k)
                    for (size_t i = 0; i < a.width; ++i) h[i * L + k] = a.rows[((size_t)b0 + k) * a.width + i];
                h += a.width * L;
            }
        });
        if (hipMemcpyAsync(d_in, h_in, sizeof(double) * in_width * L, hipMemcpyHostToDevice, nullptr) != hipSuccess)
            return set_err(-1, "upload failed");
        if (run(c->chain, d_in, (int64_t)L, d_out)) return set_err(-1, optik_hip_last_error());
        if (hipMemcpyAsync(h_out, d_out, out_bytes * L, hipMemcpyDeviceToHost, nullptr) != hipSuccess
            || hipStreamSynchronize(nullptr) != hipSuccess)
            return set_err(-1, "download failed");
        take((size_t)b0, L, h_out);
    }
    return 0;
}

}  // namespace robot
}  // namespace optik
