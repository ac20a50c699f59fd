// robot_host.cpp -- the reference's host API on top of the HIP kernel layer.
//
// Mirrors `Robot` (/root/reference/crates/optik/src/lib.rs:36-99, 241-415) and
// exports the C ABI of crates/optik-cpp/src/lib.rs:26-183 (include/optik.h).
// What stays on the host is what the reference does once per call or per robot:
// URDF loading, the seed-limit check, the restart/time budget and the loop over
// launches.  FK, Jacobian, the restarts and the selection all run in the kernels
// of ik_capi.hip / ik_batch_ops.hip -- there is no CPU implementation of them in this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <memory>
#include <mutex>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "diff_ik_lp.hpp"
#include "pose_convert.hpp"
#include "robot_host.hpp"

using namespace optik::robot;
using namespace optik::pose;

thread_local std::string optik::robot::g_robot_err;

namespace {

// OPTIK_DEVICES = "all" | "N" (the first N devices) | "0,2,3": GPUs a robot spreads work over
std::vector<int> devices_from_env() {
    std::vector<int> ids;
    const char *e = std::getenv("OPTIK_DEVICES");
    if (!e || !*e) return ids;
    int have = 0;
    (void)hipGetDeviceCount(&have);
    const std::string v(e);
    if (v == "all") { for (int i = 0; i < have; ++i) ids.push_back(i); return ids; }
    if (v.find(',') == std::string::npos) {
        const int cnt = std::atoi(v.c_str());
        for (int i = 0; i < cnt && i < have; ++i) ids.push_back(i);
        return ids;
    }
    std::stringstream ss(v);
    for (std::string tok; std::getline(ss, tok, ',');)
        if (!tok.empty()) ids.push_back(std::atoi(tok.c_str()));
    return ids;
}

optik_robot *make_robot(const std::string &urdf, const char *base, const char *ee) {
    auto *r = new optik_robot();
    try {
        r->chain = optik_host::chain_from_urdf(urdf, base, ee);
    } catch (...) {
        delete r;
        throw;
    }
    r->n = r->chain.num_positions();
    if (r->n > OPTIK_HIP_MAX_DOF) {
        const int n = r->n;
        delete r;
        throw std::runtime_error("chain has " + std::to_string(n) + " joint positions; the gfx950 kernels are built for "
                                 "at most " + std::to_string(OPTIK_HIP_MAX_DOF) + " (a limit of this implementation, not of the reference)");
    }
    for (const auto &j : r->chain.joints) {
        for (int k = 0; k < 3; ++k) r->origins.push_back(j.origin.t[k]);
        for (int k = 0; k < 4; ++k) r->origins.push_back(j.origin.q[k]);
        for (int k = 0; k < 3; ++k) r->axes.push_back(j.axis[k]);
        r->types.push_back(j.kind);
        if (j.kind != optik_host::FIXED) {  // joint_limits(), lib.rs:78-84
            r->lb.push_back(j.lower);
            r->ub.push_back(j.upper);
            r->vel.push_back(j.velocity);
        }
    }
    r->device_ids = devices_from_env();
    return r;
}

size_t device_count(const optik_robot *r) { return r->device_ids.empty() ? 1 : r->device_ids.size(); }

int fk_on_device(const optik_robot *r, const double *x, const double *ee16, double *pose7, double *jac) {
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    optik_hip_chain *h = c->chain;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    std::lock_guard<std::mutex> lock(r->mu);
    optik::DeviceScope dev_scope(c->device);
    if (!dev_scope.ok()) return set_err(-1, kSetDeviceMsg);
    // one configuration: the kernel reads q from and writes the pose / Jacobian to pinned host
    // memory (one launch and one wait instead of three copies around them: 43 -> ~20 us per call)
    double *p_q = c->h_scratch.get(), *p_pose = p_q + r->n, *p_jac = p_pose + 7;
    std::memcpy(p_q, x, sizeof(double) * (size_t)r->n);
    if (optik_hip_fk_batch(h, ee16 ? ee7 : nullptr, p_q, 1, p_pose, jac ? p_jac : nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (hipStreamSynchronize(nullptr) != hipSuccess) return set_err(-1, "kernel failed");
    if (pose7) std::memcpy(pose7, p_pose, sizeof(double) * 7);
    if (jac) std::memcpy(jac, p_jac, sizeof(double) * 6 * (size_t)r->n);
    return 0;
}

double *malloc_copy(const double *src, size_t count) {
    double *p = (double *)std::malloc(sizeof(double) * (count ? count : 1));
    if (!p) panic("out of memory");
    std::memcpy(p, src, sizeof(double) * count);
    return p;
}

// targets16 [T][16] (row-major or column-major 4x4) -> [T][7] poses, the iterative or the closed-form conversion
std::vector<double> targets_pose7(int32_t T, const double *targets16, bool row_major, bool iterative) {
    std::vector<double> tgt7((size_t)T * 7);
    parallel_ranges((size_t)T, [&](size_t t0, size_t t1) {
        for (size_t t = t0; t < t1; ++t) {
            const double *m = targets16 + t * 16;
            double cm[16];
            if (row_major) {
                for (int a = 0; a < 4; ++a)
                    for (int b = 0; b < 4; ++b) cm[b * 4 + a] = m[a * 4 + b];
                m = cm;
            }
            if (iterative) pose7_from_mat16_iterative(m, &tgt7[t * 7]);
            else pose7_from_mat16(m, &tgt7[t * 7]);
        }
    });
    return tgt7;
}

// The host-side checks of a batch of targets (optik_robot_ik_batch_poses, optik_robot_ik_solutions,
// optik_robot_ik_path): with OPTIK_BATCH_VALIDATE_POSES every target's isometry test (-3), then every seed against the
// joint limits (-2).  S: the number of seeds, T by default.
int check_batch_inputs(const optik_robot *r, int32_t T, const double *targets16, uint32_t flags, const double *x0,
                                    int32_t S = -1) {
    const int n = r->n;
    const bool row_major = (flags & OPTIK_BATCH_ROW_MAJOR) != 0;
    if (flags & OPTIK_BATCH_VALIDATE_POSES) {
        // nalgebra try_convert::<Matrix4, Isometry3> (optik-py/src/lib.rs:8-15): bottom row exactly
        // (0, 0, 0, 1), R'R = I within 100 eps per entry, det R > 0.  Neither test depends on
        // whether the 3x3 block is read by rows or by columns up to the bottom-row position.
        const double eps = 100.0 * 2.220446049250313e-16;
        std::atomic<bool> all_ok{true};
        parallel_ranges((size_t)T, [&](size_t t0, size_t t1) {
        for (size_t t = t0; t < t1; ++t) {
            const double *m = targets16 + t * 16;
            auto M = [&](int a, int b) { return row_major ? m[a * 4 + b] : m[b * 4 + a]; };
            bool ok = M(3, 0) == 0.0 && M(3, 1) == 0.0 && M(3, 2) == 0.0 && M(3, 3) == 1.0;
            for (int a = 0; a < 3 && ok; ++a)
                for (int b = 0; b < 3 && ok; ++b) {
                    const double d = M(0, a) * M(0, b) + M(1, a) * M(1, b) + M(2, a) * M(2, b) - (a == b ? 1.0 : 0.0);
                    ok = std::fabs(d) <= eps;  // false for NaN
                }
            if (ok) {
                const double det = M(0, 0) * (M(1, 1) * M(2, 2) - M(1, 2) * M(2, 1))
                                   - M(0, 1) * (M(1, 0) * M(2, 2) - M(1, 2) * M(2, 0))
                                   + M(0, 2) * (M(1, 0) * M(2, 1) - M(1, 1) * M(2, 0));
                ok = det > 0.0;
            }
            if (!ok) { all_ok = false; return; }
        }
        });
        if (!all_ok) return set_err(-3, "invalid target transform specified");
    }
    if (S < 0) S = T;
    for (int t = 0; t < S; ++t)
        for (int i = 0; i < n; ++i)
            if (x0[(size_t)t * n + i] < r->lb[i] || x0[(size_t)t * n + i] > r->ub[i])
                return set_err(-2, "seed joint position outside of joint limits");
    return 0;
}

// fn(ctx, t0, t1, err) -> rc for one contiguous part [t0, t1) of the T targets per device of the robot, each part
// on its own host thread; last_parts is set.  0, or -1 with the first failing part's message.
template <class Fn>
int run_device_parts(const optik_robot *r, int32_t T, Fn fn) {
    size_t G = device_count(r);
    if (G > (size_t)T) G = (size_t)T;
    struct Part { DeviceCtx *ctx; int32_t t0, t1; int rc; std::string err; };
    std::vector<Part> parts;
    for (size_t g = 0; g < G; ++g) {
        Part p{device_ctx(r, g), (int32_t)((int64_t)T * (int64_t)g / (int64_t)G),
               (int32_t)((int64_t)T * (int64_t)(g + 1) / (int64_t)G), 0, {}};
        if (!p.ctx) return -1;
        parts.push_back(p);
    }
    r->last_parts.store((int32_t)parts.size());
    return run_parts(parts, [&](Part &p) { p.rc = fn(p.ctx, p.t0, p.t1, p.err); });
}

// optik_robot_ik_batch_ex for the targets of one GPU: rounds of `round` restart indices per
// target (sizes: see the loop), each round ONE launch of optik_hip_ik_batch (which picks the solver by
// launch size); targets already solved (Speed) drop out of later rounds; max_time is enforced inside a
// launch and between rounds.
int ik_batch_on_device(const optik_robot *r, DeviceCtx *c, const CSolverConfig *config, int32_t T,
                       const double *targets16, bool row_major, bool iterative, const double *x0, const double *ee7,
                       std::chrono::steady_clock::time_point start, double *x_out, double *f_out,
                       int32_t *found_out, std::string &err) {
    const int n = r->n;
    auto elapsed = [&]() {
        return std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
    };
    const uint64_t max_restarts = config->max_restarts > 0 ? config->max_restarts : UINT64_MAX;
    const bool quality = config->solution_mode != OPTIK_MODE_SPEED;  // (Manipulability, Condition: as Quality)
    // (the collision filter: Speed takes Quality's route in each round; a target's first round with a free success
    // holds its lowest-index one, so the target still leaves the batch then.  Read before batch_mu: the setters take
    // the robot's lock first)
    const bool filtered = r->collision_active();
    // work items (target x restart index) per round: ~4 M -- 288 MB of per-restart keys, points and residuals
    const uint64_t round_items = (uint64_t)4 << 20;
    BatchGuard guard(c);
    if (!guard.ok()) { err = kSetDeviceMsg; return -1; }

    std::vector<double> tgt7 = targets_pose7(T, targets16, row_major, iterative), best_key((size_t)T, 0.0);
    std::vector<uint64_t> best_idx((size_t)T, UINT64_MAX);
    std::vector<int> live((size_t)T);
    for (int t = 0; t < T; ++t) live[t] = t;
    for (int t = 0; t < T; ++t) if (found_out) found_out[t] = 0;

    // one device block and its pinned mirror, kept with the context across calls
    const size_t n_in = (size_t)(7 + n) * (size_t)T, n_out = (size_t)(n + 3) * (size_t)T;
    if (!reserve_batch(c, n_in + n_out)) { err = kBatchAllocMsg; return -1; }
    // Speed: the first round is latency-sized -- 128 indices: with a third of the restarts succeeding
    // it leaves no reachable target unsolved, and the abandoned indices of a round still cost the
    // solve kernel's groups a queue fetch each (measured per first-round size 16 / 32 / 64 / 128 / 256:
    // 1 024 targets 3.7 / 2.0 / 2.1 / 2.2 / 2.2 ms, 16 384 targets 9.8 / 9.5 / 8.7 / 8.3 / 9.4 ms; 32 768
    // targets 15.9 ms at 64, 13.5 at 128, 16.8 at 256); what is
    // still unsolved after it is hard or unreachable and throughput-bound, so every later round covers
    // four times as many indices (ten unreachable targets x 100 000 restarts are 8 rounds instead of 390)
    const uint64_t first_round = 128;
    uint64_t speed_round = first_round;
    for (uint64_t begin = 0; begin < max_restarts && !live.empty();) {
        double deadline = 0.0;
        if (config->max_time > 0.0) {
            deadline = config->max_time - elapsed();
            if (deadline <= 0.0) break;  // lib.rs:393
        }
        const size_t L = live.size();
        uint64_t round = quality ? 256 : speed_round;
        // (a round's items are capped -- down to 64 indices per target, which still leave no reachable target
        // unsolved; batches of more than 65 536 targets down to 8: nearly all of a round's higher indices are
        // abandoned unissued -- a third to a half of the restarts succeed -- and skipping an item still costs the
        // refilling wave a queue fetch; the handful of targets a short round leaves unsolved go through the next)
        const uint64_t min_round = L <= 65536 ? (first_round < 64 ? first_round : 64u) : 8u;
        const uint64_t cap_items = L <= 65536 ? round_items : 2 * round_items;
        while (round > min_round && round * (uint64_t)L > cap_items) round >>= 1;
        if (!quality && speed_round < ((uint64_t)1 << 40)) speed_round *= 4;
        // Quality runs every restart of every target to the end: nothing to gain from short rounds -- as many
        // indices per round as ~4 M items allow
        if (quality)
            while (round * 2 * (uint64_t)L <= round_items && round < max_restarts - begin) round <<= 1;
        const uint64_t end = (max_restarts - begin > round) ? begin + round : max_restarts;
        double *h_t = c->h_batch.get(), *h_x0 = h_t + 7 * L, *h_out = h_x0 + (size_t)n * L;
        double *d_t = c->d_batch.get(), *d_x0 = d_t + 7 * L, *d_wx = d_x0 + (size_t)n * L, *d_wf = d_wx + (size_t)n * L,
               *d_wk = d_wf + L;
        uint64_t *d_wi = reinterpret_cast<uint64_t *>(d_wk + L);
        parallel_ranges(L, [&](size_t k0, size_t k1) {
            for (size_t k = k0; k < k1; ++k) {
                std::memcpy(&h_t[k * 7], &tgt7[(size_t)live[k] * 7], sizeof(double) * 7);
                std::memcpy(&h_x0[k * n], &x0[(size_t)live[k] * n], sizeof(double) * (size_t)n);
            }
        });
        if (hipMemcpyAsync(d_t, h_t, sizeof(double) * (size_t)(7 + n) * L, hipMemcpyHostToDevice, nullptr) != hipSuccess) {
            err = "upload failed";
            return -1;
        }
        optik_hip_ik_outputs o;
        std::memset(&o, 0, sizeof o);
        o.d_win_x = d_wx; o.d_win_f = d_wf; o.d_win_idx = d_wi; o.d_win_key = d_wk;
        // One launch per round.  The first rounds of a Speed batch are latency-bound -- early exit abandons most of
        // their restarts, what is left is each target's few first restarts run to the end: restart-major hand-out
        // keeps only a few restarts per target in flight (optik_hip_ik_batch then stays on the quad solver's shorter
        // trip).  Everything else -- a Quality batch, the later rounds of a Speed batch (whatever 256 restarts did
        // not solve runs nearly all of its restarts) -- is throughput-bound: target-major, the lane-per-restart form
        // from one full load of the chip on.  (Rounds 1-4 ran those rounds, and the first round of batches of 40 960
        // targets or more, on a streaming engine: retired in round 5, the single launch is 15 - 28 % faster at every
        // size where the engine was used -- profiles/r5a_engine_retire_probe.txt.)
        const uint32_t mode_flags =
            (quality || filtered) ? 0u : (OPTIK_HIP_IK_EARLY_EXIT | (r->parallelism != 1 ? OPTIK_HIP_IK_FIND_ANY : 0u));
        const int rck = optik_hip_ik_batch(c->chain, config, d_t, d_x0, (int32_t)L, ee7, begin, end,
                                           mode_flags | ((!quality && !filtered && begin < 256) ? OPTIK_HIP_IK_RESTART_MAJOR : 0u),
                                           deadline, &o, nullptr);
        if (rck) { err = optik_hip_last_error(); return -1; }
        if (hipMemcpyAsync(h_out, d_wx, sizeof(double) * (size_t)(n + 3) * L, hipMemcpyDeviceToHost, nullptr) != hipSuccess
            || hipStreamSynchronize(nullptr) != hipSuccess) {
            err = "download failed";
            return -1;
        }
        const double *wx = h_out, *wf = wx + (size_t)n * L, *wk = wf + L;
        const uint64_t *wi = reinterpret_cast<const uint64_t *>(wk + L);
        // every target appears once in `live`, so ranges of k touch disjoint targets
        std::vector<uint8_t> keep(L);
        parallel_ranges(L, [&](size_t k0, size_t k1) {
            for (size_t k = k0; k < k1; ++k) {
                const int t = live[k];
                keep[k] = 1;
                if (wi[k] == UINT64_MAX) continue;
                const bool better = best_idx[t] == UINT64_MAX || wk[k] < best_key[t]
                                    || (wk[k] == best_key[t] && wi[k] < best_idx[t]);
                if (better) {
                    best_idx[t] = wi[k]; best_key[t] = wk[k];
                    if (x_out) std::memcpy(&x_out[(size_t)t * n], &wx[k * n], sizeof(double) * (size_t)n);
                    if (f_out) f_out[t] = wf[k];
                    if (found_out) found_out[t] = 1;
                }
                if (!quality) keep[k] = 0;  // Speed: the first solution ends this target
            }
        });
        std::vector<int> still;
        for (size_t k = 0; k < L; ++k)
            if (keep[k]) still.push_back(live[k]);
        live.swap(still);
        begin = end;
    }
    return 0;
}

// optik_robot_ik_solutions for the targets of one GPU: chunks of whole targets, each ONE launch of
// optik_hip_ik_solutions over every restart index [0, R) (about 4 M work items a launch at most, as the rounds of
// ik_batch_on_device).  A chunk that starts after the max_time budget is spent is not run: its targets keep count 0.
int ik_solutions_on_device(const optik_robot *r, DeviceCtx *c, const CSolverConfig *config, int32_t T,
                           const double *targets16, bool row_major, bool iterative, const double *x0,
                           const double *ee7, std::chrono::steady_clock::time_point start, int32_t K, double min_dist,
                           int32_t *count_out, double *x_out, double *f_out, uint64_t *idx_out, std::string &err) {
    const int n = r->n;
    const uint64_t R = config->max_restarts;
    const uint64_t round_items = (uint64_t)4 << 20;
    const size_t chunk = (size_t)std::min<uint64_t>((uint64_t)T, std::max<uint64_t>(1, round_items / R));
    BatchGuard guard(c);
    if (!guard.ok()) { err = kSetDeviceMsg; return -1; }
    const std::vector<double> tgt7 = targets_pose7(T, targets16, row_major, iterative);

    // the robot's batch block: in = targets [C][7] | x0 [C][n]; out = x [C][K][n] | f [C][K] | idx [C][K] | count [C]
    const size_t KC = (size_t)K * chunk;
    const size_t n_in = (size_t)(7 + n) * chunk, n_out = KC * (size_t)(n + 2) + chunk;
    if (!reserve_batch(c, n_in + n_out)) { err = kBatchAllocMsg; return -1; }
    for (size_t t0 = 0; t0 < (size_t)T; t0 += chunk) {
        const size_t L = std::min(chunk, (size_t)T - t0), KL = (size_t)K * L;
        double deadline = 0.0;
        if (config->max_time > 0.0) {
            deadline = config->max_time - std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
            if (deadline <= 0.0) break;  // (the targets left keep count 0)
        }
        double *h_t = c->h_batch.get(), *h_out = h_t + (size_t)(7 + n) * L;
        double *d_t = c->d_batch.get(), *d_x0 = d_t + 7 * L, *d_x = d_x0 + (size_t)n * L, *d_f = d_x + KL * (size_t)n;
        uint64_t *d_idx = reinterpret_cast<uint64_t *>(d_f + KL);
        int32_t *d_count = reinterpret_cast<int32_t *>(d_idx + KL);
        std::memcpy(h_t, &tgt7[t0 * 7], sizeof(double) * 7 * L);
        std::memcpy(h_t + 7 * L, x0 + t0 * (size_t)n, sizeof(double) * (size_t)n * L);
        if (hipMemcpyAsync(d_t, h_t, sizeof(double) * (size_t)(7 + n) * L, hipMemcpyHostToDevice, nullptr) != hipSuccess) {
            err = "upload failed";
            return -1;
        }
        optik_hip_ik_solutions_outputs o;
        o.d_count = d_count; o.d_x = d_x; o.d_f = d_f; o.d_idx = d_idx; o.d_key = nullptr;
        if (optik_hip_ik_solutions(c->chain, config, d_t, d_x0, (int32_t)L, ee7, 0, R, deadline, K, min_dist, &o,
                                   nullptr)) {
            err = optik_hip_last_error();
            return -1;
        }
        const size_t out_doubles = KL * (size_t)(n + 2) + L;
        if (hipMemcpyAsync(h_out, d_x, sizeof(double) * out_doubles, hipMemcpyDeviceToHost, nullptr) != hipSuccess
            || hipStreamSynchronize(nullptr) != hipSuccess) {
            err = "download failed";
            return -1;
        }
        const double *hx = h_out, *hf = hx + KL * (size_t)n;
        const uint64_t *hi = reinterpret_cast<const uint64_t *>(hf + KL);
        const int32_t *hc = reinterpret_cast<const int32_t *>(hi + KL);
        if (x_out) std::memcpy(x_out + t0 * (size_t)K * n, hx, sizeof(double) * KL * (size_t)n);
        if (f_out) std::memcpy(f_out + t0 * (size_t)K, hf, sizeof(double) * KL);
        if (idx_out) std::memcpy(idx_out + t0 * (size_t)K, hi, sizeof(uint64_t) * KL);
        if (count_out) std::memcpy(count_out + t0, hc, sizeof(int32_t) * L);
    }
    return 0;
}

// optik_robot_ik_path for the paths of one GPU: chunks of whole paths, each ONE upload, ONE optik_hip_ik_path (every
// waypoint of the chunk, stream-ordered) and ONE download.  A chunk's waypoint launch holds about 4 M (path, restart)
// items at most, and its share of the robot's batch block about 2^24 doubles (one path at least).
int ik_path_on_device(const optik_robot *r, DeviceCtx *c, const CSolverConfig *config, int32_t P,
                                   int32_t L, const double *tgt7, const double *x0, const double *ee7, double max_step,
                                   double *x_out, double *f_out, uint64_t *idx_out, double *step_out,
                                   int32_t *found_out, std::string &err) {
    const int n = r->n;
    const uint64_t R = config->max_restarts;
    const size_t per_path = (size_t)L * (size_t)(7 + n + 3) + (size_t)n;  // doubles of the block per path
    const uint64_t round_items = (uint64_t)4 << 20;
    size_t chunk = (size_t)std::min<uint64_t>((uint64_t)P, std::max<uint64_t>(1, round_items / R));
    chunk = std::min(chunk, std::max<size_t>(1, ((size_t)1 << 24) / per_path));
    // Speed without a step limit: restart-major hand-out, so that every path's restart 0 (its warm start) runs first
    // (not under the collision filter: every restart runs to its end there, as in Quality)
    const uint32_t flags = (config->solution_mode == OPTIK_MODE_SPEED && !(max_step < __builtin_huge_val())
                            && !r->collision_active()) ? OPTIK_HIP_IK_RESTART_MAJOR : 0u;
    const double deadline = config->max_time > 0.0 ? config->max_time : 0.0;
    BatchGuard guard(c);
    if (!guard.ok()) { err = kSetDeviceMsg; return -1; }

    // the robot's batch block: in = targets [L][C][7] | x0 [C][n]; out = x [L][C][n] | f [L][C] | idx [L][C] |
    // step [L][C]
    const size_t need = per_path * chunk;
    if (!reserve_batch(c, need)) { err = kBatchAllocMsg; return -1; }
    for (size_t p0 = 0; p0 < (size_t)P; p0 += chunk) {
        const size_t C = std::min(chunk, (size_t)P - p0), LC = (size_t)L * C;
        double *h_t = c->h_batch.get(), *h_out = h_t + 7 * LC + (size_t)n * C;
        double *d_t = c->d_batch.get(), *d_x0 = d_t + 7 * LC, *d_x = d_x0 + (size_t)n * C, *d_f = d_x + LC * (size_t)n;
        uint64_t *d_idx = reinterpret_cast<uint64_t *>(d_f + LC);
        double *d_step = reinterpret_cast<double *>(d_idx + LC);
        // (paths p0.. of tgt7 [P][L][7] -> [L][C][7], waypoint-major)
        for (size_t p = 0; p < C; ++p)
            for (int32_t l = 0; l < L; ++l)
                std::memcpy(h_t + ((size_t)l * C + p) * 7, tgt7 + ((p0 + p) * (size_t)L + (size_t)l) * 7,
                            sizeof(double) * 7);
        std::memcpy(h_t + 7 * LC, x0 + p0 * (size_t)n, sizeof(double) * (size_t)n * C);
        if (hipMemcpyAsync(d_t, h_t, sizeof(double) * (7 * LC + (size_t)n * C), hipMemcpyHostToDevice, nullptr)
            != hipSuccess) {
            err = "upload failed";
            return -1;
        }
        optik_hip_ik_path_outputs o;
        std::memset(&o, 0, sizeof o);
        o.d_x = d_x; o.d_f = d_f; o.d_idx = d_idx; o.d_step = d_step;
        if (optik_hip_ik_path(c->chain, config, d_t, d_x0, (int32_t)C, L, ee7, 0, R, flags, deadline, max_step, &o,
                              nullptr)) {
            err = optik_hip_last_error();
            return -1;
        }
        const size_t out_doubles = LC * (size_t)(n + 3);
        if (hipMemcpyAsync(h_out, d_x, sizeof(double) * out_doubles, hipMemcpyDeviceToHost, nullptr) != hipSuccess
            || hipStreamSynchronize(nullptr) != hipSuccess) {
            err = "download failed";
            return -1;
        }
        const double *hx = h_out, *hf = hx + LC * (size_t)n;
        const uint64_t *hi = reinterpret_cast<const uint64_t *>(hf + LC);
        const double *hs = reinterpret_cast<const double *>(hi + LC);
        // ([L][C] -> path-major [P][L])
        for (size_t p = 0; p < C; ++p)
            for (int32_t l = 0; l < L; ++l) {
                const size_t dv = (size_t)l * C + p, hv = (p0 + p) * (size_t)L + (size_t)l;
                if (x_out) std::memcpy(x_out + hv * n, hx + dv * n, sizeof(double) * (size_t)n);
                if (f_out) f_out[hv] = hf[dv];
                if (idx_out) idx_out[hv] = hi[dv];
                if (step_out) step_out[hv] = hs[dv];
                if (found_out) found_out[hv] = hi[dv] != UINT64_MAX ? 1 : 0;
            }
    }
    return 0;
}

}  // namespace

namespace optik {
namespace robot {

DeviceCtx *device_ctx(const optik_robot *r, size_t k) {
    std::lock_guard<std::mutex> lock(r->mu);
    if (r->devs.empty()) r->devs.resize(device_count(r));
    if (k >= r->devs.size()) { g_robot_err = "no such device context"; return nullptr; }
    if (r->devs[k]) return r->devs[k].get();
    int devid = 0;
    if (r->device_ids.empty()) (void)hipGetDevice(&devid);
    else devid = r->device_ids[k];
    // (the caller's device is current again when this returns, also when the set-up fails)
    optik::DeviceScope dev_scope(devid);
    if (!dev_scope.ok()) {
        g_robot_err = "hipSetDevice(" + std::to_string(devid) + ") failed";
        return nullptr;
    }
    // (a context whose set-up fails is deleted on return, with its device still current)
    std::unique_ptr<DeviceCtx> c(new DeviceCtx());
    if (optik_hip_chain_create(r->origins.data(), r->axes.data(), r->types.data(), (int32_t)r->types.size(),
                               r->lb.data(), r->ub.data(), r->n, &c->chain)) {
        g_robot_err = std::string("GPU chain creation failed: ") + optik_hip_last_error();
        return nullptr;
    }
    optik_hip_chain *h = c->chain;
    if (c->d_scratch.reserve((size_t)(r->n + 7 + 6 * r->n)) != hipSuccess
        || c->h_scratch.reserve((size_t)(r->n + 7 + 6 * r->n)) != hipSuccess) {
        g_robot_err = "GPU scratch allocation failed";
        return nullptr;
    }
    // (a model or world set before this chain existed)
    if ((!r->coll_frames.empty()
         && optik_hip_chain_set_collision_model(h, r->coll_frames.data(), r->coll_centers.data(), r->coll_radii.data(),
                                                (int32_t)r->coll_frames.size(), r->coll_pairs.data(),
                                                (int32_t)(r->coll_pairs.size() / 2), r->coll_margin))
        || ((!r->world_spheres.empty() || !r->world_boxes.empty())
            && optik_hip_chain_set_world(h, r->world_spheres.data(), (int32_t)(r->world_spheres.size() / 4),
                                         r->world_boxes.data(), (int32_t)(r->world_boxes.size() / 10)))
        || (!r->grid_values.empty()
            && optik_hip_chain_set_world_grid(h, r->grid_origin, r->grid_voxel, r->grid_n[0], r->grid_n[1],
                                              r->grid_n[2], r->grid_values.data()))
        || (r->motion_h > 0.0 && optik_hip_chain_set_motion_resolution(h, r->motion_h))) {
        g_robot_err = std::string("collision model, world or motion resolution upload failed: ") + optik_hip_last_error();
        return nullptr;
    }
    (void)hipDeviceGetAttribute(&c->num_cus, hipDeviceAttributeMultiprocessorCount, devid);
    c->device = devid;
    r->devs[k] = std::move(c);
    return r->devs[k].get();
}

}  // namespace robot
}  // namespace optik

extern "C" {

const char *optik_robot_last_error(void) { return g_robot_err.c_str(); }

int optik_robot_try_from_urdf_str(const char *urdf, const char *base_link, const char *ee_link,
                                  optik_robot **out) {
    if (!urdf || !base_link || !ee_link || !out) return set_err(-1, "null argument");
    try {
        *out = make_robot(urdf, base_link, ee_link);
        return 0;
    } catch (const std::exception &e) {
        return set_err(-1, e.what());
    }
}

optik_robot *optik_robot_from_urdf_str(const char *urdf, const char *base_link, const char *ee_link) {
    optik_robot *r = nullptr;
    if (optik_robot_try_from_urdf_str(urdf, base_link, ee_link, &r)) panic(g_robot_err);
    return r;
}

optik_robot *optik_robot_from_urdf_file(const char *path, const char *base_link, const char *ee_link) {
    std::ifstream in(path ? path : "");
    if (!in) panic("error parsing URDF file!");  // lib.rs:55
    std::stringstream ss;
    ss << in.rdbuf();
    return optik_robot_from_urdf_str(ss.str().c_str(), base_link, ee_link);
}

void optik_robot_free(optik_robot *r) {
    if (!r) return;
    for (auto &c : r->devs) {
        if (!c) continue;
        optik::DeviceScope dev_scope(c->device);  // the caller's device is current again afterwards
        c.reset();                                // (the chain, then the context's blocks)
    }
    delete r;
}

int optik_robot_set_devices(optik_robot *r, const int32_t *device_ids, int32_t count) {
    if (!r || count < 0 || (count > 0 && !device_ids)) return set_err(-1, "bad argument");
    std::lock_guard<std::mutex> lock(r->mu);
    if (!r->devs.empty()) return set_err(-1, "set_devices must be called before the robot's first GPU call");
    int have = 0;
    if (hipGetDeviceCount(&have) != hipSuccess) have = 0;
    for (int i = 0; i < count; ++i)
        if (device_ids[i] < 0 || device_ids[i] >= have) return set_err(-1, "no such HIP device");
    r->device_ids.assign(device_ids, device_ids + count);
    return 0;
}

int32_t optik_robot_num_devices(const optik_robot *r) { return r ? (int32_t)device_count(r) : 0; }
int32_t optik_robot_last_parts(const optik_robot *r) { return r ? r->last_parts.load() : 0; }

void optik_robot_set_parallelism(optik_robot *r, unsigned int n) {
    // The GPU grid is sized from the device; n only selects Speed's early-exit rule (see optik_robot).
    if (r) r->parallelism = n;
}

unsigned int optik_robot_num_positions(const optik_robot *r) { return r ? (unsigned)r->n : 0u; }

const double *optik_robot_joint_limits(const optik_robot *r) {
    std::vector<double> v(r->lb);
    v.insert(v.end(), r->ub.begin(), r->ub.end());
    return malloc_copy(v.data(), v.size());
}

const double *optik_robot_velocity_limits(const optik_robot *r) { return malloc_copy(r->vel.data(), r->vel.size()); }

int optik_robot_fk_ex(const optik_robot *r, const double *x, const double *ee16, double *pose16) {
    double p7[7];
    if (fk_on_device(r, x, ee16, p7, nullptr)) return -1;
    mat16_from_pose7(p7, pose16);
    return 0;
}

int optik_robot_joint_jacobian_ex(const optik_robot *r, const double *x, const double *ee16, double *jac) {
    return fk_on_device(r, x, ee16, nullptr, jac);
}

const double *optik_robot_fk(const optik_robot *r, const double *x) {
    double m[16];
    if (optik_robot_fk_ex(r, x, nullptr, m)) panic(g_robot_err);
    return malloc_copy(m, 16);
}

const double *optik_robot_joint_jacobian(const optik_robot *r, const double *x) {
    std::vector<double> j(6 * (size_t)r->n);
    if (optik_robot_joint_jacobian_ex(r, x, nullptr, j.data())) panic(g_robot_err);
    return malloc_copy(j.data(), j.size());
}

const double *optik_robot_random_configuration(const optik_robot *r) {
    // rand::rng(): thread-local, non-deterministic (optik-cpp/src/lib.rs:122)
    thread_local std::mt19937_64 gen{std::random_device{}()};
    std::vector<double> q((size_t)r->n);
    for (int k = 0; k < r->n; ++k) {
        if (!std::isfinite(r->lb[k]) || !std::isfinite(r->ub[k]))
            panic("random_configuration: non-finite joint limits");  // rand: Uniform::new_inclusive fails
        q[k] = std::uniform_real_distribution<double>(r->lb[k], std::nextafter(r->ub[k], INFINITY))(gen);
        if (q[k] > r->ub[k]) q[k] = r->ub[k];
    }
    return malloc_copy(q.data(), q.size());
}

// Robot::ik, lib.rs:241-415.
int optik_robot_ik_ex(const optik_robot *r, const CSolverConfig *config, const double *target16,
                      const double *x0, const double *ee16, double *x_out, double *f_out,
                      uint64_t *winner_out) {
    return optik_robot_ik_pose(r, config, target16, 0u, x0, ee16, x_out, f_out, winner_out);
}

int optik_pose_from_matrix(const double *m16, uint32_t flags, double *pose7) {
    if (!m16 || !pose7) return set_err(-1, "null argument");
    if (flags & OPTIK_POSE_FROM_MATRIX) pose7_from_mat16_iterative(m16, pose7);
    else pose7_from_mat16(m16, pose7);
    return 0;
}

int optik_robot_ik_pose(const optik_robot *r, const CSolverConfig *config, const double *target16, uint32_t flags,
                        const double *x0, const double *ee16, double *x_out, double *f_out, uint64_t *winner_out) {
    if (!r || !config || !target16 || !x0) return set_err(-1, "null argument");
    const bool iterative = (flags & OPTIK_POSE_FROM_MATRIX) != 0;
    // lib.rs:251-254
    for (int i = 0; i < r->n; ++i)
        if (x0[i] < r->lb[i] || x0[i] > r->ub[i])
            return set_err(-2, "seed joint position outside of joint limits");
    DeviceCtx *c0 = device_ctx(r);
    if (!c0) return -1;
    double tgt7[7], ee7[7];
    if (iterative) pose7_from_mat16_iterative(target16, tgt7);
    else pose7_from_mat16(target16, tgt7);
    if (ee16) pose7_from_mat16(ee16, ee7);

    const auto start = std::chrono::steady_clock::now();
    auto elapsed = [&]() {
        return std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
    };
    const uint64_t max_restarts = config->max_restarts > 0 ? config->max_restarts : UINT64_MAX;  // lib.rs:273-277
    // (Manipulability and Condition are scheduled as Quality: every restart runs, the best key wins)
    const bool quality = config->solution_mode != OPTIK_MODE_SPEED;
    // The first launch covers as many restart indices as the chip holds resident waves (one
    // restart per wave: no wave pays for the phases of 63 other restarts, and a third to a
    // half of the restarts succeed, so it almost always contains the answer); later launches
    // cover enough 64-lane tiles to fill every CU a few times over -- on every GPU of the robot
    // at once: device g of G takes the g-th contiguous part of the round's index range
    // (lib.rs:297-300 shards the same range over rayon workers) and the host keeps the
    // minimum of the G (key, index) records.
    // A call that is still running after those two launches (a hard target, or Quality with a large
    // budget) is throughput-bound: rounds of 1 M restarts per GPU, each one launch of the lane-per-restart form.
    const uint64_t cus = (uint64_t)(c0->num_cus > 0 ? c0->num_cus : 256);
    // restarts of the first, latency-sized launch: four per CU -- one per SIMD, the most the quad solver's one-restart-
    // per-wave form takes -- under the first-success rule (the more restarts race, the sooner the first one succeeds: the
    // fastest of 512 needs 18.6 evaluations on average, of 1024 17.9; 1024 waves run each a little slower, but since
    // the call returns on the first success the launch's tail no longer counts: 201 -> 194 us per call, 221 -> 216 us
    // back to back); 128 under the deterministic rule (parallelism 1: the answer is the lowest successful index,
    // nearly always below ten, and only the restarts below it decide when the launch ends: 685 -> 660 us per call,
    // profiles/r4g_single_call.txt)
#ifndef OPTIK_FIRST_PER_CU
#define OPTIK_FIRST_PER_CU 4  // (tools/build_lib_variant.py fpcN -DOPTIK_FIRST_PER_CU=N --only=robot_host.o: the comparison above)
#endif
    const uint64_t first_per_cu = OPTIK_FIRST_PER_CU;
    const uint64_t first_batch = (!quality && r->parallelism == 1) ? 128 : cus * first_per_cu;
    const uint64_t later_batch = cus * 2 * 64 * 2;
    // (a big round is one launch of the lane-per-restart form and worth ~1 M restarts, because every launch pays its
    // own few ms of drain; rounds 1-3 ran them on a streaming engine that the lane form beat at every size in round 4
    // and that was retired in round 5: profiles/r5a_engine_retire_probe.txt)
#ifndef OPTIK_QUALITY_BATCH_LOG2
#define OPTIK_QUALITY_BATCH_LOG2 22
#endif
    // restarts per GPU per big round: 1 M under Speed (a round that finds a solution ends the call); 4 M under Quality,
    // which runs every restart anyway -- one drain (~3.5 ms) per 4 M instead of per 1 M: a 4 M-restart call 138 -> 129 ms
    // (288 MB of per-restart keys, points and residuals per device)
    // Under a time budget the rounds stay at 1 M: a launch that meets its deadline still has to fetch, seed and publish
    // every item left and the selection runs over the whole round, so the overshoot of max_time grows with the round
    // (ADVICE r5); the 4 M rounds' gain was measured without a deadline.
    const uint64_t big_batch = (uint64_t)1 << ((quality && !(config->max_time > 0.0)) ? OPTIK_QUALITY_BATCH_LOG2 : 20);
    const uint64_t big_from = 262144;              // (from this many restarts left on: rounds of big_batch)
    const size_t G = device_count(r);
    // (the collision filter: Speed takes Quality's route -- no early exit, no first-success claim -- and keeps its keys,
    // so the first round with a free success holds the lowest-index one and still ends the call)
    const uint32_t speed_flags = r->collision_active() ? 0u
                                 : OPTIK_HIP_IK_EARLY_EXIT | (r->parallelism != 1 ? OPTIK_HIP_IK_FIND_ANY : 0u);
    struct Part {
        DeviceCtx *ctx = nullptr;
        uint64_t begin = 0, end = 0, widx = UINT64_MAX;
        double wf = 0.0, wkey = 0.0;
        std::vector<double> wx;
        int rc = 0;
        std::string err;
    };
    bool have = false;
    double best_key = 0.0, best_f = 0.0;
    uint64_t best_idx = UINT64_MAX;
    std::vector<double> best_x((size_t)r->n);
    for (uint64_t begin = 0; begin < max_restarts;) {
        // lib.rs:393: stop issuing restarts once out of time
        double deadline = 0.0;
        if (config->max_time > 0.0) {
            deadline = config->max_time - elapsed();
            if (deadline <= 0.0) break;
        }
        // Quality with a restart budget and no time budget runs every restart whatever happens: no
        // latency-sized first launches (each of them waits for its slowest restart -- 1 000 restarts
        // took two launches of 2.7 ms), the whole range at once: one launch of the solve kernel
        // below ~260 000 restarts (big_from), rounds of 1 M from index 0 above.
        // (with a time budget too when the whole range is one solve-kernel launch: its waves watch the clock)
        const bool all_at_once = quality && config->max_restarts > 0
                                 && (config->max_time <= 0.0 || config->max_restarts < big_from);
        // (the latency-sized first launch stays on one GPU; a Quality range run at once is cut over the G devices as
        // soon as every part is a few waves per CU)
        const size_t g_round = (begin == 0 && !(all_at_once && max_restarts / G >= cus * 64)) ? 1 : G;
        const bool big_round = max_restarts - begin >= big_from && (all_at_once || begin >= first_batch + later_batch);
        const uint64_t batch = big_round ? big_batch
                               : all_at_once ? big_from
                               : begin == 0 ? first_batch : later_batch;
        // (several GPUs: what is left is cut evenly when it is less than a full round of each)
        uint64_t per_part = batch;
        if (g_round > 1 && max_restarts != UINT64_MAX) {
            const uint64_t even = (max_restarts - begin + g_round - 1) / g_round;
            if (even < per_part) per_part = even;
        }
        std::vector<Part> parts;
        const bool begin_was_zero = begin == 0;
        for (size_t g = 0; g < g_round && begin < max_restarts; ++g) {
            Part p;
            p.ctx = g == 0 ? c0 : device_ctx(r, g);
            if (!p.ctx) return -1;
            p.begin = begin;
            p.end = (max_restarts - begin > per_part) ? begin + per_part : max_restarts;
            p.wx.resize((size_t)r->n);
            begin = p.end;
            parts.push_back(std::move(p));
        }
        auto run_part = [&](Part &p) {
            p.rc = optik_hip_ik_host(p.ctx->chain, config, tgt7, x0, 1, ee16 ? ee7 : nullptr, p.begin, p.end,
                                     quality ? 0u : speed_flags, deadline,
                                     p.wx.data(), &p.wf, &p.widx, &p.wkey);
            if (p.rc) p.err = optik_hip_last_error();
        };
        if (begin_was_zero) r->last_parts.store(0);
        if ((int32_t)parts.size() > r->last_parts.load()) r->last_parts.store((int32_t)parts.size());
        if (run_parts(parts, run_part)) return -1;
        bool found_round = false;
        for (const Part &p : parts) {
            if (p.widx == UINT64_MAX) continue;
            found_round = true;
            // lib.rs:397-413: Quality keeps the solution closest to the seed, Speed the first one
            if (!have || p.wkey < best_key || (p.wkey == best_key && p.widx < best_idx)) {
                have = true; best_key = p.wkey; best_idx = p.widx; best_f = p.wf; best_x = p.wx;
            }
        }
        if (found_round && !quality) break;
    }
    if (!have) return 1;
    if (x_out) std::memcpy(x_out, best_x.data(), sizeof(double) * (size_t)r->n);
    if (f_out) *f_out = best_f;
    if (winner_out) *winner_out = best_idx;
    return 0;
}

// Many independent ik() calls at once (the motion-planning workload of examples/example.rs:
// a stream of targets, each with its own seed): every target gets the semantics of Robot::ik
// with the same SolverConfig.  The targets are split into contiguous parts over the robot's
// GPUs (BASELINE.json config 5: no collective, the host gathers), each part runs on its GPU
// from its own host thread.
int optik_robot_ik_batch_ex(const optik_robot *r, const CSolverConfig *config, int32_t T,
                            const double *targets16, const double *x0, const double *ee16, double *x_out,
                            double *f_out, int32_t *found_out) {
    return optik_robot_ik_batch_poses(r, config, T, targets16, OPTIK_POSE_FROM_MATRIX, x0, ee16, x_out, f_out, found_out);
}

int optik_robot_ik_batch_poses(const optik_robot *r, const CSolverConfig *config, int32_t T,
                               const double *targets16, uint32_t flags, const double *x0, const double *ee16,
                               double *x_out, double *f_out, int32_t *found_out) {
    if (!r || !config || !targets16 || !x0 || T < 1) return set_err(-1, "bad argument");
    const int n = r->n;
    const bool row_major = (flags & OPTIK_BATCH_ROW_MAJOR) != 0;
    if (int rc = check_batch_inputs(r, T, targets16, flags, x0)) return rc;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    const auto start = std::chrono::steady_clock::now();
    return run_device_parts(r, T, [&](DeviceCtx *ctx, int32_t t0, int32_t t1, std::string &err) {
        return ik_batch_on_device(r, ctx, config, t1 - t0, targets16 + (size_t)t0 * 16, row_major,
                                  (flags & OPTIK_POSE_FROM_MATRIX) != 0,
                                  x0 + (size_t)t0 * n, ee16 ? ee7 : nullptr, start,
                                  x_out ? x_out + (size_t)t0 * n : nullptr, f_out ? f_out + t0 : nullptr,
                                  found_out ? found_out + t0 : nullptr, err);
    });
}

int optik_robot_ik_solutions(const optik_robot *r, const CSolverConfig *config, int32_t T, const double *targets16,
                             uint32_t flags, const double *x0, const double *ee16, int32_t K, double min_dist,
                             int32_t *count_out, double *x_out, double *f_out, uint64_t *idx_out) {
    if (!r || !config || !targets16 || !x0 || T < 1) return set_err(-1, "bad argument");
    if (K < 1 || K > OPTIK_HIP_MAX_SOLUTIONS) return set_err(-1, "ik_solutions: K must be in 1..256");
    if (!(min_dist >= 0.0) || !std::isfinite(min_dist))
        return set_err(-1, "ik_solutions: min_dist must be finite and >= 0");
    if (config->max_restarts == 0)
        return set_err(-1, "ik_solutions: max_restarts must be set (every restart index in [0, max_restarts) runs)");
    if (config->max_restarts > OPTIK_ROBOT_MAX_SOLUTION_RESTARTS)
        return set_err(-1, "ik_solutions: max_restarts must be at most 2^22");
    const int n = r->n;
    if (int rc = check_batch_inputs(r, T, targets16, flags, x0)) return rc;
    // (slots of targets whose chunk is never run stay padding)
    const size_t TK = (size_t)T * (size_t)K;
    if (count_out) std::fill(count_out, count_out + T, 0);
    if (x_out) std::fill(x_out, x_out + TK * (size_t)n, std::numeric_limits<double>::quiet_NaN());
    if (f_out) std::fill(f_out, f_out + TK, std::numeric_limits<double>::quiet_NaN());
    if (idx_out) std::fill(idx_out, idx_out + TK, UINT64_MAX);
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    const auto start = std::chrono::steady_clock::now();
    return run_device_parts(r, T, [&](DeviceCtx *ctx, int32_t t0, int32_t t1, std::string &err) {
        return ik_solutions_on_device(r, ctx, config, t1 - t0, targets16 + (size_t)t0 * 16,
                                      (flags & OPTIK_BATCH_ROW_MAJOR) != 0, (flags & OPTIK_POSE_FROM_MATRIX) != 0,
                                      x0 + (size_t)t0 * n, ee16 ? ee7 : nullptr, start, K, min_dist,
                                      count_out ? count_out + t0 : nullptr, x_out ? x_out + (size_t)t0 * K * n : nullptr,
                                      f_out ? f_out + (size_t)t0 * K : nullptr,
                                      idx_out ? idx_out + (size_t)t0 * K : nullptr, err);
    });
}

int optik_robot_ik_path(const optik_robot *r, const CSolverConfig *config, int32_t P, int32_t L,
                        const double *targets16, uint32_t flags, const double *x0, const double *ee16,
                        double max_step, double *x_out, double *f_out, uint64_t *idx_out, double *step_out,
                        int32_t *found_out) {
    if (!r || !config || !targets16 || !x0 || P < 1 || L < 1) return set_err(-1, "bad argument");
    if ((int64_t)P * (int64_t)L > INT32_MAX) return set_err(-1, "ik_path: too many waypoints (P * L >= 2^31)");
    if (config->max_restarts == 0)
        return set_err(-1, "ik_path: max_restarts must be set (every waypoint runs restarts [0, max_restarts))");
    if (config->max_restarts > OPTIK_HIP_PATH_MAX_RESTARTS)
        return set_err(-1, "ik_path: max_restarts must be at most 4096");
    if (!(max_step >= 0.0)) return set_err(-1, "ik_path: max_step must be >= 0 (+inf: no limit)");
    const int n = r->n;
    if (int rc = check_batch_inputs(r, P * L, targets16, flags, x0, P)) return rc;
    const std::vector<double> tgt7 = targets_pose7(P * L, targets16, (flags & OPTIK_BATCH_ROW_MAJOR) != 0,
                                                   (flags & OPTIK_POSE_FROM_MATRIX) != 0);
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    return run_device_parts(r, P, [&](DeviceCtx *ctx, int32_t p0, int32_t p1, std::string &err) {
        const size_t w = (size_t)p0 * (size_t)L;
        return ik_path_on_device(r, ctx, config, p1 - p0, L, tgt7.data() + w * 7, x0 + (size_t)p0 * n,
                                 ee16 ? ee7 : nullptr, max_step, x_out ? x_out + w * n : nullptr,
                                 f_out ? f_out + w : nullptr, idx_out ? idx_out + w : nullptr,
                                 step_out ? step_out + w : nullptr, found_out ? found_out + w : nullptr, err);
    });
}

const double *optik_robot_ik(const optik_robot *r, const CSolverConfig *config, const double *target,
                             const double *x0) {
    std::vector<double> x((size_t)r->n);
    // (the C path converts the target with the iterative UnitQuaternion::from_matrix: optik-cpp/src/lib.rs:141-142)
    const int rc = optik_robot_ik_pose(r, config, target, OPTIK_POSE_FROM_MATRIX, x0, nullptr, x.data(), nullptr, nullptr);
    if (rc < 0) panic(g_robot_err);
    if (rc == 1) return nullptr;  // optik-cpp/src/lib.rs:158-160
    return malloc_copy(x.data(), x.size());
}

// Robot::diff_ik, lib.rs:123-239: the largest 0 <= alpha <= 1 for which joint velocities v with
// |v_i| <= v_max_i realise the end-effector twist alpha * V_WE (world frame).  The reference hands this LP to
// Clarabel (an interior-point solver; un-vendored); here it is solved exactly by diff_ik_lp.hpp -- the same
// function diff_ik_batch_kernel runs on the device, so a row of optik_robot_diff_ik_batch returns these bits.
// FK and the Jacobian come from the HIP kernels.
int optik_robot_diff_ik_ex(const optik_robot *r, const double *x0, const double *V_WE, const double *v_max,
                           const double *ee16, double *alpha_out, double *v_out) {
    if (!r || !x0 || !V_WE || !v_max) return set_err(-1, "null argument");
    const int n = r->n;
    if (n > 8) return set_err(-1, kDiffIkMaxNMsg);
    double p7[7], jac[6 * 8];
    if (fk_on_device(r, x0, ee16, p7, jac)) return -1;
    double alpha = 0.0, v[8];
    if (optik::lp::diff_ik_lp<8>(n, p7 + 3, jac, V_WE, v_max, &alpha, v)) return 1;
    if (alpha_out) *alpha_out = alpha;
    if (v_out) std::memcpy(v_out, v, sizeof(double) * (size_t)n);
    return 0;
}

// lib.rs:165-183 of optik-cpp: the joint velocities only, malloc'ed; NULL = no solution.
const double *optik_robot_diff_ik(const optik_robot *r, const double *x0, const double *V_WE, const double *v_max) {
    if (!r) panic("null robot");
    std::vector<double> v((size_t)r->n);
    double alpha = 0.0;
    const int rc = optik_robot_diff_ik_ex(r, x0, V_WE, v_max, nullptr, &alpha, v.data());
    if (rc < 0) panic(g_robot_err);
    if (rc != 0) return nullptr;
    return malloc_copy(v.data(), v.size());
}

int optik_robot_chain_tables_n(const optik_robot *r, int32_t capacity, int32_t *n_joints, double *origins7,
                               double *axes3, int32_t *types) {
    if (!r || !n_joints) return set_err(-1, "null argument");
    *n_joints = (int32_t)r->types.size();
    if ((origins7 || axes3 || types) && capacity < *n_joints)
        return set_err(-1, "chain_tables: buffers too small for the chain's joints");
    if (origins7) std::memcpy(origins7, r->origins.data(), sizeof(double) * r->origins.size());
    if (axes3) std::memcpy(axes3, r->axes.data(), sizeof(double) * r->axes.size());
    if (types) std::memcpy(types, r->types.data(), sizeof(int32_t) * r->types.size());
    return 0;
}

// (the original, in/out contract: with buffers, *n_joints holds their capacity in joints on entry -- a buffer that is
// too small is an error, never an overrun; without buffers it is written only)
int optik_robot_chain_tables(const optik_robot *r, int32_t *n_joints, double *origins7, double *axes3,
                             int32_t *types) {
    if (!r || !n_joints) return set_err(-1, "null argument");
    const int32_t capacity = (origins7 || axes3 || types) ? *n_joints : 0;
    return optik_robot_chain_tables_n(r, capacity, n_joints, origins7, axes3, types);
}

optik_hip_chain *optik_robot_hip_chain(const optik_robot *r) {
    if (!r) return nullptr;
    DeviceCtx *c = device_ctx(r);
    return c ? c->chain : nullptr;
}

}  // extern "C"
