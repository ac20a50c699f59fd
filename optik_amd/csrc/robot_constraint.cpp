// robot_constraint.cpp -- pose constraints in the host API (include/optik.h): the three row batches of
// ik_constraint.hip, each one stage_rows over the robot's first device (robot_host.hpp: the robot object and the shared
// plumbing; robot_rows.cpp: the other row batches).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "pose_convert.hpp"
#include "robot_host.hpp"

using namespace optik::robot;
using optik::pose::pose7_from_mat16;

namespace {

constexpr int64_t kRowChunk = (int64_t)1 << 18;     // rows per launch
constexpr int64_t kMotionChunk = (int64_t)1 << 16;  // segments per launch (each is many samples)

}  // namespace

extern "C" {

int optik_robot_constraint_batch(const optik_robot *r, int64_t B, const double *x, const double *ref7,
                                 const double *lo6, const double *hi6, const double *ee16, double *residual_out,
                                 double *violation_out) {
    if (!r || !x || !ref7 || !lo6 || !hi6) return set_err(-1, "null argument");
    if (B < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    // (B = 0: the kernel layer's refusals of the constraint and the chain, before anything is staged)
    if (optik_hip_constraint_batch(c->chain, nullptr, ref7, lo6, hi6, nullptr, 0, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (B == 0 || (!residual_out && !violation_out)) return 0;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    // per row: q n doubles in; r 6 | v 1 doubles out
    const RowInput in[] = {{x, (size_t)r->n}};
    return stage_rows(
        c, B, in, 7 * sizeof(double), kRowChunk,
        [&](optik_hip_chain *ch, const double *d_q, int64_t L, double *d_r) {
            return optik_hip_constraint_batch(ch, ee16 ? ee7 : nullptr, ref7, lo6, hi6, d_q, L, d_r, d_r + 6 * L,
                                              nullptr);
        },
        [&](size_t b0, size_t L, const double *h_r) {
            if (residual_out)
                parallel_ranges(L, [&](size_t k0, size_t k1) {
                    for (size_t k = k0; k < k1; ++k)
                        for (size_t i = 0; i < 6; ++i) residual_out[(b0 + k) * 6 + i] = h_r[i * L + k];
                });
            if (violation_out) std::memcpy(violation_out + b0, h_r + 6 * L, sizeof(double) * L);
        });
}

int optik_robot_constraint_project_batch(const optik_robot *r, int64_t B, const double *x, const double *ref7,
                                         const double *lo6, const double *hi6, double tol, int32_t iters,
                                         double damping, double max_step, const double *ee16, double *x_out,
                                         double *violation_out, int32_t *status_out, int32_t *iterations_out) {
    if (!r || !x || !ref7 || !lo6 || !hi6) return set_err(-1, "null argument");
    if (B < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    if (optik_hip_constraint_project_batch(c->chain, nullptr, ref7, lo6, hi6, nullptr, 0, tol, iters, damping,
                                           max_step, nullptr, nullptr, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (B == 0 || (!x_out && !violation_out && !status_out && !iterations_out)) return 0;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    const size_t n = (size_t)r->n;
    // per row: x n doubles in; x n | v 1 doubles, then the status and iteration words in one more double out
    const RowInput in[] = {{x, n}};
    return stage_rows(
        c, B, in, sizeof(double) * (n + 2), kRowChunk,
        [&](optik_hip_chain *ch, const double *d_q, int64_t L, double *d_x) {
            double *d_v = d_x + n * (size_t)L;
            int32_t *d_st = reinterpret_cast<int32_t *>(d_v + L);
            return optik_hip_constraint_project_batch(ch, ee16 ? ee7 : nullptr, ref7, lo6, hi6, d_q, L, tol, iters,
                                                      damping, max_step, d_x, d_v, d_st, d_st + L, nullptr);
        },
        [&](size_t b0, size_t L, const double *h_x) {
            const double *h_v = h_x + n * L;
            const int32_t *h_st = reinterpret_cast<const int32_t *>(h_v + L);
            if (x_out)
                parallel_ranges(L, [&](size_t k0, size_t k1) {
                    for (size_t k = k0; k < k1; ++k)
                        for (size_t i = 0; i < n; ++i) x_out[(b0 + k) * n + i] = h_x[i * L + k];
                });
            if (violation_out) std::memcpy(violation_out + b0, h_v, sizeof(double) * L);
            if (status_out) std::memcpy(status_out + b0, h_st, sizeof(int32_t) * L);
            if (iterations_out) std::memcpy(iterations_out + b0, h_st + L, sizeof(int32_t) * L);
        });
}

int optik_robot_constraint_motion_batch(const optik_robot *r, int64_t B, const double *xa, const double *xb,
                                        double resolution, const double *ref7, const double *lo6, const double *hi6,
                                        double tol, const double *ee16, double *violation_out, uint8_t *ok_out,
                                        int32_t *first_out, int32_t *steps_out) {
    if (!r || !xa || !xb || !ref7 || !lo6 || !hi6) return set_err(-1, "null argument");
    if (B < 0) return set_err(-1, "bad argument");
    DeviceCtx *c = device_ctx(r);
    if (!c) return -1;
    if (optik_hip_constraint_motion_batch(c->chain, nullptr, ref7, lo6, hi6, nullptr, nullptr, 0, resolution, tol,
                                          nullptr, nullptr, nullptr, nullptr, nullptr))
        return set_err(-1, optik_hip_last_error());
    if (B == 0 || (!violation_out && !ok_out && !first_out && !steps_out)) return 0;
    double ee7[7];
    if (ee16) pose7_from_mat16(ee16, ee7);
    const size_t n = (size_t)r->n;
    // per segment: qa and qb (2 n doubles) in; the violation, then first and steps in a second double and the ok flag
    // in the bytes of a third out
    const RowInput in[] = {{xa, n}, {xb, n}};
    return stage_rows(
        c, B, in, 3 * sizeof(double), kMotionChunk,
        [&](optik_hip_chain *ch, const double *d_q, int64_t L, double *d_out) {
            int32_t *d_first = reinterpret_cast<int32_t *>(d_out + L);
            return optik_hip_constraint_motion_batch(ch, ee16 ? ee7 : nullptr, ref7, lo6, hi6, d_q, d_q + n * (size_t)L,
                                                     L, resolution, tol, d_out,
                                                     reinterpret_cast<uint8_t *>(d_out + 2 * L), d_first, d_first + L,
                                                     nullptr);
        },
        [&](size_t b0, size_t L, const double *h_out) {
            const int32_t *h_first = reinterpret_cast<const int32_t *>(h_out + L);
            if (violation_out) std::memcpy(violation_out + b0, h_out, sizeof(double) * L);
            if (first_out) std::memcpy(first_out + b0, h_first, sizeof(int32_t) * L);
            if (steps_out) std::memcpy(steps_out + b0, h_first + L, sizeof(int32_t) * L);
            if (ok_out) std::memcpy(ok_out + b0, reinterpret_cast<const uint8_t *>(h_out + 2 * L), L);
        });
}

}  // extern "C"
