// motion_measure.hpp -- the motion check between two configurations, one source for the host and the device
// (optik_hip_collision_motion_batch and the motion key pass of optik_hip_ik_path, optik_hip.h).
// The distances and the clearance of a configuration are collision_measure.hpp's, unchanged.
//
// A motion is the straight joint-space segment qa -> qb of a chain with n joint positions, sampled at a resolution
// h > 0 (L-infinity, radians).  The exact operation order (the tests depend on it; -ffp-contract=off on both sides,
// only the correctly rounded - * / +, fabs, ceil and comparisons):
//
//  1. d = max_i fabs(qb_i - qa_i), i ascending from d = 0, a NaN term taken and then kept: d is NaN as soon as one
//     joint of qa or qb is (motion_distance).
//  2. r = ceil(d / h).  The motion is NOT SAMPLED when r <= 4096.0 is false: d NaN or infinite, or more than
//     OPTIK_HIP_MAX_MOTION_STEPS steps.  Its outputs are clearance NaN, free 0, first -1, steps -1.
//     Otherwise K = max(1, (int)r) (qa == qb gives K = 1) and steps = K (motion_steps).
//  3. There are K + 1 samples k = 0 .. K.  Sample 0 is qa and sample K is qb, copied.  For 0 < k < K:
//     t = (double)k / (double)K and q_k,i = qa_i + t * (qb_i - qa_i): the difference, the product, then the sum
//     (motion_sample).
//  4. The motion clearance is the minimum over k of the clearance of q_k (collision_measure.hpp step 4: the same
//     frames, model, world and ee_offset), NaN if any sample's clearance is NaN.  The motion is free iff every sample
//     is free (clearance >= margin; a NaN sample is not free).  `first` is the lowest k whose sample is not free, -1
//     for a free motion.  Without a model every sample's clearance is +inf (NaN for a NaN sample), as
//     optik_hip_collision_batch defines it.
//
// The minimum of the clearances and the minimum of the non-free k are exact in any order, so the result does not
// depend on how the samples are spread over lanes, on the grouping, or on whether a pass that only classifies has
// skipped samples above a non-free one it already knows.
//
// Plain host C++ compiles this header too (no HIP runtime): tests/test_motion_host.py drives it with g++.
#pragma once

#include "collision_measure.hpp"

#ifndef OPTIK_HIP_MAX_MOTION_STEPS
#define OPTIK_HIP_MAX_MOTION_STEPS 4096  // (include/optik_hip.h)
#endif

namespace optik {
namespace motion {

constexpr int MAX_STEPS = OPTIK_HIP_MAX_MOTION_STEPS;

// Step 1, one term: the running maximum d with the term e.
OPTIK_CM_HD inline double distance_take(double d, double e) { return (e > d || e != e) ? e : d; }

// Step 1: qa_i = qa[i * sa], qb_i = qb[i * sb].
OPTIK_CM_HD inline double motion_distance(int n, const double *qa, long long sa, const double *qb, long long sb) {
    double d = 0.0;
    for (int i = 0; i < n; ++i) d = distance_take(d, fabs(qb[i * sb] - qa[i * sa]));
    return d;
}

// Step 2: K, or -1 for a motion that is not sampled.
OPTIK_CM_HD inline int motion_steps(double d, double h) {
    const double r = ceil(d / h);
    if (!(r <= (double)MAX_STEPS)) return -1;
    return r < 1.0 ? 1 : (int)r;
}

// Step 3, one joint of sample k of K.
OPTIK_CM_HD inline double motion_sample(double qa, double qb, int k, int K) {
    if (k == 0) return qa;
    if (k == K) return qb;
    const double t = (double)k / (double)K;
    return qa + t * (qb - qa);
}

struct Result {
    double clearance;
    int free_flag, first, steps;
};

OPTIK_CM_HD inline Result not_sampled() {
#if defined(__HIP_DEVICE_COMPILE__)
    return Result{__builtin_nan(""), 0, -1, -1};
#else
    return Result{NAN, 0, -1, -1};
#endif
}

// Step 4, the reference form (the tests' g++ driver): clearance_of(k) is the clearance of sample k.
template <class ClearanceFn>
inline Result motion_reduce(int K, double margin, ClearanceFn &&clearance_of) {
    if (K < 0) return not_sampled();
    Result r{INFINITY, 1, -1, K};
    bool nan = false;
    for (int k = 0; k <= K; ++k) {
        const double c = clearance_of(k);
        if (c != c) nan = true;
        else r.clearance = fmin(r.clearance, c);
        if (!(c >= margin) && r.first < 0) r.first = k;
    }
    if (nan) r.clearance = NAN;
    r.free_flag = r.first < 0 ? 1 : 0;
    return r;
}

}  // namespace motion
}  // namespace optik
