// time_measure.hpp -- velocity- and acceleration-limited timing of joint paths and the sampling of the timed
// trajectory, one source for the host and the device (optik_hip_path_time / _trajectory_sample, optik_hip.h;
// ik_time.hip).
//
// The method is time-optimal path parameterisation by reachability analysis (TOPP-RA, Pham and Pham 2018) in its
// collocation discretisation, with the path's own waypoints as the grid: the path parameter is the waypoint index, so
// the grid step is 1 -- which is why the natural input is optik_hip_path_resample's evenly spaced output.
//
// A path is a polyline of m = len joint-space waypoints q_0 .. q_(m-1), 3 <= m <= L <= 64, joint j of waypoint t at
// path[t * st + j], of a chain with n <= 16 joint positions.  v_j > 0 (may be +inf) and a_j > 0 (finite) are the
// velocity and acceleration limits.  The exact operation order (the tests depend on it; -ffp-contract=off on both
// sides, only the correctly rounded + - * /, fabs, comparisons and the correctly rounded __builtin_sqrt):
//
//  1. Derivatives in the waypoint index (deriv_d, deriv_c): d_i = (q_(i+1) - q_(i-1)) / 2 inside, d_0 = q_1 - q_0,
//     d_(m-1) = q_(m-1) - q_(m-2);  c_i = (q_(i+1) - q_i) - (q_i - q_(i-1)) inside, c = 0 at both ends.
//  2. The unknowns are x_i = (ds/dt)^2 at waypoint i and u_i, constant on [i, i + 1], with x_(i+1) = x_i + 2 u_i; the
//     motion is rest to rest, x_0 = x_(m-1) = 0.  Stage i = 0 .. m-2 asks d_ij^2 x_i <= v_j^2 and
//     |d_ij u_i + c_ij x_i| <= a_j of every joint j.  Written in x' = x_(i+1), a joint with d_ij != 0 is a MEMBER
//     (member):  lo_j(x) <= x' <= hi_j(x),  hi_j(x) = s_j * x + k_j,  lo_j(x) = s_j * x - k_j,
//         s_j = 1 - (2 * c_ij) / d_ij,    k_j = (2 * a_j) / fabs(d_ij).
//     A joint with d_ij == 0 is no member; it is stored with the slope NaN, which no comparison below admits.
//     Two more members close the set: the upper hi(x) = beta_(i+1) and the lower lo(x) = 0, both with slope 0.
//  3. The bounds on x_i alone (cap_term), per joint: r = v_j / fabs(d_ij), r * r for d_ij != 0; a_j / fabs(c_ij) for
//     d_ij == 0 and c_ij != 0; +inf otherwise.  xcap_i is their minimum.
//  4. Every minimum is take_min folded from +inf: a term replaces the running value when `term < value`, so a NaN
//     never enters, no term is -0 (all are quotients or squares of nonnegative numbers), and the result does not
//     depend on the order the terms are visited in -- the lanes of the device split them any way.
//  5. Backward pass: beta_(m-1) = 0; for i = m-2 down to 0, beta_i is the minimum of xcap_i and, over all
//     (n + 1)^2 pairs (upper p, lower q) whose slopes have s_p - s_q < 0, of (hi_p(0) - lo_q(0)) / (s_q - s_p)
//     (pair_term; pair e = p * (n + 1) + q, the index n being the extra member: stage_pair).  That is exact: every
//     gap hi_p - lo_q is linear in x and nonnegative at 0, so the x that admit an x' are the interval [0, beta_i].  No
//     LP solver, no iteration.  A beta_i that is not < +inf means the stage bounds nothing -- every d and c of it is 0:
//     a waypoint repeated three times, or twice at the start -- and the path is refused (BAD_LENGTH's value 2,
//     UNBOUNDED).  Infinite velocity limits alone do not refuse a path: the acceleration members still bound x.
//  6. Forward pass: x_0 = 0; x_(i+1) = max(0, min(beta_(i+1), min over the members of s_j * x_i + k_j)) (hi_value: the
//     product, then the sum; max as `h > 0 ? h : 0`).  The clamp is needed: rounding reaches -1e-17.
//  7. Outputs per waypoint: u_i = (x_(i+1) - x_i) / 2; r_i = sqrt(x_i); qd_ij = d_ij * r_i;
//     qdd_ij = d_ij * u_i + c_ij * x_i (the two products, then the sum), 0 at the last waypoint.  The segment time is
//     2 / (r_i + r_(i+1)) (segment_time) and t_0 = 0, t_(i+1) = t_i + segment_i, added serially in ascending i; the
//     duration is t_(m-1).
//  8. Status, in this order: BAD_LENGTH (2) when len is outside 3 .. min(L, 64); PATH_NAN (3) when one of the m
//     waypoints is not finite (x - x == 0 fails); UNBOUNDED (2) from step 5; STALLED (1) when a segment has
//     r_i + r_(i+1) not > 0 (x_i = x_(i+1) = 0: the profile never leaves waypoint i) or not < +inf, or the duration
//     is not finite; else TIMED (0).  Unless TIMED every time and the duration are NaN.  TIMED and STALLED write x,
//     the velocities and the accelerations of step 7 -- a STALLED profile still satisfies every constraint --, the
//     other statuses write 0 for them.  For TIMED the waypoints behind the path's own, m .. L - 1, hold the duration;
//     their velocity, acceleration and x are 0 whatever the status.
//  9. Sampling (sample_waypoint): cubic Hermite interpolation in time over (t_i, q_i, qd_i) -- what a joint-trajectory
//     controller does with positions and velocities -- at tau = (double)k * dt.  A path that is not TIMED gives its
//     start and velocity 0.  tau >= duration gives the goal and velocity 0.  Otherwise the segment is the LAST
//     i <= m-2 with t_i <= tau, h = t_(i+1) - t_i, r = (tau - t_i) / h; r == 0 copies q_i and qd_i bit for bit; else
//     with w = 1 - r:
//         q = (((1 + 2 r) * (w * w)) * q_i + ((r * (w * w)) * h) * qd_i) + (((r * r) * (3 - 2 r)) * q_(i+1)
//             + (((r * r) * (r - 1)) * h) * qd_(i+1))
//         v = ((((6 r) * (r - 1)) * q_i + ((((3 r) * r - 4 r) + 1) * h) * qd_i) + (((6 r) * w) * q_(i+1)
//             + ((((3 r) * r - 2 r)) * h) * qd_(i+1))) / h
//     exactly as hermite_q / hermite_v write them.
//
// The limit of the method, stated rather than hidden: the greedy forward pass of step 6 is pointwise maximal only
// when every slope s_j >= 0, that is |c| <= |d| / 2: a dense, gently curved path.  There it equals an exact LP
// maximising sum x over the same constraints (HiGHS; to 4e-16 of max x on straight lines and on gently curved 7-joint
// paths of 16 and 64 waypoints, tests/test_time_host.py).  Where a slope is negative a larger x_i forces a SMALLER
// x_(i+1) and the greedy pass runs into it: at a sharp corner the profile stops at the next waypoint (x = 0 there),
// and on a jagged path two such stops can be neighbours, which is STALLED.  Of unbiased random walks (steps uniform
// in +-0.3 rad per joint, any n, 4 or more waypoints) about a third end so, and some of the rest carry an x of 1e-14
// where rounding kept it off 0 and with it a duration of 1e7 s.  The result satisfies every constraint of step 2 in
// every case (the largest excess seen is 1e-14 of the limit), sum x never exceeds the LP's, and it is optimal where
// the path is smooth: resample first, and smooth a path whose corners matter.
//
// Plain host C++ compiles this header too (no HIP runtime): tests/time_util.py drives it with g++, and the serial
// reference of the whole of 1 to 9 at its end (time_reference, sample_reference) is what the tests compare the device
// with.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OPTIK_TM_HD __host__ __device__
#else
#define OPTIK_TM_HD
#endif

#ifndef OPTIK_HIP_PATH_TIME_MAX_WAYPOINTS
#define OPTIK_HIP_PATH_TIME_MAX_WAYPOINTS 64  // (include/optik_hip.h)
#endif

namespace optik {
namespace timing {

constexpr int MIN_POINTS = 3, MAX_POINTS = OPTIK_HIP_PATH_TIME_MAX_WAYPOINTS;
constexpr int MAX_JOINTS = 16;  // joint positions of a chain (ik_wide.hpp: WIDE_MAX_DOF)
constexpr int TIMED = 0, STALLED = 1, BAD_LENGTH = 2, UNBOUNDED = 2, PATH_NAN = 3;

OPTIK_TM_HD inline double inf() { return __builtin_huge_val(); }
OPTIK_TM_HD inline double nan() { return __builtin_nan(""); }
OPTIK_TM_HD inline bool is_finite(double x) { return x - x == 0.0; }
OPTIK_TM_HD inline double tm_sqrt(double x) { return __builtin_sqrt(x); }

// Step 4.
OPTIK_TM_HD inline double take_min(double value, double term) { return term < value ? term : value; }

OPTIK_TM_HD inline bool length_ok(int len, int L) {
    return len >= MIN_POINTS && len <= L && len <= MAX_POINTS;
}

// Step 1: q points at one joint's waypoint 0, waypoint t at q[t * st].
OPTIK_TM_HD inline double deriv_d(const double *q, long long st, int m, int i) {
    if (i == 0) return q[st] - q[0];
    if (i == m - 1) return q[(m - 1) * st] - q[(m - 2) * st];
    return (q[(i + 1) * st] - q[(i - 1) * st]) / 2.0;
}
OPTIK_TM_HD inline double deriv_c(const double *q, long long st, int m, int i) {
    if (i == 0 || i == m - 1) return 0.0;
    return (q[(i + 1) * st] - q[i * st]) - (q[i * st] - q[(i - 1) * st]);
}

// Step 2: one joint's member of a stage.
struct Member {
    double s, k;
};
OPTIK_TM_HD inline Member member(double d, double c, double a) {
    if (d != 0.0) return Member{1.0 - (2.0 * c) / d, (2.0 * a) / fabs(d)};
    return Member{nan(), 0.0};
}

// Step 3: one joint's bound on x alone.
OPTIK_TM_HD inline double cap_term(double d, double c, double v, double a) {
    if (d != 0.0) {
        const double r = v / fabs(d);
        return r * r;
    }
    if (c != 0.0) return a / fabs(c);
    return inf();
}

// Step 5: the pair of the upper member (slope sp, hi(0) = ip) with the lower member (slope sq, lo(0) = iq).
OPTIK_TM_HD inline double pair_term(double sp, double ip, double sq, double iq) {
    if (sp - sq < 0.0) return (ip - iq) / (sq - sp);
    return inf();
}

// Step 5: pair e of a stage whose joint j has the slope s[j * stride] and the offset k[j * stride]; bnext = beta_(i+1).
OPTIK_TM_HD inline double stage_pair(int n, const double *s, const double *k, int stride, double bnext, int e) {
    const int p = e / (n + 1), q = e % (n + 1);
    const double sp = p < n ? s[p * stride] : 0.0, ip = p < n ? k[p * stride] : bnext;
    const double sq = q < n ? s[q * stride] : 0.0, iq = q < n ? -k[q * stride] : 0.0;
    return pair_term(sp, ip, sq, iq);
}

// Step 6.
OPTIK_TM_HD inline double hi_value(double s, double k, double x) { return s * x + k; }
OPTIK_TM_HD inline double clamp_x(double h) { return h > 0.0 ? h : 0.0; }

// Step 7.
OPTIK_TM_HD inline double accel_u(double x0, double x1) { return (x1 - x0) / 2.0; }
OPTIK_TM_HD inline double out_qd(double d, double r) { return d * r; }
OPTIK_TM_HD inline double out_qdd(double d, double u, double c, double x) { return d * u + c * x; }
OPTIK_TM_HD inline double segment_time(double r0, double r1) { return 2.0 / (r0 + r1); }
OPTIK_TM_HD inline bool segment_bad(double r0, double r1) {
    const double s = r0 + r1;
    return !(s > 0.0) || !(s < inf());
}

// Step 9.
OPTIK_TM_HD inline double hermite_q(double r, double h, double q0, double v0, double q1, double v1) {
    const double w = 1.0 - r, ww = w * w, rr = r * r;
    const double h00 = (1.0 + 2.0 * r) * ww, h10 = (r * ww) * h, h01 = rr * (3.0 - 2.0 * r), h11 = (rr * (r - 1.0)) * h;
    return (h00 * q0 + h10 * v0) + (h01 * q1 + h11 * v1);
}
OPTIK_TM_HD inline double hermite_v(double r, double h, double q0, double v0, double q1, double v1) {
    const double w = 1.0 - r;
    const double g00 = (6.0 * r) * (r - 1.0), g10 = (((3.0 * r) * r - 4.0 * r) + 1.0) * h, g01 = (6.0 * r) * w,
                 g11 = ((3.0 * r) * r - 2.0 * r) * h;
    return ((g00 * q0 + g10 * v0) + (g01 * q1 + g11 * v1)) / h;
}

// Step 9, sample k of one path: waypoint t's joint j at path[t * st + j], its time at t[t * tst], its velocity at
// qd[t * st + j]; q_out and v_out take n doubles at stride so.
OPTIK_TM_HD inline void sample_waypoint(int n, const double *path, long long st, int len, int L, const double *t,
                                        long long tst, const double *qd, int status, double dt, long long k,
                                        double *q_out, double *v_out, long long so) {
    if (status != TIMED || !length_ok(len, L)) {
        for (int j = 0; j < n; ++j) {
            q_out[j * so] = path[j];
            v_out[j * so] = 0.0;
        }
        return;
    }
    const int m = len;
    const double tau = (double)k * dt;
    if (tau >= t[(m - 1) * tst]) {
        for (int j = 0; j < n; ++j) {
            q_out[j * so] = path[(m - 1) * st + j];
            v_out[j * so] = 0.0;
        }
        return;
    }
    int lo = 0, hi = m - 2;  // the last i <= m - 2 with t_i <= tau (t_0 = 0 <= tau)
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (t[mid * tst] <= tau) lo = mid;
        else hi = mid - 1;
    }
    const int i = lo;
    const double t0 = t[i * tst], h = t[(i + 1) * tst] - t0, r = (tau - t0) / h;
    for (int j = 0; j < n; ++j) {
        const double q0 = path[i * st + j], v0 = qd[i * st + j];
        if (r == 0.0) {
            q_out[j * so] = q0;
            v_out[j * so] = v0;
        } else {
            const double q1 = path[(i + 1) * st + j], v1 = qd[(i + 1) * st + j];
            q_out[j * so] = hermite_q(r, h, q0, v0, q1, v1);
            v_out[j * so] = hermite_v(r, h, q0, v0, q1, v1);
        }
    }
}

struct Result {
    int status;
    double duration;
};

#if !defined(__HIP_DEVICE_COMPILE__)
// The serial reference of steps 1 to 8 for one path: t [L], qd [L][n], qdd [L][n], x [L] (any may be null).
inline Result time_reference(int n, const double *path, long long st, int len, int L, const double *vmax,
                             const double *amax, double *t, double *qd, double *qdd, double *x) {
    double s[MAX_POINTS][MAX_JOINTS], k[MAX_POINTS][MAX_JOINTS];
    double xcap[MAX_POINTS], beta[MAX_POINTS], xs[MAX_POINTS], r[MAX_POINTS], ts[MAX_POINTS];
    auto fail = [&](int status) {
        for (int i = 0; i < L; ++i) {
            if (t) t[i] = nan();
            if (x) x[i] = 0.0;
            for (int j = 0; j < n; ++j) {
                if (qd) qd[i * n + j] = 0.0;
                if (qdd) qdd[i * n + j] = 0.0;
            }
        }
        return Result{status, nan()};
    };
    if (!length_ok(len, L)) return fail(BAD_LENGTH);
    const int m = len;
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < n; ++j)
            if (!is_finite(path[i * st + j])) return fail(PATH_NAN);
    for (int i = 0; i < m - 1; ++i) {
        xcap[i] = inf();
        for (int j = 0; j < n; ++j) {
            const double d = deriv_d(path + j, st, m, i), c = deriv_c(path + j, st, m, i);
            const Member mb = member(d, c, amax[j]);
            s[i][j] = mb.s;
            k[i][j] = mb.k;
            xcap[i] = take_min(xcap[i], cap_term(d, c, vmax[j], amax[j]));
        }
    }
    beta[m - 1] = 0.0;
    bool unbounded = false;
    for (int i = m - 2; i >= 0; --i) {
        double b = xcap[i];
        for (int e = 0; e < (n + 1) * (n + 1); ++e) b = take_min(b, stage_pair(n, s[i], k[i], 1, beta[i + 1], e));
        beta[i] = b;
        if (!(b < inf())) unbounded = true;
    }
    if (unbounded) return fail(UNBOUNDED);
    xs[0] = 0.0;
    for (int i = 0; i < m - 1; ++i) {
        double h = inf();
        for (int j = 0; j < n; ++j) h = take_min(h, hi_value(s[i][j], k[i][j], xs[i]));
        h = take_min(h, beta[i + 1]);
        xs[i + 1] = clamp_x(h);
    }
    for (int i = 0; i < m; ++i) r[i] = tm_sqrt(xs[i]);
    bool bad = false;
    ts[0] = 0.0;
    for (int i = 0; i < m - 1; ++i) {
        bad = bad || segment_bad(r[i], r[i + 1]);
        ts[i + 1] = ts[i] + segment_time(r[i], r[i + 1]);
    }
    const bool stalled = bad || !is_finite(ts[m - 1]);
    for (int i = 0; i < L; ++i) {
        const bool own = i < m;
        if (t) t[i] = stalled ? nan() : (own ? ts[i] : ts[m - 1]);
        if (x) x[i] = own ? xs[i] : 0.0;
        for (int j = 0; j < n; ++j) {
            double v = 0.0, acc = 0.0;
            if (own) {
                const double d = deriv_d(path + j, st, m, i), c = deriv_c(path + j, st, m, i);
                v = out_qd(d, r[i]);
                if (i < m - 1) acc = out_qdd(d, accel_u(xs[i], xs[i + 1]), c, xs[i]);
            }
            if (qd) qd[i * n + j] = v;
            if (qdd) qdd[i * n + j] = acc;
        }
    }
    if (stalled) return Result{STALLED, nan()};
    return Result{TIMED, ts[m - 1]};
}

// The serial reference of step 9 for one path [L][n] with times t [L], velocities qd [L][n]: q_out, v_out [Tout][n].
inline void sample_reference(int n, const double *path, int len, int L, const double *t, const double *qd, int status,
                             double dt, int Tout, double *q_out, double *v_out) {
    for (int k = 0; k < Tout; ++k)
        sample_waypoint(n, path, n, len, L, t, 1, qd, status, dt, k, q_out + (long long)k * n, v_out + (long long)k * n, 1);
}
#endif

}  // namespace timing
}  // namespace optik
