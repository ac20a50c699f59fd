// time_spline_measure.hpp -- spline retiming of timed joint paths: the C2 cubic spline through the timed waypoints,
// slowed uniformly until velocity, acceleration and jerk limits hold along the whole curve; one source for the host
// and the device (optik_hip_path_time_spline, optik_hip.h; ik_time.hip).
//
// The input is what time_measure.hpp produces: a path of m = len joint-space waypoints q_0 .. q_(m-1), 3 <= m <= L <=
// 64, of a chain with n <= 16 joint positions, and its times t_0 = 0 < t_1 < .. < t_(m-1).  The output keeps the
// waypoints and gives them new times, velocities and accelerations: the knot values of the clamped (rest to rest) C2
// cubic spline through (t'_i, q_i) with t' = k t.  A C2 cubic spline is the cubic Hermite curve of its own knot
// velocities, so (t', q, v) goes into time_measure.hpp's sample_waypoint as it is.  v_j > 0, a_j > 0, jk_j > 0 are the
// limits of joint j, each may be +inf.  The exact operation order (the tests depend on it; -ffp-contract=off on both
// sides, only the correctly rounded + - * /, fabs, comparisons and the correctly rounded __builtin_sqrt):
//
//  1. Knot velocities (inv_spacing, chord, sweep_row, back_row).  g_i = 1 / (t_(i+1) - t_i) and delta_ij =
//     (q_(i+1)j - q_ij) * g_i for the segments i = 0 .. m-2.  Per joint v_0 = v_(m-1) = 0 and row i = 1 .. m-2 of
//         g_(i-1) v_(i-1) + 2 (g_(i-1) + g_i) v_i + g_i v_(i+1) = 3 (delta_(i-1) g_(i-1) + delta_i g_i)
//     is solved by the Thomas recurrence, which needs no pivoting because the system is strictly diagonally dominant.
//     Forward, ascending i from e_0 = d_0 = 0:  b = 2 * (g_(i-1) + g_i);  r = 3 * (delta_(i-1) * g_(i-1) + delta_i *
//     g_i);  w = b - g_(i-1) * e_(i-1);  e_i = g_i / w;  d_i = (r - g_(i-1) * d_(i-1)) / w.  Backward, descending i from
//     v_(m-1) = 0:  v_i = d_i - e_i * v_(i+1).  m = 3 is the one row i = 1.
//  2. Per segment (segment):  A0 = ((6 * delta - 4 * v_i) - 2 * v_(i+1)) * g_i,  A1 = ((2 * v_i - 6 * delta) + 4 *
//     v_(i+1)) * g_i, the accelerations at its two ends, and the jerk J = (A1 - A0) * g_i, constant on it.  The
//     acceleration returned at knot i is A0_i, at the last knot A1_(m-2).
//  3. Peaks over the whole curve, as ratios to the limits (fold_segment).  Of segment i and joint j: the velocity peak
//     is |v_i|, and where A0 * A1 < 0 the larger of it and |v_i - (A0 * A0) / (2 * J)|, the interior extremum (the last
//     knot's velocity is 0); the acceleration peak is the larger of |A0| and |A1| (the acceleration is linear on the
//     segment); the jerk peak is |J|.  Each is divided by the joint's limit -- a quotient is 0 for an infinite limit --
//     and F_v, F_a, F_j are the maxima of the quotients over all segments and joints.  Every maximum is take_max
//     folded from 0: a term replaces the running value when `term > value`, so a NaN never enters and the result does
//     not depend on the order the terms are visited in -- the lanes of the device split them any way.  Dividing a
//     segment's peak is the same as dividing the joint's peak over all segments: rounding is monotone.  A v, A0, A1, J
//     or velocity peak that is not finite (x - x == 0 fails) is remembered in `ok`, which is order-free too.
//  4. The factor (cube_root_up, factor): k = the largest of 1, F_v, sqrt(F_a) and c, folded with take_max from 1,
//     where c = 0 unless F_j > 1 and else a cube root of F_j by this sequence: s_1 = sqrt(sqrt(F_j)), s_2 =
//     sqrt(sqrt(s_1)), s_3 = sqrt(sqrt(s_2)), s_4 = sqrt(sqrt(s_3)); c = ((s_1 * s_2) * s_3) * s_4 (the exponents 1/4 +
//     1/16 + 1/64 + 1/256 miss 1/3 by 1/768: c is within a factor 2.5 of the root for every finite F_j); then
//     NEWTON_STEPS = 8 times c = (2 * c + F_j / (c * c)) / 3; then NUDGES = 4 times: if c * c * c < F_j, c = c + c *
//     2^-52.  If k > 1 it is multiplied by 1 + 2^-40, which leaves 3e-12 of headroom on the jerk ratio (2e-12 on the
//     acceleration's, 1e-12 on the velocity's).  What that headroom stands against is not the rounding of the second
//     solve (about 1e-14) but that of the products k * t_i of step 5: half an ulp on a knot time moves a spacing of
//     1/100 of the duration by 1e-14 of itself, and the jerk, a third difference over that spacing, by up to 1e-12.
//     At 64 waypoints the final jerk ratio scatters by a few 1e-12, so OVER_LIMIT (step 6) is reachable on ordinary
//     inputs when the jerk binds (seen: 1 + 3e-12); the acceleration's ratio scatters by 1e-13 and the velocity's
//     less.  k = 1 leaves the times untouched bit for bit.  k is +inf when a measure was not `ok` or F_j is not
//     finite.
//  5. Finish: t'_i = k * t_i, one product each; steps 1 to 3 again on t' (nothing changes when k = 1, and the device
//     does not repeat them then).  Outputs: t', v, the accelerations of step 2, the duration t'_(m-1), k and the
//     three final ratios F_v, F_a, F_j.
//  6. Status, in this order: BAD_LENGTH (2) when len is outside 3 .. min(L, 64); NOT_FINITE (3) when one of the m
//     waypoints is not finite, or -- the input being timed -- one of the m times; BAD_TIMES (1) when the input is not
//     timed (the times of such a path are NaN as time_measure.hpp writes them and are not read: the status is passed
//     on as 1), when t_0 == 0 or t_(i+1) > t_i fails for a segment, when k is not finite or the final measure is not
//     `ok`; OVER_LIMIT (4) when a final ratio is still > 1; else SMOOTH (0).  An input is timed (input_timed) when its
//     status is 0 or OVER_LIMIT: an OVER_LIMIT result carries valid times, and a second pass over it is how a caller
//     clears it -- the ratio of 1 + 3e-12 gives a k of 1 + 2e-12.  For 1, 2 and 3 every time and the duration are NaN
//     and the velocities, the accelerations, k and the ratios are 0.  For 0 and 4 the waypoints behind the path's
//     own, m .. L - 1, hold the duration, velocity 0 and acceleration 0.
//
// What the result is not: the clamped spline starts and stops with a finite acceleration step, as every trapezoid
// does, so the jerk is bounded on the open interval only; the slow-down is uniform, the one exact choice (scaling the
// times by k scales v by 1/k, a by 1/k^2 and the jerk by 1/k^3; stretching single segments makes uneven knot spacing,
// which creates jerk by itself: DESIGN.md section 5.36).
//
// Plain host C++ compiles this header too (no HIP runtime): tests/time_spline_util.py drives it with g++, and the
// serial reference of the whole of 1 to 6 at its end (spline_reference) is what the tests compare the device with.
#pragma once

#include "time_measure.hpp"

namespace optik {
namespace splinetime {

constexpr int SMOOTH = 0, BAD_TIMES = 1, BAD_LENGTH = 2, NOT_FINITE = 3, OVER_LIMIT = 4;
constexpr int NEWTON_STEPS = 8, NUDGES = 4;

// Step 3.
OPTIK_TM_HD inline double take_max(double value, double term) { return term > value ? term : value; }

// Step 1.
OPTIK_TM_HD inline double inv_spacing(double t0, double t1) { return 1.0 / (t1 - t0); }
OPTIK_TM_HD inline double chord(double q0, double q1, double g) { return (q1 - q0) * g; }

struct Sweep {
    double e, d;
};
// Row i: gm = g_(i-1), gi = g_i, dm = delta_(i-1), di = delta_i, (ep, dp) = (e, d) of row i - 1.
OPTIK_TM_HD inline Sweep sweep_row(double gm, double gi, double dm, double di, double ep, double dp) {
    const double b = 2.0 * (gm + gi);
    const double r = 3.0 * (dm * gm + di * gi);
    const double w = b - gm * ep;
    return Sweep{gi / w, (r - gm * dp) / w};
}
OPTIK_TM_HD inline double back_row(double e, double d, double vnext) { return d - e * vnext; }

// Step 2.
struct Segment {
    double a0, a1, j;
};
OPTIK_TM_HD inline Segment segment(double delta, double v0, double v1, double g) {
    const double a0 = ((6.0 * delta - 4.0 * v0) - 2.0 * v1) * g;
    const double a1 = ((2.0 * v0 - 6.0 * delta) + 4.0 * v1) * g;
    return Segment{a0, a1, (a1 - a0) * g};
}

// Step 3: the ratios so far.
struct Peaks {
    double v, a, j;
    bool ok;
};
OPTIK_TM_HD inline Peaks no_peaks() { return Peaks{0.0, 0.0, 0.0, true}; }
OPTIK_TM_HD inline void fold_segment(Peaks &pk, const Segment &s, double v0, double vlim, double alim, double jlim) {
    double pv = fabs(v0);
    if (s.a0 * s.a1 < 0.0) pv = take_max(pv, fabs(v0 - (s.a0 * s.a0) / (2.0 * s.j)));
    const double pa = take_max(fabs(s.a0), fabs(s.a1));
    pk.v = take_max(pk.v, pv / vlim);
    pk.a = take_max(pk.a, pa / alim);
    pk.j = take_max(pk.j, fabs(s.j) / jlim);
    pk.ok = pk.ok && timing::is_finite(v0) && timing::is_finite(pv) && timing::is_finite(s.a0)
            && timing::is_finite(s.a1) && timing::is_finite(s.j);
}
OPTIK_TM_HD inline bool over_limit(const Peaks &pk) { return pk.v > 1.0 || pk.a > 1.0 || pk.j > 1.0; }

// Step 4.
OPTIK_TM_HD inline double cube_root_up(double f) {
    if (!(f > 1.0)) return 0.0;
    if (!(f < timing::inf())) return timing::inf();
    const double s1 = timing::tm_sqrt(timing::tm_sqrt(f)), s2 = timing::tm_sqrt(timing::tm_sqrt(s1)),
                 s3 = timing::tm_sqrt(timing::tm_sqrt(s2)), s4 = timing::tm_sqrt(timing::tm_sqrt(s3));
    double c = ((s1 * s2) * s3) * s4;
    for (int it = 0; it < NEWTON_STEPS; ++it) c = (2.0 * c + f / (c * c)) / 3.0;
    for (int it = 0; it < NUDGES; ++it)
        if (c * c * c < f) c = c + c * 0x1p-52;
    return c;
}
OPTIK_TM_HD inline double factor(const Peaks &pk) {
    if (!pk.ok) return timing::inf();
    double k = 1.0;
    k = take_max(k, pk.v);
    k = take_max(k, timing::tm_sqrt(pk.a));
    k = take_max(k, cube_root_up(pk.j));
    if (k > 1.0) k = k * (1.0 + 0x1p-40);
    return k;
}

// Step 6: whether an input status says that the path has times.
OPTIK_TM_HD inline bool input_timed(int status_in) { return status_in == SMOOTH || status_in == OVER_LIMIT; }

// Step 6: segment i's part of the test of the times (i = 0 also looks at t_0).
OPTIK_TM_HD inline bool times_step_ok(int i, double t0, double t1) { return t1 > t0 && (i != 0 || t0 == 0.0); }

struct Result {
    int status;
    double duration, factor, ratios[3];
};

#if !defined(__HIP_DEVICE_COMPILE__)
// Steps 1 to 3 for one path with the times ts [m]: v, acc [m][MAX_JOINTS].
inline Peaks measure_reference(int n, const double *path, long long st, int m, const double *ts, const double *vmax,
                               const double *amax, const double *jmax, double (*v)[timing::MAX_JOINTS],
                               double (*acc)[timing::MAX_JOINTS]) {
    double g[timing::MAX_POINTS], e[timing::MAX_POINTS], d[timing::MAX_POINTS];
    for (int i = 0; i < m - 1; ++i) g[i] = inv_spacing(ts[i], ts[i + 1]);
    Peaks pk = no_peaks();
    for (int j = 0; j < n; ++j) {
        const double *q = path + j;
        e[0] = d[0] = 0.0;
        for (int i = 1; i < m - 1; ++i) {
            const Sweep s = sweep_row(g[i - 1], g[i], chord(q[(i - 1) * st], q[i * st], g[i - 1]),
                                      chord(q[i * st], q[(i + 1) * st], g[i]), e[i - 1], d[i - 1]);
            e[i] = s.e;
            d[i] = s.d;
        }
        v[m - 1][j] = v[0][j] = 0.0;
        for (int i = m - 2; i >= 1; --i) v[i][j] = back_row(e[i], d[i], v[i + 1][j]);
        for (int i = 0; i < m - 1; ++i) {
            const Segment s = segment(chord(q[i * st], q[(i + 1) * st], g[i]), v[i][j], v[i + 1][j], g[i]);
            fold_segment(pk, s, v[i][j], vmax[j], amax[j], jmax[j]);
            acc[i][j] = s.a0;
            if (i == m - 2) acc[m - 1][j] = s.a1;
        }
    }
    return pk;
}

// The serial reference of steps 1 to 6 for one path: t_in [L] and status_in as time_reference wrote them; t [L], qd
// [L][n], qdd [L][n] (any may be null).
inline Result spline_reference(int n, const double *path, long long st, int len, int L, const double *t_in,
                               int status_in, const double *vmax, const double *amax, const double *jmax, double *t,
                               double *qd, double *qdd) {
    double ts[timing::MAX_POINTS], v[timing::MAX_POINTS][timing::MAX_JOINTS], acc[timing::MAX_POINTS][timing::MAX_JOINTS];
    auto fail = [&](int status) {
        for (int i = 0; i < L; ++i) {
            if (t) t[i] = timing::nan();
            for (int j = 0; j < n; ++j) {
                if (qd) qd[i * n + j] = 0.0;
                if (qdd) qdd[i * n + j] = 0.0;
            }
        }
        return Result{status, timing::nan(), 0.0, {0.0, 0.0, 0.0}};
    };
    if (!timing::length_ok(len, L)) return fail(BAD_LENGTH);
    const int m = len;
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < n; ++j)
            if (!timing::is_finite(path[i * st + j])) return fail(NOT_FINITE);
    if (input_timed(status_in))
        for (int i = 0; i < m; ++i)
            if (!timing::is_finite(t_in[i])) return fail(NOT_FINITE);
    if (!input_timed(status_in)) return fail(BAD_TIMES);
    for (int i = 0; i < m - 1; ++i)
        if (!times_step_ok(i, t_in[i], t_in[i + 1])) return fail(BAD_TIMES);
    for (int i = 0; i < m; ++i) ts[i] = t_in[i];
    Peaks pk = measure_reference(n, path, st, m, ts, vmax, amax, jmax, v, acc);
    const double k = factor(pk);
    if (!timing::is_finite(k)) return fail(BAD_TIMES);
    for (int i = 0; i < m; ++i) ts[i] = k * ts[i];
    pk = measure_reference(n, path, st, m, ts, vmax, amax, jmax, v, acc);
    if (!pk.ok) return fail(BAD_TIMES);
    for (int i = 0; i < L; ++i) {
        const bool own = i < m;
        if (t) t[i] = own ? ts[i] : ts[m - 1];
        for (int j = 0; j < n; ++j) {
            if (qd) qd[i * n + j] = own ? v[i][j] : 0.0;
            if (qdd) qdd[i * n + j] = own ? acc[i][j] : 0.0;
        }
    }
    return Result{over_limit(pk) ? OVER_LIMIT : SMOOTH, ts[m - 1], k, {pk.v, pk.a, pk.j}};
}
#endif

}  // namespace splinetime
}  // namespace optik
