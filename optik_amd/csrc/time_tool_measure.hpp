// time_tool_measure.hpp -- path timing with limits on the tool as well as on the joints: the speed, the tangential and
// the normal acceleration and the angular speed of the end effector; one source for the host and the device
// (optik_hip_path_time_tool, optik_hip.h; ik_time.hip).
//
// It is time_measure.hpp's method with one more member and three more cap terms per stage; nothing of that header
// changes, and every step below that is not restated is that header's.  The tool limits are lim[4] = (v_tool, a_t, a_n,
// w_tool): the tool centre point's speed (m/s), its tangential and its normal acceleration (m/s^2) and the end
// effector's angular speed (rad/s); each is > 0, and +inf means the limit is absent.  The exact operation order (the
// tests depend on it; -ffp-contract=off on both sides; only the correctly rounded + - * /, fabs, comparisons, the
// correctly rounded __builtin_sqrt, and the functions of ik_math.hpp, which are used as they are):
//
//  T1. Tool pose (fk_ee): ee_i, the end effector's pose at waypoint i, is constraint::fk's sequence
//      (constraint_measure.hpp step 1) with the trailing fixed joint and the optional ee_offset, without the store of
//      the joint frames: the same operations on the same operands, hence constraint::fk's result bit for bit.
//      p_i = ee_i.t.
//  T2. Tool derivatives in the waypoint index (stage_terms): D_i and C_i are timing::deriv_d and timing::deriv_c of
//      each component of p, with the joints' end rules.  g_i = sqrt((D.x^2 + D.y^2) + D.z^2).
//      g_i != 0:  T = D / g_i (per component), ct = (C.x T.x + C.y T.y) + C.z T.z, N = C - ct T (per component: the
//                 product, then the difference), cn = sqrt((N.x^2 + N.y^2) + N.z^2).
//      g_i == 0:  no tangent: ct = 0, N = C, cn = sqrt((C.x^2 + C.y^2) + C.z^2).
//      The rotation: with (a, b) the index pair deriv_d differences -- (0, 1) at i = 0, (m-2, m-1) at i = m-1,
//      (i-1, i+1) inside --, wv = so3_log(qmul(qconj(ee_a.q), ee_b.q)), each component divided by 2 inside (not at the
//      ends), and w_i = sqrt((wv.x^2 + wv.y^2) + wv.z^2).  Two quaternions equal component by component give wv = 0
//      without the product, whose rounding would leave 1e-17: a repeated waypoint has g_i = cn = w_i = 0 exactly, so
//      a stage the joints do not bound is not bounded by the tool either and keeps time_measure.hpp's status.
//  T3. Tool member (tool_member): g_i != 0 and a_t < +inf make the tangential row |g_i u_i + ct x_i| <= a_t the member
//      timing::member(g_i, ct, a_t).  Otherwise the slope NaN is stored, which no comparison admits -- as a joint with
//      d = 0 is stored today.  It is member n of the stage; the closing member moves to the index n + 1, and the
//      backward pass takes its minimum over the (n + 2)^2 pairs of timing::stage_pair(n + 1, ..): pair e =
//      p * (n + 2) + q.
//  T4. Tool caps on x_i alone (tool_cap), folded by take_min from +inf and then into xcap_i by take_min:
//      r = v_tool / g_i, r * r when g_i != 0;   a_n / cn when cn != 0 (the centripetal part: it does not depend on u,
//      so it is a cap and not a member);   r = w_tool / w_i, r * r when w_i != 0.  A limit of +inf gives +inf.
//  T5. Backward and forward pass, the times and the status: time_measure.hpp steps 5 - 8 with the n + 1 stored
//      members.  The status rules are unchanged: a stage whose joints do not move does not move the tool either.
//  T6. Outputs per waypoint, beside time_measure.hpp's: tool_speed = g_i * r_i;  tool_accel = (g_i * u_i + ct * x_i as
//      timing::out_qdd forms it, cn * x_i), the first component 0 at the last waypoint;  tool_wspeed = w_i * r_i.  All
//      are 0 wherever time_measure.hpp step 8 writes 0 for the velocities.
//
// Identity: with all four limits +inf the tool member is the NaN slope and every tool cap is +inf, so no take_min takes
// either, and every output shared with timing::time_reference has its bits (the folds are order-independent).
//
// What is guaranteed, at the waypoints and in this discretisation: the tool's speed g_i sqrt(x_i) <= v_tool, its
// tangential acceleration |g_i u_i + ct x_i| <= a_t, its normal acceleration cn x_i <= a_n, and the angular speed
// w_i sqrt(x_i) <= w_tool (up to the roundings of the rows: 1e-12 of the limit where the tests recompute them); hence
// |a_tool| <= sqrt(a_t^2 + a_n^2).
// What is NOT bounded: the angular acceleration; anything between the waypoints (the tool follows the joint-space
// polyline's image, and a coarse grid under-reads a curved tool path: resample first); and, as for the joints, the
// greedy forward pass is pointwise maximal only where every slope is >= 0 -- the tool row's, 1 - 2 ct / g, included.
// Where ct > g / 2 (the tool's path derivative grows by more than half of itself in one step) that slope is negative;
// the profile is still feasible and may be longer than the optimum, exactly as time_measure.hpp states for a joint.
//
// Plain host C++ compiles this header under OPTIK_LANE_EMU, as ik_math.hpp needs it (tests/time_tool_util.py); the
// serial reference of the whole at its end (time_tool_reference) is what the tests compare the device with.
#pragma once

#include "constraint_measure.hpp"
#include "time_measure.hpp"

namespace optik {
namespace tooltime {

using timing::Member;
using timing::Result;

enum { V_TOOL = 0, A_TANGENTIAL = 1, A_NORMAL = 2, W_TOOL = 3, LIMITS = 4 };
constexpr int POSE_ROWS = 7;  // t.x t.y t.z q.i q.j q.k q.w

// Step T1: joint j of the waypoint at q[j * st].
template <class CH>
__device__ inline Pose fk_ee(const CH &ch, const EvalParams &ep, int n, const double *q, long long st) {
    Pose state;
    state.t = V3{0.0, 0.0, 0.0};
    state.q = Q4{0.0, 0.0, 0.0, 1.0};
#pragma unroll 1
    for (int j = 0; j < n; ++j) {
        double s, c;
        sincos_dev(q[j * st] / 2.0, s, c);
        const Q4 local{ch.axis[j][0] * s, ch.axis[j][1] * s, ch.axis[j][2] * s, c};
        Pose jt;
        jt.t = V3{ch.origin[j][0], ch.origin[j][1], ch.origin[j][2]};
        jt.q = qmul(Q4{ch.origin[j][3], ch.origin[j][4], ch.origin[j][5], ch.origin[j][6]}, local);
        state = (j == 0) ? jt : pose_mul(state, jt);
    }
    if (ch.has_tip) state = pose_mul(state, load_pose(ch.origin[n]));
    return ep.has_ee_offset ? pose_mul(state, load_pose(ep.ee_offset)) : state;
}

// Row r of waypoint t's pose at ee[r * rs + t * ts].
__device__ inline void store_ee(double *ee, long long rs, long long ts, int t, const Pose &p) {
    double *o = ee + t * ts;
    o[0] = p.t.x; o[rs] = p.t.y; o[2 * rs] = p.t.z;
    o[3 * rs] = p.q.i; o[4 * rs] = p.q.j; o[5 * rs] = p.q.k; o[6 * rs] = p.q.w;
}
__device__ inline Q4 load_q(const double *ee, long long rs, long long ts, int t) {
    const double *o = ee + t * ts;
    return Q4{o[3 * rs], o[4 * rs], o[5 * rs], o[6 * rs]};
}

// Step T2.
struct Stage {
    double g, ct, cn, w;
};
__device__ inline Stage stage_terms(const double *ee, long long rs, long long ts, int m, int i) {
    const double Dx = timing::deriv_d(ee, ts, m, i), Dy = timing::deriv_d(ee + rs, ts, m, i),
                 Dz = timing::deriv_d(ee + 2 * rs, ts, m, i);
    const double Cx = timing::deriv_c(ee, ts, m, i), Cy = timing::deriv_c(ee + rs, ts, m, i),
                 Cz = timing::deriv_c(ee + 2 * rs, ts, m, i);
    Stage o;
    o.g = timing::tm_sqrt((Dx * Dx + Dy * Dy) + Dz * Dz);
    o.ct = 0.0;
    double Nx = Cx, Ny = Cy, Nz = Cz;
    if (o.g != 0.0) {
        const double Tx = Dx / o.g, Ty = Dy / o.g, Tz = Dz / o.g;
        o.ct = (Cx * Tx + Cy * Ty) + Cz * Tz;
        Nx = Cx - o.ct * Tx;
        Ny = Cy - o.ct * Ty;
        Nz = Cz - o.ct * Tz;
    }
    o.cn = timing::tm_sqrt((Nx * Nx + Ny * Ny) + Nz * Nz);
    const bool end = i == 0 || i == m - 1;
    const int a = i == 0 ? 0 : (i == m - 1 ? m - 2 : i - 1), b = i == 0 ? 1 : (i == m - 1 ? m - 1 : i + 1);
    const Q4 qa = load_q(ee, rs, ts, a), qb = load_q(ee, rs, ts, b);
    V3 wv{0.0, 0.0, 0.0};
    if (qa.i != qb.i || qa.j != qb.j || qa.k != qb.k || qa.w != qb.w) wv = so3_log(qmul(qconj(qa), qb));
    if (!end) {
        wv.x = wv.x / 2.0;
        wv.y = wv.y / 2.0;
        wv.z = wv.z / 2.0;
    }
    o.w = timing::tm_sqrt((wv.x * wv.x + wv.y * wv.y) + wv.z * wv.z);
    return o;
}

// Step T3.
__device__ inline Member tool_member(const Stage &t, const double *lim) {
    if (t.g != 0.0 && lim[A_TANGENTIAL] < timing::inf()) return timing::member(t.g, t.ct, lim[A_TANGENTIAL]);
    return Member{timing::nan(), 0.0};
}

// Step T4.
__device__ inline double tool_cap(const Stage &t, const double *lim) {
    double cap = timing::inf();
    if (t.g != 0.0) {
        const double r = lim[V_TOOL] / t.g;
        cap = timing::take_min(cap, r * r);
    }
    if (t.cn != 0.0) cap = timing::take_min(cap, lim[A_NORMAL] / t.cn);
    if (t.w != 0.0) {
        const double r = lim[W_TOOL] / t.w;
        cap = timing::take_min(cap, r * r);
    }
    return cap;
}

// Step T6.
__device__ inline double out_speed(const Stage &t, double r) { return t.g * r; }
__device__ inline double out_tangential(const Stage &t, double u, double x) { return timing::out_qdd(t.g, u, t.ct, x); }
__device__ inline double out_normal(const Stage &t, double x) { return t.cn * x; }
__device__ inline double out_wspeed(const Stage &t, double r) { return t.w * r; }

// A tool limit the entries accept: > 0, +inf allowed, no NaN.
inline bool limit_ok(double v) { return v > 0.0; }

#if !defined(__HIP_DEVICE_COMPILE__)
// The serial reference for one path (waypoint t's joint j at path[t * st + j]): time_measure.hpp's outputs t [L],
// qd [L][n], qdd [L][n], x [L], and tool_speed [L], tool_accel [L][2], tool_wspeed [L] (any may be null).
template <class CH>
__device__ inline Result time_tool_reference(const CH &ch, const EvalParams &ep, int n, const double *path,
                                             long long st, int len, int L, const double *vmax, const double *amax,
                                             const double *lim, double *t, double *qd, double *qdd, double *x,
                                             double *tool_speed, double *tool_accel, double *tool_wspeed) {
    using namespace timing;
    constexpr int MM = timing::MAX_JOINTS + 1;  // the joints' members and the tool's
    double s[MAX_POINTS][MM], k[MAX_POINTS][MM], ee[MAX_POINTS][POSE_ROWS];
    double xcap[MAX_POINTS], beta[MAX_POINTS], xs[MAX_POINTS], r[MAX_POINTS], ts[MAX_POINTS];
    Stage tool[MAX_POINTS];
    auto fail = [&](int status) {
        for (int i = 0; i < L; ++i) {
            if (t) t[i] = nan();
            if (x) x[i] = 0.0;
            if (tool_speed) tool_speed[i] = 0.0;
            if (tool_wspeed) tool_wspeed[i] = 0.0;
            if (tool_accel) tool_accel[2 * i] = tool_accel[2 * i + 1] = 0.0;
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
    for (int i = 0; i < m; ++i) store_ee(&ee[0][0], 1, POSE_ROWS, i, fk_ee(ch, ep, n, path + i * st, 1));
    for (int i = 0; i < m; ++i) tool[i] = stage_terms(&ee[0][0], 1, POSE_ROWS, m, i);
    for (int i = 0; i < m - 1; ++i) {
        xcap[i] = inf();
        for (int j = 0; j < n; ++j) {
            const double d = deriv_d(path + j, st, m, i), c = deriv_c(path + j, st, m, i);
            const Member mb = member(d, c, amax[j]);
            s[i][j] = mb.s;
            k[i][j] = mb.k;
            xcap[i] = take_min(xcap[i], cap_term(d, c, vmax[j], amax[j]));
        }
        const Member mb = tool_member(tool[i], lim);
        s[i][n] = mb.s;
        k[i][n] = mb.k;
        xcap[i] = take_min(xcap[i], tool_cap(tool[i], lim));
    }
    beta[m - 1] = 0.0;
    bool unbounded = false;
    for (int i = m - 2; i >= 0; --i) {
        double b = xcap[i];
        for (int e = 0; e < (n + 2) * (n + 2); ++e) b = take_min(b, stage_pair(n + 1, s[i], k[i], 1, beta[i + 1], e));
        beta[i] = b;
        if (!(b < inf())) unbounded = true;
    }
    if (unbounded) return fail(UNBOUNDED);
    xs[0] = 0.0;
    for (int i = 0; i < m - 1; ++i) {
        double h = inf();
        for (int j = 0; j <= n; ++j) h = take_min(h, hi_value(s[i][j], k[i][j], xs[i]));
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
        const double u = own && i < m - 1 ? accel_u(xs[i], xs[i + 1]) : 0.0;
        for (int j = 0; j < n; ++j) {
            double v = 0.0, acc = 0.0;
            if (own) {
                const double d = deriv_d(path + j, st, m, i), c = deriv_c(path + j, st, m, i);
                v = out_qd(d, r[i]);
                if (i < m - 1) acc = out_qdd(d, u, c, xs[i]);
            }
            if (qd) qd[i * n + j] = v;
            if (qdd) qdd[i * n + j] = acc;
        }
        if (tool_speed) tool_speed[i] = own ? out_speed(tool[i], r[i]) : 0.0;
        if (tool_wspeed) tool_wspeed[i] = own ? out_wspeed(tool[i], r[i]) : 0.0;
        if (tool_accel) {
            tool_accel[2 * i] = own && i < m - 1 ? out_tangential(tool[i], u, xs[i]) : 0.0;
            tool_accel[2 * i + 1] = own ? out_normal(tool[i], xs[i]) : 0.0;
        }
    }
    if (stalled) return Result{STALLED, nan()};
    return Result{TIMED, ts[m - 1]};
}
#endif

}  // namespace tooltime
}  // namespace optik
