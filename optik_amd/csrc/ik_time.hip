// ik_time.hip -- velocity- and acceleration-limited timing of joint paths and the sampling of the timed trajectory on
// the device (time_measure.hpp: the arithmetic and its operation order).
// optik_hip_path_time / _trajectory_sample (include/optik_hip.h).
//
//   path_time_kernel           one wave per path.  The waypoints are staged [joint][64] in LDS (lane t reads its own
//                              column without a bank conflict, a stage's column is a broadcast); lane i forms d and c of
//                              waypoint i, the stage's members [joint][64] and its cap.  Both passes are serial in i.  In
//                              the backward pass the lanes split the (n + 1)^2 pairs of the stage -- 4 at n = 1, 289 at
//                              n = 16 -- and a butterfly takes the minimum, which is exact in any order; in the forward
//                              pass lane l holds joint l & 15, so every group of 16 lanes ends with the same minimum
//                              after four butterfly steps.  The square roots and the segment times are the owning
//                              lanes', the time prefix is lane 0's, in the header's order.  Dynamic LDS: (3 n + 5) * 64
//                              doubles (4 608 bytes at n = 1, 13 824 at n = 7, 27 136 at n = 16); no workspace.
//   path_time_tool_kernel<CH>  path_time_kernel with the tool's limits (time_tool_measure.hpp; DESIGN.md section 5.35;
//                              optik_hip_path_time_tool), a kernel of its own so that path_time_kernel stays what it
//                              is.  CH is ChainDev (n <= 8) or WideChainDev (9 .. 16), the table staged in static LDS.
//                              Lane i runs the forward kinematics of waypoint i from its own LDS column -- the rolled
//                              joint loop without the joint frames, so the pose is seven doubles of registers -- and
//                              stages the pose [7][64]; after a barrier it forms the tool's derivatives from its
//                              neighbours' columns (conflict-free like the joints': lane t reads column t +- 1), the
//                              tool member as row n of the members and the tool caps into the stage's cap.  The
//                              backward pass splits (n + 2)^2 pairs -- 9 at n = 1, 324 at n = 16, six a lane.  The
//                              forward pass has up to 17 members, which lane & 15 does not cover: it FOLDS OVER 32
//                              LANES, lane l holding member l & 31, five butterfly steps, so that either half of the
//                              wave ends with the minimum.  Dynamic LDS: (3 n + 14) * 64 doubles -- path_time_kernel's
//                              (3 n + 5) rows, one more slope and one more offset row for the tool member, seven pose
//                              rows -- 8 704 bytes at n = 1, 17 920 at n = 7, 31 744 at n = 16; plus the chain table,
//                              840 or 1 736 bytes static; no workspace.
//   trajectory_sample_kernel   one thread per (path, sample), the path running fastest so that a wave writes
//                              neighbouring paths (beyond 2^28 samples a thread strides on); no LDS, no workspace.
//   path_time_spline_kernel    spline retiming (time_spline_measure.hpp; DESIGN.md section 5.36;
//                              optik_hip_path_time_spline): one wave per path, the wave striding over the paths when
//                              the grid is smaller than P.  Waypoints q, and the two work columns e and d of the
//                              Thomas recurrence, are [joint][64] in LDS with row j rotated by j columns (spl_at): in
//                              the recurrences lane j < n walks row j serially, and without the rotation the n lanes
//                              would read n addresses 512 bytes apart, one bank; with it they read n neighbouring
//                              columns.  In the measure lane i < m - 1 walks column i of every row, neighbouring
//                              addresses with or without the rotation.  The times and the inverse spacings are one
//                              row each: (3 n + 2) * 64 doubles of dynamic LDS (2 560 bytes at n = 1, 11 776 at n = 7,
//                              25 600 at n = 16); no workspace.  A butterfly takes the three maxima; every lane then
//                              holds the same ratios and computes the same factor.
//
// A path's block sees only that path, so nothing depends on P or on the launch shape.
#include "constraint_device.hpp"
#include "time_measure.hpp"
#include "time_spline_measure.hpp"
#include "time_tool_measure.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::colldev;
using namespace optik::condev;

static_assert(timing::MAX_POINTS == OPTIK_HIP_PATH_TIME_MAX_WAYPOINTS && timing::MAX_POINTS == 64,
              "one lane of a wave per waypoint");
static_assert(timing::MAX_JOINTS == WIDE_MAX_DOF && timing::MAX_JOINTS == 16,
              "time_measure.hpp states the cap on the joint positions; the forward pass folds 16 lanes");

namespace {

constexpr int TM_WAVE = 64, SAMPLE_BLOCK = 256;
constexpr int MP = timing::MAX_POINTS;
constexpr long long MAX_PATHS = 1ll << 30;
constexpr long long SAMPLE_MAX_GRID = 1ll << 20;  // blocks; a thread strides over the rest

struct TimeLaunch {
    const double *path;  // [L][P][n]
    const int32_t *len;  // [P] or null: L
    const double *vmax, *amax;  // [n]
    long long P;
    int n, L;
    double *t;         // [L][P] or null
    double *qd, *qdd;  // [L][P][n] or null
    double *x;         // [L][P] or null
    double *duration;  // [P] or null
    int32_t *status;   // [P] or null
};

__device__ __forceinline__ double wave_min(double b, int first) {
#pragma unroll
    for (int o = first; o >= 1; o >>= 1) b = timing::take_min(b, __shfl_xor(b, o, TM_WAVE));
    return b;
}

__global__ __launch_bounds__(TM_WAVE) void path_time_kernel(const TimeLaunch a) {
    extern __shared__ double tm_lds[];
    const int n = a.n, L = a.L, lane = threadIdx.x;
    double *q = tm_lds;          // [n][64] joint j of waypoint t at q[j * 64 + t]
    double *s = q + n * MP;      // [n][64] the members' slopes, stage i at s[j * 64 + i]
    double *k = s + n * MP;      // [n][64] and offsets
    double *bet = k + n * MP;    // [64] xcap, then beta
    double *xs = bet + MP;       // [64]
    double *rt = xs + MP;        // [64] sqrt x
    double *seg = rt + MP;       // [64] segment times
    double *ts = seg + MP;       // [64]
    const long long p = blockIdx.x;
    const double *path = a.path + p * n;
    const long long st = a.P * n;
    const int m = __builtin_amdgcn_readfirstlane(a.len ? a.len[p] : L);
    int status = timing::TIMED;
    if (!timing::length_ok(m, L)) status = timing::BAD_LENGTH;
    if (status == timing::TIMED) {
        bool fin = true;
        if (lane < m)
            for (int j = 0; j < n; ++j) {
                const double v = path[lane * st + j];
                q[j * MP + lane] = v;
                fin = fin && timing::is_finite(v);
            }
        if (!__syncthreads_and(fin)) status = timing::PATH_NAN;
    }
    double duration = timing::nan();
    double x_mine = 0.0;
    if (status == timing::TIMED) {
        // the stage of lane i: members and cap
        if (lane < m - 1) {
            double cap = timing::inf();
            for (int j = 0; j < n; ++j) {
                const double d = timing::deriv_d(q + j * MP, 1, m, lane), c = timing::deriv_c(q + j * MP, 1, m, lane);
                const double aj = a.amax[j];
                const timing::Member mb = timing::member(d, c, aj);
                s[j * MP + lane] = mb.s;
                k[j * MP + lane] = mb.k;
                cap = timing::take_min(cap, timing::cap_term(d, c, a.vmax[j], aj));
            }
            bet[lane] = cap;
        }
        __syncthreads();
        // backward
        const int pairs = (n + 1) * (n + 1);
        double bnext = 0.0, beta_mine = 0.0;  // beta_(m-1)
        bool unbounded = false;
        for (int i = m - 2; i >= 0; --i) {
            double b = bet[i];
            for (int e = lane; e < pairs; e += TM_WAVE)
                b = timing::take_min(b, timing::stage_pair(n, s + i, k + i, MP, bnext, e));
            b = wave_min(b, TM_WAVE / 2);
            if (lane == i) beta_mine = b;
            if (!(b < timing::inf())) unbounded = true;
            bnext = b;
        }
        __syncthreads();
        if (lane < m) bet[lane] = beta_mine;
        __syncthreads();
        if (unbounded) status = timing::UNBOUNDED;
    }
    if (status == timing::TIMED) {
        // forward
        const int j = lane & (timing::MAX_JOINTS - 1);
        double xi = 0.0;
        for (int i = 0; i < m - 1; ++i) {
            double h = timing::inf();
            if (j < n) h = timing::take_min(h, timing::hi_value(s[j * MP + i], k[j * MP + i], xi));
            h = wave_min(h, timing::MAX_JOINTS / 2);
            h = timing::take_min(h, bet[i + 1]);
            xi = timing::clamp_x(h);
            if (lane == i + 1) x_mine = xi;
        }
        if (lane < m) {
            xs[lane] = x_mine;
            rt[lane] = timing::tm_sqrt(x_mine);
        }
        __syncthreads();
        bool bad = false;
        if (lane < m - 1) {
            bad = timing::segment_bad(rt[lane], rt[lane + 1]);
            seg[lane] = timing::segment_time(rt[lane], rt[lane + 1]);
        }
        const bool any_bad = __syncthreads_or(bad) != 0;
        if (lane == 0) {
            double acc = 0.0;
            ts[0] = acc;
            for (int i = 0; i < m - 1; ++i) {
                acc = acc + seg[i];
                ts[i + 1] = acc;
            }
        }
        __syncthreads();
        duration = ts[m - 1];
        if (any_bad || !timing::is_finite(duration)) status = timing::STALLED;
    }
    const bool timed = status == timing::TIMED;
    if (!timed) duration = timing::nan();
    if (lane == 0) {
        if (a.duration) a.duration[p] = duration;
        if (a.status) a.status[p] = status;
    }
    if (lane >= L) return;
    const bool own = (timed || status == timing::STALLED) && lane < m;  // (STALLED: the profile is still written)
    if (a.t) a.t[(long long)lane * a.P + p] = timed && lane < m ? ts[lane] : duration;
    if (a.x) a.x[(long long)lane * a.P + p] = own ? x_mine : 0.0;
    if (!a.qd && !a.qdd) return;
    const long long o = ((long long)lane * a.P + p) * n;
    for (int j = 0; j < n; ++j) {
        double v = 0.0, acc = 0.0;
        if (own) {
            const double d = timing::deriv_d(q + j * MP, 1, m, lane), c = timing::deriv_c(q + j * MP, 1, m, lane);
            v = timing::out_qd(d, rt[lane]);
            if (lane < m - 1) acc = timing::out_qdd(d, timing::accel_u(x_mine, xs[lane + 1]), c, x_mine);
        }
        if (a.qd) a.qd[o + j] = v;
        if (a.qdd) a.qdd[o + j] = acc;
    }
}

struct ToolLaunch {
    TimeLaunch t;
    ConstraintDev d;                // the chain's tables and the ee_offset (no box)
    double lim[tooltime::LIMITS];   // v_tool, a_t, a_n, w_tool; +inf: absent
    double *tool_speed;             // [L][P] or null
    double *tool_accel;             // [L][P][2] or null
    double *tool_wspeed;            // [L][P] or null
};

// rows of 64 doubles of dynamic LDS: the waypoints [n], the members' slopes and offsets [n + 1] each (the tool's is row
// n), the five rows of path_time_kernel, the end effector's pose per waypoint [7]
constexpr int tool_lds_rows(int n) { return 3 * n + 14; }

template <class CH>
__global__ __launch_bounds__(TM_WAVE) void path_time_tool_kernel(const ToolLaunch b) {
    extern __shared__ double tm_lds[];
    __shared__ CH sch;
    const TimeLaunch &a = b.t;
    const int n = a.n, L = a.L, lane = threadIdx.x, nm = n + 1;  // nm: the stored members of a stage
    double *q = tm_lds;          // [n][64] joint j of waypoint t at q[j * 64 + t]
    double *s = q + n * MP;      // [n + 1][64] the members' slopes, stage i at s[j * 64 + i]; row n: the tool's
    double *k = s + nm * MP;     // [n + 1][64] and offsets
    double *bet = k + nm * MP;   // [64] xcap, then beta
    double *xs = bet + MP;       // [64]
    double *rt = xs + MP;        // [64] sqrt x
    double *seg = rt + MP;       // [64] segment times
    double *ts = seg + MP;       // [64]
    double *pe = ts + MP;        // [7][64] the end effector's pose, component r of waypoint t at pe[r * 64 + t]
    copy_table(sch, table_of<CH>(b.d));  // (the barrier behind the waypoints' staging is the table's too)
    const long long p = blockIdx.x;
    const double *path = a.path + p * n;
    const long long st = a.P * n;
    const int m = __builtin_amdgcn_readfirstlane(a.len ? a.len[p] : L);
    int status = timing::TIMED;
    if (!timing::length_ok(m, L)) status = timing::BAD_LENGTH;
    if (status == timing::TIMED) {
        bool fin = true;
        if (lane < m)
            for (int j = 0; j < n; ++j) {
                const double v = path[lane * st + j];
                q[j * MP + lane] = v;
                fin = fin && timing::is_finite(v);
            }
        if (!__syncthreads_and(fin)) status = timing::PATH_NAN;
    }
    double duration = timing::nan();
    double x_mine = 0.0;
    tooltime::Stage tool{0.0, 0.0, 0.0, 0.0};
    if (status == timing::TIMED) {
        // the tool at waypoint `lane`: its pose from the lane's own column, then its derivatives from the neighbours'
        if (lane < m) tooltime::store_ee(pe, MP, 1, lane, tooltime::fk_ee(sch, b.d.ep, n, q + lane, MP));
        __syncthreads();
        if (lane < m) tool = tooltime::stage_terms(pe, MP, 1, m, lane);
        // the stage of lane i: members and cap
        if (lane < m - 1) {
            double cap = timing::inf();
            for (int j = 0; j < n; ++j) {
                const double d = timing::deriv_d(q + j * MP, 1, m, lane), c = timing::deriv_c(q + j * MP, 1, m, lane);
                const double aj = a.amax[j];
                const timing::Member mb = timing::member(d, c, aj);
                s[j * MP + lane] = mb.s;
                k[j * MP + lane] = mb.k;
                cap = timing::take_min(cap, timing::cap_term(d, c, a.vmax[j], aj));
            }
            const timing::Member mb = tooltime::tool_member(tool, b.lim);
            s[n * MP + lane] = mb.s;
            k[n * MP + lane] = mb.k;
            bet[lane] = timing::take_min(cap, tooltime::tool_cap(tool, b.lim));
        }
        __syncthreads();
        // backward
        const int pairs = (nm + 1) * (nm + 1);
        double bnext = 0.0, beta_mine = 0.0;  // beta_(m-1)
        bool unbounded = false;
        for (int i = m - 2; i >= 0; --i) {
            double bb = bet[i];
            for (int e = lane; e < pairs; e += TM_WAVE)
                bb = timing::take_min(bb, timing::stage_pair(nm, s + i, k + i, MP, bnext, e));
            bb = wave_min(bb, TM_WAVE / 2);
            if (lane == i) beta_mine = bb;
            if (!(bb < timing::inf())) unbounded = true;
            bnext = bb;
        }
        __syncthreads();
        if (lane < m) bet[lane] = beta_mine;
        __syncthreads();
        if (unbounded) status = timing::UNBOUNDED;
    }
    if (status == timing::TIMED) {
        // forward: lane l holds member l & 31 (17 of them at n = 16), so either half of the wave ends with the minimum
        const int j = lane & (TM_WAVE / 2 - 1);
        double xi = 0.0;
        for (int i = 0; i < m - 1; ++i) {
            double h = timing::inf();
            if (j < nm) h = timing::take_min(h, timing::hi_value(s[j * MP + i], k[j * MP + i], xi));
            h = wave_min(h, TM_WAVE / 4);
            h = timing::take_min(h, bet[i + 1]);
            xi = timing::clamp_x(h);
            if (lane == i + 1) x_mine = xi;
        }
        if (lane < m) {
            xs[lane] = x_mine;
            rt[lane] = timing::tm_sqrt(x_mine);
        }
        __syncthreads();
        bool bad = false;
        if (lane < m - 1) {
            bad = timing::segment_bad(rt[lane], rt[lane + 1]);
            seg[lane] = timing::segment_time(rt[lane], rt[lane + 1]);
        }
        const bool any_bad = __syncthreads_or(bad) != 0;
        if (lane == 0) {
            double acc = 0.0;
            ts[0] = acc;
            for (int i = 0; i < m - 1; ++i) {
                acc = acc + seg[i];
                ts[i + 1] = acc;
            }
        }
        __syncthreads();
        duration = ts[m - 1];
        if (any_bad || !timing::is_finite(duration)) status = timing::STALLED;
    }
    const bool timed = status == timing::TIMED;
    if (!timed) duration = timing::nan();
    if (lane == 0) {
        if (a.duration) a.duration[p] = duration;
        if (a.status) a.status[p] = status;
    }
    if (lane >= L) return;
    const bool own = (timed || status == timing::STALLED) && lane < m;  // (STALLED: the profile is still written)
    const long long lp = (long long)lane * a.P + p;
    if (a.t) a.t[lp] = timed && lane < m ? ts[lane] : duration;
    if (a.x) a.x[lp] = own ? x_mine : 0.0;
    const double r = own ? rt[lane] : 0.0, u = own && lane < m - 1 ? timing::accel_u(x_mine, xs[lane + 1]) : 0.0;
    if (b.tool_speed) b.tool_speed[lp] = own ? tooltime::out_speed(tool, r) : 0.0;
    if (b.tool_wspeed) b.tool_wspeed[lp] = own ? tooltime::out_wspeed(tool, r) : 0.0;
    if (b.tool_accel) {
        b.tool_accel[2 * lp] = own && lane < m - 1 ? tooltime::out_tangential(tool, u, x_mine) : 0.0;
        b.tool_accel[2 * lp + 1] = own ? tooltime::out_normal(tool, x_mine) : 0.0;
    }
    if (!a.qd && !a.qdd) return;
    const long long o = lp * n;
    for (int j = 0; j < n; ++j) {
        double v = 0.0, acc = 0.0;
        if (own) {
            const double d = timing::deriv_d(q + j * MP, 1, m, lane), c = timing::deriv_c(q + j * MP, 1, m, lane);
            v = timing::out_qd(d, r);
            if (lane < m - 1) acc = timing::out_qdd(d, u, c, x_mine);
        }
        if (a.qd) a.qd[o + j] = v;
        if (a.qdd) a.qdd[o + j] = acc;
    }
}

struct SampleLaunch {
    const double *path;     // [L][P][n]
    const int32_t *len;     // [P] or null: L
    const double *t;        // [L][P]
    const double *qd;       // [L][P][n]
    const int32_t *status;  // [P]
    long long P;
    int n, L, Tout;
    double dt;
    double *q_out, *v_out;  // [Tout][P][n]
};

__global__ __launch_bounds__(SAMPLE_BLOCK) void trajectory_sample_kernel(const SampleLaunch a) {
    const long long total = a.P * a.Tout, stride = (long long)gridDim.x * SAMPLE_BLOCK;
    for (long long g = (long long)blockIdx.x * SAMPLE_BLOCK + threadIdx.x; g < total; g += stride) {
        const long long k = g / a.P, p = g % a.P;
        const long long o = g * a.n;
        timing::sample_waypoint(a.n, a.path + p * a.n, a.P * a.n, a.len ? a.len[p] : a.L, a.L, a.t + p, a.P,
                                a.qd + p * a.n, a.status[p], a.dt, k, a.q_out + o, a.v_out + o, 1);
    }
}

struct SplineLaunch {
    const double *path;         // [L][P][n]
    const int32_t *len;         // [P] or null: L
    const double *t_in;         // [L][P]
    const int32_t *status_in;   // [P] or null: 0
    const double *vmax, *amax, *jmax;  // [n]
    long long P;
    int n, L;
    double *t;                  // [L][P] or null
    double *qd, *qdd;           // [L][P][n] or null
    double *duration, *factor;  // [P] or null
    double *ratios;             // [P][3] or null
    int32_t *status;            // [P] or null
};

constexpr int SPLINE_BLOCKS_PER_CU = 32;  // one wave each; the LDS admits 6 (n = 16) to 64 (n = 1) of them
constexpr int spline_lds_rows(int n) { return 3 * n + 2; }

// joint j of waypoint (or row, or segment) i in a [joint][64] block whose row j is rotated by j columns
__device__ __forceinline__ int spl_at(int j, int i) { return j * MP + ((i + j) & (MP - 1)); }

__device__ __forceinline__ double wave_max(double b) {
#pragma unroll
    for (int o = TM_WAVE / 2; o >= 1; o >>= 1) b = splinetime::take_max(b, __shfl_xor(b, o, TM_WAVE));
    return b;
}

// Steps 1 to 3 of time_spline_measure.hpp on the times ts: the knot velocities into d, the wave's ratios returned.
__device__ splinetime::Peaks spline_measure(const SplineLaunch &a, int m, int lane, const double *q, double *e,
                                            double *d, const double *ts, double *g) {
    const int n = a.n;
    if (lane < m - 1) g[lane] = splinetime::inv_spacing(ts[lane], ts[lane + 1]);
    __syncthreads();
    if (lane < n) {
        const int j = lane;
        double ep = 0.0, dp = 0.0, gm = g[0], q1 = q[spl_at(j, 1)];
        double dm = splinetime::chord(q[spl_at(j, 0)], q1, gm);
        for (int i = 1; i < m - 1; ++i) {
            const double gi = g[i], q2 = q[spl_at(j, i + 1)], di = splinetime::chord(q1, q2, gi);
            const splinetime::Sweep s = splinetime::sweep_row(gm, gi, dm, di, ep, dp);
            e[spl_at(j, i)] = s.e;
            d[spl_at(j, i)] = s.d;
            ep = s.e;
            dp = s.d;
            gm = gi;
            dm = di;
            q1 = q2;
        }
        double v = 0.0;
        d[spl_at(j, m - 1)] = v;
        for (int i = m - 2; i >= 1; --i) {
            v = splinetime::back_row(e[spl_at(j, i)], d[spl_at(j, i)], v);
            d[spl_at(j, i)] = v;
        }
        d[spl_at(j, 0)] = 0.0;
    }
    __syncthreads();
    splinetime::Peaks pk = splinetime::no_peaks();
    if (lane < m - 1) {
        const double gi = g[lane];
        for (int j = 0; j < n; ++j) {
            const double v0 = d[spl_at(j, lane)];
            const splinetime::Segment s = splinetime::segment(
                splinetime::chord(q[spl_at(j, lane)], q[spl_at(j, lane + 1)], gi), v0, d[spl_at(j, lane + 1)], gi);
            splinetime::fold_segment(pk, s, v0, a.vmax[j], a.amax[j], a.jmax[j]);
        }
    }
    pk.v = wave_max(pk.v);
    pk.a = wave_max(pk.a);
    pk.j = wave_max(pk.j);
    pk.ok = __syncthreads_and(pk.ok) != 0;
    return pk;
}

__global__ __launch_bounds__(TM_WAVE) void path_time_spline_kernel(const SplineLaunch a) {
    extern __shared__ double tm_lds[];
    const int n = a.n, L = a.L, lane = threadIdx.x;
    double *q = tm_lds;       // [n][64] rotated: joint j of waypoint t at q[spl_at(j, t)]
    double *e = q + n * MP;   // [n][64] rotated: the recurrence's e of row i
    double *d = e + n * MP;   // [n][64] rotated: its d, then the knot velocities
    double *ts = d + n * MP;  // [64] the times
    double *g = ts + MP;      // [64] the inverse spacings
    const long long st = a.P * n;
    for (long long p = blockIdx.x; p < a.P; p += gridDim.x) {
        const double *path = a.path + p * n;
        const int m = __builtin_amdgcn_readfirstlane(a.len ? a.len[p] : L);
        const int sin = __builtin_amdgcn_readfirstlane(a.status_in ? a.status_in[p] : 0);
        const bool timed_in = splinetime::input_timed(sin);  // (0, or a former result's 4: its times are valid)
        int status = splinetime::SMOOTH;
        if (!timing::length_ok(m, L)) status = splinetime::BAD_LENGTH;
        if (status == splinetime::SMOOTH) {
            bool fin = true;
            if (lane < m) {
                for (int j = 0; j < n; ++j) {
                    const double v = path[lane * st + j];
                    q[spl_at(j, lane)] = v;
                    fin = fin && timing::is_finite(v);
                }
                if (timed_in) {
                    const double tv = a.t_in[(long long)lane * a.P + p];
                    ts[lane] = tv;
                    fin = fin && timing::is_finite(tv);
                }
            }
            if (!__syncthreads_and(fin)) status = splinetime::NOT_FINITE;
        }
        if (status == splinetime::SMOOTH && !timed_in) status = splinetime::BAD_TIMES;
        if (status == splinetime::SMOOTH) {
            const bool inc = lane < m - 1 ? splinetime::times_step_ok(lane, ts[lane], ts[lane + 1]) : true;
            if (!__syncthreads_and(inc)) status = splinetime::BAD_TIMES;
        }
        double k = 0.0;
        splinetime::Peaks pk = splinetime::no_peaks();
        if (status == splinetime::SMOOTH) {
            pk = spline_measure(a, m, lane, q, e, d, ts, g);
            k = splinetime::factor(pk);
            if (!timing::is_finite(k)) {
                status = splinetime::BAD_TIMES;
            } else if (k > 1.0) {  // (k == 1: t' = t, and the second measure would repeat the first bit for bit)
                const double tv = lane < m ? k * ts[lane] : 0.0;
                __syncthreads();
                if (lane < m) ts[lane] = tv;
                __syncthreads();
                pk = spline_measure(a, m, lane, q, e, d, ts, g);
                if (!pk.ok) status = splinetime::BAD_TIMES;
            }
            if (status == splinetime::SMOOTH && splinetime::over_limit(pk)) status = splinetime::OVER_LIMIT;
        }
        const bool good = status == splinetime::SMOOTH || status == splinetime::OVER_LIMIT;
        const double duration = good ? ts[m - 1] : timing::nan();
        if (lane == 0) {
            if (a.duration) a.duration[p] = duration;
            if (a.factor) a.factor[p] = good ? k : 0.0;
            if (a.ratios) {
                a.ratios[3 * p] = good ? pk.v : 0.0;
                a.ratios[3 * p + 1] = good ? pk.a : 0.0;
                a.ratios[3 * p + 2] = good ? pk.j : 0.0;
            }
            if (a.status) a.status[p] = status;
        }
        if (lane < L) {
            const bool own = good && lane < m;
            const long long lp = (long long)lane * a.P + p;
            if (a.t) a.t[lp] = own ? ts[lane] : duration;
            if (a.qd || a.qdd) {
                // the segment whose end this knot is read at: its own, the last knot the one before it
                const int i = lane < m - 1 ? lane : m - 2;
                const double gi = own ? g[i] : 0.0;
                for (int j = 0; j < n; ++j) {
                    double v = 0.0, acc = 0.0;
                    if (own) {
                        v = d[spl_at(j, lane)];
                        const splinetime::Segment s = splinetime::segment(
                            splinetime::chord(q[spl_at(j, i)], q[spl_at(j, i + 1)], gi), d[spl_at(j, i)],
                            d[spl_at(j, i + 1)], gi);
                        acc = lane < m - 1 ? s.a0 : s.a1;
                    }
                    if (a.qd) a.qd[lp * n + j] = v;
                    if (a.qdd) a.qdd[lp * n + j] = acc;
                }
            }
        }
        __syncthreads();  // (the next path of this wave reuses the LDS)
    }
}

bool points_ok(int v) { return v >= timing::MIN_POINTS && v <= timing::MAX_POINTS; }

}  // namespace

extern "C" {

int optik_hip_path_time(const optik_hip_chain *ch, const double *d_path, const int32_t *d_len, int32_t L, int64_t P,
                        const double *d_vmax, const double *d_amax, double *d_t, double *d_qd, double *d_qdd,
                        double *d_x, double *d_duration, int32_t *d_status, void *stream) {
    if (!ch || P < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (!points_ok(L)) return fail(OPTIK_HIP_EINVAL, "path_time: a path has 3 .. 64 waypoints");
    if (P > MAX_PATHS) return fail(OPTIK_HIP_EINVAL, "path_time: more than 2^30 paths in one launch");
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, prismatic_msg());
    if (P == 0 || (!d_t && !d_qd && !d_qdd && !d_x && !d_duration && !d_status)) return 0;
    if (!d_path || !d_vmax || !d_amax) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    TimeLaunch a{d_path, d_len, d_vmax, d_amax, P, ch->n, L, d_t, d_qd, d_qdd, d_x, d_duration, d_status};
    const size_t lds = sizeof(double) * (size_t)(3 * ch->n + 5) * MP;
    hipLaunchKernelGGL(path_time_kernel, dim3((unsigned)P), dim3(TM_WAVE), lds, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int optik_hip_path_time_tool(const optik_hip_chain *ch, const double *d_path, const int32_t *d_len, int32_t L,
                             int64_t P, const double *d_vmax, const double *d_amax, const double *tool_limits4,
                             const double *ee_offset7, double *d_t, double *d_qd, double *d_qdd, double *d_x,
                             double *d_duration, int32_t *d_status, double *d_tool_speed, double *d_tool_accel,
                             double *d_tool_wspeed, void *stream) {
    if (!ch || P < 0 || !tool_limits4) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (!points_ok(L)) return fail(OPTIK_HIP_EINVAL, "path_time_tool: a path has 3 .. 64 waypoints");
    if (P > MAX_PATHS) return fail(OPTIK_HIP_EINVAL, "path_time_tool: more than 2^30 paths in one launch");
    for (int i = 0; i < tooltime::LIMITS; ++i)
        if (!tooltime::limit_ok(tool_limits4[i]))
            return fail(OPTIK_HIP_EINVAL, "path_time_tool: a tool limit must be > 0 (+inf: no limit), no NaN");
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, prismatic_msg());
    if (P == 0 || (!d_t && !d_qd && !d_qdd && !d_x && !d_duration && !d_status && !d_tool_speed && !d_tool_accel
                   && !d_tool_wspeed))
        return 0;
    if (!d_path || !d_vmax || !d_amax) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    ToolLaunch a;
    std::memset(&a, 0, sizeof a);
    a.t = TimeLaunch{d_path, d_len, d_vmax, d_amax, P, ch->n, L, d_t, d_qd, d_qdd, d_x, d_duration, d_status};
    fill_constraint(ch, ee_offset7, nullptr, nullptr, nullptr, a.d);
    std::memcpy(a.lim, tool_limits4, sizeof a.lim);
    a.tool_speed = d_tool_speed;
    a.tool_accel = d_tool_accel;
    a.tool_wspeed = d_tool_wspeed;
    const size_t lds = sizeof(double) * (size_t)tool_lds_rows(ch->n) * MP;
    if (ch->wide)
        hipLaunchKernelGGL(path_time_tool_kernel<WideChainDev>, dim3((unsigned)P), dim3(TM_WAVE), lds,
                           (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(path_time_tool_kernel<ChainDev>, dim3((unsigned)P), dim3(TM_WAVE), lds, (hipStream_t)stream,
                           a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int optik_hip_path_time_spline(const optik_hip_chain *ch, const double *d_path, const int32_t *d_len, int32_t L,
                               int64_t P, const double *d_t_in, const int32_t *d_status_in, const double *d_vmax,
                               const double *d_amax, const double *d_jmax, double *d_t, double *d_qd, double *d_qdd,
                               double *d_duration, double *d_factor, double *d_ratios, int32_t *d_status,
                               void *stream) {
    if (!ch || P < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (!points_ok(L)) return fail(OPTIK_HIP_EINVAL, "path_time_spline: a path has 3 .. 64 waypoints");
    if (P > MAX_PATHS) return fail(OPTIK_HIP_EINVAL, "path_time_spline: more than 2^30 paths in one launch");
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, prismatic_msg());
    if (P == 0 || (!d_t && !d_qd && !d_qdd && !d_duration && !d_factor && !d_ratios && !d_status)) return 0;
    if (!d_path || !d_t_in || !d_vmax || !d_amax || !d_jmax) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    SplineLaunch a{d_path, d_len, d_t_in, d_status_in, d_vmax, d_amax, d_jmax, P, ch->n, L,
                   d_t,    d_qd,  d_qdd,  d_duration,  d_factor, d_ratios, d_status};
    const size_t lds = sizeof(double) * (size_t)spline_lds_rows(ch->n) * MP;
    const unsigned grid = (unsigned)grid_for(ch, P, 1, SPLINE_BLOCKS_PER_CU);
    hipLaunchKernelGGL(path_time_spline_kernel, dim3(grid), dim3(TM_WAVE), lds, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int optik_hip_trajectory_sample(const optik_hip_chain *ch, const double *d_path, const int32_t *d_len, int32_t L,
                                int64_t P, const double *d_t, const double *d_qd, const int32_t *d_status, double dt,
                                int32_t Tout, double *d_q, double *d_qd_out, void *stream) {
    if (!ch || P < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (!points_ok(L)) return fail(OPTIK_HIP_EINVAL, "trajectory_sample: a path has 3 .. 64 waypoints");
    if (P > MAX_PATHS) return fail(OPTIK_HIP_EINVAL, "trajectory_sample: more than 2^30 paths in one launch");
    if (!(dt > 0.0) || !std::isfinite(dt)) return fail(OPTIK_HIP_EINVAL, "trajectory_sample: dt must be finite and > 0");
    if (Tout < 1 || Tout > OPTIK_HIP_TRAJECTORY_MAX_SAMPLES)
        return fail(OPTIK_HIP_EINVAL, "trajectory_sample: 1 .. 65536 samples per path");
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, prismatic_msg());
    if (P == 0) return 0;
    if (!d_path || !d_t || !d_qd || !d_status || !d_q || !d_qd_out) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    SampleLaunch a{d_path, d_len, d_t, d_qd, d_status, P, ch->n, L, Tout, dt, d_q, d_qd_out};
    const unsigned grid =
        (unsigned)stride_grid((unsigned long long)(P * Tout), SAMPLE_BLOCK, SAMPLE_MAX_GRID, opt().grid_cap);
    hipLaunchKernelGGL(trajectory_sample_kernel, dim3(grid), dim3(SAMPLE_BLOCK), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
