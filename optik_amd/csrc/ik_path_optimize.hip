// ik_path_optimize.hip -- bending joint paths out of collision: covariant gradient smoothing of a batch of paths
// (path_optimize.hpp: the arithmetic and its operation order).
//
//   path_optimize_kernel<N, TIP>   one wave per path, lane t = waypoint t (lanes >= L idle), the whole iteration
//                                  loop in one launch
//   path_optimize_constrained_kernel<N, TIP>   the same loop under a pose constraint (path_optimize.hpp step 7;
//                                  DESIGN.md section 5.32), kept as a kernel of its own: one body for both moved
//                                  the plain kernel's register record (profiles/constraint_plumbing_refactor.txt).
//                                  After the step every interior lane projects its own
//                                  waypoint back onto the box (constraint::project, the header's own function, as
//                                  shortcut_cgather_kernel calls it) and keeps the old one where that fails; the
//                                  last evaluation also measures every waypoint's violation.  The projection reads
//                                  no other lane; lanes whose loops differ in length cost the wave the longest of
//                                  them, which piters bounds.  Its per-lane tables live in scratch.
// 256 threads = 4 paths per block, grid-stride over the paths; the chain table and the model are staged in LDS once
// per block as collision_witness_kernel stages them.  A wave keeps its path's iterate and its gradient g in LDS,
// [N][64] doubles each (joint-major: a lane reads its neighbours' waypoints and the wave-uniform g_k without bank
// conflicts), and three [64] rows of per-waypoint partial sums (four under a constraint: the violation).  Per
// evaluation every lane runs FK and the witness distance pass of its own waypoint (collision_witness_device.hpp,
// unchanged), folds the rows' hinge and gradients into o_t and gobs_t, and reads its neighbours from LDS for s_t and
// g_t; the update is the closed-form Ainv sum, M terms read from LDS per lane, no serial solve.  Lane 0 sums the partials in ascending order at the first and the
// last evaluation.  Nothing crosses a wave: after the staging barrier the waves of a block never meet again, so the
// result does not depend on the launch shape.
#include "collision_witness_device.hpp"
#include "constraint_device.hpp"
#include "path_optimize.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::hostparams;
using namespace optik::colldev;
using namespace optik::condev;

static_assert(pathopt::MAX_WAYPOINTS == OPTIK_HIP_PATH_OPTIMIZE_MAX_WAYPOINTS && pathopt::MAX_WAYPOINTS == 64,
              "one lane of a wave per waypoint; optik_hip.h states the cap of path_optimize.hpp");
static_assert(constraint::PROJECTED == OPTIK_HIP_CONSTRAINT_PROJECTED, "optik_hip.h states the projection's status");

namespace {

constexpr int WAVES = 4;  // paths per block

struct PathOptLaunch {
    CollLaunch c;          // chain, ee_offset, model, world (q and B unused)
    const uint16_t *orig;  // [S + P]: the caller's index of the sphere in a slot, of the pair at a position
    const double *q_in;    // [L][P][n]
    double *q_out;         // [L][P][n] or null; may be q_in
    long long P;
    int L, iters;
    pathopt::Params p;
    double *cost_first, *cost_last;  // [P][3] or null
    double *clearance;               // [P] or null
    int32_t *status;                 // [P] or null
};

// LDS written by some lanes of the wave is about to be read by others
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <int N, bool TIP>
__global__ __launch_bounds__(64 * WAVES) void path_optimize_kernel(const PathOptLaunch a) {
    __shared__ ChainDev sch;
    __shared__ ModelDev sm;
    __shared__ double s_q[WAVES][N][64];     // the iterate
    __shared__ double s_g[WAVES][N][64];     // g of the update
    __shared__ double s_part[WAVES][3][64];  // o_t, s_t, the waypoint's clearance
    stage_chain(sch, a.c.chain);
    if (a.c.model) stage_model(sm, a.c);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int L = a.L, M = L - 2;
    const bool act = lane < L, interior = lane >= 1 && lane <= M;
    const double e = a.p.influence - a.p.safety;
    double(&sq)[N][64] = s_q[wave];
    double(&sg)[N][64] = s_g[wave];
    double(&part)[3][64] = s_part[wave];
    const size_t P = (size_t)a.P;
    for (long long path = (long long)blockIdx.x * WAVES + wave; path < a.P; path += (long long)gridDim.x * WAVES) {
        double q[N];
#pragma unroll
        for (int j = 0; j < N; ++j) q[j] = act ? a.q_in[((size_t)lane * P + (size_t)path) * N + j] : 0.0;
        for (int it = 0;; ++it) {
            double o = 0.0, gobs[N], clr = __builtin_huge_val();
#pragma unroll
            for (int j = 0; j < N; ++j) gobs[j] = 0.0;
            if (act) {
#pragma unroll
                for (int j = 0; j < N; ++j) sq[j][lane] = q[j];
                Kin<N, TIP> kin;
                forward_kinematics<N, TIP>(sch, a.c.ep, q, kin);
                const bool nan = kin_has_nan<N, TIP>(kin);
                Rows<N> rows;
#pragma unroll
                for (int k = 0; k < N + 2; ++k) { rows.dist[k] = __builtin_huge_val(); rows.wit[k] = -1; }
                if (a.c.model) witness_pass<N, TIP>(sm, a, kin, rows);
                bool row_nan = false;
                for (int f = 0; f < N + 2; ++f) {
                    double d;
                    int32_t w;
                    row_get<N>(rows, __builtin_amdgcn_readfirstlane(f), d, w);
                    if (nan) { d = __builtin_nan(""); w = -1; }
                    pathopt::clearance_take(d, clr, row_nan);
                    if (interior) {
                        double c, cp;
                        pathopt::hinge(d, a.p.safety, e, c, cp);
                        o = o + c;
                        if (w >= 0) {
                            row_gradient<N, TIP>(sch, sm, a, kin, f, w, [&](int j, double v) {
#pragma unroll
                                for (int k = 0; k < N; ++k)
                                    if (j == k) gobs[k] = pathopt::add_scaled(gobs[k], cp, v);
                            });
                        } else {
                            const double fill = nan ? __builtin_nan("") : 0.0;
#pragma unroll
                            for (int k = 0; k < N; ++k) gobs[k] = pathopt::add_scaled(gobs[k], cp, fill);
                        }
                    }
                }
                if (row_nan) clr = __builtin_nan("");
                part[0][lane] = o;
                part[2][lane] = clr;
            }
            wave_lds_sync();
            if (act && lane <= M) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < N; ++j) s = pathopt::add_square(s, q[j], sq[j][lane + 1]);
                part[1][lane] = s;
            }
            wave_lds_sync();
            const bool first = it == 0, last = it == a.iters;
            if ((first || last) && lane == 0) {
                double sum_s = 0.0, sum_o = 0.0, cost3[3];
                for (int t = 0; t + 1 < L; ++t) sum_s = sum_s + part[1][t];
                for (int t = 1; t + 1 < L; ++t) sum_o = sum_o + part[0][t];
                pathopt::costs(a.p, sum_s, sum_o, cost3);
                if (first && a.cost_first)
                    for (int k = 0; k < 3; ++k) a.cost_first[(size_t)path * 3 + k] = cost3[k];
                if (last) {
                    if (a.cost_last)
                        for (int k = 0; k < 3; ++k) a.cost_last[(size_t)path * 3 + k] = cost3[k];
                    double best = __builtin_huge_val();
                    bool any_nan = false;
                    for (int t = 0; t < L; ++t) pathopt::clearance_take(part[2][t], best, any_nan);
                    if (a.clearance) a.clearance[path] = any_nan ? __builtin_nan("") : best;
                    if (a.status) a.status[path] = cost3[0] != cost3[0] ? 1 : 0;
                }
            }
            if (last) break;
            if (interior) {
#pragma unroll
                for (int j = 0; j < N; ++j)
                    sg[j][lane] = pathopt::gradient_term(a.p, sq[j][lane - 1], q[j], sq[j][lane + 1], gobs[j]);
            }
            wave_lds_sync();
            if (interior) {
                double y[N];
#pragma unroll
                for (int j = 0; j < N; ++j) y[j] = 0.0;
                for (int k = 1; k <= M; ++k) {
                    const double ai = pathopt::ainv(lane, k, M);
#pragma unroll
                    for (int j = 0; j < N; ++j) y[j] = y[j] + ai * sg[j][k];
                }
#pragma unroll
                for (int j = 0; j < N; ++j) q[j] = pathopt::stepped(a.p, q[j], y[j], sch.lb[j], sch.ub[j]);
            }
            wave_lds_sync();  // (the next evaluation overwrites the iterate and the partials)
        }
        if (a.q_out && act) {
#pragma unroll
            for (int j = 0; j < N; ++j) a.q_out[((size_t)lane * P + (size_t)path) * N + j] = q[j];
        }
        wave_lds_sync();
    }
}

// The constraint's side of a constrained launch: it travels with the call, the chain handle keeps nothing of it.
struct PathConLaunch {
    constraint::Box c;               // (the chain and ee_offset of a ConstraintDev are PathOptLaunch's already)
    ProjectArgs p;
    double *violation;               // [P] or null
    int32_t *projected;              // [2][P] or null
};

template <int N, bool TIP>
__global__ __launch_bounds__(64 * WAVES) void path_optimize_constrained_kernel(const PathOptLaunch a,
                                                                                   const PathConLaunch con) {
    __shared__ ChainDev sch;
    __shared__ ModelDev sm;
    __shared__ double s_q[WAVES][N][64];     // the iterate
    __shared__ double s_g[WAVES][N][64];     // g of the update
    __shared__ double s_part[WAVES][4][64];  // o_t, s_t, the waypoint's clearance, its violation
    stage_chain(sch, a.c.chain);
    if (a.c.model) stage_model(sm, a.c);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int L = a.L, M = L - 2;
    const bool act = lane < L, interior = lane >= 1 && lane <= M;
    const double e = a.p.influence - a.p.safety;
    const bool free_box = pathopt::box_is_free(con.c.lo, con.c.hi);
    double(&sq)[N][64] = s_q[wave];
    double(&sg)[N][64] = s_g[wave];
    double(&part)[4][64] = s_part[wave];
    const size_t P = (size_t)a.P;
    for (long long path = (long long)blockIdx.x * WAVES + wave; path < a.P; path += (long long)gridDim.x * WAVES) {
        double q[N];
#pragma unroll
        for (int j = 0; j < N; ++j) q[j] = act ? a.q_in[((size_t)lane * P + (size_t)path) * N + j] : 0.0;
        int attempted = 0, ended = 0;  // this lane's projections
        for (int it = 0;; ++it) {
            double o = 0.0, gobs[N], clr = __builtin_huge_val();
#pragma unroll
            for (int j = 0; j < N; ++j) gobs[j] = 0.0;
            if (act) {
#pragma unroll
                for (int j = 0; j < N; ++j) sq[j][lane] = q[j];
                Kin<N, TIP> kin;
                forward_kinematics<N, TIP>(sch, a.c.ep, q, kin);
                const bool nan = kin_has_nan<N, TIP>(kin);
                Rows<N> rows;
#pragma unroll
                for (int k = 0; k < N + 2; ++k) { rows.dist[k] = __builtin_huge_val(); rows.wit[k] = -1; }
                if (a.c.model) witness_pass<N, TIP>(sm, a, kin, rows);
                bool row_nan = false;
                for (int f = 0; f < N + 2; ++f) {
                    double d;
                    int32_t w;
                    row_get<N>(rows, __builtin_amdgcn_readfirstlane(f), d, w);
                    if (nan) { d = __builtin_nan(""); w = -1; }
                    pathopt::clearance_take(d, clr, row_nan);
                    if (interior) {
                        double c, cp;
                        pathopt::hinge(d, a.p.safety, e, c, cp);
                        o = o + c;
                        if (w >= 0) {
                            row_gradient<N, TIP>(sch, sm, a, kin, f, w, [&](int j, double v) {
#pragma unroll
                                for (int k = 0; k < N; ++k)
                                    if (j == k) gobs[k] = pathopt::add_scaled(gobs[k], cp, v);
                            });
                        } else {
                            const double fill = nan ? __builtin_nan("") : 0.0;
#pragma unroll
                            for (int k = 0; k < N; ++k) gobs[k] = pathopt::add_scaled(gobs[k], cp, fill);
                        }
                    }
                }
                if (row_nan) clr = __builtin_nan("");
                part[0][lane] = o;
                part[2][lane] = clr;
            }
            wave_lds_sync();
            if (act && lane <= M) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < N; ++j) s = pathopt::add_square(s, q[j], sq[j][lane + 1]);
                part[1][lane] = s;
            }
            const bool first = it == 0, last = it == a.iters;
            if (last && act) {
                double x[N], r[6];  // (a copy: the header indexes its configuration in rolled loops)
#pragma unroll
                for (int j = 0; j < N; ++j) x[j] = q[j];
                part[3][lane] = constraint::measure(sch, a.c.ep, con.c, N, x, r);
            }
            wave_lds_sync();
            if ((first || last) && lane == 0) {
                double sum_s = 0.0, sum_o = 0.0, cost3[3];
                for (int t = 0; t + 1 < L; ++t) sum_s = sum_s + part[1][t];
                for (int t = 1; t + 1 < L; ++t) sum_o = sum_o + part[0][t];
                pathopt::costs(a.p, sum_s, sum_o, cost3);
                if (first && a.cost_first)
                    for (int k = 0; k < 3; ++k) a.cost_first[(size_t)path * 3 + k] = cost3[k];
                if (last) {
                    if (a.cost_last)
                        for (int k = 0; k < 3; ++k) a.cost_last[(size_t)path * 3 + k] = cost3[k];
                    double best = __builtin_huge_val();
                    bool any_nan = false;
                    for (int t = 0; t < L; ++t) pathopt::clearance_take(part[2][t], best, any_nan);
                    if (a.clearance) a.clearance[path] = any_nan ? __builtin_nan("") : best;
                    if (a.status) a.status[path] = cost3[0] != cost3[0] ? 1 : 0;
                    double v = 0.0;
                    for (int t = 0; t < L; ++t) v = constraint::max_take(v, part[3][t]);
                    if (con.violation) con.violation[path] = v;
                }
            }
            if (last) break;
            if (interior) {
#pragma unroll
                for (int j = 0; j < N; ++j)
                    sg[j][lane] = pathopt::gradient_term(a.p, sq[j][lane - 1], q[j], sq[j][lane + 1], gobs[j]);
            }
            wave_lds_sync();
            if (interior) {
                double y[N];
#pragma unroll
                for (int j = 0; j < N; ++j) y[j] = 0.0;
                for (int k = 1; k <= M; ++k) {
                    const double ai = pathopt::ainv(lane, k, M);
#pragma unroll
                    for (int j = 0; j < N; ++j) y[j] = y[j] + ai * sg[j][k];
                }
                double x[N];
#pragma unroll
                for (int j = 0; j < N; ++j) x[j] = pathopt::stepped(a.p, q[j], y[j], sch.lb[j], sch.ub[j]);
                const bool take = pathopt::settle(free_box, x, [&](double *z) {
                    return constraint::project(sch, a.c.ep, con.c, N, con.p.tol, con.p.iters, con.p.damping, con.p.max_step,
                                               z).status == constraint::PROJECTED;
                }, attempted, ended);
                // (q itself is never handed to the projection: it stays in registers, and the fallback is a select)
#pragma unroll
                for (int j = 0; j < N; ++j) q[j] = take ? x[j] : q[j];
            }
            wave_lds_sync();  // (the next evaluation overwrites the iterate and the partials)
        }
        if (a.q_out && act) {
#pragma unroll
            for (int j = 0; j < N; ++j) a.q_out[((size_t)lane * P + (size_t)path) * N + j] = q[j];
        }
        // the path's two counters: the lanes' own, summed over the wave (integers: any order)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            attempted += __shfl_xor(attempted, o, 64);
            ended += __shfl_xor(ended, o, 64);
        }
        if (lane == 0 && con.projected) {
            con.projected[path] = attempted;
            con.projected[P + (size_t)path] = ended;
        }
        wave_lds_sync();
    }
}

// What both entries put into the record, their arguments checked.
void fill_path_launch(const optik_hip_chain *ch, const double *ee_offset7, const double *d_q_in, int32_t L, int64_t P,
                      int32_t iters, const pathopt::Params &prm, double *d_q_out, double *d_cost_first,
                      double *d_cost_last, double *d_clearance, int32_t *d_status, PathOptLaunch &a) {
    std::memset(&a, 0, sizeof a);
    fill_launch(ch, ee_offset7, nullptr, P, a.c);
    a.orig = ch->coll_orig.get();
    a.q_in = d_q_in; a.q_out = d_q_out;
    a.P = P; a.L = L; a.iters = iters;
    a.p = prm;
    a.cost_first = d_cost_first; a.cost_last = d_cost_last;
    a.clearance = d_clearance; a.status = d_status;
}

const char *const kPathOptWideMsg = "path_optimize: chains of more than 8 joint positions are not supported";

}  // namespace

extern "C" {

int optik_hip_path_optimize(const optik_hip_chain *ch, const double *ee_offset7, const double *d_q_in, int32_t L,
                            int64_t P, int32_t iters, double step, double w_smooth, double w_obs, double influence,
                            double safety, double *d_q_out, double *d_cost_first, double *d_cost_last,
                            double *d_clearance, int32_t *d_status, void *stream) {
    // (the chain's refusals come first, as optik_hip_diff_ik_avoid_batch has them)
    if (!ch || P < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (ch->wide || ch->n > 8) return fail(OPTIK_HIP_EUNSUPPORTED, kPathOptWideMsg);
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, prismatic_msg());
    if (L < pathopt::MIN_WAYPOINTS || L > pathopt::MAX_WAYPOINTS)
        return fail(OPTIK_HIP_EINVAL, "path_optimize: a path has 3 .. 64 waypoints");
    if (iters < 0) return fail(OPTIK_HIP_EINVAL, "path_optimize: iters must be >= 0");
    const pathopt::Params prm{step, w_smooth, w_obs, influence, safety};
    if (!pathopt::params_ok(prm))
        return fail(OPTIK_HIP_EINVAL, "path_optimize: needs step > 0, w_smooth >= 0, w_obs >= 0 and "
                                      "influence > safety >= 0, all finite");
    if (P == 0 || (!d_q_out && !d_cost_first && !d_cost_last && !d_clearance && !d_status)) return 0;
    if (!d_q_in) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    PathOptLaunch a;
    fill_path_launch(ch, ee_offset7, d_q_in, L, P, iters, prm, d_q_out, d_cost_first, d_cost_last, d_clearance, d_status,
                     a);
    const int grid = grid_for(ch, P * 64, 64 * WAVES, 8);
#define CALL(NN, TT) hipLaunchKernelGGL((path_optimize_kernel<NN, TT>), dim3(grid), dim3(64 * WAVES), 0, (hipStream_t)stream, a)
    OPTIK_DISPATCH(ch, CALL);
#undef CALL
    HIP_TRY(hipGetLastError());
    return 0;
}

int optik_hip_path_optimize_constrained(const optik_hip_chain *ch, const double *ee_offset7, const double *d_q_in,
                                        int32_t L, int64_t P, int32_t iters, double step, double w_smooth, double w_obs,
                                        double influence, double safety, const double *ref7, const double *lo6,
                                        const double *hi6, double ptol, int32_t piters, double damping, double max_step,
                                        double *d_q_out, double *d_cost_first, double *d_cost_last, double *d_clearance,
                                        int32_t *d_status, double *d_violation, int32_t *d_projected, void *stream) {
    // (P = 0: optik_hip_path_optimize's own refusals -- the chain, L, iters and the parameters)
    if (!ch || P < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (int rc = optik_hip_path_optimize(ch, nullptr, nullptr, L, 0, iters, step, w_smooth, w_obs, influence, safety,
                                         nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
        return rc;
    // (B = 0: the projection's own refusals -- the reference, the bounds, ptol, piters, damping and max_step -- as
    // optik_hip_path_shortcut_constrained takes them)
    if (int rc = optik_hip_constraint_project_batch(ch, nullptr, ref7, lo6, hi6, nullptr, 0, ptol, piters, damping,
                                                    max_step, nullptr, nullptr, nullptr, nullptr, nullptr))
        return rc;
    if (P == 0
        || (!d_q_out && !d_cost_first && !d_cost_last && !d_clearance && !d_status && !d_violation && !d_projected))
        return 0;
    if (!d_q_in) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    PathOptLaunch a;
    fill_path_launch(ch, ee_offset7, d_q_in, L, P, iters, pathopt::Params{step, w_smooth, w_obs, influence, safety},
                     d_q_out, d_cost_first, d_cost_last, d_clearance, d_status, a);
    ConstraintDev d;
    fill_constraint(ch, ee_offset7, ref7, lo6, hi6, d);
    PathConLaunch con{};
    con.c = d.c;
    con.p = ProjectArgs{ptol, damping, max_step, piters};
    con.violation = d_violation; con.projected = d_projected;
    const int grid = grid_for(ch, P * 64, 64 * WAVES, 8);
#define CALL(NN, TT) hipLaunchKernelGGL((path_optimize_constrained_kernel<NN, TT>), dim3(grid), dim3(64 * WAVES), 0, (hipStream_t)stream, a, con)
    OPTIK_DISPATCH(ch, CALL);
#undef CALL
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
