// ik_repair.hip -- collision repair: configurations pushed out of collision along the gradient of their clearance,
// the end effector kept inside a pose box (repair_measure.hpp: the rules and their operation order; DESIGN.md section
// 5.37): optik_hip_collision_repair_batch (include/optik_hip.h).
//
//   repair_kernel<N, TIP>   one configuration per lane, grid-stride, 256 threads; the chain table and the model are
//                           staged in LDS once per block as collision_witness_kernel stages them.  The body is
//                           repair::run over the witness distance pass and the row gradients of
//                           collision_witness_device.hpp (unchanged; folded into the hinge sum row by row, as
//                           path_optimize_constrained_kernel folds them) and constraint::project / measure on the same
//                           LDS table.  The whole loop of a configuration runs in one launch.
// No lane waits for another and nothing is shared after the staging barrier, so the result does not depend on the
// launch shape; lanes whose loops differ in length cost their wave the longest of them, which iters * piters bounds.
// The projection's run-time-indexed tables live in scratch, as path_optimize_constrained_kernel's do.
//
//   region_repair_kernel<N, TIP>   the same lane body behind ik_region_kernel (optik_hip_ik_region_repair): one column
//                           of the region launch per lane, only the columns whose key is finite, each under its own
//                           region's box at the region's tol; a column that ends FREE after at least one step takes
//                           the repaired x and violation, its key is recomputed by region_measure.hpp's rule (steps
//                           3 and 4) and its region's counter goes up by one (an integer atomic: any order).
#include "collision_witness_device.hpp"
#include "constraint_device.hpp"
#include "region_measure.hpp"
#include "repair_device.hpp"
#include "repair_measure.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::hostparams;
using namespace optik::colldev;
using namespace optik::condev;

static_assert(repair::MAX_ITERS == OPTIK_HIP_REPAIR_MAX_ITERS, "optik_hip.h states the cap of repair_measure.hpp");
static_assert(repair::FREE == OPTIK_HIP_REPAIR_FREE && repair::LIMIT == OPTIK_HIP_REPAIR_LIMIT
                  && repair::STUCK == OPTIK_HIP_REPAIR_STUCK && repair::NOT_A_NUMBER == OPTIK_HIP_REPAIR_NAN,
              "optik_hip.h states the statuses of repair_measure.hpp");

namespace {

struct RepairLaunch {
    CollLaunch c;          // chain, ee_offset, model, world, q = x in [n][B], B
    const uint16_t *orig;  // [S + P]: the caller's index of the sphere in a slot, of the pair at a position
    repair::Params p;
    int has_box;           // 0: no box (box and pr unused)
    constraint::Box box;
    ProjectArgs pr;
    double *x;             // [n][B] or null; may be c.q
    double *clearance, *violation, *moved;  // [B] or null
    int32_t *status, *iterations;           // [B] or null
};

// Steps 1 - 5 of repair_measure.hpp for the configuration x of one lane, under `box` unless free_box.
template <int N, bool TIP, class Launch>
__device__ __forceinline__ repair::Result repair_lane(const ChainDev &sch, const ModelDev &sm, const Launch &a,
                                                      const repair::Params &p, const constraint::Box &box, bool free_box,
                                                      const ProjectArgs &pr, double (&x)[N]) {
    const double e = p.influence - p.safety;
    return repair::run(
        N, sch.lb, sch.ub, p, free_box, x,
        [&](const double *xx, double *gobs) {
            double q[N];
#pragma unroll
            for (int j = 0; j < N; ++j) { q[j] = xx[j]; gobs[j] = 0.0; }
            Kin<N, TIP> kin;
            forward_kinematics<N, TIP>(sch, a.c.ep, q, kin);
            const bool nan = kin_has_nan<N, TIP>(kin);
            Rows<N> rows;
#pragma unroll
            for (int k = 0; k < N + 2; ++k) { rows.dist[k] = __builtin_huge_val(); rows.wit[k] = -1; }
            witness_pass<N, TIP>(sm, a, kin, rows);
            double best = __builtin_huge_val();
            bool row_nan = false;
            for (int f = 0; f < N + 2; ++f) {
                double d;
                int32_t w;
                row_get<N>(rows, __builtin_amdgcn_readfirstlane(f), d, w);
                if (nan) { d = __builtin_nan(""); w = -1; }
                const double cp = repair::row_take(d, p.safety, e, best, row_nan);
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
            return row_nan ? __builtin_nan("") : best;
        },
        [&](double *y) {
            return constraint::project(sch, a.c.ep, box, N, pr.tol, pr.iters, pr.damping, pr.max_step, y).status
                   == constraint::PROJECTED;
        },
        [&](const double *xx) {
            double rr[6];
            return constraint::measure(sch, a.c.ep, box, N, xx, rr);
        });
}

template <int N, bool TIP>
__global__ __launch_bounds__(256) void repair_kernel(const RepairLaunch a) {
    __shared__ ChainDev sch;
    __shared__ ModelDev sm;
    stage_chain(sch, a.c.chain);
    stage_model(sm, a.c);  // (the entry refuses a chain without a model)
    const size_t B = (size_t)a.c.B;
    const bool free_box = !a.has_box || pathopt::box_is_free(a.box.lo, a.box.hi);
    for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < a.c.B;
         b += (long long)gridDim.x * blockDim.x) {
        double x[N];
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = a.c.q[(size_t)i * B + b];
        const repair::Result r = repair_lane<N, TIP>(sch, sm, a, a.p, a.box, free_box, a.pr, x);
        if (a.x) {
#pragma unroll
            for (int i = 0; i < N; ++i) a.x[(size_t)i * B + b] = x[i];
        }
        if (a.clearance) a.clearance[b] = r.clearance;
        if (a.violation) a.violation[b] = r.violation;
        if (a.moved) a.moved[b] = r.moved;
        if (a.status) a.status[b] = r.status;
        if (a.iterations) a.iterations[b] = r.iterations;
    }
}

// The repair pass of optik_hip_ik_region_repair.
struct RegionRepairLaunch {
    CollLaunch c;            // chain, ee_offset, model, world; q and B unused
    const uint16_t *orig;
    repair::Params p;
    ProjectArgs pr;          // the region launch's: ptol = its tol
    const double *regions;   // [T][19]
    const double *x0;        // [T][n]
    unsigned long long cols, R;
    int mode, keep_on;
    constraint::Box keep;
    double keep_tol;
    double *x;               // [n][cols], in place
    double *violation, *key;  // [cols], in place
    int32_t *repaired;       // [T] or null
};

template <int N, bool TIP>
__global__ __launch_bounds__(256) void region_repair_kernel(const RegionRepairLaunch a) {
    __shared__ ChainDev sch;
    __shared__ ModelDev sm;
    stage_chain(sch, a.c.chain);
    stage_model(sm, a.c);
    for (unsigned long long b = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; b < a.cols;
         b += (unsigned long long)gridDim.x * blockDim.x) {
        const double key = a.key[b];
        if (!(key < __builtin_huge_val())) continue;  // +inf or NaN: not a candidate, left bit for bit
        const unsigned long long t = b / a.R;
        constraint::Box box;
        region::load_box(a.regions + (size_t)t * region::DOUBLES, box);
        double x[N];
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = a.x[(size_t)i * a.cols + b];
        const repair::Result r =
            repair_lane<N, TIP>(sch, sm, a, a.p, box, pathopt::box_is_free(box.lo, box.hi), a.pr, x);
        if (r.status != repair::FREE || r.iterations == 0) continue;
        // the key by region_measure.hpp's rule from the new x: Speed keeps the index, every other mode the distance
        // from x0[t] in the same summation order; then the keep box
        double nk = key;
        if (a.mode != region::MODE_SPEED) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const double d = x[k] - a.x0[(size_t)t * N + k];
                acc += d * d;
            }
            nk = __builtin_sqrt(acc);
        }
        if (a.keep_on) {
            double xx[N], rr[6];
#pragma unroll
            for (int k = 0; k < N; ++k) xx[k] = x[k];
            const double v = constraint::measure(sch, a.c.ep, a.keep, N, xx, rr);
            if (!(v <= a.keep_tol)) nk = __builtin_huge_val();
        }
#pragma unroll
        for (int i = 0; i < N; ++i) a.x[(size_t)i * a.cols + b] = x[i];
        a.violation[b] = r.violation;
        a.key[b] = nk;
        if (a.repaired) atomicAdd(a.repaired + t, 1);
    }
}

const char *const kRepairWideMsg = "collision_repair: chains of more than 8 joint positions are not supported";

}  // namespace

namespace optik {
namespace repairdev {

int check_region_repair(const optik_hip_chain *ch, const optik_hip_region_repair *rep) {
    if (ch->wide || ch->n > 8) return fail(OPTIK_HIP_EUNSUPPORTED, kRepairWideMsg);
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, prismatic_msg());
    if (!repair::params_ok(repair::Params{rep->influence, rep->safety, rep->step, rep->max_move, rep->iters}))
        return fail(OPTIK_HIP_EINVAL, "collision_repair: needs influence > safety >= 0 and step > 0, all finite, "
                                      "iters in 0 .. 4096 and max_move >= 0");
    if (ch->coll_S <= 0) return fail(OPTIK_HIP_EINVAL, "collision_repair: the chain has no collision model");
    return 0;
}

int region_repair_launch(const optik_hip_chain *ch, const double *ee_offset7, const optik_hip_region_repair *rep,
                         const double *d_regions, const double *d_x0, int32_t T, unsigned long long R, size_t cols,
                         int mode, const ProjectArgs &pr, const constraint::Box &keep_box, int keep_on, double keep_tol,
                         double *d_x, double *d_violation, double *d_key, hipStream_t stream) {
    RegionRepairLaunch a;
    std::memset(&a, 0, sizeof a);
    fill_launch(ch, ee_offset7, nullptr, 0, a.c);
    a.orig = ch->coll_orig.get();
    a.p = repair::Params{rep->influence, rep->safety, rep->step, rep->max_move, rep->iters};
    a.pr = pr;
    a.regions = d_regions; a.x0 = d_x0;
    a.cols = (unsigned long long)cols; a.R = R;
    a.mode = mode; a.keep_on = keep_on; a.keep = keep_box; a.keep_tol = keep_tol;
    a.x = d_x; a.violation = d_violation; a.key = d_key;
    a.repaired = rep->d_repaired;
    if (rep->d_repaired) HIP_TRY(hipMemsetAsync(rep->d_repaired, 0, sizeof(int32_t) * (size_t)T, stream));
    const int grid = grid_for(ch, (long long)cols, 256, 8);
#define CALL(NN, TT) hipLaunchKernelGGL((region_repair_kernel<NN, TT>), dim3(grid), dim3(256), 0, stream, a)
    OPTIK_DISPATCH(ch, CALL);
#undef CALL
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace repairdev
}  // namespace optik

extern "C" {

int optik_hip_collision_repair_batch(const optik_hip_chain *ch, const double *ee_offset7, const double *d_x, int64_t B,
                                     double influence, double safety, double step, int32_t iters, double max_move,
                                     const double *ref7, const double *lo6, const double *hi6, double ptol,
                                     int32_t piters, double damping, double project_max_step,
                                     const optik_hip_collision_repair_outputs *out, void *stream) {
    // (the chain's refusals come first, as optik_hip_path_optimize has them)
    if (!ch || B < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (ch->wide || ch->n > 8) return fail(OPTIK_HIP_EUNSUPPORTED, kRepairWideMsg);
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, prismatic_msg());
    const repair::Params prm{influence, safety, step, max_move, iters};
    if (!repair::params_ok(prm))
        return fail(OPTIK_HIP_EINVAL, "collision_repair: needs influence > safety >= 0 and step > 0, all finite, "
                                      "iters in 0 .. 4096 and max_move >= 0");
    const bool box = ref7 || lo6 || hi6;
    if (box) {
        if (int rc = check_box(ref7, lo6, hi6)) return rc;
        if (int rc = check_project_args(ptol, piters, damping, project_max_step)) return rc;
    }
    if (ch->coll_S <= 0) return fail(OPTIK_HIP_EINVAL, "collision_repair: the chain has no collision model");
    if (B == 0 || !out
        || (!out->d_x && !out->d_clearance && !out->d_violation && !out->d_moved && !out->d_status
            && !out->d_iterations))
        return 0;
    if (!d_x) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    RepairLaunch a;
    std::memset(&a, 0, sizeof a);
    fill_launch(ch, ee_offset7, d_x, B, a.c);
    a.orig = ch->coll_orig.get();
    a.p = prm;
    if (box) {
        ConstraintDev d;
        fill_constraint(ch, ee_offset7, ref7, lo6, hi6, d);
        a.has_box = 1;
        a.box = d.c;
        a.pr = ProjectArgs{ptol, damping, project_max_step, piters};
    }
    a.x = out->d_x; a.clearance = out->d_clearance; a.violation = out->d_violation; a.moved = out->d_moved;
    a.status = out->d_status; a.iterations = out->d_iterations;
    const int grid = grid_for(ch, B, 256, 8);
#define CALL(NN, TT) hipLaunchKernelGGL((repair_kernel<NN, TT>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a)
    OPTIK_DISPATCH(ch, CALL);
#undef CALL
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
