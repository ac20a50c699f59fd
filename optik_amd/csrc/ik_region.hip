// ik_region.hip -- distinct IK solutions inside a pose region (region_measure.hpp):
// optik_hip_ik_region (include/optik_hip.h).
//
//   ik_region_kernel<CH>   one restart per lane: its start (the region's x0 or the ChaCha restart seed), the damped
//                          Gauss-Newton projection of constraint_measure.hpp onto the region's box, the key and the
//                          keep-constraint; x [n][T*R], violation, status, iterations, key [T*R]
// CH is ChainDev (n <= 8) or WideChainDev (9 .. 16): one run-time-n body each, the chain table staged in LDS, as
// constraint_project_kernel (ik_constraint.hip).  A grid-stride row kernel without atomics; no lane waits for
// another, so restarts whose projections differ in length cost their wave the longest of them and nothing else.  The
// region of a row is read from device memory ([T][19]); the keep box travels with the launch (kernel arguments) as the
// box of the record's ConstraintDev head (constraint_device.hpp, whose refusals validate it).
// Behind the kernel, on the same stream: the key pass of modes 3 and 4 (ik_manip.hip), the collision filter
// (ik_collision.hip) and the selection of ik_solutions.hip, in the order ik_capi.hip runs them behind its solver.
#include "constraint_device.hpp"
#include "region_measure.hpp"
#include "repair_device.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::hostparams;
using namespace optik::condev;

namespace {

struct RegionLaunch {
    ConstraintDev d;             // d.c: the keep box (keep_on != 0)
    int keep_on;
    double keep_tol;
    uint32_t key[8];
    double scale[WIDE_MAX_DOF];
    const double *regions;       // [T][19]
    const double *x0;            // [T][n]
    unsigned long long cols, R, restart_begin;
    ProjectArgs p;
    int mode;
    double *x;                   // [n][cols]
    double *violation, *out_key;  // [cols]
    int32_t *status, *iterations;  // [cols]
};

template <class CH>
__global__ __launch_bounds__(256) void ik_region_kernel(const RegionLaunch a) {
    __shared__ CH sch;
    stage_table(sch, table_of<CH>(a.d));
    const int n = sch.n_pos;
    const region::Keep keep{a.keep_on, a.d.c, a.keep_tol};
    for (unsigned long long b = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; b < a.cols;
         b += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long t = b / a.R;
        const unsigned long long index = a.restart_begin + (b - t * a.R);
        constraint::Box box;
        region::load_box(a.regions + (size_t)t * region::DOUBLES, box);
        double x0[constraint::MAXN], x[constraint::MAXN];
        for (int i = 0; i < n; ++i) x0[i] = a.x0[(size_t)t * n + i];
        const region::Row r = region::restart(sch, a.d.ep, box, keep, a.key, a.scale, x0, index, n, a.p.tol, a.p.iters,
                                              a.p.damping, a.p.max_step, a.mode, x);
        if (a.x)
            for (int i = 0; i < n; ++i) a.x[(size_t)i * a.cols + b] = x[i];
        if (a.violation) a.violation[b] = r.violation;
        if (a.status) a.status[b] = r.status;
        if (a.iterations) a.iterations[b] = r.iterations;
        if (a.out_key) a.out_key[b] = r.key;
    }
}

// The one body of optik_hip_ik_region (rep null: not one launch more) and optik_hip_ik_region_repair.
int region_body(optik_hip_chain *ch, const double *ee_offset7, const double *d_regions, const double *d_x0, int32_t T,
                uint64_t restart_begin, uint64_t restart_end, double tol, int32_t iters, double damping, double max_step,
                int32_t mode, const double *keep_ref7, const double *keep_lo6, const double *keep_hi6, double keep_tol,
                int32_t K, double min_dist, const optik_hip_region_repair *rep, const optik_hip_ik_region_outputs *out,
                void *stream_v) {
    if (!ch || !out || T < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (restart_end <= restart_begin) return fail(OPTIK_HIP_EINVAL, "empty restart range");
    if (mode < OPTIK_MODE_QUALITY || mode > OPTIK_MODE_CONDITION)
        return fail(OPTIK_HIP_EINVAL,
                    "solution_mode must be 1 (Quality), 2 (Speed), 3 (Manipulability) or 4 (Condition)");
    // the projection's rules (optik_hip_constraint_project_batch)
    if (int rc = check_project_args(tol, iters, damping, max_step)) return rc;
    // the selection's rules (optik_hip_ik_solutions)
    if (K < 1 || K > OPTIK_HIP_MAX_SOLUTIONS) return fail(OPTIK_HIP_EINVAL, "K must be in 1..256");
    if (!(min_dist >= 0.0) || !std::isfinite(min_dist))
        return fail(OPTIK_HIP_EINVAL, "min_dist must be finite and >= 0");
    const uint64_t R = restart_end - restart_begin;
    LaunchPlan plan{};
    if (plan_selection_tiles(T, R, plan) != PLAN_OK)
        return fail(OPTIK_HIP_EINVAL, "too many restarts / targets in one launch (2^24 or more selection tiles)");
    // the keep box
    const bool keep = keep_ref7 || keep_lo6 || keep_hi6;
    if (keep) {
        if (int rc = check_box(keep_ref7, keep_lo6, keep_hi6)) return rc;
        if (int rc = check_tol(keep_tol)) return rc;
    }
    if (restart_end > 1)
        for (int k = 0; k < ch->n; ++k)
            if (std::isnan(ch->scale[k]))
            return fail(OPTIK_HIP_EINVAL, "random restarts need finite joint limits (reference: random_range panics)");
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, colldev::prismatic_msg());
    if (rep)
        if (int rc = repairdev::check_region_repair(ch, rep)) return rc;
    if (T == 0) return 0;
    if (!d_regions || !d_x0) return fail(OPTIK_HIP_EINVAL, "bad argument");

    std::lock_guard<std::mutex> lock(ch->mu);
    hipStream_t stream = (hipStream_t)stream_v;
    const bool manip = mode == OPTIK_MODE_MANIPULABILITY || mode == OPTIK_MODE_CONDITION;
    const bool coll = ch->coll_S > 0;
    const size_t cols = (size_t)plan.cols;

    // the workspace, as solve_locked (ik_capi.hip) keeps it: tmp_x and tmp_f follow tmp_key's capacity.  The keys
    // always live there -- the multi-tile selection uses them as scratch --; x and the violation when the caller
    // gives no buffer (the selection reads both: the violation goes into the selection's f slot)
    BIND_DEVICE(ch);
    if (ch->claim_pending && stream != nullptr) { HIP_TRY(hipStreamSynchronize(nullptr)); ch->claim_pending = false; }
    HIP_TRY(ch->tile_recs.reserve((size_t)plan.n_tiles));
    if (plan.tiles_per_target > 1) HIP_TRY(ch->sol_pick.reserve((size_t)T));
    if (cols > ch->tmp_key.capacity()) {
        HIP_TRY(ch->tmp_x.reset());
        HIP_TRY(ch->tmp_f.reset());
        HIP_TRY(ch->tmp_key.reserve(cols));
    }
    if (!out->d_x) HIP_TRY(ch->tmp_x.reserve(ch->tmp_key.capacity() * (size_t)ch->n));
    if (!out->d_violation) HIP_TRY(ch->tmp_f.reserve(ch->tmp_key.capacity()));
    double *px = out->d_x ? out->d_x : ch->tmp_x.get();
    double *pv = out->d_violation ? out->d_violation : ch->tmp_f.get();
    double *pk = ch->tmp_key.get();

    RegionLaunch a;
    std::memset(&a, 0, sizeof a);
    fill_constraint(ch, ee_offset7, keep ? keep_ref7 : nullptr, keep_lo6, keep_hi6, a.d);
    a.keep_on = keep ? 1 : 0;
    a.keep_tol = keep ? keep_tol : 0.0;
    std::memcpy(a.key, ch->key, sizeof a.key);
    std::memcpy(a.scale, ch->scale, sizeof a.scale);
    a.regions = d_regions;
    a.x0 = d_x0;
    a.cols = (unsigned long long)cols;
    a.R = R;
    a.restart_begin = restart_begin;
    a.p = ProjectArgs{tol, damping, max_step, iters};
    a.mode = mode;
    a.x = px; a.violation = pv; a.out_key = pk;
    a.status = out->d_status; a.iterations = out->d_iterations;
    const int grid = grid_for(ch, (long long)cols, 256, 8);
    CONSTRAINT_LAUNCH(ik_region_kernel, ch, grid, 256, stream, a);
    // the repair pass: between the region kernel and the key passes, on the same stream
    if (rep)
        if (int rc = repairdev::region_repair_launch(ch, ee_offset7, rep, d_regions, d_x0, T, R, cols, mode, a.p, a.d.c,
                                                     a.keep_on, a.keep_tol, px, pv, pk, stream))
            return rc;
    // the key passes, in ik_capi.hip's order: modes 3 and 4, then the collision filter
    if (manip)
        if (int rc = manip_key_launch(ch, mode, ee_offset7, px, pk, cols, stream)) return rc;
    if (coll)
        if (int rc = collision_key_launch(ch, ee_offset7, px, pk, cols, stream)) return rc;
    if (out->d_key) HIP_TRY(hipMemcpyAsync(out->d_key, pk, sizeof(double) * cols, hipMemcpyDeviceToDevice, stream));
    ch->last.grid = grid; ch->last.block = 256; ch->last.lds_bytes = (int)(ch->wide ? sizeof(WideChainDev) : sizeof(ChainDev));
    ch->last.tiles = plan.n_tiles;

    if (out->d_count || out->d_sol_x || out->d_sol_violation || out->d_sol_idx || out->d_sol_key) {
        optik_hip_ik_solutions_outputs so;
        so.d_count = out->d_count; so.d_x = out->d_sol_x; so.d_f = out->d_sol_violation;
        so.d_idx = out->d_sol_idx; so.d_key = out->d_sol_key;
        const SelectionIn in{pk, px, pv, restart_begin, R, plan.tiles_per_target, cols};
        // (the work-item counter of the solver launches is not used here and stays as it is)
        HIP_TRY(solutions_launch(make_solutions_launch(ch, in, K, min_dist, &so, nullptr), T, stream));
    }
    return 0;
}

}  // namespace

extern "C" {

int optik_hip_ik_region(optik_hip_chain *ch, const double *ee_offset7, const double *d_regions, const double *d_x0,
                        int32_t T, uint64_t restart_begin, uint64_t restart_end, double tol, int32_t iters,
                        double damping, double max_step, int32_t mode, const double *keep_ref7, const double *keep_lo6,
                        const double *keep_hi6, double keep_tol, int32_t K, double min_dist,
                        const optik_hip_ik_region_outputs *out, void *stream_v) {
    return region_body(ch, ee_offset7, d_regions, d_x0, T, restart_begin, restart_end, tol, iters, damping, max_step,
                       mode, keep_ref7, keep_lo6, keep_hi6, keep_tol, K, min_dist, nullptr, out, stream_v);
}

int optik_hip_ik_region_repair(optik_hip_chain *ch, const double *ee_offset7, const double *d_regions,
                               const double *d_x0, int32_t T, uint64_t restart_begin, uint64_t restart_end, double tol,
                               int32_t iters, double damping, double max_step, int32_t mode, const double *keep_ref7,
                               const double *keep_lo6, const double *keep_hi6, double keep_tol, int32_t K,
                               double min_dist, const optik_hip_region_repair *repair,
                               const optik_hip_ik_region_outputs *out, void *stream_v) {
    return region_body(ch, ee_offset7, d_regions, d_x0, T, restart_begin, restart_end, tol, iters, damping, max_step,
                       mode, keep_ref7, keep_lo6, keep_hi6, keep_tol, K, min_dist, repair, out, stream_v);
}

}  // extern "C"
