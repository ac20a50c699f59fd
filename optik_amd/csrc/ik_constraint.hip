// ik_constraint.hip -- pose constraints on the device (constraint_measure.hpp): the residual
// and violation of configurations against a box on the pose error, their projection onto it, and the check of the box
// along straight joint-space motions.  optik_hip_constraint_batch, optik_hip_constraint_project_batch,
// optik_hip_constraint_motion_batch and optik_hip_constraint_motion_mask (include/optik_hip.h).
//
//   constraint_kernel<CH>          one row per lane: FK, error, residual [6][B], violation [B]
//   constraint_project_kernel<CH>  one row per lane: the damped Gauss-Newton loop of the header, x [n][B], violation,
//                                  status, iterations [B]
//   constraint_motion_kernel<CH>   one segment per lane: its K + 1 samples in turn, violation, ok, first, steps [B]
//   constraint_motion_mask_kernel<CH>  the same body (motion_body) with another store: a segment whose flag is 0
//                                  already is not sampled, every other flag becomes the motion's ok.  The shortcutter
//                                  reaches it through constraint_mask_launch (ik_host.hpp).
// CH is ChainDev (n <= 8) or WideChainDev (9 .. 16): one run-time-n body each, the chain table staged in LDS.  All four
// are grid-stride row kernels without atomics; no lane waits for another, so rows whose loops differ in length (the
// projection's iterations, a motion's samples) cost their wave the longest of them and nothing else.  The record's
// head, the refusals of a box and the dispatch on CH are constraint_device.hpp's, shared with the other users of a
// constraint.
#include "constraint_device.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::hostparams;
using namespace optik::condev;

namespace {

struct ConstraintLaunch {
    ConstraintDev d;
    const double *q;             // [n][B]: the configurations (motion: qa)
    const double *qb;            // motion: [n][B]
    long long B;
    ProjectArgs p;               // project
    double h, tol;               // motion: the resolution, the violation a sample may have
    double *residual;            // [6][B]
    double *violation;           // [B]
    double *x;                   // project: [n][B]
    int32_t *status, *iterations;  // project: [B]
    uint8_t *ok;                 // motion: [B]; the mask form reads it first
    int32_t *first, *steps;      // motion: [B]
};

template <class CH>
__global__ __launch_bounds__(256) void constraint_kernel(const ConstraintLaunch a) {
    __shared__ CH sch;
    stage_table(sch, table_of<CH>(a.d));
    const int n = sch.n_pos;
    for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < a.B;
         b += (long long)gridDim.x * blockDim.x) {
        double q[constraint::MAXN], r[6];
        for (int i = 0; i < n; ++i) q[i] = a.q[(size_t)i * a.B + b];
        const double v = constraint::measure(sch, a.d.ep, a.d.c, n, q, r);
        if (a.residual)
            for (int i = 0; i < 6; ++i) a.residual[(size_t)i * a.B + b] = r[i];
        if (a.violation) a.violation[b] = v;
    }
}

template <class CH>
__global__ __launch_bounds__(256) void constraint_project_kernel(const ConstraintLaunch a) {
    __shared__ CH sch;
    stage_table(sch, table_of<CH>(a.d));
    const int n = sch.n_pos;
    for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < a.B;
         b += (long long)gridDim.x * blockDim.x) {
        double x[constraint::MAXN];
        for (int i = 0; i < n; ++i) x[i] = a.q[(size_t)i * a.B + b];
        const constraint::Projected p = project(sch, a.d, a.p, n, x);
        if (a.x)
            for (int i = 0; i < n; ++i) a.x[(size_t)i * a.B + b] = x[i];
        if (a.violation) a.violation[b] = p.violation;
        if (a.status) a.status[b] = p.status;
        if (a.iterations) a.iterations[b] = p.iterations;
    }
}

// MASK: a.ok [B] is read and written in place, nothing else is stored.
template <class CH, bool MASK>
__device__ __forceinline__ void motion_body(const ConstraintLaunch &a) {
    __shared__ CH sch;
    stage_table(sch, table_of<CH>(a.d));
    const int n = sch.n_pos;
    for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < a.B;
         b += (long long)gridDim.x * blockDim.x) {
        if constexpr (MASK)
            if (a.ok[b] == 0) continue;  // (the verdict is the AND; the skip only saves the samples)
        const constraint::MotionResult m =
            constraint::motion(sch, a.d.ep, a.d.c, n, a.q + b, a.B, a.qb + b, a.B, a.h, a.tol);
        if constexpr (MASK) {
            a.ok[b] = (uint8_t)m.ok;
        } else {
            if (a.violation) a.violation[b] = m.violation;
            if (a.ok) a.ok[b] = (uint8_t)m.ok;
            if (a.first) a.first[b] = m.first;
            if (a.steps) a.steps[b] = m.steps;
        }
    }
}

template <class CH>
__global__ __launch_bounds__(256) void constraint_motion_kernel(const ConstraintLaunch a) { motion_body<CH, false>(a); }

template <class CH>
__global__ __launch_bounds__(256) void constraint_motion_mask_kernel(const ConstraintLaunch a) { motion_body<CH, true>(a); }

// The refusals every entry shares, in this order: the handle, the constraint, tol, the chain.  0 or a fail() code.
int check_call(const optik_hip_chain *ch, const double *ref7, const double *lo6, const double *hi6, double tol,
               int64_t B) {
    if (!ch || B < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (int rc = check_box(ref7, lo6, hi6)) return rc;
    if (int rc = check_tol(tol)) return rc;
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, colldev::prismatic_msg());
    return 0;
}

void fill(const optik_hip_chain *ch, const double *ee_offset7, const double *ref7, const double *lo6,
          const double *hi6, int64_t B, ConstraintLaunch &a) {
    std::memset(&a, 0, sizeof a);
    fill_constraint(ch, ee_offset7, ref7, lo6, hi6, a.d);
    a.B = B;
}

}  // namespace

namespace optik {
namespace host {

int constraint_mask_launch(const optik_hip_chain *ch, const double *ee_offset7, const double *ref7, const double *lo6,
                           const double *hi6, const double *qa, const double *qb, long long B, double resolution,
                           double tol, uint8_t *flag, hipStream_t stream) {
    BIND_DEVICE(ch);
    ConstraintLaunch a;
    fill(ch, ee_offset7, ref7, lo6, hi6, B, a);
    a.q = qa;
    a.qb = qb;
    a.h = resolution;
    a.tol = tol;
    a.ok = flag;
    CONSTRAINT_LAUNCH(constraint_motion_mask_kernel, ch, grid_for(ch, B, 256, 8), 256, stream, a);
    return 0;
}

}  // namespace host
}  // namespace optik

extern "C" {

int optik_hip_constraint_batch(const optik_hip_chain *ch, const double *ee_offset7, const double *ref7,
                               const double *lo6, const double *hi6, const double *d_q, int64_t B,
                               double *d_residual, double *d_violation, void *stream) {
    if (int rc = check_call(ch, ref7, lo6, hi6, 0.0, B)) return rc;
    if (B == 0 || (!d_residual && !d_violation)) return 0;
    if (!d_q) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    ConstraintLaunch a;
    fill(ch, ee_offset7, ref7, lo6, hi6, B, a);
    a.q = d_q;
    a.residual = d_residual;
    a.violation = d_violation;
    CONSTRAINT_LAUNCH(constraint_kernel, ch, grid_for(ch, B, 256, 8), 256, (hipStream_t)stream, a);
    return 0;
}

int optik_hip_constraint_project_batch(const optik_hip_chain *ch, const double *ee_offset7, const double *ref7,
                                       const double *lo6, const double *hi6, const double *d_q, int64_t B, double tol,
                                       int32_t iters, double damping, double max_step, double *d_x,
                                       double *d_violation, int32_t *d_status, int32_t *d_iterations, void *stream) {
    if (int rc = check_call(ch, ref7, lo6, hi6, tol, B)) return rc;
    if (int rc = check_project_args(tol, iters, damping, max_step)) return rc;
    if (B == 0 || (!d_x && !d_violation && !d_status && !d_iterations)) return 0;
    if (!d_q) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    ConstraintLaunch a;
    fill(ch, ee_offset7, ref7, lo6, hi6, B, a);
    a.q = d_q;
    a.p = ProjectArgs{tol, damping, max_step, iters};
    a.x = d_x;
    a.violation = d_violation;
    a.status = d_status;
    a.iterations = d_iterations;
    CONSTRAINT_LAUNCH(constraint_project_kernel, ch, grid_for(ch, B, 256, 8), 256, (hipStream_t)stream, a);
    return 0;
}

int optik_hip_constraint_motion_batch(const optik_hip_chain *ch, const double *ee_offset7, const double *ref7,
                                      const double *lo6, const double *hi6, const double *d_qa, const double *d_qb,
                                      int64_t B, double resolution, double tol, double *d_violation, uint8_t *d_ok,
                                      int32_t *d_first, int32_t *d_steps, void *stream) {
    if (int rc = check_call(ch, ref7, lo6, hi6, tol, B)) return rc;
    if (!(resolution > 0.0) || !std::isfinite(resolution))
        return fail(OPTIK_HIP_EINVAL, "motion resolution must be finite and > 0");
    if (B == 0 || (!d_violation && !d_ok && !d_first && !d_steps)) return 0;
    if (!d_qa || !d_qb) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    ConstraintLaunch a;
    fill(ch, ee_offset7, ref7, lo6, hi6, B, a);
    a.q = d_qa;
    a.qb = d_qb;
    a.h = resolution;
    a.tol = tol;
    a.violation = d_violation;
    a.ok = d_ok;
    a.first = d_first;
    a.steps = d_steps;
    CONSTRAINT_LAUNCH(constraint_motion_kernel, ch, grid_for(ch, B, 256, 8), 256, (hipStream_t)stream, a);
    return 0;
}

int optik_hip_constraint_motion_mask(const optik_hip_chain *ch, const double *ee_offset7, const double *ref7,
                                     const double *lo6, const double *hi6, const double *d_qa, const double *d_qb,
                                     int64_t B, double resolution, double tol, uint8_t *d_flag, void *stream) {
    // (B = 0: optik_hip_constraint_motion_batch's own refusals)
    if (int rc = optik_hip_constraint_motion_batch(ch, nullptr, ref7, lo6, hi6, nullptr, nullptr, 0, resolution, tol,
                                                   nullptr, nullptr, nullptr, nullptr, nullptr))
        return rc;
    if (B < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (B == 0) return 0;
    if (!d_qa || !d_qb || !d_flag) return fail(OPTIK_HIP_EINVAL, "bad argument");
    return constraint_mask_launch(ch, ee_offset7, ref7, lo6, hi6, d_qa, d_qb, B, resolution, tol, d_flag,
                                  (hipStream_t)stream);
}

}  // extern "C"
