// ik_constraint.hip -- pose constraints on the device (constraint_measure.hpp): the residual
// and violation of configurations against a box on the pose error, their projection onto it, and the check of the box
// along straight joint-space motions.  optik_hip_constraint_batch, optik_hip_constraint_project_batch and
// optik_hip_constraint_motion_batch (include/optik_hip.h).
//
//   constraint_kernel<CH>          one row per lane: FK, error, residual [6][B], violation [B]
//   constraint_project_kernel<CH>  one row per lane: the damped Gauss-Newton loop of the header, x [n][B], violation,
//                                  status, iterations [B]
//   constraint_motion_kernel<CH>   one segment per lane: its K + 1 samples in turn, violation, ok, first, steps [B]
// CH is ChainDev (n <= 8) or WideChainDev (9 .. 16): one run-time-n body each, the chain table staged in LDS.  All three
// are grid-stride row kernels without atomics; no lane waits for another, so rows whose loops differ in length (the
// projection's iterations, a motion's samples) cost their wave the longest of them and nothing else.  The constraint
// travels with the launch (kernel arguments); the chain handle keeps nothing of it.
#include "collision_device.hpp"
#include "constraint_measure.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::hostparams;

namespace {

struct ConstraintLaunch {
    const ChainDev *chain;       // n <= 8
    const WideChainDev *wchain;  // 9 .. 16 joint positions
    EvalParams ep;               // only the ee_offset part is used
    constraint::Box c;
    const double *q;             // [n][B]: the configurations (motion: qa)
    const double *qb;            // motion: [n][B]
    long long B;
    double tol, damping, max_step, h;
    int iters;
    double *residual;            // [6][B]
    double *violation;           // [B]
    double *x;                   // project: [n][B]
    int32_t *status, *iterations;  // project: [B]
    uint8_t *ok;                 // motion: [B]
    int32_t *first, *steps;      // motion: [B]
};

template <class CH>
__device__ __forceinline__ const CH *table_of(const ConstraintLaunch &a);
template <>
__device__ __forceinline__ const ChainDev *table_of<ChainDev>(const ConstraintLaunch &a) { return a.chain; }
template <>
__device__ __forceinline__ const WideChainDev *table_of<WideChainDev>(const ConstraintLaunch &a) { return a.wchain; }

template <class CH>
__device__ __forceinline__ void stage_table(CH &dst, const CH *src) {
    constexpr int ND = (int)(sizeof(CH) / sizeof(double));
    static_assert(sizeof(CH) % sizeof(double) == 0, "the chain table is a whole number of doubles");
    const double *s = reinterpret_cast<const double *>(src);
    double *d = reinterpret_cast<double *>(&dst);
    for (int i = threadIdx.x; i < ND; i += blockDim.x) d[i] = s[i];
    __syncthreads();
}

template <class CH>
__global__ __launch_bounds__(256) void constraint_kernel(const ConstraintLaunch a) {
    __shared__ CH sch;
    stage_table(sch, table_of<CH>(a));
    const int n = sch.n_pos;
    for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < a.B;
         b += (long long)gridDim.x * blockDim.x) {
        double q[constraint::MAXN], r[6];
        for (int i = 0; i < n; ++i) q[i] = a.q[(size_t)i * a.B + b];
        const double v = constraint::measure(sch, a.ep, a.c, n, q, r);
        if (a.residual)
            for (int i = 0; i < 6; ++i) a.residual[(size_t)i * a.B + b] = r[i];
        if (a.violation) a.violation[b] = v;
    }
}

template <class CH>
__global__ __launch_bounds__(256) void constraint_project_kernel(const ConstraintLaunch a) {
    __shared__ CH sch;
    stage_table(sch, table_of<CH>(a));
    const int n = sch.n_pos;
    for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < a.B;
         b += (long long)gridDim.x * blockDim.x) {
        double x[constraint::MAXN];
        for (int i = 0; i < n; ++i) x[i] = a.q[(size_t)i * a.B + b];
        const constraint::Projected p =
            constraint::project(sch, a.ep, a.c, n, a.tol, a.iters, a.damping, a.max_step, x);
        if (a.x)
            for (int i = 0; i < n; ++i) a.x[(size_t)i * a.B + b] = x[i];
        if (a.violation) a.violation[b] = p.violation;
        if (a.status) a.status[b] = p.status;
        if (a.iterations) a.iterations[b] = p.iterations;
    }
}

template <class CH>
__global__ __launch_bounds__(256) void constraint_motion_kernel(const ConstraintLaunch a) {
    __shared__ CH sch;
    stage_table(sch, table_of<CH>(a));
    const int n = sch.n_pos;
    for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < a.B;
         b += (long long)gridDim.x * blockDim.x) {
        const constraint::MotionResult m =
            constraint::motion(sch, a.ep, a.c, n, a.q + b, a.B, a.qb + b, a.B, a.h, a.tol);
        if (a.violation) a.violation[b] = m.violation;
        if (a.ok) a.ok[b] = (uint8_t)m.ok;
        if (a.first) a.first[b] = m.first;
        if (a.steps) a.steps[b] = m.steps;
    }
}

// The refusals every entry shares, in this order: the handle, the constraint, tol, the chain.  0 or a fail() code.
int check_call(const optik_hip_chain *ch, const double *ref7, const double *lo6, const double *hi6, double tol,
               int64_t B) {
    if (!ch || B < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (!ref7 || !lo6 || !hi6) return fail(OPTIK_HIP_EINVAL, "pose constraint: null reference or bounds");
    double n2 = 0.0;
    for (int i = 0; i < 7; ++i) {
        if (!std::isfinite(ref7[i])) return fail(OPTIK_HIP_EINVAL, "pose constraint: the reference pose must be finite");
        if (i >= 3) n2 += ref7[i] * ref7[i];
    }
    // (the tolerance the Python layer applies to a target's rotation: 100 machine epsilons)
    if (!(std::fabs(n2 - 1.0) <= 100.0 * 2.220446049250313e-16))
        return fail(OPTIK_HIP_EINVAL, "pose constraint: the reference quaternion must have unit norm");
    for (int i = 0; i < 6; ++i)
        if (!(lo6[i] <= hi6[i])) return fail(OPTIK_HIP_EINVAL, "pose constraint: needs lo <= hi on every axis, no NaN");
    if (!(tol >= 0.0) || !std::isfinite(tol))
        return fail(OPTIK_HIP_EINVAL, "pose constraint: tol must be finite and >= 0");
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, colldev::prismatic_msg());
    return 0;
}

void fill(const optik_hip_chain *ch, const double *ee_offset7, const double *ref7, const double *lo6,
          const double *hi6, int64_t B, ConstraintLaunch &a) {
    std::memset(&a, 0, sizeof a);
    a.chain = ch->dev;
    a.wchain = ch->wdev;
    const double one[3] = {1, 1, 1};
    make_eval_params(one, one, ee_offset7, a.ep);
    std::memcpy(a.c.ref, ref7, sizeof a.c.ref);
    std::memcpy(a.c.lo, lo6, sizeof a.c.lo);
    std::memcpy(a.c.hi, hi6, sizeof a.c.hi);
    a.B = B;
}

#define CONSTRAINT_LAUNCH(KERNEL, CHAIN, A, STREAM)                                                              \
    do {                                                                                                         \
        const int grid_ = grid_for((CHAIN), (A).B, 256, 8);                                                      \
        if ((CHAIN)->wide) hipLaunchKernelGGL(KERNEL<WideChainDev>, dim3(grid_), dim3(256), 0, (STREAM), (A));   \
        else hipLaunchKernelGGL(KERNEL<ChainDev>, dim3(grid_), dim3(256), 0, (STREAM), (A));                     \
        HIP_TRY(hipGetLastError());                                                                              \
    } while (0)

}  // namespace

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
    CONSTRAINT_LAUNCH(constraint_kernel, ch, a, (hipStream_t)stream);
    return 0;
}

int optik_hip_constraint_project_batch(const optik_hip_chain *ch, const double *ee_offset7, const double *ref7,
                                       const double *lo6, const double *hi6, const double *d_q, int64_t B, double tol,
                                       int32_t iters, double damping, double max_step, double *d_x,
                                       double *d_violation, int32_t *d_status, int32_t *d_iterations, void *stream) {
    if (int rc = check_call(ch, ref7, lo6, hi6, tol, B)) return rc;
    if (iters < 0 || iters > OPTIK_HIP_CONSTRAINT_MAX_ITERS)
        return fail(OPTIK_HIP_EINVAL, "pose constraint: iters must be 0 .. 4096");
    if (!(damping >= 0.0) || !std::isfinite(damping) || !(max_step > 0.0) || !std::isfinite(max_step))
        return fail(OPTIK_HIP_EINVAL, "pose constraint: needs damping >= 0 and max_step > 0, both finite");
    if (B == 0 || (!d_x && !d_violation && !d_status && !d_iterations)) return 0;
    if (!d_q) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    ConstraintLaunch a;
    fill(ch, ee_offset7, ref7, lo6, hi6, B, a);
    a.q = d_q;
    a.tol = tol;
    a.iters = iters;
    a.damping = damping;
    a.max_step = max_step;
    a.x = d_x;
    a.violation = d_violation;
    a.status = d_status;
    a.iterations = d_iterations;
    CONSTRAINT_LAUNCH(constraint_project_kernel, ch, a, (hipStream_t)stream);
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
    CONSTRAINT_LAUNCH(constraint_motion_kernel, ch, a, (hipStream_t)stream);
    return 0;
}

}  // extern "C"
