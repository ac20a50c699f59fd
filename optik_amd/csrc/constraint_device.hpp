// constraint_device.hpp -- the device side of a pose constraint that its translation units share: the head of their
// launch records, the choice of the chain table, the refusals of a box and of the projection's arguments, and the
// dispatch on the chain's kind.
//
//   ik_constraint.hip      residual, projection, the check along a motion and its mask form
//   ik_region.hip          restarts projected onto a row's region; the record's box is the keep box
//   ik_rrt.hip             the projection inside the tree planner's extension
//   ik_shortcut.hip        projected vertices and resampled waypoints
//   ik_path_optimize.hip   the projection behind every step of the smoothing (the box and ProjectArgs only: the
//                          chain and ee_offset are CollLaunch's there)
//
// All of them run constraint_measure.hpp's functions on a chain table staged in LDS (stage_table, ik_launch.hpp), so a
// configuration has the same bits in every one of them.  The constraint travels with the launch (kernel arguments);
// the chain handle keeps nothing of it.
#pragma once

#include "collision_device.hpp"
#include "constraint_measure.hpp"

namespace optik {
namespace condev {

using namespace optik::host;
using namespace optik::hostparams;

// What every constrained launch record opens with.
struct ConstraintDev {
    const ChainDev *chain;       // n <= 8
    const WideChainDev *wchain;  // 9 .. 16 joint positions
    EvalParams ep;               // only the ee_offset part is used
    constraint::Box c;
};

// The arguments of constraint::project.
struct ProjectArgs {
    double tol, damping, max_step;
    int iters;
};

// CH is ChainDev (n <= 8) or WideChainDev (9 .. 16): one run-time-n body each.
template <class CH>
__device__ __forceinline__ const CH *table_of(const ConstraintDev &d);
template <>
__device__ __forceinline__ const ChainDev *table_of<ChainDev>(const ConstraintDev &d) { return d.chain; }
template <>
__device__ __forceinline__ const WideChainDev *table_of<WideChainDev>(const ConstraintDev &d) { return d.wchain; }

template <class CH>
__device__ __forceinline__ constraint::Projected project(const CH &sch, const ConstraintDev &d, const ProjectArgs &p,
                                                         int n, double *x) {
    return constraint::project(sch, d.ep, d.c, n, p.tol, p.iters, p.damping, p.max_step, x);
}

// ---- the host's side: every refusal is 0 or a fail() code, in the order the entries of ik_constraint.hip keep ----

inline int check_box(const double *ref7, const double *lo6, const double *hi6) {
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
    return 0;
}

inline int check_tol(double tol) {
    if (!(tol >= 0.0) || !std::isfinite(tol))
        return fail(OPTIK_HIP_EINVAL, "pose constraint: tol must be finite and >= 0");
    return 0;
}

inline int check_project_args(double tol, int32_t iters, double damping, double max_step) {
    if (int rc = check_tol(tol)) return rc;
    if (iters < 0 || iters > OPTIK_HIP_CONSTRAINT_MAX_ITERS)
        return fail(OPTIK_HIP_EINVAL, "pose constraint: iters must be 0 .. 4096");
    if (!(damping >= 0.0) || !std::isfinite(damping) || !(max_step > 0.0) || !std::isfinite(max_step))
        return fail(OPTIK_HIP_EINVAL, "pose constraint: needs damping >= 0 and max_step > 0, both finite");
    return 0;
}

// The chain's tables and the box as a launch sees them.  ref7 null: no box (ik_region.hip without a keep box).
inline void fill_constraint(const optik_hip_chain *ch, const double *ee_offset7, const double *ref7, const double *lo6,
                            const double *hi6, ConstraintDev &d) {
    std::memset(&d, 0, sizeof d);
    d.chain = ch->dev;
    d.wchain = ch->wdev;
    const double one[3] = {1, 1, 1};
    make_eval_params(one, one, ee_offset7, d.ep);
    if (!ref7) return;
    std::memcpy(d.c.ref, ref7, sizeof d.c.ref);
    std::memcpy(d.c.lo, lo6, sizeof d.c.lo);
    std::memcpy(d.c.hi, hi6, sizeof d.c.hi);
}

// KERNEL<WideChainDev> or KERNEL<ChainDev> by the chain's kind, and the launch's own error.
#define CONSTRAINT_LAUNCH(KERNEL, CHAIN, GRID, BLOCK, STREAM, ...)                                                      \
    do {                                                                                                                \
        if ((CHAIN)->wide) hipLaunchKernelGGL(KERNEL<WideChainDev>, dim3(GRID), dim3(BLOCK), 0, (STREAM), __VA_ARGS__); \
        else hipLaunchKernelGGL(KERNEL<ChainDev>, dim3(GRID), dim3(BLOCK), 0, (STREAM), __VA_ARGS__);                   \
        HIP_TRY(hipGetLastError());                                                                                     \
    } while (0)

}  // namespace condev
}  // namespace optik
