// ik_jacobian.hpp -- the body Jacobian device code that the batch kernels share (joint_jacobian, kinematics.rs:166-196):
// fk_batch_kernel and diff_ik_batch_kernel (ik_batch_ops.hip), wide_fk_batch_kernel (ik_wide_kernel.hip) and the
// manipulability kernels (ik_manip.hip).  The same operations on the same operands in every one of them, so the same
// bits: column k = (linear, angular) in the end-effector frame.
#pragma once

#include "ik_platform.hpp"

#include "ik_launch.hpp"
#include "ik_wide_launch.hpp"

namespace optik {

// Column k of the body Jacobian of a chain of N joint positions, from its forward kinematics.
template <int N, bool TIP>
__device__ __forceinline__ void jacobian_column(const ChainDev &sch, const Kin<N, TIP> &kin, const Q4 eeqc, int k,
                                                double (&c6)[6]) {
    const V3 ax{sch.axis[k][0], sch.axis[k][1], sch.axis[k][2]};
    const V3 angular = qrot(kin.tf[k].q, ax);
    const V3 d{kin.ee.t.x - kin.tf[k].t.x, kin.ee.t.y - kin.tf[k].t.y, kin.ee.t.z - kin.tf[k].t.z};
    const V3 linear = cross(angular, d);
    const V3 al = qrot(eeqc, angular);
    const V3 ll = qrot(eeqc, linear);
    c6[0] = ll.x; c6[1] = ll.y; c6[2] = ll.z; c6[3] = al.x; c6[4] = al.y; c6[5] = al.z;
}

// The same for a wide chain (9 .. 16 joint positions): tf = the joint frames wide_forward wrote (7 per joint:
// t, then the quaternion i, j, k, w), ee = its end-effector pose, eeqc = conj(ee.q).
__device__ __forceinline__ void wide_jacobian_column(const WideChainDev &sch, const double *tf, const Pose &ee,
                                                     const Q4 eeqc, int k, double (&c6)[6]) {
    const V3 tk{tf[7 * k + 0], tf[7 * k + 1], tf[7 * k + 2]};
    const Q4 tq{tf[7 * k + 3], tf[7 * k + 4], tf[7 * k + 5], tf[7 * k + 6]};
    const V3 ax{sch.axis[k][0], sch.axis[k][1], sch.axis[k][2]};
    const V3 angular = qrot(tq, ax);
    const V3 d{ee.t.x - tk.x, ee.t.y - tk.y, ee.t.z - tk.z};
    const V3 linear = cross(angular, d);
    const V3 al = qrot(eeqc, angular);
    const V3 ll = qrot(eeqc, linear);
    c6[0] = ll.x; c6[1] = ll.y; c6[2] = ll.z; c6[3] = al.x; c6[4] = al.y; c6[5] = al.z;
}

// A wide chain's table into the block's LDS copy.
__device__ __forceinline__ void stage_wide_chain(WideChainDev &dst, const WideChainDev *src) { stage_table(dst, src); }

}  // namespace optik
