// region_measure.hpp -- one restart of IK into a pose region: the restart's start, its projection onto the region's
// box, the selection key and the optional keep-constraint; one source for the host and the device
// (optik_hip_ik_region, optik_hip.h; ik_region.hip).
//
// A region is 19 doubles, constraint::Box laid out flat: ref[7] (t, quaternion i j k w), lo[6], hi[6].  Nothing here
// validates it: a NaN in a region's reference gives a NaN error, so a NaN violation, so FAILED rows
// (constraint_measure.hpp steps 2 - 4 and 6 b), whose key is +inf; a NaN bound makes step 3's comparison false, so it
// bounds nothing on its side.  The chain has 1 <= n <= constraint::MAXN revolute joints; CH is ChainDev or
// WideChainDev (or any table with their members).  The exact operation order for region t and restart index i (the
// tests depend on it; -ffp-contract=off on both sides):
//
//  1. Start (region::seed for i > 0).  i == 0: x_k = x0[t][k].  i > 0: the restart seed of ChaCha stream i, the row
//     optik_hip_seed_batch(first = i, count = 1) writes, the same for every region: for k0 = 0, 8, .. < n the block
//     chacha8_block(key, k0 / 8, i), and for k = k0 .. min(k0 + 8, n) - 1 bits = blk[2 (k - k0)] | blk[2 (k - k0) + 1]
//     << 32, x_k = uniform_inclusive(lb_k, scale_k, bits) -- ik_solve.hpp's restart_seed<N> for n <= 8 (one block) and
//     ik_wide.hpp's wide_restart_seed for 9 .. 16 (two), restated with n at run time.
//  2. Projection: constraint::project(ch, ep, box_t, n, tol, iters, damping, max_step, x), unchanged
//     (constraint_measure.hpp step 6): x, violation, status (constraint::PROJECTED, BUDGET_SPENT, FAILED) and
//     iterations.
//  3. Key.  +inf unless the status is PROJECTED.  Otherwise, Speed (mode 2): (double)i.  Every other mode (Quality 1,
//     and Manipulability 3 and Condition 4, whose keys the key pass of ik_manip.hip replaces afterwards): acc = 0,
//     then for k ascending d = x_k - x0[t][k], acc = acc + d * d; key = sqrt(acc) -- the Quality key of the IK solvers
//     (ik_lane64.hpp, "selection key"), with the projected x in the place of the solver's best x.
//  4. Keep (region::Keep, on != 0): v = constraint::measure(ch, ep, keep.box, n, x, r) at the projected x (steps 1 - 4
//     of constraint_measure.hpp); the key becomes +inf where v <= keep.tol is false (a NaN v included).  Nothing is
//     projected onto the keep box, and x, violation, status and iterations stay as step 2 left them.  It is evaluated
//     only for a row whose key is finite: the result is the same.
//
// Plain host C++ compiles this header too, under OPTIK_LANE_EMU as ik_math.hpp needs it (tests/region_util.py).
#pragma once

#include "constraint_measure.hpp"
#include "ik_solve.hpp"

namespace optik {
namespace region {

constexpr int DOUBLES = 19;   // ref[7], lo[6], hi[6]
constexpr int MODE_SPEED = 2;  // OPTIK_MODE_SPEED (optik_hip.h)

struct Keep {
    int on;
    constraint::Box box;
    double tol;
};

struct Row {
    double violation, key;
    int status, iterations;
};

// A region's 19 doubles as a box.
template <class P>
OPTIK_DEV void load_box(P reg, constraint::Box &b) {
    for (int i = 0; i < 7; ++i) b.ref[i] = reg[i];
    for (int i = 0; i < 6; ++i) b.lo[i] = reg[7 + i];
    for (int i = 0; i < 6; ++i) b.hi[i] = reg[13 + i];
}

// Step 1, i > 0.
OPTIK_DEV void seed(const uint32_t (&key)[8], const double *lb, const double *scale, uint64_t index, int n, double *x) {
    uint32_t blk[16];
#pragma unroll 1
    for (int k0 = 0; k0 < n; k0 += 8) {
        chacha8_block(key, (uint64_t)(k0 / 8), index, blk);
        for (int kk = 0; kk < 8; ++kk) {
            const int k = k0 + kk;
            if (k < n) {
                const uint64_t bits = (uint64_t)blk[2 * kk] | ((uint64_t)blk[2 * kk + 1] << 32);
                x[k] = uniform_inclusive(lb[k], scale[k], bits);
            }
        }
    }
}

// Steps 1 - 4: x0 [n] is the region's own start, x [n] comes back projected.
template <class CH>
__device__ inline Row restart(const CH &ch, const EvalParams &ep, const constraint::Box &box, const Keep &keep,
                              const uint32_t (&key)[8], const double *scale, const double *x0, uint64_t index, int n,
                              double tol, int iters, double damping, double max_step, int mode, double *x) {
    if (index == 0) {
        for (int k = 0; k < n; ++k) x[k] = x0[k];
    } else {
        seed(key, ch.lb, scale, index, n, x);
    }
    const constraint::Projected p = constraint::project(ch, ep, box, n, tol, iters, damping, max_step, x);
    Row out{p.violation, __builtin_huge_val(), p.status, p.iterations};
    if (p.status != constraint::PROJECTED) return out;
    if (mode == MODE_SPEED) {
        out.key = (double)index;
    } else {
        double acc = 0.0;
        for (int k = 0; k < n; ++k) {
            const double d = x[k] - x0[k];
            acc += d * d;
        }
        out.key = __builtin_sqrt(acc);
    }
    if (keep.on) {
        double r[6];
        const double v = constraint::measure(ch, ep, keep.box, n, x, r);
        if (!(v <= keep.tol)) out.key = __builtin_huge_val();
    }
    return out;
}

}  // namespace region
}  // namespace optik
