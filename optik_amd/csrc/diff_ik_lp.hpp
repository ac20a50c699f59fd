// diff_ik_lp.hpp -- the LP of Robot::diff_ik (lib.rs:123-239), one function for the host and the device.
//
//     max alpha   s.t.   J_W(q) v = alpha V,   -v_max <= v <= v_max,   0 <= alpha <= 1
//
// optik_robot_diff_ik_ex (robot_host.cpp) calls it after one FK launch; diff_ik_batch_kernel (ik_batch_ops.hip)
// calls it in every thread after the same FK / Jacobian device code.  Both sides are compiled with
// -ffp-contract=off, and the function uses only +, -, *, / (correctly rounded on both sides), comparisons,
// fabs and isfinite -- no libm, no std::min / std::max / std::swap (replaced below by the same expressions,
// NaN behaviour included) -- so one source gives one set of bits wherever it runs.
//
// The LP has at most MAXN + 1 <= 9 unknowns and is solved exactly: the equality constraints are eliminated (null
// space of [J_W | -V] by Gauss-Jordan with full pivoting) and the vertices of the remaining polytope (any dimension
// d = n + 1 - rank) are enumerated.  The optimal alpha is unique.  Where the reference's own code can run the
// optimal v is unique too: lib.rs:196-197 sizes the equality block as `b.extend(vec![0.0; n]); K.push(ZeroConeT(n))`
// for a 6-row matrix, so DefaultSolver::new only accepts n = 6 (for any other n the dimensions disagree and the
// `expect("solver initialization failed")` panics), and a non-singular 6 x 6 Jacobian leaves a single ray
// v = alpha J^-1 V.  For n != 6 -- an extension -- and at singularities the optimal face may have positive
// dimension: for d = 2 the minimum-norm point of the optimal edge is returned, for d > 2 an optimal vertex of
// minimum norm among the vertices (an interior-point solver would return a point inside the face).
//
// Cost: C(2(n+1), d) small d x d solves -- 14 for a non-singular 6-joint arm (d = 1), 120 for a 7-joint one
// (d = 2), 816 for 8 joints (d = 3); a singular configuration has a larger d and more.  On the device each thread
// runs its own enumeration: threads of one wave with different d diverge, and the runtime-indexed pivots put the
// small matrices in scratch.
//
// Plain host C++ compiles this header too (no HIP runtime): tests/test_diff_ik_batch_host.py drives it with g++.
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OPTIK_LP_HD __host__ __device__
#else
#define OPTIK_LP_HD
#endif

namespace optik {
namespace lp {

// std::max / std::min / std::swap as the standard library defines them: max(a, b) = (a < b) ? b : a,
// min(a, b) = (b < a) ? b : a -- with a NaN operand both return the first argument
OPTIK_LP_HD inline double lp_max(double a, double b) { return (a < b) ? b : a; }
OPTIK_LP_HD inline double lp_min(double a, double b) { return (b < a) ? b : a; }
OPTIK_LP_HD inline void lp_swap(double &a, double &b) {
    const double t = a;
    a = b;
    b = t;
}

// n <= MAXN joint positions.  quat = the end-effector orientation (i, j, k, w) of the FK pose; jac = the body
// Jacobian, column-major 6 x n (jac[c * 6 + r]: rows 0-2 linear, 3-5 angular -- what fk_batch writes per
// configuration); V = the world-frame twist (6); v_max = the joint speed limits (n).
// Returns 1 (no solution: some v_max_i < 0 or NaN; nothing written) or 0 with *alpha_out and v_out[0..n).
template <int MAXN>
OPTIK_LP_HD inline int diff_ik_lp(int n, const double *quat, const double *jac, const double *V, const double *v_max,
                                  double *alpha_out, double *v_out) {
    const int nz = n + 1;
    for (int i = 0; i < n; ++i)
        if (!(v_max[i] >= 0.0)) return 1;  // infeasible box
    // body-frame Jacobian -> world frame: both 3-row blocks rotated by R_WE (lib.rs:190-197)
    const double qi = quat[0], qj = quat[1], qk = quat[2], qw = quat[3];
    const double R[3][3] = {{qw * qw + qi * qi - qj * qj - qk * qk, 2 * (qi * qj - qw * qk), 2 * (qw * qj + qi * qk)},
                            {2 * (qw * qk + qi * qj), qw * qw - qi * qi + qj * qj - qk * qk, 2 * (qj * qk - qw * qi)},
                            {2 * (qi * qk - qw * qj), 2 * (qw * qi + qj * qk), qw * qw - qi * qi - qj * qj + qk * qk}};
    double M[6][MAXN + 1];  // [J_W | -V], 6 x (n + 1)
    for (int c = 0; c < n; ++c)
        for (int blk = 0; blk < 2; ++blk)
            for (int a = 0; a < 3; ++a) {
                double acc = 0.0;
                for (int b = 0; b < 3; ++b) acc += R[a][b] * jac[c * 6 + blk * 3 + b];
                M[blk * 3 + a][c] = acc;
            }
    double scale = 0.0;
    for (int a = 0; a < 6; ++a) {
        M[a][n] = -V[a];
        for (int c = 0; c < nz; ++c) scale = lp_max(scale, __builtin_fabs(M[a][c]));
    }
    // Gauss-Jordan with full pivoting: pivot columns pc[0..rank), the others are free
    int pc[6], rank = 0;
    bool is_pivot[MAXN + 1];
    for (int c = 0; c < nz; ++c) is_pivot[c] = false;
    for (int step = 0; step < 6; ++step) {
        int br = -1, bc = -1;
        double best = 1e-12 * (scale > 0.0 ? scale : 1.0);
        for (int a = step; a < 6; ++a)
            for (int c = 0; c < nz; ++c)
                if (!is_pivot[c] && __builtin_fabs(M[a][c]) > best) { best = __builtin_fabs(M[a][c]); br = a; bc = c; }
        if (br < 0) break;
        for (int c = 0; c < nz; ++c) lp_swap(M[step][c], M[br][c]);
        const double piv = M[step][bc];
        for (int c = 0; c < nz; ++c) M[step][c] /= piv;
        for (int a = 0; a < 6; ++a)
            if (a != step) {
                const double f = M[a][bc];
                if (f != 0.0) for (int c = 0; c < nz; ++c) M[a][c] -= f * M[step][c];
            }
        is_pivot[bc] = true;
        pc[rank++] = bc;
    }
    const int d = nz - rank;  // dimension of {z = (v, alpha) : [J_W | -V] z = 0}
    double best_z[MAXN + 1];  // z = 0 (alpha = 0, v = 0) is always feasible
    for (int c = 0; c < nz; ++c) best_z[c] = 0.0;
    double best_alpha = 0.0, best_norm = 0.0;
    if (d >= 1) {
        // basis B (nz x d): free variable k = 1, pivot variables from the reduced rows
        int freec[MAXN + 1], nf = 0;
        for (int c = 0; c < nz; ++c) if (!is_pivot[c]) freec[nf++] = c;
        double B[MAXN + 1][MAXN + 1];
        for (int k = 0; k < d; ++k) {
            for (int c = 0; c < nz; ++c) B[c][k] = 0.0;
            B[freec[k]][k] = 1.0;
            for (int rr = 0; rr < rank; ++rr) B[pc[rr]][k] = -M[rr][freec[k]];
        }
        // half-spaces lo_c <= (B t)_c <= hi_c; vertices = d of them tight
        const int nh = 2 * nz;
        auto bound = [&](int h, double &sgn) -> double {  // constraint h: sgn * (B t)_c <= value
            const int c = h / 2;
            const bool upper = (h % 2) == 0;
            sgn = upper ? 1.0 : -1.0;
            if (c == n) return upper ? 1.0 : 0.0;
            return v_max[c];
        };
        const double tol = 1e-9;
        auto consider = [&](const double *t) {
            double z[MAXN + 1];
            for (int c = 0; c < nz; ++c) { z[c] = 0.0; for (int k = 0; k < d; ++k) z[c] += B[c][k] * t[k]; }
            for (int h = 0; h < nh; ++h) {
                double sgn; const double val = bound(h, sgn);
                if (sgn * z[h / 2] > val + tol * (1.0 + val)) return;
            }
            double nrm = 0.0;
            for (int c = 0; c < n; ++c) nrm += z[c] * z[c];
            if (z[n] > best_alpha + 1e-12 || (__builtin_fabs(z[n] - best_alpha) <= 1e-12 && nrm < best_norm)) {
                best_alpha = z[n]; best_norm = nrm;
                for (int c = 0; c < nz; ++c) best_z[c] = z[c];
            }
        };
        auto vertex = [&](const int *idx) {  // the point where the d constraints idx[] are tight
            double A[MAXN + 1][MAXN + 2];
            for (int q = 0; q < d; ++q) {
                double sgn; const double val = bound(idx[q], sgn);
                for (int k = 0; k < d; ++k) A[q][k] = sgn * B[idx[q] / 2][k];
                A[q][d] = val;
            }
            for (int q = 0; q < d; ++q) {  // Gauss-Jordan, partial pivoting
                int pr = q;
                for (int a = q + 1; a < d; ++a) if (__builtin_fabs(A[a][q]) > __builtin_fabs(A[pr][q])) pr = a;
                if (__builtin_fabs(A[pr][q]) < 1e-13) return;  // the constraints are parallel: no vertex
                for (int k = 0; k <= d; ++k) lp_swap(A[q][k], A[pr][k]);
                for (int a = 0; a < d; ++a)
                    if (a != q) {
                        const double f = A[a][q] / A[q][q];
                        for (int k = q; k <= d; ++k) A[a][k] -= f * A[q][k];
                    }
            }
            double t[MAXN + 1];
            for (int q = 0; q < d; ++q) t[q] = A[q][d] / A[q][q];
            consider(t);
        };
        // every choice of d of the nh half-spaces (d <= 9, nh <= 18: at most 48 620 small solves,
        // and d > 2 only at a kinematic singularity or for n = 8)
        int idx[MAXN + 1];
        for (int q = 0; q < d; ++q) idx[q] = q;
        for (bool more = d <= nh; more;) {
            vertex(idx);
            int q = d - 1;
            while (q >= 0 && idx[q] == nh - d + q) --q;
            if (q < 0) { more = false; break; }
            ++idx[q];
            for (int k = q + 1; k < d; ++k) idx[k] = idx[k - 1] + 1;
        }
        // a redundant arm at the optimum: slide along the optimal face to the minimum-norm v
        if (d == 2) {
            // direction inside the face: alpha fixed -> B[n] . dt = 0
            const double dt[2] = {-B[n][1], B[n][0]};
            double dz[MAXN + 1], dd = 0.0, zd = 0.0;
            for (int c = 0; c < nz; ++c) dz[c] = B[c][0] * dt[0] + B[c][1] * dt[1];
            for (int c = 0; c < n; ++c) { dd += dz[c] * dz[c]; zd += best_z[c] * dz[c]; }
            if (dd > 0.0) {
                double lo = -1e300, hi = 1e300;  // feasible range of the step along dz
                for (int c = 0; c < n; ++c) {
                    if (__builtin_fabs(dz[c]) < 1e-14) continue;
                    double a1 = (-v_max[c] - best_z[c]) / dz[c], a2 = (v_max[c] - best_z[c]) / dz[c];
                    if (a1 > a2) lp_swap(a1, a2);
                    lo = lp_max(lo, a1); hi = lp_min(hi, a2);
                }
                double step = -zd / dd;
                step = lp_min(lp_max(step, lo), hi);
                if (lo <= hi && __builtin_isfinite(step))
                    for (int c = 0; c < n; ++c) best_z[c] += step * dz[c];
            }
        }
    }
    *alpha_out = lp_min(lp_max(best_z[n], 0.0), 1.0);
    for (int c = 0; c < n; ++c) v_out[c] = best_z[c];
    return 0;
}

// The damped LP of collision-avoiding diff_ik: the same problem plus m <= MAX_DAMPER_ROWS
// velocity-damper rows G_r . v >= h_r (G row-major [m][n]) -- Faverjon and Tournassoud's half-spaces, one per close
// (link, obstacle) pair.  The same elimination, the same vertex enumeration over 2(n + 1) + m half-spaces, the same
// tolerances and tie-break, and with m = 0 every operation of diff_ik_lp in its order: the same bits.  What changes:
//   - z = 0 is a candidate only if every h_r <= tol (a configuration already inside the safety distance has h_r > 0);
//   - if no candidate is feasible the function returns 1 and writes nothing;
//   - the d == 2 minimum-norm slide clips its step by the damper rows as well as by the box.
// A damper row is held to the absolute tolerance: a point with G_r . v < h_r - tol is not feasible.
// The cap on m bounds the enumeration: C(2(n + 1) + m, d) small solves, C(22, 3) = 1540 for 8 joints.
constexpr int MAX_DAMPER_ROWS = 4;

template <int MAXN>
OPTIK_LP_HD inline int diff_ik_lp_damped(int n, const double *quat, const double *jac, const double *V,
                                         const double *v_max, int m, const double *G, const double *h,
                                         double *alpha_out, double *v_out) {
    const int nz = n + 1;
    if (m < 0 || m > MAX_DAMPER_ROWS) return 1;
    for (int i = 0; i < n; ++i)
        if (!(v_max[i] >= 0.0)) return 1;  // infeasible box
    const double qi = quat[0], qj = quat[1], qk = quat[2], qw = quat[3];
    const double R[3][3] = {{qw * qw + qi * qi - qj * qj - qk * qk, 2 * (qi * qj - qw * qk), 2 * (qw * qj + qi * qk)},
                            {2 * (qw * qk + qi * qj), qw * qw - qi * qi + qj * qj - qk * qk, 2 * (qj * qk - qw * qi)},
                            {2 * (qi * qk - qw * qj), 2 * (qw * qi + qj * qk), qw * qw - qi * qi - qj * qj + qk * qk}};
    double M[6][MAXN + 1];  // [J_W | -V], 6 x (n + 1)
    for (int c = 0; c < n; ++c)
        for (int blk = 0; blk < 2; ++blk)
            for (int a = 0; a < 3; ++a) {
                double acc = 0.0;
                for (int b = 0; b < 3; ++b) acc += R[a][b] * jac[c * 6 + blk * 3 + b];
                M[blk * 3 + a][c] = acc;
            }
    double scale = 0.0;
    for (int a = 0; a < 6; ++a) {
        M[a][n] = -V[a];
        for (int c = 0; c < nz; ++c) scale = lp_max(scale, __builtin_fabs(M[a][c]));
    }
    int pc[6], rank = 0;
    bool is_pivot[MAXN + 1];
    for (int c = 0; c < nz; ++c) is_pivot[c] = false;
    for (int step = 0; step < 6; ++step) {
        int br = -1, bc = -1;
        double best = 1e-12 * (scale > 0.0 ? scale : 1.0);
        for (int a = step; a < 6; ++a)
            for (int c = 0; c < nz; ++c)
                if (!is_pivot[c] && __builtin_fabs(M[a][c]) > best) { best = __builtin_fabs(M[a][c]); br = a; bc = c; }
        if (br < 0) break;
        for (int c = 0; c < nz; ++c) lp_swap(M[step][c], M[br][c]);
        const double piv = M[step][bc];
        for (int c = 0; c < nz; ++c) M[step][c] /= piv;
        for (int a = 0; a < 6; ++a)
            if (a != step) {
                const double f = M[a][bc];
                if (f != 0.0) for (int c = 0; c < nz; ++c) M[a][c] -= f * M[step][c];
            }
        is_pivot[bc] = true;
        pc[rank++] = bc;
    }
    const int d = nz - rank;
    const double tol = 1e-9;
    double best_z[MAXN + 1];
    for (int c = 0; c < nz; ++c) best_z[c] = 0.0;
    double best_alpha = 0.0, best_norm = 0.0;
    bool have = true;  // z = 0: feasible unless a damper row asks for motion (h_r > 0)
    for (int r = 0; r < m; ++r)
        if (!(h[r] <= tol)) have = false;
    if (d >= 1) {
        int freec[MAXN + 1], nf = 0;
        for (int c = 0; c < nz; ++c) if (!is_pivot[c]) freec[nf++] = c;
        double B[MAXN + 1][MAXN + 1];
        for (int k = 0; k < d; ++k) {
            for (int c = 0; c < nz; ++c) B[c][k] = 0.0;
            B[freec[k]][k] = 1.0;
            for (int rr = 0; rr < rank; ++rr) B[pc[rr]][k] = -M[rr][freec[k]];
        }
        // damper row r in the reduced space: -(G_r B) t <= -h_r
        double GB[MAX_DAMPER_ROWS][MAXN + 1];
        for (int r = 0; r < m; ++r)
            for (int k = 0; k < d; ++k) {
                double acc = 0.0;
                for (int c = 0; c < n; ++c) acc += G[r * n + c] * B[c][k];
                GB[r][k] = -acc;
            }
        const int nbox = 2 * nz, nh = nbox + m;
        auto bound = [&](int hh, double &sgn) -> double {  // box constraint hh: sgn * (B t)_c <= value
            const int c = hh / 2;
            const bool upper = (hh % 2) == 0;
            sgn = upper ? 1.0 : -1.0;
            if (c == n) return upper ? 1.0 : 0.0;
            return v_max[c];
        };
        auto consider = [&](const double *t) {
            double z[MAXN + 1];
            for (int c = 0; c < nz; ++c) { z[c] = 0.0; for (int k = 0; k < d; ++k) z[c] += B[c][k] * t[k]; }
            for (int hh = 0; hh < nbox; ++hh) {
                double sgn; const double val = bound(hh, sgn);
                if (sgn * z[hh / 2] > val + tol * (1.0 + val)) return;
            }
            for (int r = 0; r < m; ++r) {
                double gz = 0.0;
                for (int c = 0; c < n; ++c) gz += G[r * n + c] * z[c];
                if (!(gz >= h[r] - tol)) return;
            }
            double nrm = 0.0;
            for (int c = 0; c < n; ++c) nrm += z[c] * z[c];
            if (!have || z[n] > best_alpha + 1e-12
                || (__builtin_fabs(z[n] - best_alpha) <= 1e-12 && nrm < best_norm)) {
                have = true;
                best_alpha = z[n]; best_norm = nrm;
                for (int c = 0; c < nz; ++c) best_z[c] = z[c];
            }
        };
        auto vertex = [&](const int *idx) {  // the point where the d constraints idx[] are tight
            double A[MAXN + 1][MAXN + 2];
            for (int q = 0; q < d; ++q) {
                if (idx[q] < nbox) {
                    double sgn; const double val = bound(idx[q], sgn);
                    for (int k = 0; k < d; ++k) A[q][k] = sgn * B[idx[q] / 2][k];
                    A[q][d] = val;
                } else {
                    for (int k = 0; k < d; ++k) A[q][k] = GB[idx[q] - nbox][k];
                    A[q][d] = -h[idx[q] - nbox];
                }
            }
            for (int q = 0; q < d; ++q) {  // Gauss-Jordan, partial pivoting
                int pr = q;
                for (int a = q + 1; a < d; ++a) if (__builtin_fabs(A[a][q]) > __builtin_fabs(A[pr][q])) pr = a;
                if (__builtin_fabs(A[pr][q]) < 1e-13) return;  // the constraints are parallel: no vertex
                for (int k = 0; k <= d; ++k) lp_swap(A[q][k], A[pr][k]);
                for (int a = 0; a < d; ++a)
                    if (a != q) {
                        const double f = A[a][q] / A[q][q];
                        for (int k = q; k <= d; ++k) A[a][k] -= f * A[q][k];
                    }
            }
            double t[MAXN + 1];
            for (int q = 0; q < d; ++q) t[q] = A[q][d] / A[q][q];
            consider(t);
        };
        int idx[MAXN + 1];
        for (int q = 0; q < d; ++q) idx[q] = q;
        for (bool more = d <= nh; more;) {
            vertex(idx);
            int q = d - 1;
            while (q >= 0 && idx[q] == nh - d + q) --q;
            if (q < 0) { more = false; break; }
            ++idx[q];
            for (int k = q + 1; k < d; ++k) idx[k] = idx[k - 1] + 1;
        }
        // a redundant arm at the optimum: slide along the optimal face to the minimum-norm v
        if (d == 2 && have) {
            const double dt[2] = {-B[n][1], B[n][0]};
            double dz[MAXN + 1], dd = 0.0, zd = 0.0;
            for (int c = 0; c < nz; ++c) dz[c] = B[c][0] * dt[0] + B[c][1] * dt[1];
            for (int c = 0; c < n; ++c) { dd += dz[c] * dz[c]; zd += best_z[c] * dz[c]; }
            if (dd > 0.0) {
                double lo = -1e300, hi = 1e300;  // feasible range of the step along dz
                bool bounded = false;
                for (int c = 0; c < n; ++c) {
                    if (__builtin_fabs(dz[c]) < 1e-14) continue;
                    bounded = true;
                    double a1 = (-v_max[c] - best_z[c]) / dz[c], a2 = (v_max[c] - best_z[c]) / dz[c];
                    if (a1 > a2) lp_swap(a1, a2);
                    lo = lp_max(lo, a1); hi = lp_min(hi, a2);
                }
                // With alpha pinned by the equalities B[n] is 0 up to rounding, and dz is rounding noise that no
                // bound clips.  With damper rows the best vertex need not be z = 0 there, and a step of -zd / dd
                // along noise would leave the box: no slide then (`bounded` below).  Without rows the steps of
                // diff_ik_lp are kept.
                for (int r = 0; r < m; ++r) {  // G_r . (z + s dz) >= h_r
                    double gd = 0.0, gz = 0.0;
                    for (int c = 0; c < n; ++c) { gd += G[r * n + c] * dz[c]; gz += G[r * n + c] * best_z[c]; }
                    if (__builtin_fabs(gd) < 1e-14) continue;
                    const double s0 = (h[r] - gz) / gd;
                    if (gd > 0.0) lo = lp_max(lo, s0);
                    else hi = lp_min(hi, s0);
                }
                double step = -zd / dd;
                step = lp_min(lp_max(step, lo), hi);
                if (lo <= hi && (m == 0 || bounded) && __builtin_isfinite(step))
                    for (int c = 0; c < n; ++c) best_z[c] += step * dz[c];
            }
        }
    }
    if (!have) return 1;
    *alpha_out = lp_min(lp_max(best_z[n], 0.0), 1.0);
    for (int c = 0; c < n; ++c) v_out[c] = best_z[c];
    return 0;
}

}  // namespace lp
}  // namespace optik
