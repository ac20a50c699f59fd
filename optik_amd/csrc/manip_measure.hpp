// manip_measure.hpp -- the manipulability and condition measures of a body Jacobian, one function for the host and
// the device (the keys of solution modes 3 and 4, optik_hip.h).
//
// J is the 6 x n body Jacobian of fk_batch / joint_jacobian: column-major, jac[c * 6 + r], rows 0-2 linear (metres),
// rows 3-5 angular (radians), 1 <= n <= MAXN.  Both measures are functions of the m = min(n, 6) largest singular
// values of J, so they do not depend on the frame J is expressed in (a world-frame Jacobian is diag(R, R) J).
//
//   manipulability  w = sqrt(det G)              = sigma_1 * ... * sigma_m
//   condition       c = sqrt(lambda_min / lambda_max) of G = sigma_min / sigma_max, in [0, 1]
//
// The exact operation order (the tests depend on it; both sides are compiled with -ffp-contract=off and use only
// the correctly rounded + - * / sqrt and fabs, so one source gives one set of bits wherever it runs):
//
//  1. Gram matrix G (m x m, symmetric): G = J^T J for n <= 6 (G[a][b] = sum over the 6 rows r), G = J J^T for n > 6
//     (G[a][b] = sum over the n columns k).  For a >= b the entry is s = x_0 * y_0, then s = s + x_i * y_i for
//     i = 1, 2, ... in ascending order, with x the a-th and y the b-th vector; G[b][a] = G[a][b].
//  2. LDL^T, left-looking, column j = 0 .. m-1:
//         acc = G[j][j];  acc = acc - (L[j][k] * L[j][k]) * d[k]   for k = 0 .. j-1;   d[j] = acc
//         if !(d[j] > 0) or d[j] is not finite: w = 0 and c = 0 (exactly; steps 3-4 are skipped)
//         for i = j+1 .. m-1:  acc = G[i][j];  acc = acc - (L[i][k] * L[j][k]) * d[k]  for k = 0 .. j-1;
//                              L[i][j] = acc / d[j]
//     det = d[0], then det = det * d[j] for j = 1 .. m-1 (left to right);  w = sqrt(det).
//     (Two equal columns of J -- n <= 6 -- or equal rows -- n > 6 -- give equal rows of G; the symmetric products
//     above then make the second one's multiplier exactly 1 and its pivot exactly 0 or less: w = 0, not a
//     rounding-sized number.  A zero column / row gives a zero pivot the same way.)
//  3. Cyclic Jacobi on a copy A of G (full symmetric storage), at most JACOBI_MAX_SWEEPS sweeps.  Before each sweep:
//         off = sum of A[p][q]^2 over p < q in row-major order (left to right, from 0.0),
//         dia = sum of A[p][p]^2 over p ascending (from 0.0);   stop unless off > JACOBI_TOL2 * dia.
//     A sweep visits (p, q), p < q, in row-major order; a pair with A[p][q] == 0 is skipped, otherwise
//         theta = (A[q][q] - A[p][p]) / (2 * A[p][q])
//         t = 1 / (fabs(theta) + sqrt(theta * theta + 1)),  t = -t if theta < 0
//         cs = 1 / sqrt(t * t + 1),  sn = t * cs
//         A[p][p] = A[p][p] - t * A[p][q],  A[q][q] = A[q][q] + t * A[p][q],  A[p][q] = A[q][p] = 0
//         for r = 0 .. m-1, r != p, q:  u = A[r][p], v = A[r][q];
//             A[r][p] = A[p][r] = cs * u - sn * v;   A[r][q] = A[q][r] = sn * u + cs * v
//     (theta * theta may overflow: t = 0 then, and the pair's entry is dropped -- it is below the diagonal's
//     rounding.)
//  4. lambda_min / lambda_max = the smallest / largest A[p][p] (scanned p ascending, strict comparisons);
//     c = 0 unless lambda_min > 0 and lambda_max is finite, else c = sqrt(lambda_min / lambda_max).
//
// Cost: at most 6 x 6 x 16 multiply-adds for G, 56 for the LDL^T, and a handful of Jacobi sweeps of 15 rotations.
// Plain host C++ compiles this header too (no HIP runtime): tests/test_manip_host.py drives it with g++.
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OPTIK_MM_HD __host__ __device__
#else
#define OPTIK_MM_HD
#endif

namespace optik {
namespace manip {

constexpr int MAXN = 16;               // joint positions (the general solver's limit)
constexpr int JACOBI_MAX_SWEEPS = 32;  // (a 6 x 6 matrix converges in well under 10)
constexpr double JACOBI_TOL2 = 0x1p-106;  // off-diagonal mass against the diagonal's: (2^-53)^2
constexpr double MM_DBL_MAX = 1.7976931348623157e308;

OPTIK_MM_HD inline double mm_sqrt(double x) { return __builtin_sqrt(x); }
OPTIK_MM_HD inline double mm_fabs(double x) { return x < 0.0 ? -x : x; }
OPTIK_MM_HD inline bool mm_positive_finite(double x) { return x > 0.0 && x <= MM_DBL_MAX; }

// Step 1: G (the leading m x m block of g); returns m.
OPTIK_MM_HD inline int gram(int n, const double *jac, double (&g)[6][6]) {
    if (n <= 6) {
        for (int a = 0; a < n; ++a)
            for (int b = 0; b <= a; ++b) {
                const double *x = jac + a * 6, *y = jac + b * 6;
                double s = x[0] * y[0];
                for (int r = 1; r < 6; ++r) s = s + x[r] * y[r];
                g[a][b] = s;
                g[b][a] = s;
            }
        return n;
    }
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b <= a; ++b) {
            double s = jac[a] * jac[b];
            for (int k = 1; k < n; ++k) s = s + jac[k * 6 + a] * jac[k * 6 + b];
            g[a][b] = s;
            g[b][a] = s;
        }
    return 6;
}

// Step 2: w = sqrt(det G) by LDL^T; false (and *w = 0) when a pivot is not positive and finite.
// (m is a template parameter so that the device code keeps these small arrays in registers)
template <int m>
OPTIK_MM_HD inline bool ldl_manipulability(const double (&g)[6][6], double *w) {
    double L[6][6];
    double d[6];
    for (int j = 0; j < m; ++j) {
        double acc = g[j][j];
        for (int k = 0; k < j; ++k) acc = acc - (L[j][k] * L[j][k]) * d[k];
        if (!mm_positive_finite(acc)) {
            *w = 0.0;
            return false;
        }
        d[j] = acc;
        for (int i = j + 1; i < m; ++i) {
            double a = g[i][j];
            for (int k = 0; k < j; ++k) a = a - (L[i][k] * L[j][k]) * d[k];
            L[i][j] = a / d[j];
        }
    }
    double det = d[0];
    for (int j = 1; j < m; ++j) det = det * d[j];
    *w = mm_sqrt(det);
    return true;
}

// Steps 3-4: c = sqrt(lambda_min / lambda_max) of G by cyclic Jacobi.
template <int m>
OPTIK_MM_HD inline double jacobi_condition(const double (&g)[6][6]) {
    double A[6][6];
    for (int p = 0; p < m; ++p)
        for (int q = 0; q < m; ++q) A[p][q] = g[p][q];
    for (int sweep = 0; sweep < JACOBI_MAX_SWEEPS; ++sweep) {
        double off = 0.0, dia = 0.0;
        for (int p = 0; p < m; ++p)
            for (int q = p + 1; q < m; ++q) off = off + A[p][q] * A[p][q];
        for (int p = 0; p < m; ++p) dia = dia + A[p][p] * A[p][p];
        if (!(off > JACOBI_TOL2 * dia)) break;
        for (int p = 0; p < m; ++p)
            for (int q = p + 1; q < m; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                double t = 1.0 / (mm_fabs(theta) + mm_sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double cs = 1.0 / mm_sqrt(t * t + 1.0);
                const double sn = t * cs;
                A[p][p] = A[p][p] - t * apq;
                A[q][q] = A[q][q] + t * apq;
                A[p][q] = 0.0;
                A[q][p] = 0.0;
                for (int r = 0; r < m; ++r) {
                    if (r == p || r == q) continue;
                    const double u = A[r][p], v = A[r][q];
                    const double np = cs * u - sn * v, nq = sn * u + cs * v;
                    A[r][p] = np; A[p][r] = np;
                    A[r][q] = nq; A[q][r] = nq;
                }
            }
    }
    double lmin = A[0][0], lmax = A[0][0];
    for (int p = 1; p < m; ++p) {
        if (A[p][p] < lmin) lmin = A[p][p];
        if (A[p][p] > lmax) lmax = A[p][p];
    }
    if (!(lmin > 0.0) || !mm_positive_finite(lmax)) return 0.0;
    return mm_sqrt(lmin / lmax);
}

// Both measures of one Jacobian (jac: 6 x n column-major, M = min(n, 6), 1 <= n <= MAXN); either output may be
// null.  The condition is only computed when it is asked for and the LDL^T found G positive definite.
template <int M>
OPTIK_MM_HD inline void manip_measures_m(int n, const double *jac, double *w_out, double *c_out) {
    double g[6][6];
    (void)gram(n, jac, g);
    double w = 0.0;
    const bool pd = ldl_manipulability<M>(g, &w);
    if (w_out) *w_out = w;
    if (c_out) *c_out = (pd && c_out) ? jacobi_condition<M>(g) : 0.0;
}

// The same for a run-time n.
OPTIK_MM_HD inline void manip_measures(int n, const double *jac, double *w_out, double *c_out) {
    switch (n < 6 ? n : 6) {
    case 1: manip_measures_m<1>(n, jac, w_out, c_out); break;
    case 2: manip_measures_m<2>(n, jac, w_out, c_out); break;
    case 3: manip_measures_m<3>(n, jac, w_out, c_out); break;
    case 4: manip_measures_m<4>(n, jac, w_out, c_out); break;
    case 5: manip_measures_m<5>(n, jac, w_out, c_out); break;
    default: manip_measures_m<6>(n, jac, w_out, c_out); break;
    }
}

}  // namespace manip
}  // namespace optik
