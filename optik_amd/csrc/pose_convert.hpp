// pose_convert.hpp -- 4x4 homogeneous matrices <-> pose7 (translation, quaternion i j k w) as the reference's two
// bindings convert them: nalgebra's closed-form and iterative rotation-to-quaternion conversions, operation for
// operation (tests/test_pose_from_matrix.py compares the bits with the oracle's).
#pragma once

#include <cmath>
#include <cstring>

namespace optik {
namespace pose {

// UnitQuaternion::from_rotation_matrix (nalgebra 0.34, not vendored): the four closed-form branches.  It ends in
// Self::new_unchecked(res): NO normalisation -- both bindings' conversions go through it, so one function serves both
// (round 5 normalised on the Python path only: ADVICE r5).
inline void quat_from_rotation(const double R[3][3], double &w, double &i, double &j, double &k) {
    const double tr = R[0][0] + R[1][1] + R[2][2];
    if (tr > 0.0) {
        const double d = std::sqrt(tr + 1.0) * 2.0;
        w = 0.25 * d; i = (R[2][1] - R[1][2]) / d; j = (R[0][2] - R[2][0]) / d; k = (R[1][0] - R[0][1]) / d;
    } else if (R[0][0] > R[1][1] && R[0][0] > R[2][2]) {
        const double d = std::sqrt(1.0 + R[0][0] - R[1][1] - R[2][2]) * 2.0;
        w = (R[2][1] - R[1][2]) / d; i = 0.25 * d; j = (R[0][1] + R[1][0]) / d; k = (R[0][2] + R[2][0]) / d;
    } else if (R[1][1] > R[2][2]) {
        const double d = std::sqrt(1.0 + R[1][1] - R[0][0] - R[2][2]) * 2.0;
        w = (R[0][2] - R[2][0]) / d; i = (R[0][1] + R[1][0]) / d; j = 0.25 * d; k = (R[1][2] + R[2][1]) / d;
    } else {
        const double d = std::sqrt(1.0 + R[2][2] - R[0][0] - R[1][1]) * 2.0;
        w = (R[1][0] - R[0][1]) / d; i = (R[0][2] + R[2][0]) / d; j = (R[1][2] + R[2][1]) / d; k = 0.25 * d;
    }
}

// 4x4 column-major homogeneous matrix -> pose7 as the pyo3 path does it (optik-py/src/lib.rs:8-15:
// try_convert::<Matrix4, Isometry3> -> Isometry3::from_superset_unchecked -> UnitQuaternion::from_rotation_matrix on the
// upper-left block, as it stands).  The C path's iterative UnitQuaternion::from_matrix is pose7_from_mat16_iterative
// below: the same rotation, last bits apart.
inline void pose7_from_mat16(const double *m, double *p) {
    double R[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[r][c] = m[c * 4 + r];
    p[0] = m[12]; p[1] = m[13]; p[2] = m[14];
    quat_from_rotation(R, p[6], p[3], p[4], p[5]);
}

// Rotation3::from_axis_angle (nalgebra: Rodrigues' formula entry by entry; angle == 0 -> identity).
inline void rot_from_axis_angle(const double u[3], double angle, double O[3][3]) {
    if (angle == 0.0) {
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) O[r][c] = r == c ? 1.0 : 0.0;
        return;
    }
    const double ux = u[0], uy = u[1], uz = u[2];
    const double sqx = ux * ux, sqy = uy * uy, sqz = uz * uz;
    double sn, cs;  // (f64::sin_cos: platform libm; ONE sincos call here and in the oracle -- sin + cos can differ from it in the last bit)
    ::sincos(angle, &sn, &cs);
    const double omc = 1.0 - cs;
    O[0][0] = sqx + (1.0 - sqx) * cs; O[0][1] = ux * uy * omc - uz * sn; O[0][2] = ux * uz * omc + uy * sn;
    O[1][0] = ux * uy * omc + uz * sn; O[1][1] = sqy + (1.0 - sqy) * cs; O[1][2] = uy * uz * omc - ux * sn;
    O[2][0] = ux * uz * omc - uy * sn; O[2][1] = uy * uz * omc + ux * sn; O[2][2] = sqz + (1.0 - sqz) * cs;
}

// 3x3 product as nalgebra forms it (gemv per column: the terms of an entry accumulated in order k = 0, 1, 2).
inline void mat3_mul(const double A[3][3], const double B[3][3], double O[3][3]) {
    double T[3][3];
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) {
            double acc = A[r][0] * B[0][c];
            acc = A[r][1] * B[1][c] + acc;
            acc = A[r][2] * B[2][c] + acc;
            T[r][c] = acc;
        }
    std::memcpy(O, T, sizeof T);
}

// ||M - R||_F^2, column by column (Matrix::norm_squared).
inline double diff_norm_squared(const double M[3][3], const double R[3][3]) {
    double res = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double d0 = M[0][c] - R[0][c], d1 = M[1][c] - R[1][c], d2 = M[2][c] - R[2][c];
        res += d0 * d0 + d1 * d1 + d2 * d2;
    }
    return res;
}

// UnitQuaternion::from_matrix (optik-cpp/src/lib.rs:141-142) = Rotation3::from_matrix_eps(m, f64::EPSILON, 0 =
// unlimited, identity) -- nalgebra 0.34 (Cargo.lock:579-581, not vendored), "A Robust Method to Extract the
// Rotational Part of Deformations" (Mueller et al.) with nalgebra's perturbation step at a stalled iterate --
// followed by from_rotation_matrix.  Restated from the crate's published source; the iteration cap is this
// implementation's (nalgebra's is usize::MAX: a rotation matrix converges in a few dozen steps).
inline void quat_from_matrix_iterative(const double M[3][3], double &w, double &i, double &j, double &k) {
    const double eps = 2.220446049250313e-16;
    const double eps_disturbance = std::fmax(std::sqrt(eps), eps * eps);
    double axes[3] = {1.0, 0.0, 0.0};  // perturbation_axes = Vector3::x_axis()
    double rot[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int it = 0; it < 100000; ++it) {
        // axis = sum_c rot.col(c) x m.col(c), denom = sum_c rot.col(c) . m.col(c)
        double axis[3] = {0, 0, 0}, denom = 0.0;
        for (int c = 0; c < 3; ++c) {
            const double a0 = rot[0][c], a1 = rot[1][c], a2 = rot[2][c], b0 = M[0][c], b1 = M[1][c], b2 = M[2][c];
            const double cr[3] = {a1 * b2 - a2 * b1, a2 * b0 - a0 * b2, a0 * b1 - a1 * b0};
            const double dt = a0 * b0 + a1 * b1 + a2 * b2;
            if (c == 0) { axis[0] = cr[0]; axis[1] = cr[1]; axis[2] = cr[2]; denom = dt; }
            else { axis[0] += cr[0]; axis[1] += cr[1]; axis[2] += cr[2]; denom += dt; }
        }
        const double dv = std::fabs(denom) + eps;
        double aa[3] = {axis[0] / dv, axis[1] / dv, axis[2] / dv};
        // Unit::try_new_and_get(axisangle, eps)
        const double sq = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2];
        if (sq > eps * eps) {
            const double nrm = std::sqrt(sq);
            const double u[3] = {aa[0] / nrm, aa[1] / nrm, aa[2] / nrm};
            double Rd[3][3];
            rot_from_axis_angle(u, nrm, Rd);
            mat3_mul(Rd, rot, rot);
        } else {
            // stuck at a stationary point of ||m - rot||: a maximum, unless a small rotation makes it worse
            double pert[3][3];
            std::memcpy(pert, rot, sizeof pert);
            const double n0 = diff_norm_squared(M, rot);
            double n1;
            for (;;) {
                double Rp[3][3];
                rot_from_axis_angle(axes, eps_disturbance, Rp);
                mat3_mul(pert, Rp, pert);
                n1 = diff_norm_squared(M, pert);
                if (!(std::fabs(n0 - n1) <= eps)) break;  // abs_diff_ne!(.., epsilon = f64::EPSILON): true for NaN too
            }
            if (n0 < n1) break;  // a minimum: done
            const double t = axes[0];  // perturbation_axes.yzx()
            axes[0] = axes[1]; axes[1] = axes[2]; axes[2] = t;
            std::memcpy(rot, pert, sizeof pert);
        }
    }
    quat_from_rotation(rot, w, i, j, k);
}

// 4x4 column-major -> pose7 as the C path of the reference does it (optik-cpp/src/lib.rs:137-144).
inline void pose7_from_mat16_iterative(const double *m, double *p) {
    double M[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) M[r][c] = m[c * 4 + r];
    p[0] = m[12]; p[1] = m[13]; p[2] = m[14];
    quat_from_matrix_iterative(M, p[6], p[3], p[4], p[5]);
}

// pose7 -> 4x4 column-major (Isometry3::to_matrix, optik-cpp/src/lib.rs:115).
inline void mat16_from_pose7(const double *p, double *m) {
    const double i = p[3], j = p[4], k = p[5], w = p[6];
    const double ww = w * w, ii = i * i, jj = j * j, kk = k * k;
    const double ij = i * j * 2.0, wk = w * k * 2.0, wj = w * j * 2.0, ik = i * k * 2.0, jk = j * k * 2.0,
                 wi = w * i * 2.0;
    const double R[3][3] = {{ww + ii - jj - kk, ij - wk, wj + ik},
                            {wk + ij, ww - ii + jj - kk, jk - wi},
                            {ik - wj, wi + jk, ww - ii - jj + kk}};
    for (int c = 0; c < 3; ++c) {
        for (int r = 0; r < 3; ++r) m[c * 4 + r] = R[r][c];
        m[c * 4 + 3] = 0.0;
    }
    m[12] = p[0]; m[13] = p[1]; m[14] = p[2]; m[15] = 1.0;
}

}  // namespace pose
}  // namespace optik
