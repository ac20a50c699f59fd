"""CPU checks of batched diff_ik: the library exports the new entry points, and the LP that both the host
layer and the device kernel run (optik_amd/csrc/diff_ik_lp.hpp) -- compiled here as plain C++ with g++, no HIP
runtime -- solves random LPs as scipy's HiGHS does."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "optik_amd", "csrc")
MAXN = 8
CASE_IN = 1 + 4 + 6 * MAXN + 6 + MAXN   # n, quat, jac (6 x n column-major), V, v_max
CASE_OUT = 2 + MAXN                     # status, alpha, v

DRIVER = r"""
#include <cstdio>
#include "diff_ik_lp.hpp"

int main(int argc, char **argv) {
    FILE *in = std::fopen(argv[1], "rb");
    FILE *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    double rec[%(cin)d];
    while (std::fread(rec, sizeof(double), %(cin)d, in) == %(cin)d) {
        const int n = (int)rec[0];
        const double *quat = rec + 1, *jac = quat + 4, *V = jac + 6 * %(maxn)d, *vmax = V + 6;
        double res[%(cout)d] = {0};
        const int st = optik::lp::diff_ik_lp<%(maxn)d>(n, quat, jac, V, vmax, &res[1], &res[2]);
        res[0] = st;
        std::fwrite(res, sizeof(double), %(cout)d, out);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
""" % dict(cin=CASE_IN, cout=CASE_OUT, maxn=MAXN)


@pytest.fixture(scope="module")
def built():
    from optik_amd import build
    build.build()
    from optik_amd import _native
    return _native.lib()


def test_batch_symbols_are_exported(built):
    for s in ("optik_hip_diff_ik_batch", "optik_robot_diff_ik_batch"):
        assert hasattr(built, s), f"{s} is not exported by liboptik_amd.so"


@pytest.fixture(scope="module")
def lp_driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the LP header on its own"
    d = tmp_path_factory.mktemp("diff_ik_lp")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, str(src),
                    "-o", str(exe)], check=True)

    def run(cases):
        recs = np.zeros((len(cases), CASE_IN))
        for i, (n, quat, jac, V, vmax) in enumerate(cases):
            recs[i, 0] = n
            recs[i, 1:5] = quat
            recs[i, 5:5 + 6 * n] = np.asarray(jac).T.ravel()  # 6 x n -> column-major
            recs[i, 5 + 6 * MAXN:11 + 6 * MAXN] = V
            recs[i, 11 + 6 * MAXN:11 + 6 * MAXN + n] = vmax
        fin, fout = d / "in.bin", d / "out.bin"
        recs.tofile(fin)
        subprocess.run([str(exe), str(fin), str(fout)], check=True)
        return np.fromfile(fout, dtype=np.float64).reshape(len(cases), CASE_OUT)
    return run


def _rot(quat):
    i, j, k, w = quat
    return np.array([[w * w + i * i - j * j - k * k, 2 * (i * j - w * k), 2 * (w * j + i * k)],
                     [2 * (w * k + i * j), w * w - i * i + j * j - k * k, 2 * (j * k - w * i)],
                     [2 * (i * k - w * j), 2 * (w * i + j * k), w * w - i * i - j * j + k * k]])


def _random_cases(rng, count):
    cases = []
    for t in range(count):
        n = 1 + t % MAXN
        if t % 4 == 3 and n >= 2:
            r = int(rng.integers(1, min(6, n)))          # rank-deficient J_W
            J = rng.normal(size=(6, r)) @ rng.normal(size=(r, n))
        else:
            J = rng.normal(size=(6, n))
        if t % 2:
            quat = rng.normal(size=4)
            quat /= np.linalg.norm(quat)
        else:
            quat = np.array([0.0, 0.0, 0.0, 1.0])        # R = I exactly
        V = rng.normal(size=6) * (0.02 if t % 3 == 0 else 1.0)
        vmax = rng.uniform(0.1, 2.0, size=n)
        if t % 5 == 0:
            vmax[rng.integers(n)] = 0.0                  # a locked joint
        cases.append((n, quat, J, V, vmax))
    return cases


def test_lp_matches_highs_on_random_lps(lp_driver):
    from scipy.optimize import linprog
    rng = np.random.default_rng(2024)
    cases = _random_cases(rng, 400)
    out = lp_driver(cases)
    for (n, quat, J, V, vmax), res in zip(cases, out):
        assert res[0] == 0
        alpha, v = res[1], res[2:2 + n]
        JW = np.vstack([_rot(quat) @ J[:3], _rot(quat) @ J[3:]])
        c = np.zeros(n + 1)
        c[n] = -1.0
        ref = linprog(c, A_eq=np.hstack([JW, -V[:, None]]), b_eq=np.zeros(6),
                      bounds=[(-m, m) for m in vmax] + [(0.0, 1.0)], method="highs")
        assert ref.status == 0
        assert abs(alpha - ref.x[n]) <= 1e-7, (n, alpha, ref.x[n])
        assert 0.0 <= alpha <= 1.0
        assert np.all(np.abs(v) <= vmax + 1e-9), (n, v, vmax)
        assert np.allclose(JW @ v, alpha * V, rtol=0, atol=1e-8), (n, JW @ v - alpha * V)


def test_lp_negative_or_nan_limit_has_no_solution(lp_driver):
    rng = np.random.default_rng(7)
    cases = []
    for n in range(1, MAXN + 1):
        for bad in (-1e-3, -1.0, np.nan):
            vmax = rng.uniform(0.1, 2.0, size=n)
            vmax[rng.integers(n)] = bad
            cases.append((n, np.array([0.0, 0.0, 0.0, 1.0]), rng.normal(size=(6, n)), rng.normal(size=6), vmax))
    out = lp_driver(cases)
    assert np.all(out[:, 0] == 1)
    assert np.all(out[:, 1:] == 0.0)  # nothing written


def test_lp_zero_twist_and_reachable_twist(lp_driver):
    """V = 0: alpha = 1 with J_W v = 0, v = 0 itself up to n = 7 (d <= 2: the minimum-norm point of the optimal
    face; for n = 8 a vertex of the face); a twist J_W w with |w| < v_max: alpha = 1."""
    rng = np.random.default_rng(11)
    cases = []
    for n in range(1, MAXN + 1):
        J = rng.normal(size=(6, n))
        vmax = rng.uniform(0.5, 2.0, size=n)
        cases.append((n, np.array([0.0, 0.0, 0.0, 1.0]), J, np.zeros(6), vmax))
        w = rng.uniform(-0.1, 0.1, size=n) * vmax
        cases.append((n, np.array([0.0, 0.0, 0.0, 1.0]), J, J @ w, vmax))
    out = lp_driver(cases)
    for k, res in enumerate(out):
        n = 1 + k // 2
        assert res[0] == 0 and res[1] == 1.0, (n, res[:2])
        if k % 2 == 0:
            assert np.allclose(cases[k][2] @ res[2:2 + n], 0.0, rtol=0, atol=1e-8)
            if n <= 7:
                assert np.all(res[2:2 + n] == 0.0), (n, res[2:2 + n])
