"""The manipulability / condition measure of optik_amd/csrc/manip_measure.hpp compiled with g++ as plain C++ (no HIP
runtime), for the host and the -m gpu tests of the manipulability and condition solution modes."""
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optik_amd", "csrc")
MAXN = 16
CASE_IN = 1 + 6 * MAXN  # n, jac (6 x n column-major)

DRIVER = r"""
#include <cstdio>
#include "manip_measure.hpp"

int main(int argc, char **argv) {
    FILE *in = std::fopen(argv[1], "rb");
    FILE *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    double rec[%(cin)d];
    while (std::fread(rec, sizeof(double), %(cin)d, in) == %(cin)d) {
        double res[2];
        optik::manip::manip_measures((int)rec[0], rec + 1, &res[0], &res[1]);
        std::fwrite(res, sizeof(double), 2, out);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
""" % dict(cin=CASE_IN)


def build_measure(workdir=None):
    """Compile the driver; returns run(jacobians: list of 6 x n arrays) -> (w [B], c [B])."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the measure header on its own"
    d = workdir or tempfile.mkdtemp(prefix="manip_measure_")
    src, exe = os.path.join(d, "driver.cpp"), os.path.join(d, "driver")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe],
                   check=True)

    def run(jacs):
        if len(jacs) == 0:
            return np.zeros(0), np.zeros(0)
        recs = np.zeros((len(jacs), CASE_IN))
        for i, J in enumerate(jacs):
            n = J.shape[1]
            recs[i, 0] = n
            recs[i, 1:1 + 6 * n] = np.asarray(J, dtype=np.float64).T.ravel()  # 6 x n -> column-major
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        recs.tofile(fin)
        subprocess.run([exe, fin, fout], check=True)
        out = np.fromfile(fout, dtype=np.float64).reshape(len(jacs), 2)
        return out[:, 0], out[:, 1]
    return run
