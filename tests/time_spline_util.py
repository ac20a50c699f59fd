"""optik_amd/csrc/time_spline_measure.hpp compiled with g++ as plain C++ (no HIP runtime) for the host and the -m gpu
tests of spline retiming; the spline's segment quantities in numpy on the header's definitions; mixed test batches."""
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

from collision_util import CSRC
import time_util as tu

SMOOTH, BAD_TIMES, BAD_LENGTH, NOT_FINITE, OVER_LIMIT = 0, 1, 2, 3, 4

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "time_spline_measure.hpp"

using namespace optik;

static std::vector<double> read_all(const char *path) {
    std::vector<double> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) return v;
    double x;
    while (std::fread(&x, sizeof(double), 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return v;
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    const std::vector<double> in = read_all(argv[2]);
    FILE *out = std::fopen(argv[3], "wb");
    if (!out) return 2;
    if (argv[1][0] == 'r') {
        // retime: n, L, P, vmax [n], amax [n], jmax [n], then per path len, status, path [L][n], t [L]
        // -> status, duration, factor, ratios [3], t [L], qd [L][n], qdd [L][n]
        const int n = (int)in[0], L = (int)in[1], P = (int)in[2];
        const double *vmax = &in[3], *amax = vmax + n, *jmax = amax + n, *p = jmax + n;
        std::vector<double> t(L), qd(L * n), qdd(L * n);
        for (int k = 0; k < P; ++k, p += 2 + L * n + L) {
            const splinetime::Result r = splinetime::spline_reference(n, p + 2, n, (int)p[0], L, p + 2 + L * n, (int)p[1],
                                                                      vmax, amax, jmax, t.data(), qd.data(), qdd.data());
            const double head[6] = {(double)r.status, r.duration, r.factor, r.ratios[0], r.ratios[1], r.ratios[2]};
            std::fwrite(head, sizeof(double), 6, out);
            std::fwrite(t.data(), sizeof(double), t.size(), out);
            std::fwrite(qd.data(), sizeof(double), qd.size(), out);
            std::fwrite(qdd.data(), sizeof(double), qdd.size(), out);
        }
    } else if (argv[1][0] == 'c') {
        // cube roots: f [count] -> cube_root_up(f)
        for (double f : in) {
            const double c = splinetime::cube_root_up(f);
            std::fwrite(&c, sizeof(double), 1, out);
        }
    } else {
        // sample: n, L, P, Tout, then per path dt, len, status, path [L][n], t [L], qd [L][n] -> q [Tout][n], v [Tout][n]
        const int n = (int)in[0], L = (int)in[1], P = (int)in[2], Tout = (int)in[3];
        const double *p = &in[4];
        std::vector<double> q((size_t)Tout * n), v((size_t)Tout * n);
        for (int k = 0; k < P; ++k, p += 3 + L * n + L + L * n) {
            timing::sample_reference(n, p + 3, (int)p[1], L, p + 3 + L * n, p + 3 + L * n + L, (int)p[2], p[0], Tout,
                                     q.data(), v.data());
            std::fwrite(q.data(), sizeof(double), q.size(), out);
            std::fwrite(v.data(), sizeof(double), v.size(), out);
        }
    }
    std::fclose(out);
    return 0;
}
"""


def build_spline_ref(workdir=None):
    """Compile the driver; paths are [P, L, n] with lens [P] (None: L each).  Returns an object with
    .retime(paths, lens, times [P, L], status [P] or None, vmax, amax, jmax) -> dict(status [P] int32, duration [P],
      factor [P], ratios [P, 3], times [P, L], velocities [P, L, n], accelerations [P, L, n]),
    .cube_root_up(f [count]) -> [count],
    .sample(paths, lens, timing, dt [P], Tout) -> (q [P, Tout, n], v [P, Tout, n]): time_measure.hpp's sample_reference
      with a step of its own per path."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the timing header on its own"
    d = workdir or tempfile.mkdtemp(prefix="spline_")
    src, exe = os.path.join(d, "spline_driver.cpp"), os.path.join(d, "spline_driver")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe],
                   check=True)

    def run(mode, head, rows):
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        np.concatenate([np.asarray(head, dtype=np.float64), np.ascontiguousarray(rows, dtype=np.float64).ravel()]).tofile(fin)
        subprocess.run([exe, mode, fin, fout], check=True)
        return np.fromfile(fout, dtype=np.float64)

    def lim(v, n):
        return np.broadcast_to(np.asarray(v, dtype=np.float64), n)

    class Ref:
        @staticmethod
        def retime(paths, lens, times, status, vmax, amax, jmax):
            P, L, n = paths.shape
            st = np.zeros(P) if status is None else np.asarray(status, dtype=np.float64)
            rows = np.concatenate([tu._lens(lens, P, L)[:, None], st[:, None], paths.reshape(P, -1),
                                   np.asarray(times, dtype=np.float64).reshape(P, L)], axis=1)
            head = np.concatenate([[n, L, P], lim(vmax, n), lim(amax, n), lim(jmax, n)])
            out = run("r", head, rows).reshape(P, 6 + L + 2 * L * n)
            return dict(status=out[:, 0].astype(np.int32), duration=out[:, 1].copy(), factor=out[:, 2].copy(),
                        ratios=out[:, 3:6].copy(), times=out[:, 6:6 + L].copy(),
                        velocities=out[:, 6 + L:6 + L + L * n].reshape(P, L, n).copy(),
                        accelerations=out[:, 6 + L + L * n:].reshape(P, L, n).copy())

        @staticmethod
        def cube_root_up(f):
            return run("c", [], np.asarray(f, dtype=np.float64))

        @staticmethod
        def sample(paths, lens, timing, dt, Tout):
            P, L, n = paths.shape
            rows = np.concatenate([np.asarray(dt, dtype=np.float64).reshape(P, 1), tu._lens(lens, P, L)[:, None],
                                   np.asarray(timing["status"], dtype=np.float64)[:, None], paths.reshape(P, -1),
                                   timing["times"].reshape(P, -1), timing["velocities"].reshape(P, -1)], axis=1)
            out = run("s", [n, L, P, Tout], rows).reshape(P, 2, Tout, n)
            return out[:, 0].copy(), out[:, 1].copy()

    return Ref()


def segments(q, t, v):
    """A0, A1, J [m - 1, n] of one path q [m, n] with times t [m] and knot velocities v [m, n], by the definitions
    (divisions by h, numpy's order): what the C2 residual is taken from."""
    h = (t[1:] - t[:-1])[:, None]
    delta = (q[1:] - q[:-1]) / h
    a0 = (6.0 * delta - 4.0 * v[:-1] - 2.0 * v[1:]) / h
    a1 = (-6.0 * delta + 2.0 * v[:-1] + 4.0 * v[1:]) / h
    return a0, a1, (a1 - a0) / h


def mixed_batch(ref_time, rng, P, L, n):
    """P paths [P, L, n] with lens, times and input statuses that between them take every branch: gentle paths of
    full and of drawn lengths timed by time_measure.hpp's reference (`ref_time`), and from path 1 on, cyclically by 13:
    a length of 2, a NaN waypoint, an infinite time, a stalled input (status 1, NaN times), times that step back, a
    first time off 0.  Returns (paths, lens int32, times, status int32, vmax_t, amax_t: the limits of the timing)."""
    paths = tu.gentle_paths(rng, P, L, n)
    lens = np.where(rng.random(P) < 0.5, L, rng.integers(3, L + 1, size=P)).astype(np.int32)
    for p in range(P):
        paths[p, lens[p]:] = paths[p, lens[p] - 1]
    vmax_t, amax_t = np.linspace(1.5, 2.5, n), np.linspace(4.0, 9.0, n)
    timed = ref_time.time(paths, lens, vmax_t, amax_t)
    assert (timed["status"] == tu.TIMED).all()
    times, status = timed["times"].copy(), timed["status"].copy()
    for p in range(1, P):
        kind = p % 13
        if kind == 1:
            lens[p] = 2
        elif kind == 3:
            paths[p, lens[p] // 2, n // 2] = math.nan
        elif kind == 5:
            times[p, 1] = math.inf
        elif kind == 7:
            status[p], times[p] = tu.STALLED, math.nan
        elif kind == 9:
            times[p, lens[p] - 1] = times[p, lens[p] - 2]
        elif kind == 11:
            times[p, 0] = 1e-3
    return paths, lens, times, status, vmax_t, amax_t


OVER_LIMIT_J = 40.0


def over_limit_batch(ref_time):
    """The single-joint mixed batch (L = 64, P = 65) one of whose paths ends OVER_LIMIT under a jerk limit of 40
    rad/s^3 beside the timing's own limits: rounding of the products k * t, nothing prepared.  mixed_batch's tuple."""
    return mixed_batch(ref_time, np.random.default_rng(3000 + 640 + 65), 65, 64, 1)
