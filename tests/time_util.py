"""optik_amd/csrc/time_measure.hpp compiled with g++ as plain C++ (no HIP runtime) for the host and the -m gpu tests of
path timing and trajectory sampling; the constraint check in numpy on the header's definitions; the path generators."""
import os
import shutil
import subprocess
import tempfile

import numpy as np

from collision_util import CSRC
from roadmap_util import bits  # noqa: F401

MAX_POINTS = 64
TIMED, STALLED, BAD_LENGTH, PATH_NAN = 0, 1, 2, 3

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "time_measure.hpp"

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
    if (argv[1][0] == 't') {
        // time: n, L, P, vmax [n], amax [n], then per path len, path [L][n]
        // -> status, duration, t [L], x [L], qd [L][n], qdd [L][n]
        const int n = (int)in[0], L = (int)in[1], P = (int)in[2];
        const double *vmax = &in[3], *amax = vmax + n, *p = amax + n;
        std::vector<double> t(L), x(L), qd(L * n), qdd(L * n);
        for (int q = 0; q < P; ++q, p += 1 + L * n) {
            const timing::Result r = timing::time_reference(n, p + 1, n, (int)p[0], L, vmax, amax, t.data(), qd.data(),
                                                            qdd.data(), x.data());
            const double head[2] = {(double)r.status, r.duration};
            std::fwrite(head, sizeof(double), 2, out);
            std::fwrite(t.data(), sizeof(double), t.size(), out);
            std::fwrite(x.data(), sizeof(double), x.size(), out);
            std::fwrite(qd.data(), sizeof(double), qd.size(), out);
            std::fwrite(qdd.data(), sizeof(double), qdd.size(), out);
        }
    } else {
        // sample: n, L, P, Tout, dt, then per path len, status, path [L][n], t [L], qd [L][n] -> q [Tout][n], v [Tout][n]
        const int n = (int)in[0], L = (int)in[1], P = (int)in[2], Tout = (int)in[3];
        const double dt = in[4], *p = &in[5];
        std::vector<double> q((size_t)Tout * n), v((size_t)Tout * n);
        for (int k = 0; k < P; ++k, p += 2 + L * n + L + L * n) {
            timing::sample_reference(n, p + 2, (int)p[0], L, p + 2 + L * n, p + 2 + L * n + L, (int)p[1], dt, Tout,
                                     q.data(), v.data());
            std::fwrite(q.data(), sizeof(double), q.size(), out);
            std::fwrite(v.data(), sizeof(double), v.size(), out);
        }
    }
    std::fclose(out);
    return 0;
}
"""


def _lens(lens, P, L):
    return np.full(P, L, dtype=np.float64) if lens is None else np.asarray(lens, dtype=np.float64).reshape(P)


def build_time_ref(workdir=None):
    """Compile the driver; paths are [P, L, n] with lens [P] (None: L each).  Returns an object with
    .time(paths, lens, vmax [n], amax [n]) -> dict(status [P] int32, duration [P], times [P, L], x [P, L], velocities
      [P, L, n], accelerations [P, L, n]),
    .sample(paths, lens, timing, dt, Tout) -> (q [P, Tout, n], v [P, Tout, n]) from such a dict."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the timing header on its own"
    d = workdir or tempfile.mkdtemp(prefix="timing_")
    src, exe = os.path.join(d, "time_driver.cpp"), os.path.join(d, "time_driver")
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

    class Ref:
        @staticmethod
        def time(paths, lens, vmax, amax):
            P, L, n = paths.shape
            rows = np.concatenate([_lens(lens, P, L)[:, None], paths.reshape(P, -1)], axis=1)
            head = np.concatenate([[n, L, P], np.broadcast_to(np.asarray(vmax, dtype=np.float64), n),
                                   np.broadcast_to(np.asarray(amax, dtype=np.float64), n)])
            out = run("t", head, rows).reshape(P, 2 + 2 * L + 2 * L * n)
            return dict(status=out[:, 0].astype(np.int32), duration=out[:, 1].copy(), times=out[:, 2:2 + L].copy(),
                        x=out[:, 2 + L:2 + 2 * L].copy(),
                        velocities=out[:, 2 + 2 * L:2 + 2 * L + L * n].reshape(P, L, n).copy(),
                        accelerations=out[:, 2 + 2 * L + L * n:].reshape(P, L, n).copy())

        @staticmethod
        def sample(paths, lens, timing, dt, Tout):
            P, L, n = paths.shape
            rows = np.concatenate([_lens(lens, P, L)[:, None], np.asarray(timing["status"], dtype=np.float64)[:, None],
                                   paths.reshape(P, -1), timing["times"].reshape(P, -1),
                                   timing["velocities"].reshape(P, -1)], axis=1)
            out = run("s", [n, L, P, Tout, dt], rows).reshape(P, 2, Tout, n)
            return out[:, 0].copy(), out[:, 1].copy()

    return Ref()


def derivatives(path):
    """d, c [m, n] of one path [m, n] as time_measure.hpp step 1 defines them."""
    d, c = np.zeros_like(path), np.zeros_like(path)
    d[0], d[-1] = path[1] - path[0], path[-1] - path[-2]
    d[1:-1] = (path[2:] - path[:-2]) / 2.0
    c[1:-1] = (path[2:] - path[1:-1]) - (path[1:-1] - path[:-2])
    return d, c


def slopes(path):
    """s_j = 1 - 2 c / d of the stages 0 .. m - 2 (NaN where d = 0)."""
    d, c = derivatives(path)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d[:-1] != 0.0, 1.0 - 2.0 * c[:-1] / d[:-1], np.nan)


def constraint_excess(path, x, vmax, amax):
    """(the largest d^2 x / v^2, the largest |d u + c x| / a) over the stages of one path [m, n] with profile x [m]."""
    d, c = derivatives(path)
    u = (x[1:] - x[:-1]) / 2.0
    vmax, amax = np.broadcast_to(vmax, path.shape[1]), np.broadcast_to(amax, path.shape[1])
    vel = np.max(d * d * x[:, None] / (vmax * vmax)[None, :])
    acc = np.max(np.abs(d[:-1] * u[:, None] + c[:-1] * x[:-1, None]) / amax[None, :])
    return vel, acc


def random_walks(rng, P, L, n, lens=None, scale=0.3):
    """P random walks [P, L, n] of `lens` waypoints each, padded with the last one."""
    paths = np.cumsum(rng.uniform(-scale, scale, (P, L, n)), axis=1)
    lens = np.full(P, L) if lens is None else np.asarray(lens)
    for p, ln in enumerate(lens):
        if 1 <= ln < L:
            paths[p, ln:] = paths[p, ln - 1]
    return paths


def gentle_paths(rng, P, L, n):
    """Gently curved paths: slope * s plus 0.05 sin(2 pi f s) over s in [0, 1], slopes of magnitude 1 .. 2 with either
    sign, f in [0.5, 1]."""
    s = np.linspace(0.0, 1.0, L)[None, :, None]
    slope = rng.uniform(1.0, 2.0, (P, 1, n)) * rng.choice([-1.0, 1.0], (P, 1, n))
    f = rng.uniform(0.5, 1.0, (P, 1, n))
    return slope * s + 0.05 * np.sin(2.0 * np.pi * f * s)


def to_device_layout(a):
    """[P, L, ...] -> [L, P, ...], contiguous: what the kernel layer takes."""
    return np.ascontiguousarray(np.swapaxes(a, 0, 1))
