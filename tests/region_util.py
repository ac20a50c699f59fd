"""optik_amd/csrc/region_measure.hpp compiled as plain host C++ (no HIP runtime; the math headers under OPTIK_LANE_EMU,
as tests/constraint_util.py compiles its driver) for the host and the -m gpu tests of IK into pose regions; the key rule
in numpy; and the regions the tests use."""
import math
import os
import subprocess
import tempfile

import numpy as np

from collision_util import CSRC
from constraint_util import EMU, PROJECTED, Constraint, _compiler

MODE_QUALITY, MODE_SPEED = 1, 2

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "region_measure.hpp"
#include "ik_host_params.hpp"

using namespace optik;

struct HostChain {
    int32_t n_pos, has_tip;
    double origin[constraint::MAXN + 1][7];
    double axis[constraint::MAXN][3];
    double lb[constraint::MAXN], ub[constraint::MAXN];
};

static std::vector<double> read_all(const char *path) {
    std::vector<double> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) return v;
    double x;
    while (std::fread(&x, sizeof(double), 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return v;
}

// in: n, has_tip, has_ee, origins [(n + 1) * 7], axes [n * 3], lb [n], ub [n], scale [n], ee [7], tol, iters, damping,
//     max_step, mode, keep_on, keep [19], keep_tol, restart_begin, R, T, regions [T][19], x0 [T][n].
// out: per column t * R + r: x [n], violation, status, iterations, key.
int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::vector<double> in = read_all(argv[1]);
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const double *p = in.data();
    HostChain ch;
    std::memset(&ch, 0, sizeof ch);
    const int n = (int)*p++;
    ch.n_pos = n;
    ch.has_tip = (int)*p++;
    EvalParams ep;
    std::memset(&ep, 0, sizeof ep);
    ep.has_ee_offset = (int)*p++;
    for (int j = 0; j <= n; ++j) for (int i = 0; i < 7; ++i) ch.origin[j][i] = *p++;
    for (int j = 0; j < n; ++j) for (int i = 0; i < 3; ++i) ch.axis[j][i] = *p++;
    for (int j = 0; j < n; ++j) ch.lb[j] = *p++;
    for (int j = 0; j < n; ++j) ch.ub[j] = *p++;
    double scale[constraint::MAXN];
    for (int j = 0; j < n; ++j) scale[j] = *p++;
    for (int i = 0; i < 7; ++i) ep.ee_offset[i] = *p++;
    const double tol = *p++;
    const int iters = (int)*p++;
    const double damping = *p++, max_step = *p++;
    const int mode = (int)*p++;
    region::Keep keep;
    std::memset(&keep, 0, sizeof keep);
    keep.on = (int)*p++;
    region::load_box(p, keep.box);
    p += region::DOUBLES;
    keep.tol = *p++;
    const uint64_t restart_begin = (uint64_t)*p++, R = (uint64_t)*p++;
    const int T = (int)*p++;
    const double *regions = p, *x0 = p + (size_t)T * region::DOUBLES;
    uint32_t key[8];
    hostparams::seed_from_u64(42, key);
    for (int t = 0; t < T; ++t)
        for (uint64_t r = 0; r < R; ++r) {
            constraint::Box box;
            region::load_box(regions + (size_t)t * region::DOUBLES, box);
            double x[constraint::MAXN];
            const region::Row row = region::restart(ch, ep, box, keep, key, scale, x0 + (size_t)t * n, restart_begin + r,
                                                    n, tol, iters, damping, max_step, mode, x);
            const double t4[4] = {row.violation, (double)row.status, (double)row.iterations, row.key};
            std::fwrite(x, sizeof(double), n, out);
            std::fwrite(t4, sizeof(double), 4, out);
        }
    std::fclose(out);
    return 0;
}
"""


def region_row(c):
    """A constraint (ref7, lo, hi) as the 19 doubles of a region."""
    return np.concatenate([np.asarray(c.ref7, dtype=np.float64), np.asarray(c.lo, dtype=np.float64),
                           np.asarray(c.hi, dtype=np.float64)])


def build_region(workdir=None):
    """Compile the driver; returns an object with
    .restarts(chain, regions [T, 19], x0 [T, n], restart_begin, R, tol, iters, damping, max_step, mode, keep=None,
              ee7=None) -> dict(x [T * R, n], v [T * R], status, iterations, key [T * R]), column t * R + r;
    chain = the dict of Robot.chain_tables() / the chains fixture, keep = (Constraint, tol)."""
    d = workdir or tempfile.mkdtemp(prefix="region_")
    src, exe = os.path.join(d, "region_driver.cpp"), os.path.join(d, "region_driver")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    subprocess.run([_compiler(), "-std=c++17", "-O2", "-ffp-contract=off", "-DOPTIK_LANE_EMU", "-pthread", "-Wall",
                    "-Wno-unused-value", "-Wno-psabi", "-Wno-unused-function", "-I", EMU, "-I", CSRC, src, "-o", exe],
                   check=True)

    class Ref:
        @staticmethod
        def restarts(chain, regions, x0, restart_begin, R, tol, iters, damping, max_step, mode, keep=None, ee7=None):
            n = len(chain["lb"])
            regions = np.atleast_2d(np.asarray(regions, dtype=np.float64))
            x0 = np.atleast_2d(np.asarray(x0, dtype=np.float64))
            T = len(regions)
            assert regions.shape == (T, 19) and x0.shape == (T, n)
            origins = np.asarray(chain["origins"], dtype=np.float64).reshape(-1, 7)
            tip = len(origins) > n
            if not tip:
                origins = np.concatenate([origins, [[0.0, 0, 0, 0, 0, 0, 1]]])
            ee = np.asarray(ee7 if ee7 is not None else [0.0, 0, 0, 0, 0, 0, 1], dtype=np.float64)
            lb, ub = np.asarray(chain["lb"], dtype=np.float64), np.asarray(chain["ub"], dtype=np.float64)
            kbox = region_row(keep[0]) if keep is not None else np.zeros(19)
            parts = [[n, int(tip), int(ee7 is not None)], origins[:n + 1], np.asarray(chain["axes"]).reshape(-1, 3)[:n],
                     lb, ub, ub - lb, ee, [tol, iters, damping, max_step, mode, int(keep is not None)], kbox,
                     [keep[1] if keep is not None else 0.0, restart_begin, R, T], regions, x0]
            fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(fin)
            subprocess.run([exe, fin, fout], check=True)
            o = np.fromfile(fout, dtype=np.float64).reshape(T * R, n + 4)
            return dict(x=o[:, :n].copy(), v=o[:, n].copy(), status=o[:, n + 1].astype(np.int32),
                        iterations=o[:, n + 2].astype(np.int32), key=o[:, n + 3].copy())

    return Ref()


def np_keys(x, x0, status, index, mode):
    """Step 3 of region_measure.hpp restated: x [B, n], x0 [B, n] (each row's own), status [B], index [B]."""
    out = np.full(len(x), np.inf)
    for b in range(len(x)):
        if status[b] != PROJECTED:
            continue
        if mode == MODE_SPEED:
            out[b] = float(index[b])
        else:
            acc = 0.0
            for k in range(x.shape[1]):
                d = float(x[b, k]) - float(x0[b, k])
                acc = acc + d * d
            out[b] = math.sqrt(acc)
    return out


# ---- the regions of the tests: around fk of a mid-range configuration -----------------------------------------------
# (chosen on the CPU: tests/test_region_host.py asserts for each that the host header projects at least 4 of the 67
# restarts and that at least 2 of them are more than MIN_DIST apart)
R, T, MIN_DIST, K = 67, 3, 0.1, 4
TOL = 1e-6
PROJECT = dict(iters=256, damping=1e-6, max_step=0.5)  # optik_amd._native.CONSTRAINT_*
ROBOTS = ("panda", "panda_hand", "arm10")  # 7 joints + fixed tip, the same with another tip frame, the wide table
POS_BOX = 0.02


def mid_config(chain):
    """A configuration inside the limits, away from their middle (where a straight arm is singular)."""
    lb, ub = np.asarray(chain["lb"]), np.asarray(chain["ub"])
    lo, hi = np.maximum(lb, -2.5), np.minimum(ub, 2.5)
    f = 0.5 + 0.2 * np.cos(1.7 * np.arange(len(lb)) + 0.4)
    return lo + f * (hi - lo)


def make_regions(ref7):
    """Pinned, axis-free about z and position-only with a 2 cm box, as Constraints."""
    inf = np.inf
    z = np.zeros(6)
    return [Constraint(ref7, z, z),
            Constraint(ref7, [0, 0, 0, 0, 0, -inf], [0, 0, 0, 0, 0, inf]),
            Constraint(ref7, [-POS_BOX] * 3 + [-inf] * 3, [POS_BOX] * 3 + [inf] * 3)]


def x0_rows(chain):
    """The three regions' own starts: the mid-range configuration moved a little, inside the limits."""
    q = mid_config(chain)
    lb, ub = np.asarray(chain["lb"]), np.asarray(chain["ub"])
    return np.array([np.clip(q + 0.15 * np.sin(np.arange(len(q)) + t), lb, ub) for t in range(T)])


def greedy(x, key, begin, Rr, k, min_dist):
    """selection_util's rule restated for one region: x [R, n], key [R]; returns the accepted restart indices."""
    order = sorted((float(key[r]), r) for r in range(Rr) if key[r] < np.inf)
    acc = []
    for _, r in order:
        if all(np.abs(x[r] - x[a]).max() > min_dist for a in acc):
            acc.append(r)
            if len(acc) == k:
                break
    return [begin + r for r in acc]
