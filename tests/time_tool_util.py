"""optik_amd/csrc/time_tool_measure.hpp compiled as plain host C++ (no HIP runtime; the math headers under
OPTIK_LANE_EMU, as tests/constraint_util.py compiles constraint_measure.hpp) for the host and the -m gpu tests of path
timing with tool limits; and the tool rows of the header restated in numpy from end-effector poses the caller brings."""
import os
import subprocess
import tempfile

import numpy as np

from collision_util import CSRC
from constraint_util import EMU, _compiler
from time_util import _lens, derivatives

LIMIT_KEYS = ("tool_v_max", "tool_a_tangential", "tool_a_normal", "tool_w_max")  # the order of lim[4]
NO_LIMITS = (np.inf, np.inf, np.inf, np.inf)

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "time_tool_measure.hpp"

using namespace optik;

struct HostChain {
    int32_t n_pos, has_tip;
    double origin[constraint::MAXN + 1][7];
    double axis[constraint::MAXN][3];
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

static void put(FILE *out, const std::vector<double> &v) { std::fwrite(v.data(), sizeof(double), v.size(), out); }

// in: n, has_tip, has_ee, origins [(n + 1) * 7], axes [n * 3], ee [7], L, P, vmax [n], amax [n], lim [4], then per path
//     len, path [L][n]
// out per path: status, duration, t [L], x [L], qd [L][n], qdd [L][n], tool_speed [L], tool_accel [L][2],
//     tool_wspeed [L], then the pose of every waypoint by tooltime::fk_ee [L][7] and by constraint::fk [L][7]
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
    for (int i = 0; i < 7; ++i) ep.ee_offset[i] = *p++;
    const int L = (int)*p++, P = (int)*p++;
    const double *vmax = p, *amax = p + n, *lim = p + 2 * n;
    p += 2 * n + 4;
    std::vector<double> t(L), x(L), qd(L * n), qdd(L * n), ts(L), ta(2 * L), tw(L), pa(7 * L), pb(7 * L);
    for (int q = 0; q < P; ++q, p += 1 + L * n) {
        const timing::Result r = tooltime::time_tool_reference(ch, ep, n, p + 1, n, (int)p[0], L, vmax, amax, lim,
                                                               t.data(), qd.data(), qdd.data(), x.data(), ts.data(),
                                                               ta.data(), tw.data());
        for (int i = 0; i < L; ++i) {
            double tf[7 * constraint::MAXN];
            bool fin = true;
            for (int j = 0; j < n; ++j) fin = fin && timing::is_finite(p[1 + i * n + j]);
            for (int c = 0; c < 7; ++c) pa[7 * i + c] = pb[7 * i + c] = 0.0;
            if (!fin) continue;  // (zeros for a waypoint that is not finite)
            tooltime::store_ee(pa.data(), 1, 7, i, tooltime::fk_ee(ch, ep, n, p + 1 + i * n, 1));
            tooltime::store_ee(pb.data(), 1, 7, i, constraint::fk(ch, ep, n, p + 1 + i * n, tf));
        }
        const double head[2] = {(double)r.status, r.duration};
        std::fwrite(head, sizeof(double), 2, out);
        put(out, t); put(out, x); put(out, qd); put(out, qdd); put(out, ts); put(out, ta); put(out, tw);
        put(out, pa); put(out, pb);
    }
    std::fclose(out);
    return 0;
}
"""


def limits4(tool_v_max=np.inf, tool_a_tangential=np.inf, tool_a_normal=np.inf, tool_w_max=np.inf):
    return np.array([tool_v_max, tool_a_tangential, tool_a_normal, tool_w_max], dtype=np.float64)


def build_time_tool_ref(workdir=None):
    """Compile the driver; chain is the dict of Robot.chain_tables(), paths [P, L, n] with lens [P] (None: L each),
    lim the four tool limits in LIMIT_KEYS' order, ee7 an optional ee_offset (t, quaternion i j k w).  Returns an object
    with .time(chain, paths, lens, vmax, amax, lim, ee7=None) -> dict(status [P] int32, duration [P], times [P, L],
    x [P, L], velocities, accelerations [P, L, n], tool_speed [P, L], tool_accel [P, L, 2], tool_wspeed [P, L], and
    ee, ee_constraint [P, L, 7]: every waypoint's pose by the header's FK and by constraint::fk)."""
    d = workdir or tempfile.mkdtemp(prefix="time_tool_")
    src, exe = os.path.join(d, "time_tool_driver.cpp"), os.path.join(d, "time_tool_driver")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([_compiler(), "-std=c++17", "-O2", "-ffp-contract=off", "-DOPTIK_LANE_EMU", "-pthread", "-Wall",
                    "-Wno-unused-value", "-Wno-psabi", "-Wno-unused-function", "-I", EMU, "-I", CSRC, src, "-o", exe],
                   check=True)

    class Ref:
        @staticmethod
        def time(chain, paths, lens, vmax, amax, lim=NO_LIMITS, ee7=None):
            paths = np.ascontiguousarray(paths, dtype=np.float64)
            P, L, n = paths.shape
            assert n == len(chain["lb"])
            origins = np.asarray(chain["origins"], dtype=np.float64).reshape(-1, 7)
            tip = len(origins) > n
            if not tip:
                origins = np.concatenate([origins, [[0.0, 0, 0, 0, 0, 0, 1]]])
            ee = np.asarray(ee7 if ee7 is not None else [0.0, 0, 0, 0, 0, 0, 1], dtype=np.float64)
            rows = np.concatenate([_lens(lens, P, L)[:, None], paths.reshape(P, -1)], axis=1)
            parts = [[n, int(tip), int(ee7 is not None)], origins[:n + 1], np.asarray(chain["axes"]).reshape(-1, 3)[:n],
                     ee, [L, P], np.broadcast_to(np.asarray(vmax, dtype=np.float64), n),
                     np.broadcast_to(np.asarray(amax, dtype=np.float64), n), np.asarray(lim, dtype=np.float64), rows]
            assert np.asarray(lim).shape == (4,)
            fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(fin)
            subprocess.run([exe, fin, fout], check=True)
            out = np.fromfile(fout, dtype=np.float64).reshape(P, 2 + 2 * L + 2 * L * n + 4 * L + 14 * L)
            o, res = 2, dict(status=out[:, 0].astype(np.int32), duration=out[:, 1].copy())
            for key, shape in (("times", (L,)), ("x", (L,)), ("velocities", (L, n)), ("accelerations", (L, n)),
                               ("tool_speed", (L,)), ("tool_accel", (L, 2)), ("tool_wspeed", (L,)), ("ee", (L, 7)),
                               ("ee_constraint", (L, 7))):
                size = int(np.prod(shape))
                res[key] = out[:, o:o + size].reshape((P,) + shape).copy()
                o += size
            return res

    return Ref()


def _qmul(a, b):
    """Quaternion product, (i, j, k, w) rows."""
    ai, aj, ak, aw = a.T
    bi, bj, bk, bw = b.T
    return np.stack([aw * bi + ai * bw + aj * bk - ak * bj, aw * bj - ai * bk + aj * bw + ak * bi,
                     aw * bk + ai * bj - aj * bi + ak * bw, aw * bw - ai * bi - aj * bj - ak * bk], axis=1)


def _qrot(q, v):
    """Rows v [m, 3] rotated by the unit quaternions q [m, 4]."""
    t = 2.0 * np.cross(q[:, :3], v)
    return v + q[:, 3:] * t + np.cross(q[:, :3], t)


def np_fk(chain, q, ee7=None):
    """The end effector's pose for the configurations q [m, n] of a revolute chain (the dict of Robot.chain_tables()),
    in numpy: positions [m, 3], unit quaternions [m, 4] (i, j, k, w).  The tests' own forward kinematics."""
    q = np.atleast_2d(np.asarray(q, dtype=np.float64))
    m, n = q.shape
    origins = np.asarray(chain["origins"], dtype=np.float64).reshape(-1, 7)
    axes = np.asarray(chain["axes"], dtype=np.float64).reshape(-1, 3)
    pos, quat = np.zeros((m, 3)), np.tile([0.0, 0.0, 0.0, 1.0], (m, 1))

    def apply(pos, quat, t, r):
        return pos + _qrot(quat, np.broadcast_to(t, (m, 3))), _qmul(quat, np.broadcast_to(r, (m, 4)))

    for j in range(n):
        pos, quat = apply(pos, quat, origins[j, :3], origins[j, 3:])
        half = q[:, j:j + 1] / 2.0
        quat = _qmul(quat, np.concatenate([axes[j][None, :] * np.sin(half), np.cos(half)], axis=1))
    if len(origins) > n:
        pos, quat = apply(pos, quat, origins[n, :3], origins[n, 3:])
    if ee7 is not None:
        ee7 = np.asarray(ee7, dtype=np.float64)
        pos, quat = apply(pos, quat, ee7[:3], ee7[3:])
    return pos, quat


def tool_terms(pos, quat):
    """The header's step T2 in numpy for one path: positions [m, 3] and unit quaternions [m, 4] (i, j, k, w) of the
    end effector at the waypoints -> g, ct, cn, w [m]."""
    D, Cc = derivatives(pos)
    g = np.linalg.norm(D, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        T = np.where(g[:, None] != 0.0, D / g[:, None], 0.0)
    ct = np.sum(Cc * T, axis=1)
    cn = np.linalg.norm(Cc - ct[:, None] * T, axis=1)
    m = len(pos)
    a = np.concatenate([[0], np.arange(0, m - 2), [m - 2]])
    b = np.concatenate([[1], np.arange(2, m), [m - 1]])
    rel = _qmul(quat[a] * np.array([-1.0, -1.0, -1.0, 1.0]), quat[b])
    rel = np.where(rel[:, 3:] < 0.0, -rel, rel)
    vn = np.linalg.norm(rel[:, :3], axis=1)
    angle = 2.0 * np.arctan2(vn, rel[:, 3])
    w = angle.copy()
    w[1:-1] /= 2.0
    return g, ct, cn, w


def tool_excess(pos, quat, x, lim):
    """(speed / v_tool, |tangential| / a_t, normal / a_n, angular speed / w_tool), each the largest over the waypoints
    of one path with profile x [m]; a limit of +inf gives 0."""
    g, ct, cn, w = tool_terms(pos, quat)
    u = np.concatenate([(x[1:] - x[:-1]) / 2.0, [0.0]])
    r = np.sqrt(x)
    tang = np.abs(g * u + ct * x)
    tang[-1] = 0.0
    return (np.max(g * r) / lim[0], np.max(tang) / lim[1], np.max(cn * x) / lim[2], np.max(w * r) / lim[3])


def tool_slopes(pos):
    """The tool row's slope 1 - 2 ct / g of the stages 0 .. m - 2 (NaN where g = 0)."""
    g, ct, _, _ = tool_terms(pos, np.tile([0.0, 0, 0, 1], (len(pos), 1)))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(g[:-1] != 0.0, 1.0 - 2.0 * ct[:-1] / g[:-1], np.nan)
