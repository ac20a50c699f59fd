"""optik_amd/csrc/collision_gradient.hpp and diff_ik_lp.hpp's diff_ik_lp_damped compiled with g++ as plain C++ (no HIP
runtime), and a numpy forward kinematics from the oracle.urdf_chain tables, for the host and the -m gpu tests of the
clearance witnesses and of collision-avoiding diff_ik.  Every file the driver reads or writes holds doubles."""
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optik_amd", "csrc")
MAXN = 8
MAXM = 4
LP_IN = 1 + 4 + 6 * MAXN + 6 + MAXN + 1 + MAXM * MAXN + MAXM  # n, quat, jac, V, v_max, m, G (stride n), h
LP_OUT = 2 + MAXN                                            # status, alpha, v

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "collision_gradient.hpp"
#include "diff_ik_lp.hpp"

using namespace optik::coll;

static std::vector<double> read_all(const char *path) {
    std::vector<double> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) return v;
    double x;
    while (std::fread(&x, sizeof(double), 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return v;
}

// scene file: n, S, P, Ms, Mb, nx, ny, nz (0: no grid), origin (3), voxel, influence, safety, gain, then axes [n][3],
// frame [S], centers [S][3], radii [S], pairs [P][2], spheres [Ms][4], boxes [Mb][10], grid values
struct Scene {
    int n, S, P, Ms, Mb;
    std::vector<int32_t> frame, pairs;
    const double *axes, *centers, *radii, *sph, *box;
    std::vector<float> values;
    Grid g;
    double influence, safety, gain;
};

static void load_scene(const std::vector<double> &m, Scene &s) {
    s.n = (int)m[0]; s.S = (int)m[1]; s.P = (int)m[2]; s.Ms = (int)m[3]; s.Mb = (int)m[4];
    for (int k = 0; k < 3; ++k) { s.g.n[k] = (int32_t)m[5 + k]; s.g.origin[k] = m[8 + k]; }
    s.g.inv = 1.0 / m[11];
    s.influence = m[12]; s.safety = m[13]; s.gain = m[14];
    size_t o = 15;
    s.axes = &m[o]; o += 3 * s.n;
    s.frame.resize(s.S);
    for (int i = 0; i < s.S; ++i) s.frame[i] = (int32_t)m[o++];
    s.centers = m.data() + o; o += 3 * s.S;
    s.radii = m.data() + o; o += s.S;
    s.pairs.resize(2 * s.P);
    for (int i = 0; i < 2 * s.P; ++i) s.pairs[i] = (int32_t)m[o++];
    s.sph = m.data() + o; o += 4 * s.Ms;
    s.box = m.data() + o; o += 10 * s.Mb;
    const size_t nodes = (size_t)s.g.n[0] * s.g.n[1] * s.g.n[2];
    s.values.resize(nodes);
    for (size_t i = 0; i < nodes; ++i) s.values[i] = (float)m[o++];
    s.g.values = nodes ? s.values.data() : nullptr;
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    const std::vector<double> in = read_all(argv[2]);
    FILE *out = std::fopen(argv[3], "wb");
    if (!out) return 2;
    if (argv[1][0] == 'l' || argv[1][0] == 'p') {
        // the LPs: 'l' diff_ik_lp_damped, 'p' diff_ik_lp (m, G, h ignored)
        for (size_t i = 0; i + %(lp_in)d <= in.size(); i += %(lp_in)d) {
            const double *rec = &in[i];
            const int n = (int)rec[0];
            const double *quat = rec + 1, *jac = quat + 4, *V = jac + 6 * %(maxn)d, *vmax = V + 6;
            const int m = (int)vmax[%(maxn)d];
            const double *G = vmax + %(maxn)d + 1, *h = G + %(maxm)d * %(maxn)d;
            double res[%(lp_out)d] = {0};
            res[0] = argv[1][0] == 'l'
                         ? optik::lp::diff_ik_lp_damped<%(maxn)d>(n, quat, jac, V, vmax, m, G, h, &res[1], &res[2])
                         : optik::lp::diff_ik_lp<%(maxn)d>(n, quat, jac, V, vmax, &res[1], &res[2]);
            std::fwrite(res, sizeof(double), %(lp_out)d, out);
        }
        std::fclose(out);
        return 0;
    }
    if (argv[1][0] == 's') {
        // select_damper_rows: records of 2 + 16 doubles: nf, influence, dist [16]; out: m, sel [4]
        for (size_t i = 0; i + 18 <= in.size(); i += 18) {
            const double *d = &in[i + 2];
            int sel[4];
            const int mr = select_damper_rows((int)in[i], in[i + 1], [&](int f) { return d[f]; }, sel);
            const double res[5] = {(double)mr, (double)sel[0], (double)sel[1], (double)sel[2], (double)sel[3]};
            std::fwrite(res, sizeof(double), 5, out);
        }
        std::fclose(out);
        return 0;
    }
    if (argc < 5) return 2;
    const std::vector<double> m = read_all(argv[4]);
    Scene s;
    load_scene(m, s);
    const int n = s.n, nf = n + 2;
    std::vector<double> dist(nf), grad(nf * n), row;
    std::vector<int32_t> wit(3 * nf);
    if (argv[1][0] == 'w') {
        // witness rows: in = frames [B][nf][7]; out per configuration: dist [nf], witness [nf][3], grad [nf][n]
        for (size_t b = 0; (b + 1) * 7 * nf <= in.size(); ++b) {
            witness_rows(n, &in[b * 7 * nf], s.axes, s.S, s.frame.data(), s.centers, s.radii, s.P, s.pairs.data(), s.Ms,
                         s.sph, s.Mb, s.box, s.g, dist.data(), wit.data(), grad.data());
            row.assign(dist.begin(), dist.end());
            for (int32_t w : wit) row.push_back((double)w);
            row.insert(row.end(), grad.begin(), grad.end());
            std::fwrite(row.data(), sizeof(double), row.size(), out);
        }
    } else {
        // the chain of diff_ik_avoid: in = per row frames [nf][7], jac [6n], V [6], v_max [n];
        // out: status, alpha, v [n], m, frames of the rows [4], h [4], G [4][n]
        const size_t rec = 7 * nf + 6 * n + 6 + n;
        for (size_t b = 0; (b + 1) * rec <= in.size(); ++b) {
            const double *fr = &in[b * rec], *jac = fr + 7 * nf, *V = jac + 6 * n, *vmax = V + 6;
            witness_rows(n, fr, s.axes, s.S, s.frame.data(), s.centers, s.radii, s.P, s.pairs.data(), s.Ms, s.sph,
                         s.Mb, s.box, s.g, dist.data(), wit.data(), grad.data());
            bool nan = false;
            for (int f = 0; f < nf; ++f) nan = nan || dist[f] != dist[f];
            int sel[4];
            const int mr = select_damper_rows(nf, s.influence, [&](int f) { return dist[f]; }, sel);
            double G[4 * %(maxn)d] = {0}, h[4] = {0};
            for (int r = 0; r < mr && !nan; ++r) {
                h[r] = damper_rhs(dist[sel[r]], s.influence, s.safety, s.gain);
                for (int j = 0; j < n; ++j) G[r * n + j] = grad[sel[r] * n + j];
            }
            std::vector<double> res(2 + n + 1 + 4 + 4 + 4 * n, 0.0);
            res[0] = nan ? 1 : optik::lp::diff_ik_lp_damped<%(maxn)d>(n, fr + 7 * (n + 1) + 3, jac, V, vmax, mr, G, h,
                                                                      &res[1], &res[2]);
            if (res[0] != 0.0) for (int j = 0; j <= n; ++j) res[1 + j] = 0.0;
            res[2 + n] = mr;
            for (int r = 0; r < 4; ++r) { res[3 + n + r] = sel[r]; res[7 + n + r] = h[r]; }
            for (int k = 0; k < 4 * n; ++k) res[11 + n + k] = G[k];
            std::fwrite(res.data(), sizeof(double), res.size(), out);
        }
    }
    std::fclose(out);
    return 0;
}
""" % dict(lp_in=LP_IN, lp_out=LP_OUT, maxn=MAXN, maxm=MAXM)


def _qmul(a, b):
    ai, aj, ak, aw = a
    bi, bj, bk, bw = b
    return np.array([aw * bi + ai * bw + aj * bk - ak * bj, aw * bj - ai * bk + aj * bw + ak * bi,
                     aw * bk + ai * bj - aj * bi + ak * bw, aw * bw - ai * bi - aj * bj - ak * bk])


def _qrot(q, v):
    t = 2.0 * np.cross(q[:3], v)
    return t * q[3] + np.cross(q[:3], t) + v


def load_tables(path, base, ee):
    """The oracle's chain tables of a URDF: dict(types, origins [J, 7], axes [J, 3], lb, ub)."""
    from oracle.urdf_chain import chain_from_urdf
    with open(path) as fh:
        return chain_from_urdf(fh.read(), base, ee)


def numpy_frames(tables, q):
    """The n + 2 frames [n + 2, 7] (t, then the quaternion i, j, k, w) of a revolute chain at q: frame 0 the base,
    k after joint k (its origin, then its rotation), n + 1 the end effector (with the trailing fixed joint)."""
    n = len(q)
    out = np.zeros((n + 2, 7))
    out[0, 6] = 1.0
    t, r = np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0])
    for j in range(n):
        o = tables["origins"][j]
        half = 0.5 * q[j]
        local = np.concatenate([tables["axes"][j] * np.sin(half), [np.cos(half)]])
        t, r = t + _qrot(r, o[:3]), _qmul(r, _qmul(o[3:], local))
        out[j + 1, :3], out[j + 1, 3:] = t, r
    if len(tables["origins"]) > n:
        o = tables["origins"][n]
        t, r = t + _qrot(r, o[:3]), _qmul(r, o[3:])
    out[n + 1, :3], out[n + 1, 3:] = t, r
    return out


class Scene:
    """A model and a world as the driver reads them."""

    def __init__(self, axes, frames, centers, radii, pairs=None, spheres=None, boxes=None, grid=None,
                 influence=0.2, safety=0.05, gain=1.0):
        self.axes = np.asarray(axes, dtype=np.float64).reshape(-1, 3)
        self.n = len(self.axes)
        self.frames = np.asarray(frames, dtype=np.float64).ravel()
        S = len(self.frames)
        self.centers = np.asarray(centers, dtype=np.float64).reshape(S, 3)
        self.radii = np.broadcast_to(np.asarray(radii, dtype=np.float64), (S,))
        self.pairs = np.zeros((0, 2)) if pairs is None else np.asarray(pairs, dtype=np.float64).reshape(-1, 2)
        self.spheres = np.zeros((0, 4)) if spheres is None else np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
        self.boxes = np.zeros((0, 10)) if boxes is None else np.asarray(boxes, dtype=np.float64).reshape(-1, 10)
        self.grid = grid  # (origin [3], voxel, values float32 [nx, ny, nz]) or None
        self.influence, self.safety, self.gain = influence, safety, gain

    def blob(self):
        if self.grid is None:
            shape, origin, voxel, values = (0, 0, 0), np.zeros(3), 1.0, np.zeros(0)
        else:
            origin, voxel, values = self.grid
            values = np.asarray(values, dtype=np.float32)
            shape, values = values.shape, values.astype(np.float64).ravel()
        return np.concatenate([[self.n, len(self.frames), len(self.pairs), len(self.spheres), len(self.boxes)],
                               np.asarray(shape, dtype=np.float64), np.asarray(origin, dtype=np.float64), [voxel],
                               [self.influence, self.safety, self.gain], self.axes.ravel(), self.frames,
                               self.centers.ravel(), self.radii, self.pairs.ravel(), self.spheres.ravel(),
                               self.boxes.ravel(), values])


def build_avoid(workdir=None):
    """Compile the driver; returns an object with
    .witness(scene, frames [B, F, 7]) -> dist [B, F], witness [B, F, 3] int32, grad [B, F, n],
    .avoid(scene, frames [B, F, 7], jac [B, 6n], V [B, 6], v_max [B, n]) -> dict(status, alpha, v, m, rows, h, G),
    .select(dists, influence) -> m [N], sel [N, 4] (select_damper_rows),
    .lp(cases, damped=True) -> [N, 2 + MAXN] (status, alpha, v) for cases (n, quat, J 6 x n, V, v_max, G m x n, h)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the collision headers on their own"
    d = workdir or tempfile.mkdtemp(prefix="avoid_")
    src, exe = os.path.join(d, "avoid_driver.cpp"), os.path.join(d, "avoid_driver")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe],
                   check=True)

    def run(mode, data, scene=None):
        fin, fout, fs = (os.path.join(d, x) for x in ("in.bin", "out.bin", "scene.bin"))
        np.ascontiguousarray(data, dtype=np.float64).tofile(fin)
        cmd = [exe, mode, fin, fout]
        if scene is not None:
            scene.blob().tofile(fs)
            cmd.append(fs)
        subprocess.run(cmd, check=True)
        return np.fromfile(fout, dtype=np.float64)

    class Avoid:
        @staticmethod
        def witness(scene, frames):
            frames = np.ascontiguousarray(frames, dtype=np.float64)
            B, F, n = frames.shape[0], frames.shape[1], scene.n
            assert F == n + 2
            out = run("w", frames, scene).reshape(B, F + 3 * F + F * n)
            return (out[:, :F].copy(), out[:, F:4 * F].astype(np.int32).reshape(B, F, 3),
                    out[:, 4 * F:].reshape(B, F, n).copy())

        @staticmethod
        def avoid(scene, frames, jac, V, v_max):
            B, n = len(frames), scene.n
            rec = np.concatenate([np.asarray(frames, dtype=np.float64).reshape(B, -1),
                                  np.asarray(jac, dtype=np.float64).reshape(B, 6 * n),
                                  np.asarray(V, dtype=np.float64).reshape(B, 6),
                                  np.asarray(v_max, dtype=np.float64).reshape(B, n)], axis=1)
            out = run("a", rec, scene).reshape(B, 11 + n + 4 * n)
            return dict(status=out[:, 0].astype(np.int32), alpha=out[:, 1].copy(), v=out[:, 2:2 + n].copy(),
                        m=out[:, 2 + n].astype(np.int32), rows=out[:, 3 + n:7 + n].astype(np.int32),
                        h=out[:, 7 + n:11 + n].copy(), G=out[:, 11 + n:].reshape(B, 4, n).copy())

        @staticmethod
        def select(dists, influence):
            """select_damper_rows for each list of row distances: (m [N], sel [N, 4])."""
            recs = np.full((len(dists), 18), np.inf)
            for i, d in enumerate(dists):
                recs[i, 0], recs[i, 1] = len(d), influence
                recs[i, 2:2 + len(d)] = d
            out = run("s", recs).reshape(len(dists), 5).astype(np.int32)
            return out[:, 0], out[:, 1:]

        @staticmethod
        def lp(cases, damped=True):
            recs = np.zeros((len(cases), LP_IN))
            for i, (n, quat, jac, V, vmax, G, h) in enumerate(cases):
                m = len(h)
                recs[i, 0] = n
                recs[i, 1:5] = quat
                recs[i, 5:5 + 6 * n] = np.asarray(jac).T.ravel()  # 6 x n -> column-major
                o = 5 + 6 * MAXN
                recs[i, o:o + 6] = V
                recs[i, o + 6:o + 6 + n] = vmax
                o += 6 + MAXN
                recs[i, o] = m
                recs[i, o + 1:o + 1 + m * n] = np.asarray(G, dtype=np.float64).reshape(m, n).ravel()
                recs[i, o + 1 + MAXM * MAXN:o + 1 + MAXM * MAXN + m] = h
            return run("l" if damped else "p", recs).reshape(len(cases), LP_OUT)

    return Avoid()


def make_test_world():
    """3 spheres, 2 rotated boxes and a 6 x 5 x 4 grid within reach of the test arms (about 0.3 .. 0.9 m from the base),
    so that random configurations have witnesses of every kind."""
    spheres = np.array([[0.45, 0.10, 0.40, 0.12], [-0.20, -0.35, 0.65, 0.10], [0.10, 0.45, 0.25, 0.15]])
    c, s = np.cos(0.35), np.sin(0.35)
    boxes = np.array([[0.55, -0.30, 0.30, 0.0, 0.0, s, c, 0.10, 0.20, 0.15],
                      [-0.40, 0.30, 0.55, s * 0.6, s * 0.8, 0.0, c, 0.15, 0.08, 0.25]])
    # a sloping field over x in [-0.6, 0.9], y in [-0.6, 0.6], z in [0.6, 1.5]: a tilted ceiling near z = 0.9
    shape, origin, voxel = (6, 5, 4), np.array([-0.6, -0.6, 0.6]), 0.3
    i, j, k = np.meshgrid(*(np.arange(m) for m in shape), indexing="ij")
    values = (0.3 - voxel * k + 0.05 * voxel * i - 0.02 * voxel * j * k).astype(np.float32)
    return spheres, boxes, (origin, voxel, values)

