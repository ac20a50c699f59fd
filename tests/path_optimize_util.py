"""optik_amd/csrc/path_optimize.hpp (on top of collision_gradient.hpp) compiled with g++ as plain C++ (no HIP runtime),
for the host and the -m gpu tests of the path optimiser; the scenes, the numpy forward kinematics and the test world
are avoid_util's.  Every file the driver reads or writes holds doubles."""
import os
import shutil
import subprocess
import tempfile

import numpy as np

from avoid_util import CSRC, Scene, _qrot, load_tables, make_test_world, numpy_frames  # noqa: F401 (re-exported)

H = 1e-5      # the step of the central differences (as tests/test_collision_gradient_host.py)
REACH = 1.5   # no point of the test arms is farther than this from a joint axis: a step H moves a point by < REACH * H


def near_a_kink(scene, frames, f, w, tol):
    """The exclusion rule of tests/test_collision_gradient_host.py: is the witness point of row f within tol of a box
    face (or of the switch between two faces inside the box) or of a grid cell wall?"""
    s, kind, idx = w
    if kind not in (1, 2):
        return False
    p = frames[f, :3] + _qrot(frames[f, 3:], scene.centers[s])
    if kind == 1:
        box = scene.boxes[idx]
        qc = np.array([-box[3], -box[4], -box[5], box[6]])
        l = _qrot(qc, p - box[:3])
        e = np.sort(np.abs(l) - box[7:10])
        return bool((np.abs(e) <= tol).any() or (np.abs(l) <= tol).any() or (e[2] < 0 and e[2] - e[1] <= 2 * tol))
    origin, voxel, _ = scene.grid
    u = (p - origin) / voxel
    return bool((np.abs(u - np.round(u)) <= tol / voxel).any())

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "path_optimize.hpp"

using namespace optik::coll;
using namespace optik::pathopt;

static std::vector<double> read_all(const char *path) {
    std::vector<double> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) return v;
    double x;
    while (std::fread(&x, sizeof(double), 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return v;
}

// scene file (avoid_util.Scene.blob): n, S, P, Ms, Mb, nx, ny, nz (0: no grid), origin (3), voxel, influence, safety,
// gain, then axes [n][3], frame [S], centers [S][3], radii [S], pairs [P][2], spheres [Ms][4], boxes [Mb][10], values
struct World {
    int n, S, P, Ms, Mb;
    std::vector<int32_t> frame, pairs;
    const double *axes, *centers, *radii, *sph, *box;
    std::vector<float> values;
    Grid g;
};

static void load_world(const std::vector<double> &m, World &s) {
    s.n = (int)m[0]; s.S = (int)m[1]; s.P = (int)m[2]; s.Ms = (int)m[3]; s.Mb = (int)m[4];
    for (int k = 0; k < 3; ++k) { s.g.n[k] = (int32_t)m[5 + k]; s.g.origin[k] = m[8 + k]; }
    s.g.inv = 1.0 / m[11];
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
    if (argv[1][0] == 'h') {
        // the hinge: records (dist, safety, e) -> (c, c')
        for (size_t i = 0; i + 3 <= in.size(); i += 3) {
            double r[2];
            hinge(in[i], in[i + 1], in[i + 2], r[0], r[1]);
            std::fwrite(r, sizeof(double), 2, out);
        }
    } else if (argv[1][0] == 'a') {
        // Ainv: M -> [M][M]
        const int M = (int)in[0];
        for (int i = 1; i <= M; ++i)
            for (int k = 1; k <= M; ++k) {
                const double v = ainv(i, k, M);
                std::fwrite(&v, sizeof(double), 1, out);
            }
    } else if (argv[1][0] == 'k') {
        // params_ok: records (step, w_smooth, w_obs, influence, safety) -> 0 / 1
        for (size_t i = 0; i + 5 <= in.size(); i += 5) {
            const double v = params_ok(Params{in[i], in[i + 1], in[i + 2], in[i + 3], in[i + 4]}) ? 1.0 : 0.0;
            std::fwrite(&v, sizeof(double), 1, out);
        }
    } else {
        // one evaluation and one update of B paths.  in: L, step, w_smooth, w_obs, influence, safety, lb [n], ub [n],
        // then per path q [L][n], frames [L][n + 2][7].  out per path: q_new [L][n], g [L][n], cost [3], clearance,
        // wp_clearance [L], dist [L][n + 2], witness [L][n + 2][3]
        if (argc < 5) return 2;
        const std::vector<double> m = read_all(argv[4]);
        World s;
        load_world(m, s);
        const int n = s.n, nf = n + 2, L = (int)in[0];
        const Params p{in[1], in[2], in[3], in[4], in[5]};
        const double *lb = &in[6], *ub = lb + n;
        const size_t head = 6 + 2 * n, rec = (size_t)L * n + (size_t)L * nf * 7;
        std::vector<double> dist(L * nf), grad(L * nf * n), qn(L * n), g(L * n), wc(L), row;
        std::vector<int32_t> wit(3 * L * nf);
        for (size_t b = 0; head + (b + 1) * rec <= in.size(); ++b) {
            const double *q = &in[head + b * rec], *fr = q + L * n;
            for (int t = 0; t < L; ++t)
                witness_rows(n, fr + 7 * nf * t, s.axes, s.S, s.frame.data(), s.centers, s.radii, s.P, s.pairs.data(),
                             s.Ms, s.sph, s.Mb, s.box, s.g, &dist[t * nf], &wit[3 * t * nf], &grad[t * nf * n]);
            double cost[3], clr;
            path_step(n, L, q, dist.data(), grad.data(), lb, ub, p, cost, &clr, wc.data(), g.data(), qn.data());
            row.assign(qn.begin(), qn.end());
            row.insert(row.end(), g.begin(), g.end());
            row.insert(row.end(), cost, cost + 3);
            row.push_back(clr);
            row.insert(row.end(), wc.begin(), wc.end());
            row.insert(row.end(), dist.begin(), dist.end());
            for (int32_t w : wit) row.push_back((double)w);
            std::fwrite(row.data(), sizeof(double), row.size(), out);
        }
    }
    std::fclose(out);
    return 0;
}
"""


class Params:
    def __init__(self, step, w_smooth, w_obs, influence, safety):
        self.step, self.w_smooth, self.w_obs, self.influence, self.safety = step, w_smooth, w_obs, influence, safety

    def array(self):
        return np.array([self.step, self.w_smooth, self.w_obs, self.influence, self.safety], dtype=np.float64)


def build_path_optimize(workdir=None):
    """Compile the driver; returns an object with
    .hinge(dist, safety, e) -> c, c' (arrays),
    .ainv(M) -> [M, M],
    .params_ok(rows [N, 5]) -> bool [N],
    .step(scene, params, lb, ub, q [B, L, n], frames [B, L, n + 2, 7]) -> dict(q [B, L, n], g [B, L, n], cost [B, 3],
      clearance [B], wp_clearance [B, L], dist [B, L, n + 2], witness [B, L, n + 2, 3]): one evaluation of every
      path and the update that follows it,
    .optimize(scene, params, lb, ub, q [L, n], iters, frames_of) -> (q, first, last): `iters` updates of one path with
      frames_of(x) -> [n + 2, 7], and the step() records of the first and of the last evaluation."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the path optimiser's header on its own"
    d = workdir or tempfile.mkdtemp(prefix="pathopt_")
    src, exe = os.path.join(d, "pathopt_driver.cpp"), os.path.join(d, "pathopt_driver")
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

    class PathOptimize:
        @staticmethod
        def hinge(dist, safety, e):
            dist = np.atleast_1d(np.asarray(dist, dtype=np.float64))
            rec = np.stack([dist, np.full_like(dist, safety), np.full_like(dist, e)], axis=1)
            out = run("h", rec).reshape(len(dist), 2)
            return out[:, 0].copy(), out[:, 1].copy()

        @staticmethod
        def ainv(M):
            return run("a", np.array([float(M)])).reshape(M, M)

        @staticmethod
        def params_ok(rows):
            return run("k", np.asarray(rows, dtype=np.float64).reshape(-1, 5)) != 0.0

        @staticmethod
        def step(scene, params, lb, ub, q, frames):
            q = np.ascontiguousarray(q, dtype=np.float64)
            B, L, n = q.shape
            F = n + 2
            frames = np.ascontiguousarray(frames, dtype=np.float64).reshape(B, L, F, 7)
            assert n == scene.n
            head = np.concatenate([[float(L)], params.array(), np.asarray(lb, dtype=np.float64),
                                   np.asarray(ub, dtype=np.float64)])
            rec = np.concatenate([q.reshape(B, -1), frames.reshape(B, -1)], axis=1)
            w = 2 * L * n + 4 + L + L * F + 3 * L * F
            out = run("s", np.concatenate([head, rec.ravel()]), scene).reshape(B, w)
            o = 0
            res = {}
            for name, shape in (("q", (L, n)), ("g", (L, n)), ("cost", (3,)), ("clearance", ()), ("wp_clearance", (L,)),
                                ("dist", (L, F)), ("witness", (L, F, 3))):
                size = int(np.prod(shape, dtype=np.int64))
                res[name] = out[:, o:o + size].reshape((B,) + shape).copy()
                o += size
            res["witness"] = res["witness"].astype(np.int32)
            return res

        @staticmethod
        def optimize(scene, params, lb, ub, q, iters, frames_of):
            q = np.array(q, dtype=np.float64)
            first = last = None
            for it in range(iters + 1):
                frames = np.array([frames_of(x) for x in q])
                last = PathOptimize.step(scene, params, lb, ub, q[None], frames[None])
                if it == 0:
                    first = last
                if it < iters:
                    q = last["q"][0]
            return q, first, last

    return PathOptimize()


def blocked_scene():
    """The fixed scene of the optimiser tests: a Panda with the 6-sphere model of
    spheres_along_chain(robot, 0.05, 2), two free configurations, and one world sphere that the straight joint-space line between them
    passes through.  Returns dict(robot, frames, centers, radii, spheres, qa, qb, influence, safety, L)."""
    from conftest import ROBOT_SPECS
    from optik_amd import Robot
    from optik_amd.collision import spheres_along_chain
    robot = Robot.from_urdf_file(*ROBOT_SPECS["panda"])
    frames, centers, radii = spheres_along_chain(robot, 0.05, 2)
    return dict(robot=robot, frames=frames, centers=centers, radii=radii, qa=np.array(BLOCKED_QA),
                qb=np.array(BLOCKED_QB), spheres=np.array([BLOCKED_SPHERE]), influence=0.2, safety=0.05, L=16)


# (found on the CPU with the host reference alone: tests/test_path_optimize_host.py asserts that it is solved there)
BLOCKED_QA = [-0.9, 0.4, 0.0, -1.8, 0.0, 2.2, 0.7]
BLOCKED_QB = [0.9, 0.4, 0.0, -1.8, 0.0, 2.2, 0.7]
BLOCKED_SPHERE = [0.55, 0.0, 0.45, 0.08]


def line_path(qa, qb, L):
    """The linear interpolation of two configurations, [L, n], the endpoints exactly qa and qb."""
    s = np.linspace(0.0, 1.0, L)[:, None]
    path = (1.0 - s) * np.asarray(qa)[None] + s * np.asarray(qb)[None]
    path[0], path[-1] = qa, qb
    return path
