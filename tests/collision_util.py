"""The signed distances and the clearance of optik_amd/csrc/collision_measure.hpp compiled with g++ as plain C++ (no
HIP runtime), for the host and the -m gpu tests of the collision filter."""
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optik_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "collision_measure.hpp"

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

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    const std::vector<double> in = read_all(argv[2]);
    FILE *out = std::fopen(argv[3], "wb");
    if (!out) return 2;
    if (argv[1][0] == 'p') {
        // primitives: records of 15 doubles: kind (0 sphere, 1 box), p (3), r, obstacle (10: sphere = centre, radius)
        for (size_t i = 0; i + 15 <= in.size(); i += 15) {
            const double *r = &in[i];
            const double d = r[0] == 0.0 ? sphere_sphere(r + 1, r[4], r + 5, r[8]) : sphere_box(r + 1, r[4], r + 5);
            std::fwrite(&d, sizeof(double), 1, out);
        }
    } else {
        // clearance: argv[4] = model (nf, S, P, Ms, Mb, frame[S], centers[3S], radii[S], pairs[2P], spheres[4Ms],
        // boxes[10Mb]); argv[2] = frames [B][nf][7]
        const std::vector<double> m = read_all(argv[4]);
        const int nf = (int)m[0], S = (int)m[1], P = (int)m[2], Ms = (int)m[3], Mb = (int)m[4];
        size_t o = 5;
        std::vector<int32_t> frame(S), pairs(2 * P);
        for (int s = 0; s < S; ++s) frame[s] = (int32_t)m[o++];
        const double *centers = &m[o]; o += 3 * S;
        const double *radii = &m[o]; o += S;
        for (int k = 0; k < 2 * P; ++k) pairs[k] = (int32_t)m[o++];
        const double *sph = m.data() + o; o += 4 * Ms;
        const double *box = m.data() + o;
        for (size_t b = 0; (b + 1) * 7 * nf <= in.size(); ++b) {
            const double c = clearance(nf, &in[b * 7 * nf], S, frame.data(), centers, radii, P, pairs.data(), Ms, sph,
                                       Mb, box);
            std::fwrite(&c, sizeof(double), 1, out);
        }
    }
    std::fclose(out);
    return 0;
}
"""


def build_measure(workdir=None):
    """Compile the driver; returns an object with .primitives(records [N, 15]) -> d [N] and
    .clearance(frames [B, nf, 7], frames_of_spheres, centers, radii, pairs, spheres, boxes) -> [B]."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the collision header on its own"
    d = workdir or tempfile.mkdtemp(prefix="collision_measure_")
    src, exe = os.path.join(d, "driver.cpp"), os.path.join(d, "driver")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe],
                   check=True)

    class Measure:
        @staticmethod
        def primitives(records):
            records = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, 15)
            fin, fout = os.path.join(d, "prim.bin"), os.path.join(d, "prim_out.bin")
            records.tofile(fin)
            subprocess.run([exe, "p", fin, fout], check=True)
            return np.fromfile(fout, dtype=np.float64)

        @staticmethod
        def clearance(frames, sphere_frames, centers, radii, pairs=None, spheres=None, boxes=None):
            frames = np.ascontiguousarray(frames, dtype=np.float64)
            B, nf = frames.shape[0], frames.shape[1]
            sf = np.asarray(sphere_frames, dtype=np.float64).ravel()
            S = len(sf)
            pairs = np.zeros((0, 2)) if pairs is None else np.asarray(pairs, dtype=np.float64).reshape(-1, 2)
            spheres = np.zeros((0, 4)) if spheres is None else np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
            boxes = np.zeros((0, 10)) if boxes is None else np.asarray(boxes, dtype=np.float64).reshape(-1, 10)
            model = np.concatenate([[nf, S, len(pairs), len(spheres), len(boxes)], sf,
                                    np.asarray(centers, dtype=np.float64).ravel(),
                                    np.broadcast_to(np.asarray(radii, dtype=np.float64), (S,)),
                                    pairs.ravel(), spheres.ravel(), boxes.ravel()])
            fm, fin, fout = (os.path.join(d, x) for x in ("model.bin", "frames.bin", "clr_out.bin"))
            model.tofile(fm)
            frames.tofile(fin)
            subprocess.run([exe, "c", fin, fout, fm], check=True)
            out = np.fromfile(fout, dtype=np.float64)
            assert out.shape == (B,)
            return out

    return Measure()


def small_scene(robot):
    """A small scene for tests that need some model and world rather than a particular one: (model, spheres) -- the
    keyword arguments of Robot.set_collision_model (two spheres per link of the chain, "auto" pairs, a 1 cm margin) and
    two world spheres [2, 4] within reach, so that random configurations are a mix of free and colliding ones."""
    from optik_amd.collision import auto_pairs, spheres_along_chain
    frames, centers, radii = spheres_along_chain(robot, 0.05, 2)
    model = dict(frames=frames, centers=centers, radii=radii, self_pairs=auto_pairs(frames), margin=0.01)
    return model, np.array([[0.45, 0.10, 0.40, 0.12], [-0.20, -0.35, 0.65, 0.10]])
