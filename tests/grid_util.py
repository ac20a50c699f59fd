"""The distance-field world of optik_amd/csrc/collision_measure.hpp (steps 5 - 7: grid_distance, clearance_grid,
primitive_field) compiled with g++ as plain C++ (no HIP runtime), for the host and the -m gpu tests of the grid.

Every file the driver reads or writes holds doubles; the grid's float32 values travel as doubles (exact both ways)."""
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

// grid file: origin (3), voxel, nx, ny, nz, then the values (none for the bake)
struct HostGrid {
    Grid g;
    double voxel;
    std::vector<float> v;
};

static void load_grid(const char *path, HostGrid &h) {
    const std::vector<double> m = read_all(path);
    for (int k = 0; k < 3; ++k) h.g.origin[k] = m[k];
    h.voxel = m[3];
    h.g.inv = 1.0 / h.voxel;
    for (int k = 0; k < 3; ++k) h.g.n[k] = (int32_t)m[4 + k];
    h.v.resize(m.size() - 7);
    for (size_t i = 7; i < m.size(); ++i) h.v[i - 7] = (float)m[i];
    h.g.values = h.v.empty() ? nullptr : h.v.data();
}

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    const std::vector<double> in = read_all(argv[2]);
    FILE *out = std::fopen(argv[3], "wb");
    if (!out) return 2;
    HostGrid h;
    load_grid(argv[4], h);
    if (argv[1][0] == 'd') {
        // grid_distance: records of 4 doubles: p (3), r
        for (size_t i = 0; i + 4 <= in.size(); i += 4) {
            const double d = grid_distance(&in[i], in[i + 3], h.g);
            std::fwrite(&d, sizeof(double), 1, out);
        }
    } else if (argv[1][0] == 'b') {
        // bake: argv[2] = world (Ms, Mb, spheres[4Ms], boxes[10Mb]); every node, z fastest, as (double)(float)field
        const int Ms = (int)in[0], Mb = (int)in[1];
        const double *sph = in.data() + 2, *box = sph + 4 * Ms;
        for (int i = 0; i < h.g.n[0]; ++i)
            for (int j = 0; j < h.g.n[1]; ++j)
                for (int k = 0; k < h.g.n[2]; ++k) {
                    double p[3];
                    grid_node(h.g.origin, h.voxel, i, j, k, p);
                    const double d = (double)(float)primitive_field(p, sph, Ms, box, Mb);
                    std::fwrite(&d, sizeof(double), 1, out);
                }
    } else {
        // clearance_grid: argv[5] = model (nf, S, frame[S], centers[3S], radii[S]); argv[2] = frames [B][nf][7]
        if (argc < 6) return 2;
        const std::vector<double> m = read_all(argv[5]);
        const int nf = (int)m[0], S = (int)m[1];
        size_t o = 2;
        std::vector<int32_t> frame(S);
        for (int s = 0; s < S; ++s) frame[s] = (int32_t)m[o++];
        const double *centers = m.data() + o; o += 3 * S;
        const double *radii = m.data() + o;
        for (size_t b = 0; (b + 1) * 7 * nf <= in.size(); ++b) {
            const double c = clearance_grid(nf, &in[b * 7 * nf], S, frame.data(), centers, radii, h.g);
            std::fwrite(&c, sizeof(double), 1, out);
        }
    }
    std::fclose(out);
    return 0;
}
"""


def _grid_file(path, origin, voxel, shape, values=None):
    head = np.concatenate([np.asarray(origin, dtype=np.float64).ravel(), [float(voxel)], np.asarray(shape, dtype=np.float64)])
    if values is not None:
        values = np.asarray(values, dtype=np.float32)
        assert values.shape == tuple(shape)
        head = np.concatenate([head, values.astype(np.float64).ravel()])
    head.tofile(path)


def build_grid_measure(workdir=None):
    """Compile the driver; returns an object with
    .grid_distance(points [N, 3], radii [N], origin, voxel, values) -> d [N],
    .clearance_grid(frames [B, nf, 7], sphere_frames, centers, radii, origin, voxel, values) -> [B] and
    .bake(origin, voxel, shape, spheres, boxes) -> float32 [nx, ny, nz]."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the collision header on its own"
    d = workdir or tempfile.mkdtemp(prefix="grid_measure_")
    src, exe = os.path.join(d, "grid_driver.cpp"), os.path.join(d, "grid_driver")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe],
                   check=True)

    class GridMeasure:
        @staticmethod
        def grid_distance(points, radii, origin, voxel, values):
            points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
            recs = np.concatenate([points, np.broadcast_to(np.asarray(radii, dtype=np.float64), (len(points),))[:, None]], 1)
            fin, fout, fg = (os.path.join(d, x) for x in ("pts.bin", "dist_out.bin", "grid.bin"))
            np.ascontiguousarray(recs).tofile(fin)
            _grid_file(fg, origin, voxel, np.asarray(values).shape, values)
            subprocess.run([exe, "d", fin, fout, fg], check=True)
            out = np.fromfile(fout, dtype=np.float64)
            assert out.shape == (len(points),)
            return out

        @staticmethod
        def clearance_grid(frames, sphere_frames, centers, radii, origin, voxel, values):
            frames = np.ascontiguousarray(frames, dtype=np.float64)
            B, nf = frames.shape[0], frames.shape[1]
            sf = np.asarray(sphere_frames, dtype=np.float64).ravel()
            S = len(sf)
            model = np.concatenate([[nf, S], sf, np.asarray(centers, dtype=np.float64).ravel(),
                                    np.broadcast_to(np.asarray(radii, dtype=np.float64), (S,))])
            fm, fin, fout, fg = (os.path.join(d, x) for x in ("gmodel.bin", "gframes.bin", "gclr_out.bin", "grid.bin"))
            model.tofile(fm)
            frames.tofile(fin)
            _grid_file(fg, origin, voxel, np.asarray(values).shape, values)
            subprocess.run([exe, "c", fin, fout, fg, fm], check=True)
            out = np.fromfile(fout, dtype=np.float64)
            assert out.shape == (B,)
            return out

        @staticmethod
        def bake(origin, voxel, shape, spheres=None, boxes=None):
            spheres = np.zeros((0, 4)) if spheres is None else np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
            boxes = np.zeros((0, 10)) if boxes is None else np.asarray(boxes, dtype=np.float64).reshape(-1, 10)
            fw, fout, fg = (os.path.join(d, x) for x in ("world.bin", "bake_out.bin", "gridgeom.bin"))
            np.concatenate([[len(spheres), len(boxes)], spheres.ravel(), boxes.ravel()]).tofile(fw)
            _grid_file(fg, origin, voxel, shape)
            subprocess.run([exe, "b", fw, fout, fg], check=True)
            out = np.fromfile(fout, dtype=np.float64)
            assert out.shape == (int(np.prod(shape)),)
            f32 = out.astype(np.float32)
            assert (f32.astype(np.float64) == out).all()
            return f32.reshape(tuple(shape))

    return GridMeasure()
