"""Steps 8 and 9 of optik_amd/csrc/collision_measure.hpp (occupancy_field, voxelize) compiled with g++ as plain C++
(no HIP runtime), and the references the host and the -m gpu tests of the occupancy path share: brute-force integer
squared distances and numpy's reading of both steps.

Every file the driver reads or writes holds doubles; bytes and float32 values travel as doubles (exact both ways)."""
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
    // grid file: origin (3), voxel, max_distance, nx, ny, nz, then the occupancy of every node
    const std::vector<double> g = read_all(argv[2]);
    const double *origin = g.data(), voxel = g[3], max_distance = g[4];
    const int32_t n[3] = {(int32_t)g[5], (int32_t)g[6], (int32_t)g[7]};
    const size_t nodes = (size_t)n[0] * n[1] * n[2];
    if (g.size() != 8 + nodes) return 2;
    std::vector<uint8_t> occ(nodes);
    for (size_t i = 0; i < nodes; ++i) occ[i] = (uint8_t)g[8 + i];
    FILE *out = std::fopen(argv[3], "wb");
    if (!out) return 2;
    if (argv[1][0] == 'f') {
        // step 8: every node's value as (double)(float)
        std::vector<EdtPair> a(nodes), b(nodes);
        std::vector<float> v(nodes);
        occupancy_field(occ.data(), n[0], n[1], n[2], voxel, max_distance, a.data(), b.data(), v.data());
        for (size_t i = 0; i < nodes; ++i) {
            const double d = (double)v[i];
            std::fwrite(&d, sizeof(double), 1, out);
        }
    } else {
        // step 9: argv[4] = points [N][3], argv[5] = exclusion spheres [E][4]; the occupancy afterwards
        if (argc < 6) return 2;
        const std::vector<double> pts = read_all(argv[4]), exc = read_all(argv[5]);
        voxelize(origin, voxel, n, pts.data(), (long long)(pts.size() / 3), exc.data(), (int)(exc.size() / 4),
                 occ.data());
        for (size_t i = 0; i < nodes; ++i) {
            const double d = (double)occ[i];
            std::fwrite(&d, sizeof(double), 1, out);
        }
    }
    std::fclose(out);
    return 0;
}
"""


def build_occupancy_measure(workdir=None):
    """Compile the driver; returns an object with
    .field(voxel, occupied [nx, ny, nz], max_distance) -> float32 [nx, ny, nz] and
    .voxelize(origin, voxel, shape, points [N, 3], exclude [E, 4] or None, into=None) -> bool [nx, ny, nz]."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the collision header on its own"
    d = workdir or tempfile.mkdtemp(prefix="occupancy_measure_")
    src, exe = os.path.join(d, "occupancy_driver.cpp"), os.path.join(d, "occupancy_driver")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe],
                   check=True)

    def grid_file(path, origin, voxel, max_distance, occupied):
        occupied = np.asarray(occupied)
        np.concatenate([np.asarray(origin, dtype=np.float64).ravel(), [float(voxel), float(max_distance)],
                        np.asarray(occupied.shape, dtype=np.float64),
                        (occupied != 0).astype(np.float64).ravel()]).tofile(path)

    class OccupancyMeasure:
        @staticmethod
        def field(voxel, occupied, max_distance):
            occupied = np.asarray(occupied)
            fg, fout = os.path.join(d, "occ.bin"), os.path.join(d, "field_out.bin")
            grid_file(fg, [0.0, 0.0, 0.0], voxel, max_distance, occupied)
            subprocess.run([exe, "f", fg, fout], check=True)
            out = np.fromfile(fout, dtype=np.float64)
            assert out.shape == (occupied.size,)
            f32 = out.astype(np.float32)
            assert (f32.astype(np.float64) == out).all()
            return f32.reshape(occupied.shape)

        @staticmethod
        def voxelize(origin, voxel, shape, points, exclude=None, into=None):
            occupied = np.zeros(shape, dtype=np.uint8) if into is None else np.asarray(into)
            fg, fout, fp, fe = (os.path.join(d, x) for x in ("vgrid.bin", "vox_out.bin", "points.bin", "exclude.bin"))
            grid_file(fg, origin, voxel, 1.0, occupied)
            np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3).tofile(fp)
            (np.zeros((0, 4)) if exclude is None else np.ascontiguousarray(exclude, dtype=np.float64)).tofile(fe)
            subprocess.run([exe, "v", fg, fout, fp, fe], check=True)
            out = np.fromfile(fout, dtype=np.float64)
            assert out.shape == (int(np.prod(shape)),)
            return (out != 0).reshape(tuple(shape))

    return OccupancyMeasure()


# ---- the references ---------------------------------------------------------------------------------------------------

def brute_d2(source):
    """The exact squared distance in voxel units from every node to the nearest True node of `source` [nx, ny, nz]:
    all nodes against all source nodes, in int64.  -1 everywhere when there is no source node."""
    source = np.asarray(source, dtype=bool)
    out = np.full(source.shape, -1, dtype=np.int64)
    src = np.argwhere(source).astype(np.int64)  # [M, 3]
    if len(src) == 0:
        return out
    nodes = np.stack(np.meshgrid(*(np.arange(s, dtype=np.int64) for s in source.shape), indexing="ij"), -1).reshape(-1, 3)
    best = np.full(len(nodes), np.iinfo(np.int64).max)
    chunk = max(1, (1 << 22) // max(1, len(src)))  # ~4 M pairs at a time
    for a in range(0, len(nodes), chunk):
        d = nodes[a:a + chunk, None, :] - src[None, :, :]
        best[a:a + chunk] = (d * d).sum(-1).min(1)
    return best.reshape(source.shape)


def field_reference(voxel, occupied, max_distance, d2_occ=None, d2_free=None):
    """Step 8 as numpy reads it, from brute-force D2: float32 [nx, ny, nz]."""
    occupied = np.asarray(occupied) != 0
    d2_occ = brute_d2(occupied) if d2_occ is None else d2_occ
    d2_free = brute_d2(~occupied) if d2_free is None else d2_free
    md = float(max_distance)
    if not occupied.any():
        return np.full(occupied.shape, md, dtype=np.float32)
    if occupied.all():
        return np.full(occupied.shape, -md, dtype=np.float32)
    pos = np.float32(np.clip(float(voxel) * (np.sqrt(d2_occ.astype(np.float64)) - 0.5), -md, md))
    neg = np.float32(np.clip(-(float(voxel) * (np.sqrt(d2_free.astype(np.float64)) - 0.5)), -md, md))
    return np.where(occupied, neg, pos).astype(np.float32)


def voxelize_reference(origin, voxel, shape, points, exclude=None, into=None):
    """Step 9 as numpy reads it: bool [nx, ny, nz]."""
    occ = np.zeros(shape, dtype=bool) if into is None else (np.asarray(into) != 0).copy()
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    inv = 1.0 / float(voxel)
    with np.errstate(invalid="ignore", over="ignore"):
        w = (p - np.asarray(origin, dtype=np.float64)) * inv + 0.5
        inside = ((w >= 0.0) & (w < np.asarray(shape, dtype=np.float64))).all(1)
        keep = inside.copy()
        if exclude is not None and len(exclude):
            e = np.asarray(exclude, dtype=np.float64).reshape(-1, 4)
            d = p[:, None, :] - e[None, :, :3]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            keep &= ~(d2 <= e[None, :, 3] * e[None, :, 3]).any(1)
    idx = np.floor(w[keep]).astype(np.int64)
    occ[idx[:, 0], idx[:, 1], idx[:, 2]] = True
    return occ


def special_points(origin, voxel, shape):
    """Points that probe step 9's edges on a grid with dyadic origin and voxel: exactly on half-voxel boundaries
    (halves go up), on and just beyond both faces of the grid (w = 0 is inside, w = n is not), NaN and infinite."""
    origin = np.asarray(origin, dtype=np.float64)
    n = np.asarray(shape, dtype=np.float64)
    lo = origin - 0.5 * voxel        # w = 0 exactly: inside
    hi = origin + voxel * (n - 0.5)  # w = n exactly: outside
    mid = origin + voxel * np.floor(n / 2)
    pts = [mid, mid + 0.5 * voxel, mid - 0.5 * voxel, origin + voxel * np.array([1.5, 0.5, 0.5]), lo, hi]
    for a in range(3):
        for v in (lo[a], np.nextafter(lo[a], -np.inf), hi[a], np.nextafter(hi[a], -np.inf)):
            q = mid.copy()
            q[a] = v
            pts.append(q)
    for bad in (np.nan, np.inf, -np.inf):
        for a in range(3):
            q = mid.copy()
            q[a] = bad
            pts.append(q)
    pts.append(np.full(3, np.nan))
    return np.array(pts)
