"""optik_amd/csrc/mesh_measure.hpp (mesh_field, atan2m) compiled with g++ as plain C++ (no HIP runtime), and what the
host and the -m gpu tests of the mesh path share: an independently formulated numpy reference (Ericson's region-based
closest point on a triangle, the winding number with np.arctan2) and the meshes the tests are built from.

Every file the driver reads or writes holds doubles; float32 values travel as doubles (exact both ways)."""
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
#include "mesh_measure.hpp"

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
    if (argv[1][0] == 'f') {
        // field: origin (3), voxel, max_distance, nx, ny, nz, then the triangles [M][9]; every node as (double)(float)
        if (in.size() < 8 || (in.size() - 8) % 9) return 2;
        const int32_t n[3] = {(int32_t)in[5], (int32_t)in[6], (int32_t)in[7]};
        const size_t nodes = (size_t)n[0] * n[1] * n[2];
        std::vector<float> v(nodes);
        mesh_field(in.data(), in[3], n, in.data() + 8, (int)((in.size() - 8) / 9), in[4], v.data());
        for (size_t i = 0; i < nodes; ++i) {
            const double d = (double)v[i];
            std::fwrite(&d, sizeof(double), 1, out);
        }
    } else {
        // atan2m: records of (y, x)
        for (size_t i = 0; i + 2 <= in.size(); i += 2) {
            const double d = atan2m(in[i], in[i + 1]);
            std::fwrite(&d, sizeof(double), 1, out);
        }
    }
    std::fclose(out);
    return 0;
}
"""


def build_mesh_measure(workdir=None):
    """Compile the driver; returns an object with
    .field(origin, voxel, shape, tris [M, 3, 3] or [M, 9], max_distance) -> float32 [nx, ny, nz] and
    .atan2m(y [N], x [N]) -> float64 [N]."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the mesh header on its own"
    d = workdir or tempfile.mkdtemp(prefix="mesh_measure_")
    src, exe = os.path.join(d, "mesh_driver.cpp"), os.path.join(d, "mesh_driver")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe],
                   check=True)

    class MeshMeasure:
        @staticmethod
        def field(origin, voxel, shape, tris, max_distance):
            tris = np.ascontiguousarray(tris, dtype=np.float64).reshape(-1, 9)
            fin, fout = os.path.join(d, "mesh_in.bin"), os.path.join(d, "mesh_out.bin")
            np.concatenate([np.asarray(origin, dtype=np.float64).ravel(), [float(voxel), float(max_distance)],
                            np.asarray(shape, dtype=np.float64), tris.ravel()]).tofile(fin)
            subprocess.run([exe, "f", fin, fout], check=True)
            out = np.fromfile(fout, dtype=np.float64)
            assert out.shape == (int(np.prod(shape)),)
            f32 = out.astype(np.float32)
            assert (f32.astype(np.float64) == out).all()
            return f32.reshape(tuple(shape))

        @staticmethod
        def atan2m(y, x):
            rec = np.stack([np.asarray(y, dtype=np.float64).ravel(), np.asarray(x, dtype=np.float64).ravel()], 1)
            fin, fout = os.path.join(d, "atan_in.bin"), os.path.join(d, "atan_out.bin")
            np.ascontiguousarray(rec).tofile(fin)
            subprocess.run([exe, "a", fin, fout], check=True)
            out = np.fromfile(fout, dtype=np.float64)
            assert out.shape == (len(rec),)
            return out

    return MeshMeasure()


# ---- the reference ----------------------------------------------------------------------------------------------------

def grid_nodes(origin, voxel, shape):
    """[nodes, 3]: origin_a + voxel * i_a, z fastest (collision_measure.hpp's grid_node)."""
    ax = [np.float64(origin[a]) + np.float64(voxel) * np.arange(shape[a], dtype=np.float64) for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def _dot(u, v):
    return (u * v).sum(-1)


def closest_point_d2(p, a, b, c):
    """Squared distance from the points p [N, 3] to the triangle (a, b, c): Ericson, Real-Time Collision Detection,
    5.1.5 -- the Voronoi region of the closest feature picked from barycentric sign tests, then the closest point
    itself.  Well-shaped triangles only (it divides by edge lengths and the area)."""
    ab, ac = b - a, c - a
    ap = p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = p - b
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = p - c
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / (va + vb + vc)
    q = a + ab * (vb * den)[:, None] + ac * (vc * den)[:, None]  # the face
    # (later assignments win: the order below is the reverse of Ericson's early returns)
    m = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)
    q[m] = (b + (c - b) * w_bc[:, None])[m]
    m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    q[m] = (a + ac * w_ac[:, None])[m]
    m = (d6 >= 0) & (d5 <= d6)
    q[m] = c
    m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    q[m] = (a + ab * v_ab[:, None])[m]
    m = (d3 >= 0) & (d4 <= d3)
    q[m] = b
    m = (d1 <= 0) & (d2 <= 0)
    q[m] = a
    r = p - q
    return _dot(r, r)


def field_reference(origin, voxel, shape, tris, max_distance):
    """The field as numpy reads it: (float32 [nx, ny, nz], the float64 signed distance before the clamp)."""
    tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    p = grid_nodes(origin, voxel, shape)
    best = np.full(len(p), np.inf)
    W = np.zeros(len(p))
    for a, b, c in tris:
        best = np.minimum(best, closest_point_d2(p, a, b, c))
        A, B, C = a - p, b - p, c - p
        la, lb, lc = (np.linalg.norm(v, axis=1) for v in (A, B, C))
        num = _dot(A, np.cross(B, C))
        den = la * lb * lc + _dot(A, B) * lc + _dot(B, C) * la + _dot(C, A) * lb
        W += 2.0 * np.arctan2(num, den)
    s = np.where(np.abs(W) >= 2.0 * np.pi, -1.0, 1.0) * np.sqrt(best)
    md = float(max_distance)
    return np.clip(s, -md, md).astype(np.float32).reshape(tuple(shape)), s.reshape(tuple(shape))


def ulp_diff(x, y):
    """How many float32 values apart x and y are, elementwise (both finite; +0 and -0 count as the same value)."""
    def key(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(x) - key(y))


# ---- meshes -----------------------------------------------------------------------------------------------------------

def box_triangles(lo, hi, flip=False, skip_face=None):
    """The 12 triangles of the axis-aligned box [lo, hi], outward oriented (flip: inward), [12, 3, 3]; skip_face in
    0 .. 5 (-x, +x, -y, +y, -z, +z) leaves that face's two triangles out."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.array([[(hi if (k >> a) & 1 else lo)[a] for a in range(3)] for k in range(8)])  # bit a of k: axis a high
    quads = [(0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6)]
    tris = []
    for f, (i, j, k, l) in enumerate(quads):
        if f == skip_face:
            continue
        tris += [[v[i], v[j], v[k]], [v[i], v[k], v[l]]]
    tris = np.array(tris)
    return tris[:, ::-1, :].copy() if flip else tris


def box_sdf(p, lo, hi):
    """The signed distance of the points p [N, 3] to the box [lo, hi], as collision_measure.hpp's sphere_box reads it
    (identity rotation, radius 0)."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    e = np.abs(p - 0.5 * (lo + hi)) - 0.5 * (hi - lo)
    o = np.maximum(e, 0.0)
    outside = np.sqrt((o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1]) + o[:, 2] * o[:, 2])
    inside = np.minimum(np.maximum(np.maximum(e[:, 0], e[:, 1]), e[:, 2]), 0.0)
    return outside + inside


def random_triangles(rng, M, lo=-1.0, hi=1.0, min_area=0.05):
    """M well-shaped random triangles with O(1) coordinates, [M, 3, 3]: vertices uniform in [lo, hi]^3, redrawn until
    twice the area is at least min_area and no edge is shorter than 0.2."""
    out = []
    while len(out) < M:
        t = rng.uniform(lo, hi, size=(3, 3))
        n = np.cross(t[1] - t[0], t[2] - t[0])
        edges = [np.linalg.norm(t[(i + 1) % 3] - t[i]) for i in range(3)]
        if np.linalg.norm(n) >= min_area and min(edges) >= 0.2:
            out.append(t)
    return np.array(out)


def degenerate_triangles():
    """A zero-area triangle (three collinear, distinct vertices) and one with all three vertices equal, [2, 3, 3]."""
    return np.array([[[0.1, 0.2, 0.3], [0.3, 0.4, 0.5], [0.5, 0.6, 0.7]],
                     [[-0.4, 0.25, 0.15], [-0.4, 0.25, 0.15], [-0.4, 0.25, 0.15]]])


def write_stl_binary(path, tris, header=b""):
    tris = np.asarray(tris, dtype=np.float32).reshape(-1, 3, 3)
    rec = np.zeros(len(tris), dtype=np.dtype([("f", "<f4", (12,)), ("attr", "<u2")]))
    rec["f"][:, 3:] = tris.reshape(-1, 9)
    with open(path, "wb") as fh:
        fh.write(header.ljust(80, b" ")[:80])
        fh.write(np.uint32(len(tris)).astype("<u4").tobytes())
        fh.write(rec.tobytes())


def write_stl_ascii(path, tris, name="mesh"):
    tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    with open(path, "w") as fh:
        fh.write(f"solid {name}\n")
        for t in tris:
            fh.write("  facet normal 0 0 0\n    outer loop\n")
            for v in t:
                fh.write("      vertex " + " ".join(repr(float(x)) for x in v) + "\n")
            fh.write("    endloop\n  endfacet\n")
        fh.write(f"endsolid {name}\n")
