"""optik_amd/csrc/shortcut_measure.hpp compiled with g++ as plain C++ (no HIP runtime) for the host and the -m gpu tests
of path shortcutting and resampling; a heapq Dijkstra over a visibility matrix on Python floats; the random inputs; and
the jagged route round the wall of roadmap_util's scene, chosen on the CPU with the host motion check."""
import heapq
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

from collision_util import CSRC
from roadmap_util import bits, host_checked_weights, np_weights, path_cost_backwards, wall_scene  # noqa: F401

MAX_POINTS = 64
FOUND, NO_ROUTE, BAD_LENGTH, PATH_NAN = 0, 1, 2, 3

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "shortcut_measure.hpp"

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
    const int MP = shortcut::MAX_POINTS;
    if (argv[1][0] == 'v') {
        // vertices: n, Lin, V, P, then per path len, path [Lin][n] -> status, le, nv, verts [MP][n] (NaN past nv)
        const int n = (int)in[0], Lin = (int)in[1], V = (int)in[2], P = (int)in[3];
        const double *p = &in[4];
        std::vector<double> verts(shortcut::MAX_JOINTS * MP), w(MP), row(MP * n);
        for (int q = 0; q < P; ++q, p += 1 + Lin * n) {
            const shortcut::Prepared r = shortcut::vertices_reference(n, p + 1, (int)p[0], Lin, V, verts.data(), w.data());
            const double head[3] = {(double)r.status, (double)r.le, (double)r.nv};
            for (int v = 0; v < MP; ++v)
                for (int i = 0; i < n; ++i) row[v * n + i] = v < r.nv ? verts[i * MP + v] : NAN;
            std::fwrite(head, sizeof(double), 3, out);
            std::fwrite(row.data(), sizeof(double), row.size(), out);
        }
    } else if (argv[1][0] == 's') {
        // shortcut: n, Lin, V, Lout, hop, P, then per path len, path [Lin][n], free [pairs]
        // -> status, len, cost, cost_in, path [Lout][n], d [MP]
        const int n = (int)in[0], Lin = (int)in[1], V = (int)in[2], Lout = (int)in[3], P = (int)in[5];
        const double hop = in[4];
        const int pairs = shortcut::pair_count(V);
        const double *p = &in[6];
        std::vector<double> path(Lout * n), d(MP);
        std::vector<unsigned char> fr(pairs > 0 ? pairs : 1);
        for (int q = 0; q < P; ++q, p += 1 + Lin * n + pairs) {
            for (int e = 0; e < pairs; ++e) fr[e] = p[1 + Lin * n + e] != 0.0;
            const shortcut::Result r = shortcut::shortcut_reference(n, p + 1, (int)p[0], Lin, V, fr.data(), hop, Lout,
                                                                    path.data(), d.data());
            const double head[4] = {(double)r.status, (double)r.len, r.cost, r.cost_in};
            std::fwrite(head, sizeof(double), 4, out);
            std::fwrite(path.data(), sizeof(double), path.size(), out);
            std::fwrite(d.data(), sizeof(double), d.size(), out);
        }
    } else {
        // resample: n, Lin, Lout, P, then per path len, path [Lin][n] -> status, path [Lout][n]
        const int n = (int)in[0], Lin = (int)in[1], Lout = (int)in[2], P = (int)in[3];
        const double *p = &in[4];
        std::vector<double> path(Lout * n);
        for (int q = 0; q < P; ++q, p += 1 + Lin * n) {
            const double st = (double)shortcut::resample_reference(n, p + 1, (int)p[0], Lin, Lout, path.data());
            std::fwrite(&st, sizeof(double), 1, out);
            std::fwrite(path.data(), sizeof(double), path.size(), out);
        }
    }
    std::fclose(out);
    return 0;
}
"""


def pair_count(V):
    return V * (V - 1) // 2


def pair_index(V, i, j):
    """The index of the pair i < j among a path's V (V - 1) / 2 flags (shortcut_measure.hpp step 3)."""
    return i * (2 * V - i - 1) // 2 + (j - i - 1)


def pair_table(V):
    """(i [pairs], j [pairs]) in the order of pair_index."""
    i, j = np.triu_indices(V, 1)
    assert all(pair_index(V, int(a), int(b)) == e for e, (a, b) in enumerate(zip(i[:200], j[:200])))
    return i, j


def _lens(lens, P, L):
    return np.full(P, L, dtype=np.float64) if lens is None else np.asarray(lens, dtype=np.float64).reshape(P)


def build_shortcut_ref(workdir=None):
    """Compile the driver; paths are [P, Lin, n] with lens [P] (None: Lin each).  Returns an object with
    .vertices(paths, lens, V) -> (status [P], le [P], nv [P], verts [P, 64, n], NaN past nv; status -1: none yet),
    .shortcut(paths, lens, V, free [P, pairs], hop, Lout) -> dict(status, len [P] int32, cost, cost_in [P], path
      [P, Lout, n], d [P, 64] the objective of every vertex),
    .resample(paths, lens, Lout) -> (path [P, Lout, n], status [P] int32)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the shortcut header on its own"
    d = workdir or tempfile.mkdtemp(prefix="shortcut_")
    src, exe = os.path.join(d, "shortcut_driver.cpp"), os.path.join(d, "shortcut_driver")
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
        def vertices(paths, lens, V):
            P, L, n = paths.shape
            rows = np.concatenate([_lens(lens, P, L)[:, None], paths.reshape(P, -1)], axis=1)
            out = run("v", [n, L, V, P], rows).reshape(P, 3 + MAX_POINTS * n)
            return (out[:, 0].astype(np.int32), out[:, 1].astype(np.int32), out[:, 2].astype(np.int32),
                    out[:, 3:].reshape(P, MAX_POINTS, n).copy())

        @staticmethod
        def shortcut(paths, lens, V, free, hop, Lout):
            P, L, n = paths.shape
            free = np.asarray(free, dtype=np.float64).reshape(P, pair_count(V))
            rows = np.concatenate([_lens(lens, P, L)[:, None], paths.reshape(P, -1), free], axis=1)
            out = run("s", [n, L, V, Lout, hop, P], rows).reshape(P, 4 + Lout * n + MAX_POINTS)
            return dict(status=out[:, 0].astype(np.int32), len=out[:, 1].astype(np.int32), cost=out[:, 2].copy(),
                        cost_in=out[:, 3].copy(), path=out[:, 4:4 + Lout * n].reshape(P, Lout, n).copy(),
                        d=out[:, 4 + Lout * n:].copy())

        @staticmethod
        def resample(paths, lens, Lout):
            P, L, n = paths.shape
            rows = np.concatenate([_lens(lens, P, L)[:, None], paths.reshape(P, -1)], axis=1)
            out = run("r", [n, L, Lout, P], rows).reshape(P, 1 + Lout * n)
            return out[:, 1:].reshape(P, Lout, n).copy(), out[:, 0].astype(np.int32)

    return Ref()


def pair_segments(verts, V):
    """The segments the device checks for one path: verts [64, n] (NaN past nv) -> (qa [pairs, n], qb [pairs, n])."""
    i, j = pair_table(V)
    return verts[i].copy(), verts[j].copy()


def dag_dijkstra(verts, nv, V, free, hop):
    """d [nv]: the objective of every vertex to the last one with a heap, on Python floats: a hop i -> j costs
    (w + hop) + d[j], the route summed from the goal backwards; w is max |difference| where free[pair] else no edge."""
    d = [math.inf] * nv
    d[nv - 1] = 0.0
    heap = [(0.0, nv - 1)]
    done = [False] * nv
    while heap:
        du, u = heapq.heappop(heap)
        if done[u] or du > d[u]:
            continue
        done[u] = True
        for i in range(u):
            if not free[pair_index(V, i, u)]:
                continue
            w = float(np.max(np.abs(verts[u] - verts[i])))
            c = (w + hop) + du
            if c < d[i]:
                d[i] = c
                heapq.heappush(heap, (c, i))
    return d


def route_of(path, length, verts, nv):
    """The vertex indices of a path's waypoints (each is a vertex, bit for bit), strictly ascending: the first
    match behind the waypoint before."""
    idx, v = [], 0
    for t in range(length):
        while v < nv and not np.array_equal(bits(verts[v]), bits(path[t])):
            v += 1
        assert v < nv, f"waypoint {t} is no vertex"
        idx.append(v)
        v += 1
    return idx


def random_polylines(rng, P, L, n, lens=None, scale=1.0):
    """P random walks [P, L, n] of `lens` waypoints each, padded with the last one."""
    paths = np.cumsum(rng.uniform(-scale, scale, (P, L, n)), axis=1)
    lens = np.full(P, L) if lens is None else np.asarray(lens)
    for p, ln in enumerate(lens):
        if 1 <= ln < L:
            paths[p, ln:] = paths[p, ln - 1]
    return paths


def to_device_layout(paths):
    """[P, L, n] -> [L, P, n], contiguous: what the kernel layer takes."""
    return np.ascontiguousarray(np.transpose(paths, (1, 0, 2)))


# ---- the jagged route of the end-to-end tests -----------------------------------------------------------------------
# roadmap_util's wall scene (a Panda, six spheres, a 2 cm wall in the plane y = 0, checked at WALL_H): from WALL_START
# the arm folds back under the wall to the fifth waypoint while its wrist swings to and fro, then unfolds to WALL_GOAL.
# (Chosen on the CPU: tests/test_shortcut_host.py asserts with the host motion check that every segment is free and
# that the serial reference, with WALL_VERTICES vertices, walks the vertices WALL_SHORTCUT of the 12 it makes.)
WALL_ROUTE = [[-0.9, 0.4, 0.0, -1.8, 0.0, 2.2, 0.7],
              [-0.72, 0.12, -0.15, -2.03, 0.63, 1.87, 1.28],
              [-0.54, -0.16, -0.3, -2.26, -0.24, 2.74, 0.06],
              [-0.36, -0.44, -0.45, -2.49, 0.89, 2.01, 1.24],
              [-0.18, -0.72, -0.6, -2.72, 0.02, 2.88, 0.02],
              [0.0, -1.0, -0.75, -2.95, 0.65, 2.55, 0.6],
              [0.9, 0.4, 0.0, -1.8, 0.0, 2.2, 0.7]]
WALL_VERTICES = 16
WALL_SHORTCUT = [0, 8, 11]
