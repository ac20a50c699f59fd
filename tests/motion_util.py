"""The motion check of optik_amd/csrc/motion_measure.hpp compiled with g++ as plain C++ (no HIP runtime), the same
rules written in numpy, and a numpy FK that gives the n + 2 frames of a configuration as pose7 rows: for the host and
the -m gpu tests of the motion check."""
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

from collision_util import CSRC

MAX_STEPS = 4096

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "motion_measure.hpp"

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
    if (argv[1][0] == 's') {
        // samples: n, h, then segments (qa [n], qb [n]) -> per segment d, K, then (K + 1) * n samples when K >= 1
        const int n = (int)in[0];
        const double h = in[1];
        for (size_t o = 2; o + 2 * n <= in.size(); o += 2 * n) {
            const double *qa = &in[o], *qb = &in[o + n];
            const double d = motion::motion_distance(n, qa, 1, qb, 1);
            const int K = motion::motion_steps(d, h);
            const double Kd = (double)K;
            std::fwrite(&d, sizeof(double), 1, out);
            std::fwrite(&Kd, sizeof(double), 1, out);
            for (int k = 0; k <= K; ++k)
                for (int i = 0; i < n; ++i) {
                    const double q = motion::motion_sample(qa[i], qb[i], k, K);
                    std::fwrite(&q, sizeof(double), 1, out);
                }
        }
    } else {
        // reduce: argv[4] = model (margin, nf, S, P, Ms, Mb, frame[S], centers[3S], radii[S], pairs[2P], spheres[4Ms],
        // boxes[10Mb]); argv[2] = segments: K, then (K + 1) * nf * 7 frames when K >= 1 -> clearance, free, first, steps
        const std::vector<double> m = read_all(argv[4]);
        const double margin = m[0];
        const int nf = (int)m[1], S = (int)m[2], P = (int)m[3], Ms = (int)m[4], Mb = (int)m[5];
        size_t o = 6;
        std::vector<int32_t> frame(S), pairs(2 * P);
        for (int s = 0; s < S; ++s) frame[s] = (int32_t)m[o++];
        const double *centers = m.data() + o; o += 3 * S;
        const double *radii = m.data() + o; o += S;
        for (int k = 0; k < 2 * P; ++k) pairs[k] = (int32_t)m[o++];
        const double *sph = m.data() + o; o += 4 * Ms;
        const double *box = m.data() + o;
        for (size_t i = 0; i < in.size();) {
            const int K = (int)in[i++];
            const double *fr = in.data() + i;
            const motion::Result r = motion::motion_reduce(K, margin, [&](int k) {
                return coll::clearance(nf, fr + (size_t)k * nf * 7, S, frame.data(), centers, radii, P, pairs.data(),
                                       Ms, sph, Mb, box);
            });
            if (K >= 1) i += (size_t)(K + 1) * nf * 7;
            const double o4[4] = {r.clearance, (double)r.free_flag, (double)r.first, (double)r.steps};
            std::fwrite(o4, sizeof(double), 4, out);
        }
    }
    std::fclose(out);
    return 0;
}
"""


def np_distance(qa, qb):
    """Step 1: max_i |qb_i - qa_i|, NaN as soon as one term is."""
    e = np.abs(np.asarray(qb, dtype=np.float64) - np.asarray(qa, dtype=np.float64))
    return float(np.max(e)) if e.size else 0.0  # (np.max propagates NaN)


def np_steps(d, h):
    """Step 2: K, or -1 for a motion that is not sampled."""
    with np.errstate(all="ignore"):
        r = np.ceil(np.float64(d) / np.float64(h))
    if not r <= MAX_STEPS:
        return -1
    return 1 if r < 1.0 else int(r)


def np_samples(qa, qb, h):
    """(d, K, samples [K + 1, n] or None) in the documented operation order."""
    qa, qb = np.asarray(qa, dtype=np.float64), np.asarray(qb, dtype=np.float64)
    d = np_distance(qa, qb)
    K = np_steps(d, h)
    if K < 0:
        return d, K, None
    t = np.arange(K + 1, dtype=np.float64) / np.float64(K)
    s = qa[None, :] + t[:, None] * (qb - qa)[None, :]
    s[0], s[K] = qa, qb
    return d, K, s


def np_reduce(K, clearances, margin):
    """Step 4 over the samples' clearances: (clearance, free, first, steps)."""
    if K < 0:
        return math.nan, False, -1, -1
    c = np.asarray(clearances, dtype=np.float64)
    bad = np.nonzero(~(c >= margin))[0]
    clr = math.nan if np.isnan(c).any() else float(c.min())
    return clr, len(bad) == 0, (int(bad[0]) if len(bad) else -1), K


def _qmul(a, b):
    ai, aj, ak, aw = a
    bi, bj, bk, bw = b
    return np.array([aw * bi + ai * bw + aj * bk - ak * bj, aw * bj - ai * bk + aj * bw + ak * bi,
                     aw * bk + ai * bj - aj * bi + ak * bw, aw * bw - ai * bi - aj * bj - ak * bk])


def _qrot(q, v):
    u = 2.0 * np.cross(q[:3], v)
    return v + q[3] * u + np.cross(q[:3], u)


def _compose(a, b):
    return np.concatenate([a[:3] + _qrot(a[3:], b[:3]), _qmul(a[3:], b[3:])])


def np_frames7(d, q, ee7=None):
    """The n + 2 frames [n + 2, 7] of configuration q from the chain tables (revolute joints; numpy, its own order)."""
    origins, axes = np.asarray(d["origins"]).reshape(-1, 7), np.asarray(d["axes"]).reshape(-1, 3)
    n = len(q)
    cur = np.array([0.0, 0, 0, 0, 0, 0, 1])
    out = [cur]
    for j in range(n):
        s, c = math.sin(q[j] / 2), math.cos(q[j] / 2)
        cur = _compose(_compose(cur, origins[j]), np.concatenate([[0.0, 0, 0], axes[j] * s, [c]]))
        out.append(cur)
    if len(origins) > n:
        cur = _compose(cur, origins[n])
    if ee7 is not None:
        cur = _compose(cur, np.asarray(ee7, dtype=np.float64))
    out.append(cur)
    return np.array(out)


def build_motion(workdir=None):
    """Compile the driver; returns an object with .samples(qa [B, n], qb [B, n], h) -> [(d, K, samples or None)] and
    .reduce(Ks, frames, margin, sphere_frames, centers, radii, pairs, spheres, boxes) -> (clearance, free, first,
    steps) arrays, frames being one [K + 1, nf, 7] array (or None for K < 1) per segment."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the motion header on its own"
    d = workdir or tempfile.mkdtemp(prefix="motion_measure_")
    src, exe = os.path.join(d, "motion_driver.cpp"), os.path.join(d, "motion_driver")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe],
                   check=True)

    class Motion:
        @staticmethod
        def samples(qa, qb, h):
            qa = np.ascontiguousarray(qa, dtype=np.float64)
            qb = np.ascontiguousarray(qb, dtype=np.float64)
            B, n = qa.shape
            fin, fout = os.path.join(d, "s_in.bin"), os.path.join(d, "s_out.bin")
            np.concatenate([[float(n), float(h)], np.concatenate([qa, qb], axis=1).ravel()]).tofile(fin)
            subprocess.run([exe, "s", fin, fout], check=True)
            raw = np.fromfile(fout, dtype=np.float64)
            out, o = [], 0
            for _ in range(B):
                dist, K = raw[o], int(raw[o + 1])
                o += 2
                s = None
                if K >= 1:
                    s = raw[o:o + (K + 1) * n].reshape(K + 1, n)
                    o += (K + 1) * n
                out.append((float(dist), K, s))
            assert o == len(raw)
            return out

        @staticmethod
        def reduce(Ks, frames, margin, sphere_frames, centers, radii, pairs=None, spheres=None, boxes=None):
            sf = np.asarray(sphere_frames, dtype=np.float64).ravel()
            S = len(sf)
            nf = next((f.shape[1] for f in frames if f is not None), 1)
            pairs = np.zeros((0, 2)) if pairs is None else np.asarray(pairs, dtype=np.float64).reshape(-1, 2)
            spheres = np.zeros((0, 4)) if spheres is None else np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
            boxes = np.zeros((0, 10)) if boxes is None else np.asarray(boxes, dtype=np.float64).reshape(-1, 10)
            model = np.concatenate([[margin, nf, S, len(pairs), len(spheres), len(boxes)], sf,
                                    np.asarray(centers, dtype=np.float64).ravel(),
                                    np.broadcast_to(np.asarray(radii, dtype=np.float64), (S,)),
                                    pairs.ravel(), spheres.ravel(), boxes.ravel()])
            parts = []
            for K, f in zip(Ks, frames):
                parts.append(np.array([float(K)]))
                if K >= 1:
                    assert f.shape == (K + 1, nf, 7)
                    parts.append(np.ascontiguousarray(f, dtype=np.float64).ravel())
            fm, fin, fout = (os.path.join(d, x) for x in ("m_model.bin", "m_in.bin", "m_out.bin"))
            model.tofile(fm)
            np.concatenate(parts).tofile(fin)
            subprocess.run([exe, "m", fin, fout, fm], check=True)
            o = np.fromfile(fout, dtype=np.float64).reshape(-1, 4)
            assert len(o) == len(Ks)
            return o[:, 0], o[:, 1] != 0, o[:, 2].astype(np.int32), o[:, 3].astype(np.int32)

    return Motion()
