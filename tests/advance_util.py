"""The certified motion check of optik_amd/csrc/advance_measure.hpp compiled with g++ as plain C++ (no HIP runtime) into a
small shared library, and the walk driven step by step from Python around a caller-given FK (numpy on the host, the
library's link_frames_batch in the -m gpu tests): for the host and the -m gpu tests of conservative advancement."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from collision_util import CSRC

FREE, BLOCKED, LIMIT, NOT_A_NUMBER = 0, 1, 2, 3
MAX_JOINTS, MAX_FRAMES = 16, 18

DRIVER = r"""
#include "advance_measure.hpp"

using namespace optik;

extern "C" {

void adv_build_reach(int n, const double *origins7, int has_tip, const double *ee7, double *reach_out) {
    advance::Reach R;
    advance::build_reach(n, reinterpret_cast<const double (*)[7]>(origins7), has_tip != 0, ee7, R);
    for (int j = 0; j < advance::MAX_JOINTS; ++j)
        for (int f = 0; f < advance::MAX_FRAMES; ++f) reach_out[j * advance::MAX_FRAMES + f] = R.r[j][f];
}

double adv_lam_sphere(int n, int f, const double *a, const double *reach, const double *c3) {
    return advance::lam_sphere(n, f, a, reach, advance::norm3(c3));
}

double adv_pair_lam(int n, int fx, const double *cx3, int fy, const double *cy3, const double *a, const double *reach) {
    return advance::pair_lam(n, fx, advance::norm3(cx3), fy, advance::norm3(cy3), a, reach);
}

// B samples of B segments: the configuration of segment b at t[b] -> q [B][n]
void adv_samples(int n, long long B, const double *qa, const double *qb, const double *t, double *q) {
    for (long long b = 0; b < B; ++b)
        for (int i = 0; i < n; ++i) q[b * n + i] = advance::sample(qa[b * n + i], qb[b * n + i], t[b]);
}

int adv_segment_finite(int n, const double *qa, const double *qb) {
    return advance::segment_finite(n, qa, 1, qb, 1) ? 1 : 0;
}

// B samples: frames [B][n + 2][7], a [B][n] -> c [B], A [B], nan [B]
void adv_terms(int n, long long B, const double *frames, const double *a, int S, const int32_t *frame,
               const double *centers, const double *radii, int P, const int32_t *pairs, int Ms, const double *wsph,
               int Mb, const double *wbox, const float *gvalues, const double *gorigin, double ginv, const int32_t *gn,
               const double *reach, double m, double tol, double G, double *c, double *A, int32_t *nan) {
    coll::Grid grid;
    grid.values = gvalues;
    grid.inv = ginv;
    for (int k = 0; k < 3; ++k) {
        grid.origin[k] = gvalues ? gorigin[k] : 0.0;
        grid.n[k] = gvalues ? gn[k] : 0;
    }
    for (long long b = 0; b < B; ++b) {
        c[b] = 0.0;
        A[b] = 0.0;
        nan[b] = advance::sample_terms(n, frames + b * (n + 2) * 7, S, frame, centers, radii, P, pairs, Ms, wsph, Mb,
                                       wbox, grid, a + b * n, reach, m, tol, G, c[b], A[b]) ? 0 : 1;
    }
}

void adv_walk_begin(advance::Walk *w) { advance::walk_begin(*w); }
void adv_walk_refuse(advance::Walk *w) { advance::walk_refuse(*w); }
int adv_walk_take(advance::Walk *w, int nan, double c, double A, double m, int max_steps) {
    return advance::walk_take(*w, nan != 0, c, A, m, max_steps) ? 1 : 0;
}

}  // extern "C"
"""


class Walk(C.Structure):
    _fields_ = [("t", C.c_double), ("clearance", C.c_double), ("t_stop", C.c_double), ("steps", C.c_int32),
                ("status", C.c_int32)]


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


class Scene:
    """A model, a world and (optionally) a grid in the caller's numbering, as contiguous arrays."""

    def __init__(self, frames=(), centers=None, radii=(), pairs=None, margin=0.0, spheres=None, boxes=None, grid=None):
        self.frame = np.ascontiguousarray(frames, dtype=np.int32).ravel()
        S = len(self.frame)
        self.centers = np.ascontiguousarray(np.zeros((0, 3)) if centers is None else centers, dtype=np.float64).reshape(S, 3)
        self.radii = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, dtype=np.float64), (S,)))
        self.pairs = np.ascontiguousarray(np.zeros((0, 2)) if pairs is None else pairs, dtype=np.int32).reshape(-1, 2)
        self.margin = float(margin)
        self.spheres = np.ascontiguousarray(np.zeros((0, 4)) if spheres is None else spheres, dtype=np.float64).reshape(-1, 4)
        self.boxes = np.ascontiguousarray(np.zeros((0, 10)) if boxes is None else boxes, dtype=np.float64).reshape(-1, 10)
        self.grid = None
        if grid is not None:
            origin, voxel, values = grid
            values = np.ascontiguousarray(values, dtype=np.float32)
            self.grid = (np.ascontiguousarray(origin, dtype=np.float64), 1.0 / float(voxel), values,
                         np.array(values.shape, dtype=np.int32))


def build_advance(workdir=None):
    """Compile the driver; returns an object with the header's functions (see its methods)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the advance header on its own"
    d = workdir or tempfile.mkdtemp(prefix="advance_measure_")
    src, so = os.path.join(d, "advance_driver.cpp"), os.path.join(d, "libadvance_driver.so")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                    src, "-o", so], check=True)
    L = C.CDLL(so)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.adv_build_reach.argtypes = [C.c_int, dp, C.c_int, dp, dp]
    L.adv_lam_sphere.argtypes = [C.c_int, C.c_int, dp, dp, dp]
    L.adv_lam_sphere.restype = C.c_double
    L.adv_pair_lam.argtypes = [C.c_int, C.c_int, dp, C.c_int, dp, dp, dp]
    L.adv_pair_lam.restype = C.c_double
    L.adv_samples.argtypes = [C.c_int, C.c_longlong, dp, dp, dp, dp]
    L.adv_segment_finite.argtypes = [C.c_int, dp, dp]
    L.adv_terms.argtypes = [C.c_int, C.c_longlong, dp, dp, C.c_int, ip, dp, dp, C.c_int, ip, C.c_int, dp, C.c_int, dp,
                            C.POINTER(C.c_float), dp, C.c_double, ip, dp, C.c_double, C.c_double, C.c_double, dp, dp,
                            ip]
    L.adv_walk_begin.argtypes = [C.POINTER(Walk)]
    L.adv_walk_refuse.argtypes = [C.POINTER(Walk)]
    L.adv_walk_take.argtypes = [C.POINTER(Walk), C.c_int, C.c_double, C.c_double, C.c_double, C.c_int]

    class Advance:
        @staticmethod
        def reach(chain, n, ee7=None):
            """The reach table [16, 18] (r[j - 1, f]) of a chain dict (origins [J, 7]; J = n + 1: a trailing fixed
            joint)."""
            origins = np.ascontiguousarray(np.asarray(chain["origins"], dtype=np.float64).reshape(-1, 7))
            out = np.zeros((MAX_JOINTS, MAX_FRAMES))
            ee = None if ee7 is None else np.ascontiguousarray(ee7, dtype=np.float64)
            L.adv_build_reach(n, _dp(origins), int(len(origins) > n), _dp(ee) if ee is not None else None, _dp(out))
            return out

        @staticmethod
        def lam_sphere(n, f, a, reach, c3):
            a, c3 = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(c3, dtype=np.float64)
            return float(L.adv_lam_sphere(n, int(f), _dp(a), _dp(np.ascontiguousarray(reach)), _dp(c3)))

        @staticmethod
        def pair_lam(n, fx, cx3, fy, cy3, a, reach):
            a = np.ascontiguousarray(a, dtype=np.float64)
            cx3, cy3 = np.ascontiguousarray(cx3, dtype=np.float64), np.ascontiguousarray(cy3, dtype=np.float64)
            return float(L.adv_pair_lam(n, int(fx), _dp(cx3), int(fy), _dp(cy3), _dp(a), _dp(np.ascontiguousarray(reach))))

        @staticmethod
        def samples(qa, qb, t):
            qa, qb = np.ascontiguousarray(qa, dtype=np.float64), np.ascontiguousarray(qb, dtype=np.float64)
            t = np.ascontiguousarray(t, dtype=np.float64)
            q = np.zeros_like(qa)
            L.adv_samples(qa.shape[1], qa.shape[0], _dp(qa), _dp(qb), _dp(t), _dp(q))
            return q

        @staticmethod
        def terms(n, frames, a, scene, reach, tol, G):
            """(c [B], A [B], nan [B] bool) of B samples: frames [B, n + 2, 7], a [B, n]."""
            frames = np.ascontiguousarray(frames, dtype=np.float64)
            a = np.ascontiguousarray(a, dtype=np.float64)
            B = frames.shape[0]
            assert frames.shape == (B, n + 2, 7) and a.shape == (B, n)
            c, A, nan = np.zeros(B), np.zeros(B), np.zeros(B, dtype=np.int32)
            g = scene.grid
            L.adv_terms(n, B, _dp(frames), _dp(a), len(scene.frame), _ip(scene.frame), _dp(scene.centers),
                        _dp(scene.radii), len(scene.pairs), _ip(scene.pairs), len(scene.spheres), _dp(scene.spheres),
                        len(scene.boxes), _dp(scene.boxes),
                        g[2].ctypes.data_as(C.POINTER(C.c_float)) if g else None, _dp(g[0]) if g else None,
                        g[1] if g else 0.0, _ip(g[3]) if g else None, _dp(np.ascontiguousarray(reach)), scene.margin,
                        float(tol), float(G), _dp(c), _dp(A), _ip(nan))
            return c, A, nan != 0

        @staticmethod
        def walk(n, qa, qb, scene, reach, tol, G, max_steps, frames_of):
            """The walk of every segment qa[b] -> qb[b] ([B, n]), step by step: at step k the current configurations of
            all segments still walking go through frames_of(q [B', n]) -> [B', n + 2, 7] in one call, and the header
            turns the frames into (c, A) and advances.  Returns a dict of status, steps (int32 [B]), t_stop, clearance
            ([B]) and `t`: per segment the list of the t of its samples."""
            qa, qb = np.ascontiguousarray(qa, dtype=np.float64), np.ascontiguousarray(qb, dtype=np.float64)
            B = qa.shape[0]
            a = np.abs(qb - qa)
            walks = [Walk() for _ in range(B)]
            ts = [[] for _ in range(B)]
            live = []
            for b in range(B):
                if L.adv_segment_finite(n, _dp(np.ascontiguousarray(qa[b])), _dp(np.ascontiguousarray(qb[b]))):
                    L.adv_walk_begin(C.byref(walks[b]))
                    live.append(b)
                else:
                    L.adv_walk_refuse(C.byref(walks[b]))
            while live:
                idx = np.array(live)
                t = np.array([walks[b].t for b in live])
                q = Advance.samples(qa[idx], qb[idx], t)
                c, A, nan = Advance.terms(n, frames_of(q), a[idx], scene, reach, tol, G)
                nxt = []
                for i, b in enumerate(live):
                    ts[b].append(float(t[i]))
                    if L.adv_walk_take(C.byref(walks[b]), int(nan[i]), c[i], A[i], scene.margin, int(max_steps)):
                        nxt.append(b)
                live = nxt
            return dict(status=np.array([w.status for w in walks], dtype=np.int32),
                        steps=np.array([w.steps for w in walks], dtype=np.int32),
                        t_stop=np.array([w.t_stop for w in walks]), clearance=np.array([w.clearance for w in walks]),
                        t=ts)

    return Advance()
