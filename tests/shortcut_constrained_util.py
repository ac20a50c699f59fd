"""optik_amd/csrc/shortcut_constrained_measure.hpp compiled with g++ as plain C++ (no HIP runtime) into a small shared
library for the host and the -m gpu tests of shortcutting and resampling under a pose constraint: the serial references
with the projection AND the pair verdicts as Python callbacks.  constraint_measure.hpp on the host is
rrt_constrained_util's second library (HostConstraint); the unconstrained references and helpers are shortcut_util's.
The paths the GPU parity tests run on are made here, on the CPU (tests/test_shortcut_constrained_host.py asserts what
they hold)."""
import ctypes as C
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

from collision_util import CSRC
from constraint_util import PROJECTED, BUDGET_SPENT, FAILED, upright_constraint  # noqa: F401
from rrt_constrained_util import HostConstraint, build_host_constraint_lib  # noqa: F401
from shortcut_util import (MAX_POINTS, FOUND, NO_ROUTE, BAD_LENGTH, PATH_NAN, bits, pair_count, pair_index,  # noqa: F401
                           pair_segments, pair_table, to_device_layout)

UNPROJECTED = 4
MAX_JOINTS = 16

DRIVER = r"""
#include <cstdint>
#include "shortcut_constrained_measure.hpp"

using namespace optik;

extern "C" {

typedef int (*project_fn)(double *x, int *iterations);
typedef int (*open_fn)(int i, int j, const double *qa, const double *qb);

// verts [MAX_JOINTS][MAX_POINTS]; iterations [MAX_POINTS]; out: status, le, nv, projected[2]
void sc_vertices(int n, const double *path, int len, int Lin, int V, project_fn project, double *verts,
                 int32_t *iterations, int32_t *out) {
    double w[shortcut::MAX_POINTS];
    int its[shortcut::MAX_POINTS], projected[2];
    for (int v = 0; v < shortcut::MAX_POINTS; ++v) its[v] = -1;
    const shortcut::Prepared p = shortcut::vertices_constrained_reference(
        n, path, len, Lin, V, [&](double *x, int *it) { return project(x, it); }, verts, w, projected, its);
    for (int v = 0; v < shortcut::MAX_POINTS; ++v) iterations[v] = its[v];
    out[0] = p.status; out[1] = p.le; out[2] = p.nv; out[3] = projected[0]; out[4] = projected[1];
}

// path_out [Lout][n]; d [MAX_POINTS]; verts [MAX_JOINTS][MAX_POINTS]; costs: cost, cost_in; out: status, len, projected[2]
void sc_shortcut(int n, const double *path, int len, int Lin, int V, project_fn project, open_fn pair_open, double hop,
                 int Lout, double *path_out, double *d, double *verts, double *costs, int32_t *out) {
    int projected[2];
    const shortcut::Result r = shortcut::shortcut_constrained_reference(
        n, path, len, Lin, V, [&](double *x, int *it) { return project(x, it); },
        [&](int i, int j, const double *qa, const double *qb) { return pair_open(i, j, qa, qb) != 0; }, hop, Lout,
        path_out, d, verts, projected);
    costs[0] = r.cost; costs[1] = r.cost_in;
    out[0] = r.status; out[1] = r.len; out[2] = projected[0]; out[3] = projected[1];
}

// path_out [Lout][n]; projected [2]; returns the status
int sc_resample(int n, const double *path, int len, int Lin, int Lout, project_fn project, double *path_out,
                int32_t *projected) {
    int pr[2];
    const int st = shortcut::resample_constrained_reference(n, path, len, Lin, Lout,
                                                            [&](double *x, int *it) { return project(x, it); },
                                                            path_out, pr);
    projected[0] = pr[0]; projected[1] = pr[1];
    return st;
}

}  // extern "C"
"""


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def build_shortcut_constrained_ref(workdir=None):
    """Compile the driver; paths are [P, Lin, n] with lens [P] (None: Lin each); project(x [n]) -> (x' [n], status,
    iterations); pair_open(p, i, j, qa [n], qb [n]) -> bool, rule 3' for the motion vertex i -> vertex j of path p.
    Returns an object with
    .vertices(paths, lens, V, project) -> dict(status [P] (-1: none yet), le, nv, verts [P, 64, n] NaN past nv,
      iterations [P, 64] (-1: an input waypoint or past nv), projected [P, 2]),
    .shortcut(paths, lens, V, project, pair_open, hop, Lout) -> dict(status, len, cost, cost_in, path [P, Lout, n],
      d [P, 64], verts [P, 64, n], projected [P, 2], asked: per path the (i, j) pair_open was asked for, in order),
    .resample(paths, lens, Lout, project) -> (path [P, Lout, n], status [P], projected [P, 2])."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the header on its own"
    d = workdir or tempfile.mkdtemp(prefix="shortcut_constrained_")
    src, so = os.path.join(d, "shortcut_constrained_driver.cpp"), os.path.join(d, "libshortcut_constrained_driver.so")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                    src, "-o", so], check=True)
    lib = C.CDLL(so)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    PROJECT = C.CFUNCTYPE(C.c_int, dp, C.POINTER(C.c_int))
    OPEN = C.CFUNCTYPE(C.c_int, C.c_int, C.c_int, dp, dp)
    lib.sc_vertices.argtypes = [C.c_int, dp, C.c_int, C.c_int, C.c_int, PROJECT, dp, ip, ip]
    lib.sc_vertices.restype = None
    lib.sc_shortcut.argtypes = [C.c_int, dp, C.c_int, C.c_int, C.c_int, PROJECT, OPEN, C.c_double, C.c_int, dp, dp, dp,
                                dp, ip]
    lib.sc_shortcut.restype = None
    lib.sc_resample.argtypes = [C.c_int, dp, C.c_int, C.c_int, C.c_int, PROJECT, dp, ip]

    def lens_of(lens, P, L):
        return [L] * P if lens is None else [int(v) for v in lens]

    def wrap_project(project, n, failed):
        def prj(x, its):
            try:
                xv = np.ctypeslib.as_array(x, (n,))
                xn, status, iterations = project(xv.copy())
                xv[:] = xn
                its[0] = int(iterations)
                return int(status)
            except BaseException as e:  # (an exception cannot cross the C frames: kept, raised by the caller)
                failed.append(e)
                its[0] = 0
                return FAILED
        return PROJECT(prj)

    def verts_rows(verts, nv, n):
        out = np.full((MAX_POINTS, n), math.nan)
        out[:nv] = verts.reshape(MAX_JOINTS, MAX_POINTS)[:n, :nv].T
        return out

    class Ref:
        @staticmethod
        def vertices(paths, lens, V, project):
            paths = np.ascontiguousarray(paths, dtype=np.float64)
            P, L, n = paths.shape
            failed = []
            cb = wrap_project(project, n, failed)
            res = dict(status=np.zeros(P, dtype=np.int32), le=np.zeros(P, dtype=np.int32), nv=np.zeros(P, dtype=np.int32),
                       verts=np.zeros((P, MAX_POINTS, n)), iterations=np.zeros((P, MAX_POINTS), dtype=np.int32),
                       projected=np.zeros((P, 2), dtype=np.int32))
            for p, ln in enumerate(lens_of(lens, P, L)):
                verts = np.full(MAX_JOINTS * MAX_POINTS, math.nan)
                out = np.zeros(5, dtype=np.int32)
                lib.sc_vertices(n, _dp(paths[p]), ln, L, int(V), cb, _dp(verts), res["iterations"][p].ctypes.data_as(ip),
                                out.ctypes.data_as(ip))
                if failed:
                    raise failed[0]
                res["status"][p], res["le"][p], res["nv"][p] = out[:3]
                res["projected"][p] = out[3:]
                res["verts"][p] = verts_rows(verts, int(out[2]), n)
            return res

        @staticmethod
        def shortcut(paths, lens, V, project, pair_open, hop, Lout):
            paths = np.ascontiguousarray(paths, dtype=np.float64)
            P, L, n = paths.shape
            failed = []
            cb = wrap_project(project, n, failed)
            res = dict(status=np.zeros(P, dtype=np.int32), len=np.zeros(P, dtype=np.int32), cost=np.zeros(P),
                       cost_in=np.zeros(P), path=np.zeros((P, int(Lout), n)), d=np.zeros((P, MAX_POINTS)),
                       verts=np.zeros((P, MAX_POINTS, n)), projected=np.zeros((P, 2), dtype=np.int32), asked=[])
            for p, ln in enumerate(lens_of(lens, P, L)):
                asked = []

                def opn(i, j, qa, qb, p=p, asked=asked):
                    try:
                        asked.append((i, j))
                        return 1 if pair_open(p, i, j, np.ctypeslib.as_array(qa, (n,)).copy(),
                                              np.ctypeslib.as_array(qb, (n,)).copy()) else 0
                    except BaseException as e:
                        failed.append(e)
                        return 0

                verts = np.full(MAX_JOINTS * MAX_POINTS, math.nan)
                costs, out = np.zeros(2), np.zeros(4, dtype=np.int32)
                lib.sc_shortcut(n, _dp(paths[p]), ln, L, int(V), cb, OPEN(opn), float(hop), int(Lout),
                                _dp(res["path"][p]), _dp(res["d"][p]), _dp(verts), _dp(costs), out.ctypes.data_as(ip))
                if failed:
                    raise failed[0]
                res["status"][p], res["len"][p] = out[:2]
                res["projected"][p] = out[2:]
                res["cost"][p], res["cost_in"][p] = costs
                res["verts"][p] = verts.reshape(MAX_JOINTS, MAX_POINTS)[:n].T
                res["asked"].append(asked)
            return res

        @staticmethod
        def resample(paths, lens, Lout, project):
            paths = np.ascontiguousarray(paths, dtype=np.float64)
            P, L, n = paths.shape
            failed = []
            cb = wrap_project(project, n, failed)
            out, status = np.zeros((P, int(Lout), n)), np.zeros(P, dtype=np.int32)
            projected = np.zeros((P, 2), dtype=np.int32)
            for p, ln in enumerate(lens_of(lens, P, L)):
                status[p] = lib.sc_resample(n, _dp(paths[p]), ln, L, int(Lout), cb, _dp(out[p]),
                                            projected[p].ctypes.data_as(ip))
                if failed:
                    raise failed[0]
            return out, status, projected

    return Ref()


def flags_open(flags, V):
    """pair_open from a table of verdicts flags [P, pairs] (pair_index order)."""
    return lambda p, i, j, qa, qb: bool(flags[p, pair_index(V, i, j)])


# ---- the paths of the GPU parity tests ------------------------------------------------------------------------------
# A chain without a collision model or with the wall of test_gpu_path_shortcut.py, the end effector kept upright within
# TILT of what it is at the first waypoint of path 2.  P = 5 zigzags of 2, 3, 8 and V waypoints and one with a NaN:
# every waypoint is a projected configuration (it satisfies the constraint at PTOL <= TOL), the steps between them are
# large enough for a straight joint-space motion to leave the constraint by more than TOL at its middle -- the pairs the
# constraint closes -- and small enough for most neighbours to see each other.
TILT, TOL, PTOL = 0.3, 0.05, 1e-6
PITERS, DAMPING, MAX_STEP = 256, 1e-6, 0.5
H = 0.05
SPAN = 0.5


def scene_lens(V, Lin):
    return [2, 3, min(8, Lin), min(V, Lin), min(8, Lin)]


def scene_paths(hc, lo, hi, seed, V, Lin, home):
    """[5, Lin, n] and lens: walks from `home` whose waypoints are projected onto hc's constraint (the host header's
    projection, so the input is the same on every machine with IEEE arithmetic); the last path holds a NaN."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    n = len(lo)
    lens = scene_lens(V, Lin)
    paths = np.zeros((5, Lin, n))
    for p, ln in enumerate(lens):
        q = np.asarray(home, dtype=np.float64).copy()
        for t in range(ln):
            for _ in range(50):
                cand = np.clip(q + rng.uniform(-SPAN, SPAN, n), lo + 0.05, hi - 0.05)
                x, st, _ = hc.project(cand, PTOL, PITERS, DAMPING, MAX_STEP)
                if st == PROJECTED and np.all(x > lo) and np.all(x < hi):
                    break
            else:
                raise AssertionError("no waypoint projects")
            paths[p, t] = q = x
        paths[p, ln:] = paths[p, ln - 1]
    paths[4, 1, n - 1] = math.nan
    return paths, lens
