"""optik_amd/csrc/rrt_goals_measure.hpp compiled with g++ as plain C++ (no HIP runtime) into a small shared library for
the host and the -m gpu tests of the tree planner with a goal set: the serial reference plan_goals_reference with the
collision and motion verdicts as Python callbacks.  The scenes, the oracle and the helpers are rrt_util's."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from collision_util import CSRC
from rrt_util import (FOUND, NO_ROUTE, TOO_LONG, QUERY_NAN, MAX_NODES, LIMITS2, H2, Oracle2, disc, forward_cost,  # noqa: F401
                      samples2, wall, wall_with_gap, _dp)

MAX_GOALS = 16

DRIVER = r"""
#include "rrt_goals_measure.hpp"

using namespace optik;

extern "C" {

typedef int (*config_fn)(const double *q);
typedef void (*motions_fn)(int count, const double *qa, const double *qb, unsigned char *free_out);

// out: status, len, iters_used, nodes[2], junction[2], which, roots
void rrt_plan_goals(int n, const double *lo, const double *hi, const double *start, const double *goals, int G,
                    int count, const double *samples, int I, double eta, int M, int Lmax, config_fn config_free,
                    motions_fn motions_free, double *conf, int32_t *parent, int32_t *root_goal, double *path,
                    double *cost, int32_t *out) {
    const rrt::GoalsResult r = rrt::plan_goals_reference(
        n, lo, hi, start, goals, G, count, samples, I, eta, M, Lmax,
        [&](const double *q) { return config_free(q) != 0; },
        [&](int c, const double *qa, const double *qb, unsigned char *f) { motions_free(c, qa, qb, f); }, conf, parent,
        root_goal, path);
    *cost = r.r.cost;
    out[0] = r.r.status; out[1] = r.r.len; out[2] = r.r.iters_used;
    out[3] = r.r.nodes[0]; out[4] = r.r.nodes[1]; out[5] = r.r.junction[0]; out[6] = r.r.junction[1];
    out[7] = r.which; out[8] = r.roots;
}

int rrt_goals_caps(int which) { return which == 0 ? rrt::MAX_GOALS : rrt::min_nodes(which); }

}  // extern "C"
"""


def build_rrt_goals_ref(workdir=None):
    """Compile the driver; returns an object with
    .plan(lo, hi, start, goals [G, n], count, samples [I, n], step, max_nodes, Lmax, config_free, motions_free) ->
      dict(status, len, iters, nodes [2], junction [2], which, roots, cost, path [Lmax, n], conf [2, M, n], parent [2, M],
      root_goal [G]); the callbacks as rrt_util's;
    .caps(G) -> (MAX_GOALS, the smallest max_nodes a call with G slots may ask for)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the tree planner's header on its own"
    d = workdir or tempfile.mkdtemp(prefix="rrt_goals_")
    src, so = os.path.join(d, "rrt_goals_driver.cpp"), os.path.join(d, "librrt_goals_driver.so")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                    src, "-o", so], check=True)
    lib = C.CDLL(so)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    CONFIG = C.CFUNCTYPE(C.c_int, dp)
    MOTIONS = C.CFUNCTYPE(None, C.c_int, dp, dp, C.POINTER(C.c_uint8))
    lib.rrt_plan_goals.argtypes = [C.c_int, dp, dp, dp, dp, C.c_int, C.c_int, dp, C.c_int, C.c_double, C.c_int, C.c_int,
                                   CONFIG, MOTIONS, dp, ip, ip, dp, dp, ip]
    lib.rrt_plan_goals.restype = None
    lib.rrt_goals_caps.argtypes = [C.c_int]

    class Ref:
        @staticmethod
        def plan(lo, hi, start, goals, count, samples, step, max_nodes, Lmax, config_free, motions_free):
            lo, hi, start, goals = (np.ascontiguousarray(v, dtype=np.float64) for v in (lo, hi, start, goals))
            samples = np.ascontiguousarray(samples, dtype=np.float64)
            I, n = samples.shape
            G, M = goals.shape[0], int(max_nodes)
            assert goals.shape == (G, n) and M >= max(2, G)
            failed = []

            def cfg(q):
                try:
                    return 1 if config_free(np.ctypeslib.as_array(q, (n,)).copy()) else 0
                except BaseException as e:  # (an exception cannot cross the C frames: kept, raised below)
                    failed.append(e)
                    return 0

            def mot(count_, qa, qb, out):
                try:
                    f = motions_free(np.ctypeslib.as_array(qa, (count_, n)).copy(),
                                     np.ctypeslib.as_array(qb, (count_, n)).copy())
                    for j in range(count_):
                        out[j] = 1 if f[j] else 0
                except BaseException as e:
                    failed.append(e)
                    for j in range(count_):
                        out[j] = 0

            conf = np.full((2, M, n), np.nan)
            parent = np.full((2, M), -2, dtype=np.int32)
            root_goal = np.full(G, -2, dtype=np.int32)
            path = np.zeros((int(Lmax), n))
            cost = C.c_double(0.0)
            out = np.zeros(9, dtype=np.int32)
            lib.rrt_plan_goals(n, _dp(lo), _dp(hi), _dp(start), _dp(goals), G, int(count), _dp(samples), I, float(step),
                               M, int(Lmax), CONFIG(cfg), MOTIONS(mot), _dp(conf), parent.ctypes.data_as(ip),
                               root_goal.ctypes.data_as(ip), _dp(path), C.byref(cost), out.ctypes.data_as(ip))
            if failed:
                raise failed[0]
            return dict(status=int(out[0]), len=int(out[1]), iters=int(out[2]), nodes=out[3:5].copy(),
                        junction=out[5:7].copy(), which=int(out[7]), roots=int(out[8]), cost=float(cost.value),
                        path=path, conf=conf, parent=parent, root_goal=root_goal)

        @staticmethod
        def caps(G):
            return int(lib.rrt_goals_caps(0)), int(lib.rrt_goals_caps(int(G)))

    return Ref()


def check_forest(res, start, goals, free):
    """Tree 0 is a tree rooted at the start; tree 1 a forest whose roots are exactly the free counted goals in
    ascending g (`free`: their slots), every other node's parent index lower than its own."""
    c0, c1 = int(res["nodes"][0]), int(res["nodes"][1])
    R = len(free)
    assert res["roots"] == R and res["root_goal"][:R].tolist() == list(free) and (res["root_goal"][R:] == -1).all()
    if c0 == 0:
        assert c1 == 0
        return
    assert res["parent"][0, 0] == -1 and np.array_equal(res["conf"][0, 0], start)
    for j in range(1, c0):
        assert 0 <= res["parent"][0, j] < j
    assert c1 >= R
    for r, g in enumerate(free):
        assert res["parent"][1, r] == -1 and np.array_equal(res["conf"][1, r], goals[g])
    for j in range(R, c1):
        assert 0 <= res["parent"][1, j] < j
    assert not np.isnan(res["conf"][0, :c0]).any() and not np.isnan(res["conf"][1, :c1]).any()


def root_of(res, v):
    """The root of tree 1 that node v's branch ends in."""
    while res["parent"][1, v] >= 0:
        v = int(res["parent"][1, v])
    return v
