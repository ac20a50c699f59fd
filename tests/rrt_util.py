"""optik_amd/csrc/rrt_measure.hpp compiled with g++ as plain C++ (no HIP runtime) into a small shared library for the
host and the -m gpu tests of the bidirectional tree planner: the serial reference with the collision and motion
verdicts as Python callbacks; closed-form obstacles in a 2-joint space; and the constants of the wall-scene test, chosen
on the CPU (tests/test_rrt_host.py asserts what they promise)."""
import ctypes as C
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

from collision_util import CSRC
from motion_util import np_samples

FOUND, NO_ROUTE, TOO_LONG, QUERY_NAN = 0, 1, 2, 3
MAX_ITERS, MIN_NODES, MAX_NODES, MAX_POLL = 65536, 2, 4096, 65536

# The wall scene of roadmap_util (WALL_START -> WALL_GOAL behind a 2 cm wall, h = 0.1) through the tree planner.  With
# the host motion check and these values (first = 1: the samples the scene's roadmap uses as its nodes) the serial
# reference joins the trees after 33 iterations with 11 waypoints, and after 51 with 15 for the pair reversed; a step
# of 1.0 joins them in the first iteration and tests little.  The budget of 256 leaves room for a device whose forward
# kinematics differs from numpy's in the last bit and forks the trees; tests/test_rrt_host.py asserts that the pair is
# found within half of it.
WALL_ITERS, WALL_STEP, WALL_FIRST, WALL_NODES = 256, 0.3, 1, 128

DRIVER = r"""
#include "rrt_measure.hpp"

using namespace optik;

extern "C" {

typedef int (*config_fn)(const double *q);
typedef void (*motions_fn)(int count, const double *qa, const double *qb, unsigned char *free_out);

// out: status, len, iters_used, nodes[2], junction[2]
void rrt_plan(int n, const double *lo, const double *hi, const double *start, const double *goal, const double *samples,
              int I, double eta, int M, int Lmax, config_fn config_free, motions_fn motions_free, double *conf,
              int32_t *parent, double *path, double *cost, int32_t *out) {
    const rrt::Result r = rrt::plan_reference(
        n, lo, hi, start, goal, samples, I, eta, M, Lmax, [&](const double *q) { return config_free(q) != 0; },
        [&](int count, const double *qa, const double *qb, unsigned char *f) { motions_free(count, qa, qb, f); }, conf,
        parent, path);
    *cost = r.cost;
    out[0] = r.status; out[1] = r.len; out[2] = r.iters_used;
    out[3] = r.nodes[0]; out[4] = r.nodes[1]; out[5] = r.junction[0]; out[6] = r.junction[1];
}

int rrt_nearest(int n, double *conf, int count, const double *x, double *dist) {
    rrt::Tree t{n, count, count, conf, nullptr};
    return t.nearest(x, dist);
}

int rrt_steer(int n, const double *p, const double *x, double eta, const double *lo, const double *hi, double *c) {
    const double d = motion::motion_distance(n, p, 1, x, 1);
    if (!rrt::steers(d)) return 0;
    rrt::steer(n, p, x, d, eta, lo, hi, c);
    return 1;
}

}  // extern "C"
"""


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def build_rrt_ref(workdir=None):
    """Compile the driver; returns an object with
    .plan(lo, hi, start, goal, samples [I, n], step, max_nodes, Lmax, config_free, motions_free) -> dict(status, len,
      iters, nodes [2], junction [2], cost, path [Lmax, n], conf [2, M, n], parent [2, M]); config_free(q [n]) -> bool
      and motions_free(qa [c, n], qb [c, n]) -> c bools are called as the rules ask for the verdicts, qa -> qb being
      the direction of travel;
    .nearest(conf [count, n], x [n]) -> (index, distance); .steer(p, x, step, lo, hi) -> c [n] or None."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the tree planner's header on its own"
    d = workdir or tempfile.mkdtemp(prefix="rrt_")
    src, so = os.path.join(d, "rrt_driver.cpp"), os.path.join(d, "librrt_driver.so")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                    src, "-o", so], check=True)
    lib = C.CDLL(so)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    CONFIG = C.CFUNCTYPE(C.c_int, dp)
    MOTIONS = C.CFUNCTYPE(None, C.c_int, dp, dp, C.POINTER(C.c_uint8))
    lib.rrt_plan.argtypes = [C.c_int, dp, dp, dp, dp, dp, C.c_int, C.c_double, C.c_int, C.c_int, CONFIG, MOTIONS, dp, ip,
                             dp, dp, ip]
    lib.rrt_plan.restype = None
    lib.rrt_nearest.argtypes = [C.c_int, dp, C.c_int, dp, dp]
    lib.rrt_steer.argtypes = [C.c_int, dp, dp, C.c_double, dp, dp, dp]

    class Ref:
        @staticmethod
        def plan(lo, hi, start, goal, samples, step, max_nodes, Lmax, config_free, motions_free):
            lo, hi, start, goal = (np.ascontiguousarray(v, dtype=np.float64) for v in (lo, hi, start, goal))
            samples = np.ascontiguousarray(samples, dtype=np.float64)
            I, n = samples.shape
            M = int(max_nodes)
            failed = []

            def cfg(q):
                try:
                    return 1 if config_free(np.ctypeslib.as_array(q, (n,)).copy()) else 0
                except BaseException as e:  # (an exception cannot cross the C frames: kept, raised below)
                    failed.append(e)
                    return 0

            def mot(count, qa, qb, out):
                try:
                    f = motions_free(np.ctypeslib.as_array(qa, (count, n)).copy(),
                                     np.ctypeslib.as_array(qb, (count, n)).copy())
                    for j in range(count):
                        out[j] = 1 if f[j] else 0
                except BaseException as e:
                    failed.append(e)
                    for j in range(count):
                        out[j] = 0

            conf = np.full((2, M, n), np.nan)
            parent = np.full((2, M), -2, dtype=np.int32)
            path = np.zeros((int(Lmax), n))
            cost = C.c_double(0.0)
            out = np.zeros(7, dtype=np.int32)
            lib.rrt_plan(n, _dp(lo), _dp(hi), _dp(start), _dp(goal), _dp(samples), I, float(step), M, int(Lmax),
                         CONFIG(cfg), MOTIONS(mot), _dp(conf), parent.ctypes.data_as(ip), _dp(path), C.byref(cost),
                         out.ctypes.data_as(ip))
            if failed:
                raise failed[0]
            return dict(status=int(out[0]), len=int(out[1]), iters=int(out[2]), nodes=out[3:5].copy(),
                        junction=out[5:7].copy(), cost=float(cost.value), path=path, conf=conf, parent=parent)

        @staticmethod
        def nearest(conf, x):
            conf = np.ascontiguousarray(conf, dtype=np.float64)
            x = np.ascontiguousarray(x, dtype=np.float64)
            dist = C.c_double(0.0)
            j = lib.rrt_nearest(conf.shape[1], _dp(conf), conf.shape[0], _dp(x), C.byref(dist))
            return int(j), float(dist.value)

        @staticmethod
        def steer(p, x, step, lo, hi):
            p, x, lo, hi = (np.ascontiguousarray(v, dtype=np.float64) for v in (p, x, lo, hi))
            c = np.zeros_like(p)
            ok = lib.rrt_steer(len(p), _dp(p), _dp(x), float(step), _dp(lo), _dp(hi), _dp(c))
            return c if ok else None

    return Ref()


# ---- closed-form obstacles in a 2-joint space ----------------------------------------------------------------------

LIMITS2 = (np.array([-2.0, -2.0]), np.array([2.0, 2.0]))
H2 = 0.05


def disc(q):
    """Blocked inside the disc of radius 0.6 round the origin."""
    return q[0] * q[0] + q[1] * q[1] >= 0.36


def wall_with_gap(q):
    """Blocked for |q0| < 0.1 except where |q1 - 1.5| < 0.2."""
    return abs(q[0]) >= 0.1 or abs(q[1] - 1.5) < 0.2


def wall(q):
    return abs(q[0]) >= 0.1


class Oracle2:
    """The verdicts of a closed-form obstacle, sampled as the motion check samples a segment (motion_util.np_samples at
    H2); keeps every motion it approved, as (qa bytes, qb bytes): direction matters."""

    def __init__(self, free):
        self.free = free
        self.approved = set()
        self.asked = 0

    def config_free(self, q):
        return bool(self.free(q))

    def motions_free(self, qa, qb):
        out = []
        for a, b in zip(qa, qb):
            self.asked += 1
            _, K, s = np_samples(a, b, H2)
            ok = K >= 1 and all(self.free(x) for x in s)
            if ok:
                self.approved.add((a.tobytes(), b.tobytes()))
            out.append(ok)
        return out


def samples2(I, seed):
    lo, hi = LIMITS2
    return np.random.default_rng(seed).uniform(lo, hi, (I, 2))


def forward_cost(path, length):
    """The L-infinity lengths of a path's segments added from the start forwards."""
    c = 0.0
    for t in range(length - 1):
        c = c + float(np.max(np.abs(path[t + 1] - path[t])))
    return c


def check_trees(res, start, goal):
    """The parents form two trees rooted at the start and the goal: every parent index is lower than its node's."""
    for t, root in ((0, start), (1, goal)):
        cnt = int(res["nodes"][t])
        if cnt == 0:
            continue
        assert res["parent"][t, 0] == -1 and np.array_equal(res["conf"][t, 0], root)
        for j in range(1, cnt):
            assert 0 <= res["parent"][t, j] < j, (t, j, res["parent"][t, j])
        assert not np.isnan(res["conf"][t, :cnt]).any()
