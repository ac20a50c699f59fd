"""optik_amd/csrc/rrt_constrained_measure.hpp compiled with g++ as plain C++ (no HIP runtime) into a small shared
library for the host and the -m gpu tests of the tree planner under a pose constraint: the serial reference
plan_constrained_reference with the verdicts AND the projection as Python callbacks.  Beside it
constraint_measure.hpp as a second shared library (clang++, the math headers under OPTIK_LANE_EMU as constraint_util
compiles them) so that a host test can answer thousands of callbacks without a process each.  The scenes and the
helpers are rrt_util's, rrt_goals_util's and constraint_util's."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from collision_util import CSRC
from constraint_util import EMU, PROJECTED, BUDGET_SPENT, FAILED, _compiler  # noqa: F401
from rrt_util import FOUND, NO_ROUTE, TOO_LONG, QUERY_NAN, forward_cost, _dp  # noqa: F401

DRIVER = r"""
#include "rrt_constrained_measure.hpp"

using namespace optik;

extern "C" {

typedef int (*config_fn)(const double *q);
typedef void (*motions_fn)(int count, const double *qa, const double *qb, unsigned char *ok_out);
typedef int (*project_fn)(double *x, int *iterations);

// out: status, len, iters_used, nodes[2], junction[2], which, roots, projected[2]
void rrt_plan_constrained(int n, const double *lo, const double *hi, const double *start, const double *goals, int G,
                          int count, const double *samples, int I, double eta, int M, int Lmax, config_fn config_ok,
                          motions_fn motions_ok, project_fn project, double *conf, int32_t *parent, int32_t *root_goal,
                          double *path, double *cost, int32_t *out) {
    const rrt::ConstrainedResult r = rrt::plan_constrained_reference(
        n, lo, hi, start, goals, G, count, samples, I, eta, M, Lmax,
        [&](const double *q) { return config_ok(q) != 0; },
        [&](int c, const double *qa, const double *qb, unsigned char *f) { motions_ok(c, qa, qb, f); },
        [&](double *x, int *its) { return project(x, its); }, conf, parent, root_goal, path);
    *cost = r.r.cost;
    out[0] = r.r.status; out[1] = r.r.len; out[2] = r.r.iters_used;
    out[3] = r.r.nodes[0]; out[4] = r.r.nodes[1]; out[5] = r.r.junction[0]; out[6] = r.r.junction[1];
    out[7] = r.which; out[8] = r.roots; out[9] = r.projected[0]; out[10] = r.projected[1];
}

int rrt_takes(int status, int iterations, int same) { return rrt::takes(status, iterations, same != 0) ? 1 : 0; }

}  // extern "C"
"""

CONSTRAINT_LIB = r"""
#include "constraint_measure.hpp"

using namespace optik;

struct HostChain {
    int32_t n_pos, has_tip;
    double origin[constraint::MAXN + 1][7];
    double axis[constraint::MAXN][3];
    double lb[constraint::MAXN], ub[constraint::MAXN];
};

static HostChain g_ch;
static EvalParams g_ep;
static constraint::Box g_c;

extern "C" {

// origins [(n + 1) * 7], axes [n * 3], lb [n], ub [n], ee [7], ref [7], lo [6], hi [6]
void cm_set(int n, int has_tip, int has_ee, const double *origins, const double *axes, const double *lb,
            const double *ub, const double *ee, const double *ref, const double *lo, const double *hi) {
    std::memset(&g_ch, 0, sizeof g_ch);
    std::memset(&g_ep, 0, sizeof g_ep);
    g_ch.n_pos = n;
    g_ch.has_tip = has_tip;
    g_ep.has_ee_offset = has_ee;
    for (int j = 0; j <= n; ++j) for (int i = 0; i < 7; ++i) g_ch.origin[j][i] = origins[7 * j + i];
    for (int j = 0; j < n; ++j) for (int i = 0; i < 3; ++i) g_ch.axis[j][i] = axes[3 * j + i];
    for (int j = 0; j < n; ++j) { g_ch.lb[j] = lb[j]; g_ch.ub[j] = ub[j]; }
    for (int i = 0; i < 7; ++i) { g_ep.ee_offset[i] = ee[i]; g_c.ref[i] = ref[i]; }
    for (int i = 0; i < 6; ++i) { g_c.lo[i] = lo[i]; g_c.hi[i] = hi[i]; }
}

double cm_violation(const double *q) {
    double r[6];
    return constraint::measure(g_ch, g_ep, g_c, g_ch.n_pos, q, r);
}

int cm_project(double *x, double tol, int iters, double damping, double max_step, int *iterations, double *violation) {
    const constraint::Projected p = constraint::project(g_ch, g_ep, g_c, g_ch.n_pos, tol, iters, damping, max_step, x);
    *iterations = p.iterations;
    *violation = p.violation;
    return p.status;
}

int cm_motion_ok(const double *qa, const double *qb, double h, double tol, double *violation) {
    const constraint::MotionResult m = constraint::motion(g_ch, g_ep, g_c, g_ch.n_pos, qa, 1, qb, 1, h, tol);
    *violation = m.violation;
    return m.ok;
}

}  // extern "C"
"""


def build_rrt_constrained_ref(workdir=None):
    """Compile the driver; returns an object with
    .plan(lo, hi, start, goals [G, n], count, samples [I, n], step, max_nodes, Lmax, config_ok, motions_ok, project)
      -> dict(status, len, iters, nodes [2], junction [2], which, roots, projected [2], cost, path [Lmax, n], conf
      [2, M, n], parent [2, M], root_goal [G], projections: the (status, iterations) of every projection asked for, in
      order); config_ok(q [n]) -> bool (free AND within the constraint), motions_ok(qa [c, n], qb [c, n]) -> c bools
      (both checks, qa -> qb the direction of travel), project(x [n]) -> (x' [n], status, iterations);
    .takes(status, iterations, same) -> bool, the header's rule."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the tree planner's header on its own"
    d = workdir or tempfile.mkdtemp(prefix="rrt_constrained_")
    src, so = os.path.join(d, "rrt_constrained_driver.cpp"), os.path.join(d, "librrt_constrained_driver.so")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                    src, "-o", so], check=True)
    lib = C.CDLL(so)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    CONFIG = C.CFUNCTYPE(C.c_int, dp)
    MOTIONS = C.CFUNCTYPE(None, C.c_int, dp, dp, C.POINTER(C.c_uint8))
    PROJECT = C.CFUNCTYPE(C.c_int, dp, C.POINTER(C.c_int))
    lib.rrt_plan_constrained.argtypes = [C.c_int, dp, dp, dp, dp, C.c_int, C.c_int, dp, C.c_int, C.c_double, C.c_int,
                                         C.c_int, CONFIG, MOTIONS, PROJECT, dp, ip, ip, dp, dp, ip]
    lib.rrt_plan_constrained.restype = None
    lib.rrt_takes.argtypes = [C.c_int, C.c_int, C.c_int]

    class Ref:
        @staticmethod
        def plan(lo, hi, start, goals, count, samples, step, max_nodes, Lmax, config_ok, motions_ok, project):
            lo, hi, start, goals = (np.ascontiguousarray(v, dtype=np.float64) for v in (lo, hi, start, goals))
            samples = np.ascontiguousarray(samples, dtype=np.float64)
            I, n = samples.shape
            G, M = goals.shape[0], int(max_nodes)
            assert goals.shape == (G, n) and M >= max(2, G)
            failed, projections = [], []

            def cfg(q):
                try:
                    return 1 if config_ok(np.ctypeslib.as_array(q, (n,)).copy()) else 0
                except BaseException as e:  # (an exception cannot cross the C frames: kept, raised below)
                    failed.append(e)
                    return 0

            def mot(count_, qa, qb, out):
                try:
                    f = motions_ok(np.ctypeslib.as_array(qa, (count_, n)).copy(),
                                   np.ctypeslib.as_array(qb, (count_, n)).copy())
                    for j in range(count_):
                        out[j] = 1 if f[j] else 0
                except BaseException as e:
                    failed.append(e)
                    for j in range(count_):
                        out[j] = 0

            def prj(x, its):
                try:
                    xv = np.ctypeslib.as_array(x, (n,))
                    xn, status, iterations = project(xv.copy())
                    xv[:] = xn
                    its[0] = int(iterations)
                    projections.append((int(status), int(iterations)))
                    return int(status)
                except BaseException as e:
                    failed.append(e)
                    its[0] = 0
                    return FAILED

            conf = np.full((2, M, n), np.nan)
            parent = np.full((2, M), -2, dtype=np.int32)
            root_goal = np.full(G, -2, dtype=np.int32)
            path = np.zeros((int(Lmax), n))
            cost = C.c_double(0.0)
            out = np.zeros(11, dtype=np.int32)
            lib.rrt_plan_constrained(n, _dp(lo), _dp(hi), _dp(start), _dp(goals), G, int(count), _dp(samples), I,
                                     float(step), M, int(Lmax), CONFIG(cfg), MOTIONS(mot), PROJECT(prj), _dp(conf),
                                     parent.ctypes.data_as(ip), root_goal.ctypes.data_as(ip), _dp(path), C.byref(cost),
                                     out.ctypes.data_as(ip))
            if failed:
                raise failed[0]
            return dict(status=int(out[0]), len=int(out[1]), iters=int(out[2]), nodes=out[3:5].copy(),
                        junction=out[5:7].copy(), which=int(out[7]), roots=int(out[8]), projected=out[9:11].copy(),
                        cost=float(cost.value), path=path, conf=conf, parent=parent, root_goal=root_goal,
                        projections=projections)

        @staticmethod
        def takes(status, iterations, same):
            return bool(lib.rrt_takes(int(status), int(iterations), 1 if same else 0))

    return Ref()


class HostConstraint:
    """constraint_measure.hpp on the host for one chain (the dict of Robot.chain_tables()) and one constraint (a
    constraint_util.Constraint): .violation(q), .project(x, tol, iters, damping, max_step) -> (x', status, iterations),
    .motion_ok(qa, qb, h, tol).  One object at a time per library: the chain and the box are the library's globals."""

    def __init__(self, lib, chain, c, ee7=None):
        self._lib = lib
        n = len(chain["lb"])
        origins = np.asarray(chain["origins"], dtype=np.float64).reshape(-1, 7)
        tip = len(origins) > n
        if not tip:
            origins = np.concatenate([origins, [[0.0, 0, 0, 0, 0, 0, 1]]])
        ee = np.asarray(ee7 if ee7 is not None else [0.0, 0, 0, 0, 0, 0, 1], dtype=np.float64)
        arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in
                  (origins[:n + 1], np.asarray(chain["axes"]).reshape(-1, 3)[:n], chain["lb"], chain["ub"], ee, c.ref,
                   c.lo, c.hi)]
        lib.cm_set(n, int(tip), int(ee7 is not None), *(_dp(a) for a in arrays))
        self.n = n

    def violation(self, q):
        q = np.ascontiguousarray(q, dtype=np.float64)
        return float(self._lib.cm_violation(_dp(q)))

    def project(self, x, tol, iters, damping, max_step):
        x = np.array(x, dtype=np.float64)
        its, v = C.c_int(0), C.c_double(0.0)
        status = self._lib.cm_project(_dp(x), float(tol), int(iters), float(damping), float(max_step), C.byref(its),
                                      C.byref(v))
        return x, int(status), int(its.value)

    def motion_ok(self, qa, qb, h, tol):
        v = C.c_double(0.0)
        out = []
        for a, b in zip(np.atleast_2d(qa), np.atleast_2d(qb)):
            a, b = (np.ascontiguousarray(t, dtype=np.float64) for t in (a, b))
            out.append(bool(self._lib.cm_motion_ok(_dp(a), _dp(b), float(h), float(tol), C.byref(v))))
        return np.array(out, dtype=bool)


def build_host_constraint_lib(workdir=None):
    """constraint_measure.hpp as a shared library; HostConstraint(lib, chain, c) uses it."""
    d = workdir or tempfile.mkdtemp(prefix="rrt_constrained_cm_")
    src, so = os.path.join(d, "constraint_lib.cpp"), os.path.join(d, "libconstraint_host.so")
    with open(src, "w") as fh:
        fh.write(CONSTRAINT_LIB)
    subprocess.run([_compiler(), "-std=c++17", "-O2", "-ffp-contract=off", "-DOPTIK_LANE_EMU", "-pthread", "-Wall",
                    "-Wno-unused-value", "-Wno-psabi", "-Wno-unused-function", "-shared", "-fPIC", "-I", EMU, "-I", CSRC,
                    src, "-o", so], check=True)
    lib = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    lib.cm_set.argtypes = [C.c_int, C.c_int, C.c_int] + [dp] * 8
    lib.cm_set.restype = None
    lib.cm_violation.argtypes = [dp]
    lib.cm_violation.restype = C.c_double
    lib.cm_project.argtypes = [dp, C.c_double, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_int), dp]
    lib.cm_motion_ok.argtypes = [dp, dp, C.c_double, C.c_double, dp]
    return lib


# ---- the Panda scene of the constrained planner ---------------------------------------------------------------------
# roadmap_util.wall_scene()'s wall and upright(fk(start), TILT): the end effector keeps the
# orientation it has at the start within TILT.  The constants and what the serial reference gives with them on the host
# are in tests/test_rrt_constrained_host.py, which asserts them.
TILT, TOL, PTOL = 0.3, 0.05, 1e-6
PITERS, DAMPING, MAX_STEP = 16, 1e-6, 0.5
ITERS, STEP, FIRST, NODES = 128, 0.5, 1, 64
