"""optik_amd/csrc/constraint_measure.hpp compiled as plain host C++ (no HIP runtime; the math headers under
OPTIK_LANE_EMU, as tests/emu compiles them) for the host and the -m gpu tests of pose constraints; the same rules in
numpy where a test wants a second opinion; and the scene the constrained planner is tested on."""
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

from collision_util import CSRC
from motion_util import np_samples

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
PROJECTED, BUDGET_SPENT, FAILED = 0, 1, 2

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "constraint_measure.hpp"

using namespace optik;

struct HostChain {
    int32_t n_pos, has_tip;
    double origin[constraint::MAXN + 1][7];
    double axis[constraint::MAXN][3];
    double lb[constraint::MAXN], ub[constraint::MAXN];
};

static std::vector<double> read_all(const char *path) {
    std::vector<double> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) return v;
    double x;
    while (std::fread(&x, sizeof(double), 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return v;
}

static void put(FILE *out, const double *p, size_t count) { std::fwrite(p, sizeof(double), count, out); }

// in: n, has_tip, has_ee, origins [(n + 1) * 7], axes [n * 3], lb [n], ub [n], ee [7], ref [7], lo [6], hi [6],
//     tol, iters, damping, max_step, h, then the rows.
int main(int argc, char **argv) {
    if (argc < 4) return 2;
    const std::vector<double> in = read_all(argv[2]);
    FILE *out = std::fopen(argv[3], "wb");
    if (!out) return 2;
    const double *p = in.data();
    HostChain ch;
    std::memset(&ch, 0, sizeof ch);
    const int n = (int)*p++;
    ch.n_pos = n;
    ch.has_tip = (int)*p++;
    EvalParams ep;
    std::memset(&ep, 0, sizeof ep);
    ep.has_ee_offset = (int)*p++;
    for (int j = 0; j <= n; ++j) for (int i = 0; i < 7; ++i) ch.origin[j][i] = *p++;
    for (int j = 0; j < n; ++j) for (int i = 0; i < 3; ++i) ch.axis[j][i] = *p++;
    for (int j = 0; j < n; ++j) ch.lb[j] = *p++;
    for (int j = 0; j < n; ++j) ch.ub[j] = *p++;
    for (int i = 0; i < 7; ++i) ep.ee_offset[i] = *p++;
    constraint::Box c;
    for (int i = 0; i < 7; ++i) c.ref[i] = *p++;
    for (int i = 0; i < 6; ++i) c.lo[i] = *p++;
    for (int i = 0; i < 6; ++i) c.hi[i] = *p++;
    const double tol = *p++;
    const int iters = (int)*p++;
    const double damping = *p++, max_step = *p++, h = *p++;
    const double *end = in.data() + in.size();
    if (argv[1][0] == 'e') {
        // rows q [n] -> e [6], r [6], v, J [6 n]
        for (; p + n <= end; p += n) {
            double tf[7 * constraint::MAXN], J[6 * constraint::MAXN], r[6];
            const Pose ee = constraint::fk(ch, ep, n, p, tf);
            const constraint::ErrorTerms t = constraint::error(c, ee);
            constraint::residual(c, t.e, r);
            const double v = constraint::violation(r);
            constraint::task_jacobian(ch, n, tf, ee, t, J);
            put(out, t.e, 6); put(out, r, 6); put(out, &v, 1); put(out, J, 6 * (size_t)n);
        }
    } else if (argv[1][0] == 'p') {
        // rows x [n] -> x [n], v, status, iterations
        for (; p + n <= end; p += n) {
            double x[constraint::MAXN];
            for (int i = 0; i < n; ++i) x[i] = p[i];
            const constraint::Projected r = constraint::project(ch, ep, c, n, tol, iters, damping, max_step, x);
            const double t3[3] = {r.violation, (double)r.status, (double)r.iterations};
            put(out, x, n); put(out, t3, 3);
        }
    } else {
        // rows qa [n], qb [n] -> v, ok, first, steps
        for (; p + 2 * n <= end; p += 2 * n) {
            const constraint::MotionResult r = constraint::motion(ch, ep, c, n, p, 1, p + n, 1, h, tol);
            const double t4[4] = {r.violation, (double)r.ok, (double)r.first, (double)r.steps};
            put(out, t4, 4);
        }
    }
    std::fclose(out);
    return 0;
}
"""


def _compiler():
    # (ik_math.hpp's small vectors are ext_vector_type: clang, as tests/emu/binding.py)
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("amdclang++"), shutil.which("clang++")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("no clang++ found (the math headers need ext_vector_type)")


class Constraint:
    """(ref7, lo6, hi6) as the C layer takes them."""

    def __init__(self, ref7, lo, hi):
        self.ref = self.ref7 = np.ascontiguousarray(ref7, dtype=np.float64)
        self.lo = np.ascontiguousarray(lo, dtype=np.float64)
        self.hi = np.ascontiguousarray(hi, dtype=np.float64)
        assert self.ref.shape == (7,) and self.lo.shape == (6,) and self.hi.shape == (6,)


def free_constraint(ref7):
    return Constraint(ref7, [-np.inf] * 6, [np.inf] * 6)


def pinned_constraint(ref7, at=None):
    at = np.zeros(6) if at is None else np.asarray(at, dtype=np.float64)
    return Constraint(ref7, at, at)


def upright_constraint(ref7, tilt):
    b = tilt / math.sqrt(2.0)
    return Constraint(ref7, [-np.inf, -np.inf, -np.inf, -b, -b, -np.inf], [np.inf, np.inf, np.inf, b, b, np.inf])


def build_constraint(workdir=None):
    """Compile the driver; returns an object with (chain = the dict of Robot.chain_tables(), c a Constraint)
    .measure(chain, c, q [B, n], ee7=None) -> dict(e [B, 6], r [B, 6], v [B], J [B, 6, n]),
    .project(chain, c, x [B, n], tol, iters, damping, max_step, ee7=None) -> dict(x [B, n], v [B], status, iterations),
    .motion(chain, c, qa [B, n], qb [B, n], h, tol, ee7=None) -> dict(v [B], ok [B] bool, first, steps)."""
    d = workdir or tempfile.mkdtemp(prefix="constraint_")
    src, exe = os.path.join(d, "constraint_driver.cpp"), os.path.join(d, "constraint_driver")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([_compiler(), "-std=c++17", "-O2", "-ffp-contract=off", "-DOPTIK_LANE_EMU", "-pthread", "-Wall",
                    "-Wno-unused-value", "-Wno-psabi", "-Wno-unused-function", "-I", EMU, "-I", CSRC, src, "-o", exe],
                   check=True)

    def run(mode, chain, c, rows, ee7=None, tol=0.0, iters=0, damping=0.0, max_step=0.0, h=0.0):
        n = len(chain["lb"])
        origins = np.asarray(chain["origins"], dtype=np.float64).reshape(-1, 7)
        tip = len(origins) > n
        if not tip:
            origins = np.concatenate([origins, [[0.0, 0, 0, 0, 0, 0, 1]]])
        ee = np.asarray(ee7 if ee7 is not None else [0.0, 0, 0, 0, 0, 0, 1], dtype=np.float64)
        parts = [[n, int(tip), int(ee7 is not None)], origins[:n + 1], np.asarray(chain["axes"]).reshape(-1, 3)[:n],
                 chain["lb"], chain["ub"], ee, c.ref, c.lo, c.hi, [tol, iters, damping, max_step, h], rows]
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(fin)
        subprocess.run([exe, mode, fin, fout], check=True)
        return np.fromfile(fout, dtype=np.float64)

    class Ref:
        @staticmethod
        def measure(chain, c, q, ee7=None):
            q = np.atleast_2d(np.asarray(q, dtype=np.float64))
            B, n = q.shape
            o = run("e", chain, c, q, ee7).reshape(B, 13 + 6 * n)
            return dict(e=o[:, :6].copy(), r=o[:, 6:12].copy(), v=o[:, 12].copy(),
                        J=o[:, 13:].reshape(B, n, 6).transpose(0, 2, 1).copy())

        @staticmethod
        def project(chain, c, x, tol, iters, damping, max_step, ee7=None):
            x = np.atleast_2d(np.asarray(x, dtype=np.float64))
            B, n = x.shape
            o = run("p", chain, c, x, ee7, tol=tol, iters=iters, damping=damping, max_step=max_step).reshape(B, n + 3)
            return dict(x=o[:, :n].copy(), v=o[:, n].copy(), status=o[:, n + 1].astype(np.int32),
                        iterations=o[:, n + 2].astype(np.int32))

        @staticmethod
        def motion(chain, c, qa, qb, h, tol, ee7=None):
            qa, qb = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (qa, qb))
            o = run("m", chain, c, np.concatenate([qa, qb], axis=1), ee7, tol=tol, h=h).reshape(len(qa), 4)
            return dict(v=o[:, 0].copy(), ok=o[:, 1] != 0, first=o[:, 2].astype(np.int32),
                        steps=o[:, 3].astype(np.int32))

    return Ref()


def np_motion(ref, chain, c, qa, qb, h, tol, ee7=None):
    """Step 7 restated: the samples from motion_util.np_samples, the violations from ref.measure, numpy's max."""
    d, K, s = np_samples(qa, qb, h)
    if K < 0:
        return math.nan, False, -1, -1
    v = ref.measure(chain, c, s, ee7)["v"]
    bad = np.nonzero(~(v <= tol))[0]
    return (math.nan if np.isnan(v).any() else float(v.max())), len(bad) == 0, (int(bad[0]) if len(bad) else -1), K


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def pose7_of(m):
    """A 4x4 homogeneous matrix as (t, quaternion i j k w), w >= 0 (numpy; the tests' own conversion)."""
    m = np.asarray(m, dtype=np.float64)
    R = m[:3, :3]
    w = math.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    if w > 1e-6:
        q = [(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(max(0.0, 1.0 + R[i, i] - R[j, j] - R[k, k])) * 2.0
        q = [0.0, 0.0, 0.0, (R[k, j] - R[j, k]) / s]
        q[i], q[j], q[k] = s / 4.0, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    q = np.array(q) / np.linalg.norm(q)
    return np.concatenate([m[:3, 3], q])


# ---- the planner's scene: a Panda without a collision model, the end effector kept upright --------------------------
# (chosen on the CPU: tests/test_constraint_host.py asserts that the serial reference finds a route for at least one
# of the PLAN_Q queries and that the constraint blocks at least one edge over these nodes)
PANDA_HOME = [0.0, -0.785398163397, 0.0, -2.35619449019, 0.0, 1.57079632679, 0.785398163397]
PLAN_N, PLAN_K, PLAN_KS, PLAN_Q, PLAN_H, PLAN_LMAX = 128, 8, 4, 8, 0.1, 32
PLAN_TILT, PLAN_TOL, PLAN_PROJECT_TOL = 0.3, 0.05, 1e-6
PLAN_SEED = 5
PROJECT_DEFAULTS = dict(iters=256, damping=1e-6, max_step=0.5)  # optik_amd._native.CONSTRAINT_*


def plan_scene(ref, chain, oracle_fk_home7):
    """The scene of the planner tests, made on the CPU with the host header: PLAN_N uniform samples projected onto
    upright(home, PLAN_TILT) (NaN columns where the projection failed), and PLAN_Q projected starts and goals."""
    rng = np.random.default_rng(PLAN_SEED)
    lb, ub = np.asarray(chain["lb"]), np.asarray(chain["ub"])
    c = upright_constraint(oracle_fk_home7, PLAN_TILT)

    def projected(count):
        p = ref.project(chain, c, rng.uniform(lb, ub, (count, len(lb))), PLAN_PROJECT_TOL, **PROJECT_DEFAULTS)
        return p["x"], p["status"] == PROJECTED

    x, ok = projected(PLAN_N)
    nodes = np.where(ok[:, None], x, np.nan).T.copy()
    # starts and goals: nodes' neighbours in spirit -- a projected sample each, the failures replaced by a good one
    sg, sok = projected(4 * PLAN_Q)
    sg = sg[sok][:2 * PLAN_Q]
    assert len(sg) == 2 * PLAN_Q
    return dict(c=c, nodes=nodes, projected=int(ok.sum()), starts=sg[:PLAN_Q].T.copy(), goals=sg[PLAN_Q:].T.copy())


def cpu_plan(ref, roadmap_ref, chain, scene):
    """roadmap_build_constrained and roadmap_plan_constrained restated on the CPU for a chain without a collision
    model: kNN in numpy in (distance, index) order, the weights max_i |diff| where the motion is sampled, the
    constraint mask from the host header in the direction of travel, and the serial roadmap reference for the query.
    Returns (graph, unmasked w, queries, plan)."""
    from motion_util import np_steps
    from roadmap_util import np_knn, np_weights
    nodes, c = scene["nodes"], scene["c"]

    def links(a, b):  # a, b [n, M]: the weights of the motions a -> b, unmasked and masked
        with np.errstate(invalid="ignore"):
            w = np_weights(a, b)
        sampled = np.array([np_steps(d, PLAN_H) >= 0 for d in w])
        w = np.where(sampled, w, np.inf)
        ok = ref.motion(chain, c, a.T, b.T, PLAN_H, PLAN_TOL)["ok"]
        return w, np.where(ok, w, np.inf)

    def fan(q, idx, reverse=False):  # q [n, Q], idx [k, Q]
        k, Q = idx.shape
        a = np.repeat(q[:, None, :], k, axis=1).reshape(len(q), k * Q)
        b = nodes[:, np.maximum(idx, 0).reshape(-1)]
        w0, w = links(b, a) if reverse else links(a, b)
        dead = (idx < 0).reshape(-1)
        return np.where(dead, np.inf, w0).reshape(k, Q), np.where(dead, np.inf, w).reshape(k, Q)

    nbr, _ = np_knn(nodes, nodes, PLAN_K, exclude_self=True)
    w0, w = fan(nodes, nbr)
    sidx, _ = np_knn(scene["starts"], nodes, PLAN_KS)
    gidx, _ = np_knn(scene["goals"], nodes, PLAN_KS)
    _, sw = fan(scene["starts"], sidx)
    _, gw = fan(scene["goals"], gidx, reverse=True)
    _, direct = links(scene["starts"], scene["goals"])
    graph = dict(nodes=nodes, nbr=nbr, w=w)
    queries = dict(start=scene["starts"], goal=scene["goals"], sidx=sidx, sw=sw, gidx=gidx, gw=gw, direct=direct)
    return graph, w0, queries, roadmap_ref.query(graph, queries, PLAN_LMAX)
