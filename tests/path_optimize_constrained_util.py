"""The reference of path optimisation under a pose constraint (optik_amd/csrc/path_optimize.hpp step 7), composed from
the two host drivers the project already has: one update of path_optimize_util's driver, constraint_util's projection of
its interior rows, the fallback as a bit-copying np.where on the status, and the violation as the measure driver's v
folded in waypoint order.  No arithmetic of its own."""
import numpy as np

from constraint_util import PROJECTED, build_constraint, upright_constraint  # noqa: F401 (re-exported)
from path_optimize_util import BLOCKED_QA, BLOCKED_QB, BLOCKED_SPHERE, Params, blocked_scene, build_path_optimize, line_path  # noqa: F401

# The host scene: path_optimize_util.blocked_scene() as it is -- qa and qb differ in joint 1 only and 0.4 + 1.8 = 2.2
# keeps the tool axis of the straight joint line vertical -- under upright(FK(qa), UPRIGHT_TILT).
# (found on the CPU with the composed reference alone: tests/test_path_optimize_constrained_host.py asserts that the
# line satisfies the constraint, that the unconstrained optimiser leaves it by more than UPRIGHT_TOL and that the
# constrained one clears the sphere with every waypoint within PTOL)
UPRIGHT_TILT, UPRIGHT_TOL, PTOL = 0.05, 0.05, 1e-6
PROJECT = dict(piters=256, damping=1e-6, max_step=0.5)  # optik_amd._native.CONSTRAINT_*


def box_is_free(c):
    return bool(np.all(np.isneginf(c.lo)) and np.all(np.isposinf(c.hi)))


def fold_violation(v):
    """constraint::max_take over v [B, L] in waypoint order from 0.0: the maximum, a NaN taken and then kept."""
    v = np.asarray(v, dtype=np.float64)
    out = np.zeros(v.shape[0])
    for t in range(v.shape[1]):
        a = v[:, t]
        with np.errstate(invalid="ignore"):
            out = np.where((a > out) | np.isnan(a), a, out)
    return out


class Composed:
    """po = build_path_optimize(), cref = build_constraint(); chain = the chain tables the constraint driver reads."""

    def __init__(self, po, cref):
        self.po, self.cref = po, cref

    def violation(self, chain, c, q, ee7=None):
        """The paths' violations [B] of q [B, L, n]."""
        B, L, n = q.shape
        return fold_violation(self.cref.measure(chain, c, q.reshape(B * L, n), ee7)["v"].reshape(B, L))

    def step(self, scene, prm, chain, c, q, frames, ptol, piters, damping, max_step, ee7=None, update=True):
        """One evaluation and one constrained update of q [B, L, n] on frames [B, L, n + 2, 7]: path_optimize_util's
        step() record with q the settled waypoints, plus projected [B, 2], kept [B, L] bool (the fallback was taken)
        and iterations (of the projections attempted, flat).  update=False: the evaluation alone, q as po.step left it."""
        q = np.ascontiguousarray(q, dtype=np.float64)
        B, L, n = q.shape
        res = self.po.step(scene, prm, chain["lb"], chain["ub"], q, frames)
        res["projected"] = np.zeros((B, 2), dtype=np.int32)
        res["kept"] = np.zeros((B, L), dtype=bool)
        res["iterations"] = np.zeros(0, dtype=np.int32)
        if box_is_free(c) or not update:
            return res
        stepped = res["q"][:, 1:-1].reshape(-1, n)
        p = self.cref.project(chain, c, stepped, ptol, piters, damping, max_step, ee7)
        ok = (p["status"] == PROJECTED).reshape(B, L - 2)
        new = np.where(ok[:, :, None], p["x"].reshape(B, L - 2, n), q[:, 1:-1])  # (np.where copies bits)
        res["q"] = np.concatenate([q[:, :1], new, q[:, -1:]], axis=1)
        res["projected"][:, 0] = L - 2
        res["projected"][:, 1] = ok.sum(axis=1)
        res["kept"][:, 1:-1] = ~ok
        res["iterations"] = p["iterations"]
        return res

    def optimize(self, scene, prm, chain, c, q, iters, frames_of, ptol, piters, damping, max_step):
        """`iters` constrained updates of the paths q [B, L, n] with frames_of(x) -> [n + 2, 7]: (q, first, last,
        projected [B, 2], violation [B]) -- the step() records of the first and of the last evaluation."""
        q = np.array(q, dtype=np.float64)
        projected = np.zeros((q.shape[0], 2), dtype=np.int64)
        first = last = None
        for it in range(iters + 1):
            frames = np.array([[frames_of(x) for x in path] for path in q])
            last = self.step(scene, prm, chain, c, q, frames, ptol, piters, damping, max_step, update=it < iters)
            if it == 0:
                first = last
            if it < iters:
                q = last["q"]
                projected += last["projected"]
        return q, first, last, projected, self.violation(chain, c, q)


def build_composed(workdir_po=None, workdir_c=None):
    return Composed(build_path_optimize(workdir_po), build_constraint(workdir_c))
