"""optik_amd/csrc/roadmap_goals_lazy_measure.hpp compiled with g++ as plain C++ (no HIP runtime) for the host and the
-m gpu tests of goal-set planning on lazy roadmaps: the serial reference of the loop behind one driver, in its two
forms (every query in every pass -- the specification --, and with the freezing rule applied); the random cases both
test files run, with the condition on what their traces must show; and the prescribed cases with the answers worked
out by hand."""
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

import roadmap_goals_util as gu
import roadmap_lazy_util as lu
import roadmap_util as ru
from collision_util import CSRC

UNSETTLED = lu.UNSETTLED
MAX_ROUNDS = lu.MAX_ROUNDS

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "roadmap_goals_lazy_measure.hpp"

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

template <class T>
static std::vector<T> cast(const double *p, size_t count) {
    std::vector<T> v(count);
    for (size_t i = 0; i < count; ++i) v[i] = (T)p[i];
    return v;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::vector<double> in = read_all(argv[1]);
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    // n, N, k, ks, kg, Lmax, Q, G, rounds, reset, freeze, nodes [n][N], nbr [k][N], w0 [k][N], edge_free [k][N],
    // node_free [N], w [k][N], verdict [k][N] (read unless reset), start [Q][n], goals [Q][G][n], gcount [Q],
    // sidx [ks][Q], sw [ks][Q], gidx [G][kg][Q], gw [G][kg][Q], direct [G][Q]
    // -> per query status, len, cost, which, frozen_after, path [Lmax][n]; then w [k][N], verdict [k][N], rounds_used,
    // checked
    const int n = (int)in[0], N = (int)in[1], k = (int)in[2], ks = (int)in[3], kg = (int)in[4], Lmax = (int)in[5],
              Q = (int)in[6], G = (int)in[7], rounds = (int)in[8], reset = (int)in[9], freeze = (int)in[10];
    const size_t cells = (size_t)k * N;
    const double *p = &in[11];
    const double *nodes = p; p += (size_t)n * N;
    const std::vector<int32_t> nbr = cast<int32_t>(p, cells); p += cells;
    const double *w0 = p; p += cells;
    const std::vector<uint8_t> edge_free = cast<uint8_t>(p, cells); p += cells;
    const std::vector<uint8_t> node_free = cast<uint8_t>(p, N); p += N;
    std::vector<double> w(p, p + cells); p += cells;
    std::vector<int32_t> verdict = cast<int32_t>(p, cells); p += cells;
    const double *start = p; p += (size_t)Q * n;
    const double *goals = p; p += (size_t)Q * G * n;
    const std::vector<int32_t> gcount = cast<int32_t>(p, (size_t)Q); p += (size_t)Q;
    const std::vector<int32_t> sidx = cast<int32_t>(p, (size_t)ks * Q); p += (size_t)ks * Q;
    const double *sw = p; p += (size_t)ks * Q;
    const std::vector<int32_t> gidx = cast<int32_t>(p, (size_t)G * kg * Q); p += (size_t)G * kg * Q;
    const double *gw = p; p += (size_t)G * kg * Q;
    const double *direct = p;
    if (reset) roadmap::lazy_reset_reference(N, k, nbr.data(), w0, node_free.data(), verdict.data(), w.data());
    std::vector<double> path((size_t)Q * Lmax * n), cost(Q);
    std::vector<int32_t> status(Q), len(Q), which(Q), frozen(Q);
    const roadmap::LazyCounts c = roadmap::lazy_plan_goals_reference(
        n, N, k, nodes, nbr.data(), w.data(), verdict.data(), edge_free.data(), Q, G, start, goals, gcount.data(),
        sidx.data(), sw, ks, gidx.data(), gw, kg, direct, Lmax, rounds, freeze != 0, path.data(), status.data(),
        len.data(), cost.data(), which.data(), frozen.data());
    for (int j = 0; j < Q; ++j) {
        const double head[5] = {(double)status[j], (double)len[j], cost[j], (double)which[j], (double)frozen[j]};
        std::fwrite(head, sizeof(double), 5, out);
        std::fwrite(&path[(size_t)j * Lmax * n], sizeof(double), (size_t)Lmax * n, out);
    }
    std::fwrite(w.data(), sizeof(double), cells, out);
    for (size_t e = 0; e < cells; ++e) {
        const double v = (double)verdict[e];
        std::fwrite(&v, sizeof(double), 1, out);
    }
    const double tail[2] = {(double)c.rounds_used, (double)c.checked};
    std::fwrite(tail, sizeof(double), 2, out);
    std::fclose(out);
    return 0;
}
"""

bits = ru.bits


def build_goals_lazy_ref(workdir=None):
    """Compile the driver; returns an object with
    .plan(graph, truth, queries, Lmax, rounds, state=None, freeze=False) -> dict(status, len, which, frozen_after [Q]
      int32, cost [Q], path [Lmax, Q, n], w [k, N], verdict [k, N] int32, rounds, checked) with graph and truth as
      roadmap_lazy_util has them and queries as roadmap_goals_util.  state None: the reset runs first; state = (w,
      verdict): the loop continues from them.  freeze: the reference with the freezing rule applied."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the lazy goal-set header on its own"
    d = workdir or tempfile.mkdtemp(prefix="roadmap_goals_lazy_")
    src, exe = os.path.join(d, "goals_lazy_driver.cpp"), os.path.join(d, "goals_lazy_driver")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe],
                   check=True)

    class Ref:
        @staticmethod
        def plan(graph, truth, queries, Lmax, rounds, state=None, freeze=False):
            nodes, nbr, w0 = graph["nodes"], graph["nbr"], graph["w0"]
            n, N = nodes.shape
            k = nbr.shape[0]
            G, _, Q = queries["goals"].shape
            ks, kg = queries["sidx"].shape[0], queries["gidx"].shape[1]
            w, verdict = state if state is not None else (np.zeros((k, N)), np.zeros((k, N)))
            parts = [[n, N, k, ks, kg, Lmax, Q, G, rounds, 0 if state is not None else 1, 1 if freeze else 0], nodes,
                     nbr, w0, truth["edge_free"], truth["node_free"], w, verdict, queries["start"].T,
                     queries["goals"].transpose(2, 0, 1), queries["gcount"], queries["sidx"], queries["sw"],
                     queries["gidx"], queries["gw"], queries["direct"]]
            fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(fin)
            subprocess.run([exe, fin, fout], check=True)
            out = np.fromfile(fout, dtype=np.float64)
            rows = out[:Q * (5 + Lmax * n)].reshape(Q, 5 + Lmax * n)
            rest = out[Q * (5 + Lmax * n):]
            return dict(status=rows[:, 0].astype(np.int32), len=rows[:, 1].astype(np.int32), cost=rows[:, 2].copy(),
                        which=rows[:, 3].astype(np.int32), frozen_after=rows[:, 4].astype(np.int32),
                        path=rows[:, 5:].reshape(Q, Lmax, n).transpose(1, 0, 2).copy(),
                        w=rest[:k * N].reshape(k, N).copy(), verdict=rest[k * N:2 * k * N].reshape(k, N).astype(np.int32),
                        rounds=int(rest[2 * k * N]), checked=int(rest[2 * k * N + 1]))

    return Ref()


OUTPUTS = ("status", "len", "which", "cost", "path")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.shape == b.shape and np.array_equal(bits(a), bits(b))
    return np.array_equal(a, b)


def same_or_nan(a, b):
    """same_bits, with a NaN equal to any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def assert_same_plan(name, a, b, state=True):
    """Every output of two runs of the loop, bit for bit; with state the final w, verdict and the two counters."""
    for key in OUTPUTS + (("w", "verdict") if state else ()):
        assert same_bits(a[key], b[key]), (name, key)
    if state:
        assert (a["rounds"], a["checked"]) == (b["rounds"], b["checked"]), (name, a["rounds"], a["checked"], b["rounds"],
                                                                            b["checked"])


def assert_theorem(name, lazy, eager):
    """DESIGN.md section 5.34 on one case: the lazy plan (enough rounds) against roadmap_goals_util's eager plan over
    the same slots."""
    for j, st in enumerate(lazy["status"]):
        assert st != UNSETTLED, (name, j)
        if st == ru.TOO_LONG:
            assert lazy["cost"][j] <= eager["cost"][j], (name, j)
            continue
        assert st == eager["status"][j] and lazy["len"][j] == eager["len"][j], (name, j)
        assert lazy["which"][j] == eager["which"][j], (name, j)
        assert bits(lazy["cost"][j]) == bits(eager["cost"][j]) or (
            math.isnan(lazy["cost"][j]) and math.isnan(eager["cost"][j])), (name, j)
        a, b = lazy["path"][:, j], eager["path"][:, j]
        assert np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))), (name, j)


def eager_graph(graph, truth):
    return dict(nodes=graph["nodes"], nbr=graph["nbr"], w=lu.eager_weights(graph, truth))


# ---- the random cases -----------------------------------------------------------------------------------------------

RANDOM_SIZES = ((64, 4), (200, 6))
RANDOM_Q = 24   # queries per case: six cases per graph size
# The share of free motions: at roadmap_lazy_util's 0.7 a first optimistic route of three or four hops is blocked about
# three times in four, which is what makes queries live for several passes.
P_EDGE = 0.7


def random_cases():
    """[(name, graph, truth, queries, Lmax)]: per (N, k) of RANDOM_SIZES one random directed graph (no weight
    prejudged) with a random truth table, and goal-set queries for G in {1, 3, 16} and kg in {1, 4}: gcount from 0 to G,
    NaN past the count.  Deterministic."""
    rng = np.random.default_rng(534)
    cases = []
    for N, k in RANDOM_SIZES:
        lg = lu.lazy_graph(ru.random_graph(rng, N, k, n=3, p_blocked=0.0))
        truth = lu.random_truth(rng, lg, p_edge=P_EDGE)
        for G in (1, 3, 16):
            for kg in (1, 4):
                q = gu.random_goal_queries(rng, lg, RANDOM_Q, 3, kg, G, p_direct=0.1)
                cases.append((f"lazygoals{N}x{k}_G{G}_kg{kg}", lg, truth, q, 64))
    return cases


def trace_of(res):
    """What a case's run shows, for the condition on the draws: (FOUND and settled, NO_ROUTE, frozen after pass 1 in a
    batch of at least 3 passes, live for at least 3 passes).  The loop makes rounds + 1 passes; a query is live for
    frozen_after passes, or for all of them if it was never frozen."""
    passes = res["rounds"] + 1
    fa = res["frozen_after"]
    live_for = np.where(fa == 0, passes, fa)
    return (int((res["status"] == ru.FOUND).sum()), int((res["status"] == ru.NO_ROUTE).sum()),
            int((fa == 1).sum()) if passes >= 3 else 0, int((live_for >= 3).sum()))


def assert_draws_exercise_the_loop(traces):
    """traces: {N: [trace_of(case), ...]}.  Per graph size: at least 10 queries FOUND and settled, one NO_ROUTE, one
    frozen after pass 1 in a batch that ran at least 3 passes, one live for at least 3 passes."""
    for N, rows in traces.items():
        found, none, early, late = (sum(r[i] for r in rows) for i in range(4))
        assert found >= 10 and none >= 1 and early >= 1 and late >= 1, (N, found, none, early, late)


# ---- prescribed cases, worked out by hand ---------------------------------------------------------------------------

def short_cut_graph():
    """3 -> 2 -> 1 -> 0 at 0.5 each (slot 0) and the long jump 3 -> 0 at 5.0 (slot 1 of node 3)."""
    nodes = np.array([[0.0, 1.0, 2.0, 3.0], [0.0, 0.0, 0.0, 0.0]])
    nbr, w = ru._pad_slots([[], [(0, 0.5)], [(1, 0.5)], [(2, 0.5), (0, 5.0)]], 2, 4)
    return dict(nodes=nodes, nbr=nbr, w0=w)


def prescribed_cases():
    """{name: (graph, truth, queries, Lmax)}: the small graphs whose answers tests/test_roadmap_goals_lazy_host.py
    states."""
    det, twin, cut = lu.detour_graph(), lu.twin_slots_graph(), short_cut_graph()
    # goal 0 behind node 2 (the cheap way, 0.25 + 1.0 + 0.25), goal 1 behind node 1 (0.25 + 1.5 + 0.25)
    two = gu.goal_query(2, [(3, 0.25)], [[(2, 0.25)], [(1, 0.25)]])
    twins = gu.goal_query(2, [(2, 0.25)], [[(0, 0.25)], [(0, 0.5)]])
    # Lmax 5: the cheap route of the first query, start 3 2 1 0 goal, needs 6 waypoints; the second one's, start 2 1 0
    # goal, has 5 and holds the edge 1 -> 0
    far = gu.goal_query(2, [(3, 0.25)], [[(0, 0.25)], [(0, 0.5)]])
    near = gu.goal_query(2, [(2, 0.25)], [[(0, 0.25)], [(0, 0.5)]])
    nan_in = gu.goal_query(2, [(3, 0.25)], [[(2, 0.25)], [(1, 0.25)]])
    nan_in["goals"][1, 1, 0] = math.nan
    nan_out = gu.goal_query(2, [(3, 0.25)], [[(2, 0.25)], [(1, 0.25)]], gcount=1)
    nan_out["goals"][1, 1, 0] = math.nan
    none = gu.poison(gu.goal_query(2, [(3, 0.25)], [[(2, 0.25)], [(1, 0.25)]], directs=[1.0, 1.0], gcount=0))
    return {
        "detour_two_goals": (det, lu.blocked(det, [(0, 3)]), two, 64),
        "twin_slots": (twin, lu.all_free(twin), twins, 64),
        "twin_slots_blocked": (twin, lu.blocked(twin, [(1, 2)]), twins, 64),
        "too_long_then_found": (cut, lu.blocked(cut, [(0, 1)]), lu.join_queries(far, near), 5),
        "no_goals": (det, lu.all_free(det), none, 64),
        "nan_counted": (det, lu.all_free(det), nan_in, 64),
        "nan_uncounted": (det, lu.blocked(det, [(0, 3)]), nan_out, 64),
        "lmax2_direct": (det, lu.all_free(det),
                         gu.goal_query(2, [(3, 0.25)], [[(2, 0.25)], [(1, 0.25)]], directs=[math.inf, 1.0]), 2),
        "lmax2_none": (det, lu.all_free(det), gu.goal_query(2, [(3, 0.25)], [[(2, 0.25)], [(1, 0.25)]]), 2),
        "lmax3_one_node": (det, lu.all_free(det), gu.goal_query(2, [(3, 0.25), (1, 1.0)], [[(2, 0.25)], [(1, 0.25)]]), 3),
    }


def device_cases():
    """[(name, graph, truth, queries, Lmax, rounds)] for the -m gpu test: the random cases at MAX_ROUNDS and the
    prescribed ones at 0, 1 and 8 rounds."""
    cases = [(name, g, t, q, L, MAX_ROUNDS) for name, g, t, q, L in random_cases()]
    for name, (g, t, q, L) in prescribed_cases().items():
        cases += [(f"{name}/r{r}", g, t, q, L, r) for r in (0, 1, 8)]
    return cases


def batch_case(Q, kind, ref=None):
    """(graph, truth, queries, Lmax) with Q queries on the 200-node random graph for the batch-size tests.  kind
    "mixed": random queries; "one_live": every query but number Q // 2 has only a direct motion (frozen after pass 1),
    that one is a random query that the reference `ref` keeps live for at least three passes; "all_frozen": direct
    motions only."""
    rng = np.random.default_rng(5340 + Q)
    lg = lu.lazy_graph(ru.random_graph(rng, 200, 6, n=3, p_blocked=0.0))
    truth = lu.random_truth(rng, lg, p_edge=P_EDGE)
    q = gu.random_goal_queries(rng, lg, max(Q, 2), 3, 4, 3, p_direct=0.1)
    if kind == "mixed":
        return lg, truth, (gu.take(q, [1]) if Q == 1 else q), 64
    live = None
    if kind == "one_live":
        live = {key: v.copy() for key, v in gu.take(q, [_first_long_lived(ref, lg, truth, q)]).items()}
    q["sw"][:] = np.inf          # no way into the graph: the direct motions decide
    q["gcount"][:] = 3
    q["direct"][:] = rng.uniform(0.5, 6.0, q["direct"].shape)
    q["goals"][:] = rng.uniform(-2.0, 2.0, q["goals"].shape)
    q["gw"][:] = rng.uniform(0.1, 1.0, q["gw"].shape)
    q["gidx"][:] = rng.integers(0, 200, q["gidx"].shape)
    if live is not None:
        for key in q:
            q[key][..., Q // 2] = live[key][..., 0]
    return lg, truth, q, 64


def _first_long_lived(ref, graph, truth, q):
    for j in range(q["start"].shape[1]):
        r = ref.plan(graph, truth, gu.take(q, [j]), 64, MAX_ROUNDS)
        if r["rounds"] >= 2 and r["status"][0] == ru.FOUND:
            return j
    raise AssertionError("no draw is live for three passes")
