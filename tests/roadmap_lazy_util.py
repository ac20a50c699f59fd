"""optik_amd/csrc/roadmap_lazy_measure.hpp compiled with g++ as plain C++ (no HIP runtime) for the host and the -m gpu
tests of lazy roadmaps: the serial reference of the reset and of the plan loop behind one driver, the eager graph that
belongs to a lazy graph and a truth table, and the graphs both test files run (roadmap_util's synthetic cases and
random directed graphs, each with a truth table in place of the motion check)."""
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

import roadmap_util as ru
from collision_util import CSRC

UNKNOWN, FREE, BLOCKED = 0, 1, 2
UNSETTLED = 4
MAX_ROUNDS = 4096

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "roadmap_lazy_measure.hpp"

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
    // n, N, k, ks, kg, Lmax, Q, rounds, reset, nodes [n][N], nbr [k][N], w0 [k][N], edge_free [k][N], node_free [N],
    // w [k][N], verdict [k][N] (read unless reset), start [Q][n], goal [Q][n], sidx [ks][Q], sw [ks][Q], gidx [kg][Q],
    // gw [kg][Q], direct [Q]
    // -> per query status, len, cost, path [Lmax][n]; then w [k][N], verdict [k][N], rounds_used, checked
    const int n = (int)in[0], N = (int)in[1], k = (int)in[2], ks = (int)in[3], kg = (int)in[4], Lmax = (int)in[5],
              Q = (int)in[6], rounds = (int)in[7], reset = (int)in[8];
    const size_t cells = (size_t)k * N;
    const double *p = &in[9];
    const double *nodes = p; p += (size_t)n * N;
    const std::vector<int32_t> nbr = cast<int32_t>(p, cells); p += cells;
    const double *w0 = p; p += cells;
    const std::vector<uint8_t> edge_free = cast<uint8_t>(p, cells); p += cells;
    const std::vector<uint8_t> node_free = cast<uint8_t>(p, N); p += N;
    std::vector<double> w(p, p + cells); p += cells;
    std::vector<int32_t> verdict = cast<int32_t>(p, cells); p += cells;
    const double *start = p; p += (size_t)Q * n;
    const double *goal = p; p += (size_t)Q * n;
    const std::vector<int32_t> sidx = cast<int32_t>(p, (size_t)ks * Q); p += (size_t)ks * Q;
    const double *sw = p; p += (size_t)ks * Q;
    const std::vector<int32_t> gidx = cast<int32_t>(p, (size_t)kg * Q); p += (size_t)kg * Q;
    const double *gw = p; p += (size_t)kg * Q;
    const double *direct = p;
    if (reset) roadmap::lazy_reset_reference(N, k, nbr.data(), w0, node_free.data(), verdict.data(), w.data());
    std::vector<double> path((size_t)Q * Lmax * n), cost(Q);
    std::vector<int32_t> status(Q), len(Q);
    const roadmap::LazyCounts c = roadmap::lazy_plan_reference(
        n, N, k, nodes, nbr.data(), w.data(), verdict.data(), edge_free.data(), Q, start, goal, sidx.data(), sw, ks,
        gidx.data(), gw, kg, direct, Lmax, rounds, path.data(), status.data(), len.data(), cost.data());
    for (int j = 0; j < Q; ++j) {
        const double head[3] = {(double)status[j], (double)len[j], cost[j]};
        std::fwrite(head, sizeof(double), 3, out);
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


def build_lazy_ref(workdir=None):
    """Compile the driver; returns an object with
    .plan(graph, truth, queries, Lmax, rounds, state=None) -> dict(status, len, cost [Q], path [Lmax, Q, n], w
      [k, N], verdict [k, N] int32, rounds, checked) with graph = dict(nodes [n, N], nbr [k, N], w0 [k, N]), truth =
      dict(edge_free [k, N], node_free [N]) uint8 and queries as roadmap_util has them.  state None: the reset runs
      first; state = (w, verdict): the loop continues from them."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the lazy roadmap header on its own"
    d = workdir or tempfile.mkdtemp(prefix="roadmap_lazy_")
    src, exe = os.path.join(d, "roadmap_lazy_driver.cpp"), os.path.join(d, "roadmap_lazy_driver")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe],
                   check=True)

    class Ref:
        @staticmethod
        def plan(graph, truth, queries, Lmax, rounds, state=None):
            nodes, nbr, w0 = graph["nodes"], graph["nbr"], graph["w0"]
            n, N = nodes.shape
            k = nbr.shape[0]
            Q = queries["start"].shape[1]
            ks, kg = queries["sidx"].shape[0], queries["gidx"].shape[0]
            w, verdict = state if state is not None else (np.zeros((k, N)), np.zeros((k, N)))
            parts = [[n, N, k, ks, kg, Lmax, Q, rounds, 0 if state is not None else 1], nodes, nbr, w0,
                     truth["edge_free"], truth["node_free"], w, verdict, queries["start"].T, queries["goal"].T,
                     queries["sidx"], queries["sw"], queries["gidx"], queries["gw"], queries["direct"]]
            fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(fin)
            subprocess.run([exe, fin, fout], check=True)
            out = np.fromfile(fout, dtype=np.float64)
            rows = out[:Q * (3 + Lmax * n)].reshape(Q, 3 + Lmax * n)
            rest = out[Q * (3 + Lmax * n):]
            return dict(status=rows[:, 0].astype(np.int32), len=rows[:, 1].astype(np.int32), cost=rows[:, 2].copy(),
                        path=rows[:, 3:].reshape(Q, Lmax, n).transpose(1, 0, 2).copy(),
                        w=rest[:k * N].reshape(k, N).copy(), verdict=rest[k * N:2 * k * N].reshape(k, N).astype(np.int32),
                        rounds=int(rest[2 * k * N]), checked=int(rest[2 * k * N + 1]))

    return Ref()


def all_free(graph):
    k, N = graph["nbr"].shape
    return dict(edge_free=np.ones((k, N), dtype=np.uint8), node_free=np.ones(N, dtype=np.uint8))


def random_truth(rng, graph, p_edge=0.7, p_node=0.9):
    """A truth table in place of the motion check: which slots' motions are free, which nodes are."""
    k, N = graph["nbr"].shape
    return dict(edge_free=(rng.random((k, N)) < p_edge).astype(np.uint8),
                node_free=(rng.random(N) < p_node).astype(np.uint8))


def eager_weights(graph, truth):
    """What optik_hip_roadmap_edges gives over the same slots in the truth table's world: the weight where the motion
    is free -- which needs both its ends free --, +inf elsewhere."""
    nbr, w0 = graph["nbr"], graph["w0"]
    k, N = nbr.shape
    ok = (nbr >= 0) & (nbr < N)
    nf = truth["node_free"].astype(bool)
    free = ok & truth["edge_free"].astype(bool) & nf[None, :] & nf[np.where(ok, nbr, 0)] & np.isfinite(w0)
    return np.where(free, w0, np.inf)


def lazy_graph(graph):
    """roadmap_util's graph as a lazy one: its weights are the unchecked ones (+inf stays no edge)."""
    return dict(nodes=graph["nodes"], nbr=graph["nbr"], w0=graph["w"])


RANDOM_SIZES = [(N, k) for N in (1, 2, 65, 130, 300) for k in (1, 6, 16)]
RANDOM_JOINTS = (1, 7, 10)  # the chains the -m gpu test runs the random graphs on


def lazy_cases():
    """[(name, graph, truth, queries, Lmax, random)]: roadmap_util's synthetic cases, each with every motion free and
    with a random truth table, and random directed graphs (no weight prejudged) with random truth tables.
    Deterministic."""
    rng = np.random.default_rng(524)
    cases = []
    for name, g, q, L in ru.synthetic_cases():
        lg = lazy_graph(g)
        cases.append((name + "/free", lg, all_free(lg), q, L, False))
        cases.append((name + "/rand", lg, random_truth(rng, lg), q, L, False))
    for i, (N, k) in enumerate(RANDOM_SIZES):
        n = RANDOM_JOINTS[i % 3]
        lg = lazy_graph(ru.random_graph(rng, N, k, n=n, p_blocked=0.0))
        cases.append((f"lazy{N}x{k}", lg, random_truth(rng, lg), ru.queries_for(rng, lg, 5, 3, 2), 64, True))
    return cases


def chain_graph(weights, n=2):
    """Nodes len(weights) .. 0 in a line: node v has the one edge v -> v - 1 of weight weights[v - 1]; node 0 none."""
    N = len(weights) + 1
    nodes = np.zeros((n, N))
    nodes[0] = np.arange(N)
    nbr, w = ru._pad_slots([[]] + [[(v - 1, weights[v - 1])] for v in range(1, N)], 1, N)
    return dict(nodes=nodes, nbr=nbr, w0=w)


def detour_graph():
    """3 -> 2 -> 0 (1.0 + 0.5) and 3 -> 1 -> 0 (1.5 + 0.5): the optimistic route goes by node 2."""
    nodes = np.array([[0.0, 1.0, 1.0, 2.0], [0.0, 0.5, -0.5, 0.0]])
    nbr, w = ru._pad_slots([[], [(0, 0.5)], [(0, 0.5)], [(2, 1.0), (1, 1.5)]], 2, 4)
    return dict(nodes=nodes, nbr=nbr, w0=w)


def twin_slots_graph():
    """Node 2 lists node 1 three times, at weights 2.0, 1.0 and 1.0, in that order; 1 -> 0."""
    nodes = np.array([[0.0, 1.0, 2.0], [0.0, 0.0, 0.0]])
    nbr, w = ru._pad_slots([[], [(0, 0.5)], [(1, 2.0), (1, 1.0), (1, 1.0)]], 3, 3)
    return dict(nodes=nodes, nbr=nbr, w0=w)


def blocked(graph, slots):
    """Every motion free but those of `slots` [(s, v)]."""
    t = all_free(graph)
    for s, v in slots:
        t["edge_free"][s, v] = 0
    return t


def join_queries(*qs):
    return {key: np.ascontiguousarray(np.concatenate([q[key] for q in qs], axis=-1)) for key in qs[0]}


def prescribed_cases():
    """{name: (graph, truth, queries, Lmax)}: the small graphs whose answers the host test states."""
    det, twin = detour_graph(), twin_slots_graph()
    via3 = ru.one_query(2, [(3, 0.25)], [(0, 0.25)])
    other = ru.one_query(2, [(3, 0.75)], [(0, 0.5)])
    line = chain_graph([0.5, 0.5, 0.5])                     # 3 -> 2 -> 1 -> 0: start, four nodes, goal
    return {
        "detour_blocked": (det, blocked(det, [(0, 3)]), via3, 64),
        "shared_edge": (det, all_free(det), join_queries(via3, other), 64),
        "twin_slots": (twin, all_free(twin), ru.one_query(2, [(2, 0.25)], [(0, 0.25)]), 64),
        "twin_slots_blocked": (twin, blocked(twin, [(1, 2)]), ru.one_query(2, [(2, 0.25)], [(0, 0.25)]), 64),
        "exactly_lmax": (line, all_free(line), ru.one_query(2, [(3, 0.25)], [(0, 0.25)]), 6),
        "one_too_long": (line, all_free(line), ru.one_query(2, [(3, 0.25)], [(0, 0.25)]), 5),
    }


# The pairs the wall scene (roadmap_util.wall_scene) is planned for here.  Its own pair is routed start -> one node ->
# goal: both legs are links, checked eagerly with the query, so a lazy plan of it checks no edge and is settled by its
# first pass.  The second pair is the same move begun and ended further out (joint 0 at -2 and +2 rad): its route
# crosses several nodes and its first optimistic route runs into the wall (tests/test_roadmap_lazy_host.py asserts both
# on the CPU).
WALL_WIDE_JOINT0 = 2.0


def wall_pairs(scene):
    """(starts [2, n], goals [2, n]): the scene's own pair, then the wide one."""
    s, g = scene["start"].copy(), scene["goal"].copy()
    s[0], g[0] = -WALL_WIDE_JOINT0, WALL_WIDE_JOINT0
    return np.stack([scene["start"], s]), np.stack([scene["goal"], g])


def assert_theorem(name, lazy, eager):
    """DESIGN.md section 5.24 on one case: the lazy plan (enough rounds) against the eager plan over the same slots."""
    for j, st in enumerate(lazy["status"]):
        assert st != UNSETTLED, (name, j)
        if st == ru.TOO_LONG:
            assert lazy["cost"][j] <= eager["cost"][j], (name, j)
            continue
        assert st == eager["status"][j] and lazy["len"][j] == eager["len"][j], (name, j)
        assert ru.bits(lazy["cost"][j]) == ru.bits(eager["cost"][j]) or (
            math.isnan(lazy["cost"][j]) and math.isnan(eager["cost"][j])), (name, j)
        a, b = lazy["path"][:, j], eager["path"][:, j]
        assert np.all((ru.bits(a) == ru.bits(b)) | (np.isnan(a) & np.isnan(b))), (name, j)
