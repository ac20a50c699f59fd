"""optik_amd/csrc/roadmap_goals_measure.hpp compiled with g++ as plain C++ (no HIP runtime) for the host and the -m gpu
tests of goal-set planning: the serial reference plan_goals_reference behind a small driver; goal-set queries drawn
from roadmap_util's graphs; the theorem of DESIGN.md section 5.25 as an assertion; and the prescribed cases with their
hand-written expectations, shared by both tests."""
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

import roadmap_util as ru
from collision_util import CSRC

MAX_GOALS = 16
POISON_INDEX = -12345  # what the int32 link indices past gcount hold (the float arrays hold NaN there)

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "roadmap_goals_measure.hpp"

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

static std::vector<int32_t> ints(const double *p, size_t count) {
    std::vector<int32_t> v(count);
    for (size_t i = 0; i < count; ++i) v[i] = (int32_t)p[i];
    return v;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::vector<double> in = read_all(argv[1]);
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    // n, N, k, ks, kg, Lmax, Q, G, nodes [n][N], nbr [k][N], w [k][N], start [Q][n], goals [Q][G][n], gcount [Q],
    // sidx [ks][Q], sw [ks][Q], gidx [G][kg][Q], gw [G][kg][Q], direct [G][Q]
    // -> per query status, len, cost, which, path [Lmax][n], route [Lmax], hop [Lmax], d [N]
    const int n = (int)in[0], N = (int)in[1], k = (int)in[2], ks = (int)in[3], kg = (int)in[4], Lmax = (int)in[5],
              Q = (int)in[6], G = (int)in[7];
    const double *p = &in[8];
    const double *nodes = p; p += (size_t)n * N;
    const std::vector<int32_t> nbr = ints(p, (size_t)k * N); p += (size_t)k * N;
    const double *w = p; p += (size_t)k * N;
    const double *start = p; p += (size_t)Q * n;
    const double *goals = p; p += (size_t)Q * G * n;
    const std::vector<int32_t> gcount = ints(p, (size_t)Q); p += (size_t)Q;
    const std::vector<int32_t> sidx = ints(p, (size_t)ks * Q); p += (size_t)ks * Q;
    const double *sw = p; p += (size_t)ks * Q;
    const std::vector<int32_t> gidx = ints(p, (size_t)G * kg * Q); p += (size_t)G * kg * Q;
    const double *gw = p; p += (size_t)G * kg * Q;
    const double *direct = p;
    std::vector<double> path((size_t)Lmax * n), d(N), rh(2 * (size_t)Lmax);
    std::vector<int32_t> route(Lmax), hop(Lmax);
    for (int j = 0; j < Q; ++j) {
        roadmap::GoalsQuery z;
        z.y.N = N; z.y.k = k; z.y.nbr = nbr.data(); z.y.w = w;
        z.y.ks = ks; z.y.kg = kg;
        z.y.sidx = sidx.data() + j; z.y.sw = sw + j; z.y.gidx = nullptr; z.y.gw = nullptr;
        z.y.qs = Q;
        z.y.direct = 0.0;
        z.y.Lmax = Lmax;
        z.G = G; z.gcount = roadmap::clamp_count(gcount[j], G);
        z.gidx = gidx.data() + j; z.gw = gw + j; z.gq = Q; z.gs = (long long)kg * Q;
        z.direct = direct + j; z.ds = Q;
        const roadmap::GoalsPlan r = roadmap::plan_goals_reference(z, n, nodes, start + (size_t)j * n,
                                                                   goals + (size_t)j * G * n, path.data(), route.data(),
                                                                   hop.data(), d.data());
        const double head[4] = {(double)r.p.status, (double)r.p.len, r.p.cost, (double)r.which};
        for (int t = 0; t < Lmax; ++t) { rh[t] = route[t]; rh[Lmax + t] = hop[t]; }
        std::fwrite(head, sizeof(double), 4, out);
        std::fwrite(path.data(), sizeof(double), path.size(), out);
        std::fwrite(rh.data(), sizeof(double), rh.size(), out);
        std::fwrite(d.data(), sizeof(double), d.size(), out);
    }
    std::fclose(out);
    return 0;
}
"""

bits = ru.bits


def build_goals_ref(workdir=None):
    """Compile the driver; returns an object with .query(graph, queries, Lmax) -> dict(status, len, which [Q] int32,
    cost [Q], path [Lmax, Q, n], route, hop [Lmax, Q] int32, d [Q, N]) with graph = dict(nodes [n, N], nbr [k, N],
    w [k, N]) and queries = dict(start [n, Q], goals [G, n, Q], gcount [Q] int32, sidx, sw [ks, Q], gidx, gw
    [G, kg, Q], direct [G, Q]): the layouts of the device call."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the goal-set header on its own"
    d = workdir or tempfile.mkdtemp(prefix="roadmap_goals_")
    src, exe = os.path.join(d, "goals_driver.cpp"), os.path.join(d, "goals_driver")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe],
                   check=True)

    class Ref:
        @staticmethod
        def query(graph, queries, Lmax):
            nodes, nbr, w = graph["nodes"], graph["nbr"], graph["w"]
            n, N = nodes.shape
            k = nbr.shape[0]
            G, _, Q = queries["goals"].shape
            ks, kg = queries["sidx"].shape[0], queries["gidx"].shape[1]
            fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            parts = [[n, N, k, ks, kg, Lmax, Q, G], nodes, nbr, w, queries["start"].T,
                     queries["goals"].transpose(2, 0, 1), queries["gcount"], queries["sidx"], queries["sw"],
                     queries["gidx"], queries["gw"], queries["direct"]]
            np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(fin)
            subprocess.run([exe, fin, fout], check=True)
            out = np.fromfile(fout, dtype=np.float64).reshape(Q, 4 + Lmax * n + 2 * Lmax + N)
            o = 4 + Lmax * n
            return dict(status=out[:, 0].astype(np.int32), len=out[:, 1].astype(np.int32), cost=out[:, 2].copy(),
                        which=out[:, 3].astype(np.int32),
                        path=out[:, 4:o].reshape(Q, Lmax, n).transpose(1, 0, 2).copy(),
                        route=out[:, o:o + Lmax].T.astype(np.int32).copy(),
                        hop=out[:, o + Lmax:o + 2 * Lmax].T.astype(np.int32).copy(), d=out[:, o + 2 * Lmax:].copy())

    return Ref()


# ---- goal-set queries -----------------------------------------------------------------------------------------------

def stack_goals(singles, gcount=None):
    """A goal-set query from G single-goal queries of roadmap_util (dicts of queries_for / one_query) that share
    their start and start links: the first one's are taken."""
    q0 = singles[0]
    Q = q0["start"].shape[1]
    return dict(start=q0["start"].copy(), sidx=q0["sidx"].copy(), sw=q0["sw"].copy(),
                goals=np.ascontiguousarray(np.stack([s["goal"] for s in singles])),
                gidx=np.ascontiguousarray(np.stack([s["gidx"] for s in singles])).astype(np.int32),
                gw=np.ascontiguousarray(np.stack([s["gw"] for s in singles])),
                direct=np.ascontiguousarray(np.stack([s["direct"] for s in singles])),
                gcount=(np.full(Q, len(singles)) if gcount is None else np.asarray(gcount)).astype(np.int32))


def single(q, g):
    """Goal g of a goal-set query as a single-goal query of roadmap_util."""
    return dict(start=q["start"], goal=np.ascontiguousarray(q["goals"][g]), sidx=q["sidx"], sw=q["sw"],
                gidx=np.ascontiguousarray(q["gidx"][g]), gw=np.ascontiguousarray(q["gw"][g]),
                direct=np.ascontiguousarray(q["direct"][g]))


def poison(q):
    """NaN (POISON_INDEX in the int32 indices) in every array past gcount; returns q."""
    for g in range(q["goals"].shape[0]):
        gone = q["gcount"] <= g
        q["goals"][g][:, gone] = math.nan
        q["gw"][g][:, gone] = math.nan
        q["gidx"][g][:, gone] = POISON_INDEX
        q["direct"][g][gone] = math.nan
    return q


def random_goal_queries(rng, graph, Q, ks, kg, G, p_direct=0.3, p_inf=None):
    """Q goal-set queries: G independent queries_for draws that share start and start links, a random gcount that
    holds 0 (query 0) and G (query 1), everything past gcount poisoned.  p_inf not None: that share of the link
    weights is +inf."""
    singles = [ru.queries_for(rng, graph, Q, ks, kg, p_direct=p_direct) for _ in range(G)]
    if p_inf is not None:
        for s in singles:
            s["sw"][rng.random(s["sw"].shape) < p_inf] = np.inf
            s["gw"][rng.random(s["gw"].shape) < p_inf] = np.inf
    gcount = rng.integers(0, G + 1, Q)
    gcount[0] = 0
    if Q > 1:
        gcount[1] = G
    return poison(stack_goals(singles, gcount))


def take(q, cols):
    """Columns `cols` of a goal-set query (the query axis is the last of every array)."""
    return {k: np.ascontiguousarray(v[..., cols]) for k, v in q.items()}


def assert_theorem(name, res, per_goal, q):
    """DESIGN.md section 5.25 for a query set without NaN in its counted part: res = the goal-set plan, per_goal[g] =
    roadmap_util's single-goal plan to goal g.  Returns (queries with a finite cost, those with a unique cheapest
    goal)."""
    G, _, Q = q["goals"].shape
    finite = unique = 0
    for j in range(Q):
        c = int(min(max(q["gcount"][j], 0), G))
        costs = np.array([per_goal[g]["cost"][j] for g in range(c)])
        tag = (name, j)
        if c == 0 or not np.isfinite(costs).any():
            assert res["status"][j] == ru.NO_ROUTE and res["cost"][j] == np.inf and res["which"][j] == -1, tag
            assert all(per_goal[g]["status"][j] == ru.NO_ROUTE for g in range(c)), tag
            continue
        finite += 1
        best = costs.min()
        assert res["status"][j] != ru.NO_ROUTE, tag
        assert bits(res["cost"][j]) == bits(best), (tag, res["cost"][j], best)
        winners = np.flatnonzero(costs == best)
        if len(winners) != 1:
            continue
        unique += 1
        g = int(winners[0])
        assert res["status"][j] == per_goal[g]["status"][j] and res["len"][j] == per_goal[g]["len"][j], tag
        if res["status"][j] == ru.FOUND:
            assert res["which"][j] == g, tag
            assert np.array_equal(bits(res["path"][:, j]), bits(per_goal[g]["path"][:, j])), tag
        else:
            assert res["status"][j] == ru.TOO_LONG and res["which"][j] == -1, tag
            assert np.array_equal(bits(res["path"][0, j]), bits(q["start"][:, j])), tag
            assert np.array_equal(bits(res["path"][1:, j]),
                                  bits(np.broadcast_to(q["goals"][0, :, j], res["path"][1:, j].shape))), tag
    return finite, unique


# ---- prescribed cases, with hand-written expectations ------------------------------------------------------------------

def goal_query(n, start_links, goal_links, directs=None, gcount=None, ks=None, kg=None):
    """One goal-set query from lists of (node, weight): goal_links[g] are goal g's.  The start is -1 in every joint,
    goal g is 9 + g."""
    G = len(goal_links)
    directs = [math.inf] * G if directs is None else directs
    kg = kg or max(1, max(len(gl) for gl in goal_links))
    singles = [ru.one_query(n, start_links, gl, direct=dr, ks=ks, kg=kg) for gl, dr in zip(goal_links, directs)]
    for g, s in enumerate(singles):
        s["goal"][:] = 9.0 + g
    return stack_goals(singles, None if gcount is None else [gcount])


def prescribed_cases():
    """[(name, graph, query, Lmax, expect)] with expect = dict(status, len, cost, which, route): route the node
    indices walked.  Worked out by hand from the rules of roadmap_goals_measure.hpp."""
    eq = ru.equal_routes_graph()  # 3 -> {2, 1} -> 0, every route 1.0 + 0.5
    cases = []

    def add(name, graph, q, Lmax, status, length, cost, which, route=()):
        cases.append((name, graph, q, Lmax, dict(status=status, len=length, cost=cost, which=which, route=list(route))))

    # two goals linked to node 0 at the same weight: the lowest goal; node 3's successor is the lowest index, 1
    add("same_node_tie", eq, goal_query(2, [(3, 0.25)], [[(0, 0.25)], [(0, 0.25)]]), 64, ru.FOUND, 5, 2.0, 0, (3, 1, 0))
    # the same with goal 1 the nearer by its link: d_0 is goal 1's, goal 0's own weight does not equal it
    add("same_node_nearer", eq, goal_query(2, [(3, 0.25)], [[(0, 0.5)], [(0, 0.25)]]), 64, ru.FOUND, 5, 2.0, 1,
        (3, 1, 0))
    # equal direct weights: the lowest goal; a cheaper one behind them wins
    add("direct_tie", eq, goal_query(2, [(3, 5.0)], [[(0, 0.25)], [(0, 0.25)]], directs=[2.0, 2.0]), 64, ru.FOUND, 2,
        2.0, 0)
    add("direct_tie_third", eq, goal_query(2, [(3, 5.0)], [[(0, 0.25)]] * 3, directs=[3.0, 2.0, 2.0]), 64, ru.FOUND,
        2, 2.0, 1)
    # the direct edge of goal 1 against the graph route to goal 0 at the same cost 0.25 + 1.5 + 0.25: the direct edge
    add("direct_vs_link", eq, goal_query(2, [(3, 0.25)], [[(0, 0.25)], [(0, 4.0)]], directs=[math.inf, 2.0]), 64,
        ru.FOUND, 2, 2.0, 1)
    # ... and strictly cheaper by the graph: the route
    add("link_beats_direct", eq, goal_query(2, [(3, 0.25)], [[(0, 0.25)], [(0, 4.0)]], directs=[math.inf, 2.25]), 64,
        ru.FOUND, 5, 2.0, 0, (3, 1, 0))
    # the two equal routes end in different goals: goal 0 behind node 2, goal 1 behind node 1.  The successor of
    # node 3 is the lowest node index, 1, whatever goal lies behind it
    add("equal_routes_two_goals", eq, goal_query(2, [(3, 0.25)], [[(2, 0.5)], [(1, 0.5)]]), 64, ru.FOUND, 4, 1.75, 1,
        (3, 1))
    # a ring v -> v - 1 of 130 nodes, goal 0 behind node 0 and goal 1 behind node 65: from node 100 goal 1 is the
    # nearer (36 nodes walked), from node 40 only goal 0 lies ahead (41 nodes); node 129's distance needs 64 sweeps
    ring = ru.ring_graph(130)
    add("ring_nearer_goal", ring, goal_query(2, [(100, 0.5)], [[(0, 0.5)], [(65, 0.5)]]), 64, ru.FOUND, 38, 9.75, 1,
        range(100, 64, -1))
    add("ring_only_goal", ring, goal_query(2, [(40, 0.5)], [[(0, 0.5)], [(65, 0.5)]]), 64, ru.FOUND, 43, 11.0, 0,
        range(40, -1, -1))
    add("ring_too_long", ring, goal_query(2, [(129, 0.5)], [[(0, 0.5)], [(65, 0.5)]]), 64, ru.TOO_LONG, 2, 17.0, -1)
    # a NaN link weight of goal 1: inside the count it is status 3, outside it is not read
    nanq = goal_query(2, [(3, 0.25)], [[(0, 0.25)], [(0, math.nan)]])
    add("nan_link_counted", eq, nanq, 64, ru.QUERY_NAN, 2, math.nan, -1)
    nano = goal_query(2, [(3, 0.25)], [[(0, 0.25)], [(0, math.nan)]], gcount=1)
    add("nan_link_uncounted", eq, nano, 64, ru.FOUND, 5, 2.0, 0, (3, 1, 0))
    nand = goal_query(2, [(3, 0.25)], [[(0, 0.25)], [(0, 0.25)]], directs=[math.inf, math.nan])
    add("nan_direct_counted", eq, nand, 64, ru.QUERY_NAN, 2, math.nan, -1)
    nang = goal_query(2, [(3, 0.25)], [[(0, 0.25)], [(0, 0.25)]], gcount=1)
    nang["goals"][1, 1, 0] = math.nan
    add("nan_goal_uncounted", eq, nang, 64, ru.FOUND, 5, 2.0, 0, (3, 1, 0))
    nang2 = goal_query(2, [(3, 0.25)], [[(0, 0.25)], [(0, 0.25)]])
    nang2["goals"][1, 1, 0] = math.nan
    add("nan_goal_counted", eq, nang2, 64, ru.QUERY_NAN, 2, math.nan, -1)
    # the Lmax cap: the route needs 5 waypoints; a worse direct edge does not rescue it, a better one does
    add("lmax4", eq, goal_query(2, [(3, 0.25)], [[(0, 0.25)], [(0, 1.0)]], directs=[math.inf, 5.0]), 4, ru.TOO_LONG, 2,
        2.0, -1)
    add("lmax5", eq, goal_query(2, [(3, 0.25)], [[(0, 0.25)], [(0, 1.0)]], directs=[math.inf, 5.0]), 5, ru.FOUND, 5,
        2.0, 0, (3, 1, 0))
    add("lmax2_direct", eq, goal_query(2, [(3, 0.25)], [[(0, 0.25)], [(0, 1.0)]], directs=[math.inf, 1.5]), 2,
        ru.FOUND, 2, 1.5, 1)
    # no goal at all
    add("no_goals", eq, poison(goal_query(2, [(3, 0.25)], [[(0, 0.25)], [(0, 0.25)]], directs=[1.0, 1.0], gcount=0)),
        64, ru.NO_ROUTE, 2, math.inf, -1)
    return cases


def expected_path(graph, q, Lmax, expect):
    """The path [Lmax, n] that rule 5 prescribes for a prescribed case."""
    n = graph["nodes"].shape[0]
    start = q["start"][:, 0]
    if int(q["gcount"][0]) == 0:
        return np.tile(start, (Lmax, 1))
    tail = q["goals"][expect["which"] if expect["status"] == ru.FOUND else 0, :, 0]
    rows = [start] + [graph["nodes"][:, v] for v in expect["route"]]
    return np.stack(rows + [tail] * (Lmax - len(rows))).reshape(Lmax, n)


def assert_prescribed(name, res, graph, q, Lmax, expect):
    assert res["status"][0] == expect["status"] and res["len"][0] == expect["len"], (name, res["status"], res["len"])
    assert res["which"][0] == expect["which"], (name, res["which"])
    assert bits(res["cost"][0]) == bits(expect["cost"]) or (math.isnan(expect["cost"]) and math.isnan(res["cost"][0])), \
        (name, res["cost"])
    assert np.array_equal(bits(res["path"][:, 0]), bits(expected_path(graph, q, Lmax, expect))), (name, res["path"][:, 0])
    route = list(expect["route"]) + [-1] * (Lmax - 1 - len(expect["route"]))
    assert res["route"][:, 0].tolist() == [-1] + route, (name, res["route"][:, 0])


def random_cases():
    """[(name, graph, queries, Lmax)] for the device test: N = 64, 1100 and 4100 (the three kernel sizes), G in
    {1, 3, 16}, kg in {1, 4, 16}, Q in {1, 257}; gcount 0, partial and full.  Deterministic."""
    rng = np.random.default_rng(525)
    cases = []
    for N, k, G, kg, Q in ((64, 4, 3, 4, 257), (64, 4, 16, 16, 1), (1100, 8, 16, 1, 257), (1100, 8, 1, 16, 1),
                           (4100, 6, 3, 16, 257), (4100, 6, 16, 4, 1)):
        g = ru.random_graph(rng, N, k)
        q = random_goal_queries(rng, g, max(Q, 2), 3, kg, G)
        if Q == 1:
            q = take(q, [1])  # (the full count)
        cases.append((f"random{N}_G{G}_kg{kg}_Q{Q}", g, q, 16))
    return cases
