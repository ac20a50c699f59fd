"""optik_amd/csrc/roadmap_measure.hpp compiled with g++ as plain C++ (no HIP runtime) for the host and the -m gpu tests
of roadmap planning; the same rules in numpy and a heapq Dijkstra on Python floats; the synthetic graphs; and the wall
scene of the end-to-end test, with the host check that chooses it (motion_util's motion check over a numpy FK)."""
import heapq
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

from collision_util import CSRC
from motion_util import np_steps

K_MAX, MAX_NODES = 16, 8192
FOUND, NO_ROUTE, TOO_LONG, QUERY_NAN = 0, 1, 2, 3

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "roadmap_measure.hpp"

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
    if (argc < 4) return 2;
    const std::vector<double> in = read_all(argv[2]);
    FILE *out = std::fopen(argv[3], "wb");
    if (!out) return 2;
    if (argv[1][0] == 'w') {
        // weights: n, then records (a [n], b [n]) -> the weight
        const int n = (int)in[0];
        for (size_t o = 1; o + 2 * n <= in.size(); o += 2 * n) {
            const double w = roadmap::edge_weight(n, &in[o], 1, &in[o + n], 1);
            std::fwrite(&w, sizeof(double), 1, out);
        }
    } else if (argv[1][0] == 'r') {
        // the order: records (da, ia, db, ib) -> 0 / 1
        for (size_t o = 0; o + 4 <= in.size(); o += 4) {
            const double v = roadmap::ranks_before(in[o], (int)in[o + 1], in[o + 2], (int)in[o + 3]) ? 1.0 : 0.0;
            std::fwrite(&v, sizeof(double), 1, out);
        }
    } else if (argv[1][0] == 'k') {
        // neighbours: n, N, Q, k, exclude_self, nodes [n][N], queries [n][Q] -> per query idx [k], dist [k]
        const int n = (int)in[0], N = (int)in[1], Q = (int)in[2], k = (int)in[3], self = (int)in[4];
        const double *nodes = &in[5], *q = nodes + (size_t)n * N;
        for (int j = 0; j < Q; ++j) {
            int32_t idx[roadmap::K_MAX];
            double dist[roadmap::K_MAX], idxd[roadmap::K_MAX];
            roadmap::knn_reference(n, q + j, Q, nodes, N, k, self ? j : -1, idx, dist);
            for (int s = 0; s < k; ++s) idxd[s] = (double)idx[s];
            std::fwrite(idxd, sizeof(double), k, out);
            std::fwrite(dist, sizeof(double), k, out);
        }
    } else {
        // queries: n, N, k, ks, kg, Lmax, Q, nodes [n][N], nbr [k][N], w [k][N], start [Q][n], goal [Q][n],
        // sidx [ks][Q], sw [ks][Q], gidx [kg][Q], gw [kg][Q], direct [Q]
        // -> per query status, len, cost, path [Lmax][n], d [N]
        const int n = (int)in[0], N = (int)in[1], k = (int)in[2], ks = (int)in[3], kg = (int)in[4], Lmax = (int)in[5],
                  Q = (int)in[6];
        const double *p = &in[7];
        const double *nodes = p; p += (size_t)n * N;
        const std::vector<int32_t> nbr = ints(p, (size_t)k * N); p += (size_t)k * N;
        const double *w = p; p += (size_t)k * N;
        const double *start = p; p += (size_t)Q * n;
        const double *goal = p; p += (size_t)Q * n;
        const std::vector<int32_t> sidx = ints(p, (size_t)ks * Q); p += (size_t)ks * Q;
        const double *sw = p; p += (size_t)ks * Q;
        const std::vector<int32_t> gidx = ints(p, (size_t)kg * Q); p += (size_t)kg * Q;
        const double *gw = p; p += (size_t)kg * Q;
        const double *direct = p;
        std::vector<double> path((size_t)Lmax * n), d(N);
        for (int j = 0; j < Q; ++j) {
            roadmap::Query y;
            y.N = N; y.k = k; y.nbr = nbr.data(); y.w = w;
            y.ks = ks; y.kg = kg;
            y.sidx = sidx.data() + j; y.sw = sw + j; y.gidx = gidx.data() + j; y.gw = gw + j;
            y.qs = Q;
            y.direct = direct[j];
            y.Lmax = Lmax;
            const roadmap::Plan r = roadmap::plan_reference(y, n, nodes, start + (size_t)j * n, goal + (size_t)j * n,
                                                            path.data(), d.data());
            const double head[3] = {(double)r.status, (double)r.len, r.cost};
            std::fwrite(head, sizeof(double), 3, out);
            std::fwrite(path.data(), sizeof(double), path.size(), out);
            std::fwrite(d.data(), sizeof(double), d.size(), out);
        }
    }
    std::fclose(out);
    return 0;
}
"""


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def build_roadmap_ref(workdir=None):
    """Compile the driver; returns an object with
    .weight(a [B, n], b [B, n]) -> [B],
    .ranks_before(rows [B, 4]) -> bool [B],
    .knn(q [n, Q], nodes [n, N], k, exclude_self) -> (idx [k, Q] int32, dist [k, Q]),
    .query(graph, queries, Lmax) -> dict(status [Q], len [Q], cost [Q], path [Lmax, Q, n], d [Q, N]) with
      graph = dict(nodes [n, N], nbr [k, N], w [k, N]) and queries = dict(start [n, Q], goal [n, Q], sidx, sw
      [ks, Q], gidx, gw [kg, Q], direct [Q]): the layouts of the device call."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the roadmap header on its own"
    d = workdir or tempfile.mkdtemp(prefix="roadmap_")
    src, exe = os.path.join(d, "roadmap_driver.cpp"), os.path.join(d, "roadmap_driver")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe],
                   check=True)

    def run(mode, parts):
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(fin)
        subprocess.run([exe, mode, fin, fout], check=True)
        return np.fromfile(fout, dtype=np.float64)

    class Ref:
        @staticmethod
        def weight(a, b):
            a, b = np.atleast_2d(a), np.atleast_2d(b)
            return run("w", [[a.shape[1]], np.concatenate([a, b], axis=1)])

        @staticmethod
        def ranks_before(rows):
            return run("r", [rows]) != 0.0

        @staticmethod
        def knn(q, nodes, k, exclude_self=False):
            n, Q = q.shape
            N = nodes.shape[1]
            out = run("k", [[n, N, Q, k, 1 if exclude_self else 0], nodes, q]).reshape(Q, 2, k)
            return out[:, 0].T.astype(np.int32).copy(), out[:, 1].T.copy()

        @staticmethod
        def query(graph, queries, Lmax):
            nodes, nbr, w = graph["nodes"], graph["nbr"], graph["w"]
            n, N = nodes.shape
            k = nbr.shape[0]
            Q = queries["start"].shape[1]
            ks, kg = queries["sidx"].shape[0], queries["gidx"].shape[0]
            out = run("q", [[n, N, k, ks, kg, Lmax, Q], nodes, nbr, w, queries["start"].T, queries["goal"].T,
                            queries["sidx"], queries["sw"], queries["gidx"], queries["gw"], queries["direct"]])
            out = out.reshape(Q, 3 + Lmax * n + N)
            return dict(status=out[:, 0].astype(np.int32), len=out[:, 1].astype(np.int32), cost=out[:, 2].copy(),
                        path=out[:, 3:3 + Lmax * n].reshape(Q, Lmax, n).transpose(1, 0, 2).copy(),
                        d=out[:, 3 + Lmax * n:].copy())

    return Ref()


# ---- the same rules in numpy and in plain Python -----------------------------------------------------------------

def np_weights(a, b):
    """max_i |b_i - a_i| over axis 0 (np.max propagates a NaN, as the header's rule does)."""
    return np.max(np.abs(np.asarray(b, dtype=np.float64) - np.asarray(a, dtype=np.float64)), axis=0)


def np_knn(q, nodes, k, exclude_self=False):
    """(idx [k, Q] int32, dist [k, Q]): abs, max and a stable lexicographic sort on (is NaN, distance, index)."""
    n, Q = q.shape
    N = nodes.shape[1]
    idx = np.full((k, Q), -1, dtype=np.int32)
    dist = np.full((k, Q), np.inf)
    for j in range(Q):
        d = np.max(np.abs(nodes - q[:, j:j + 1]), axis=0)
        cand = np.arange(N)
        if exclude_self:
            cand = cand[cand != j]
        dc = d[cand]
        nan = np.isnan(dc)
        order = np.lexsort((cand, np.where(nan, 0.0, dc), nan))[:k]
        idx[:len(order), j] = cand[order]
        dist[:len(order), j] = dc[order]
    return idx, dist


def dijkstra(N, nbr, w, gidx, gw):
    """The distance of every node to the goal with a heap, on Python floats: d[u] starts as the least goal-link
    weight of u; an edge v -> u costs w + d[u], the route summed from the goal backwards."""
    d = [math.inf] * N
    for u, g in zip(gidx, gw):
        if 0 <= u < N and g < d[u]:
            d[u] = float(g)
    into = [[] for _ in range(N)]  # u -> [(v, w(v, u))]
    for s in range(nbr.shape[0]):
        for v in range(N):
            u = int(nbr[s, v])
            if 0 <= u < N and not math.isnan(w[s, v]):
                into[u].append((v, float(w[s, v])))
    heap = [(d[u], u) for u in range(N) if d[u] < math.inf]
    heapq.heapify(heap)
    done = [False] * N
    while heap:
        du, u = heapq.heappop(heap)
        if done[u] or du > d[u]:
            continue
        done[u] = True
        for v, wv in into[u]:
            c = wv + du
            if c < d[v]:
                d[v] = c
                heapq.heappush(heap, (c, v))
    return np.array(d)


# ---- synthetic graphs and queries (no collision model: the weights are given) -------------------------------------

def _pad_slots(lists, k, N, fill_idx=-1):
    nbr = np.full((k, N), fill_idx, dtype=np.int32)
    w = np.full((k, N), np.inf)
    for v, edges in enumerate(lists):
        for s, (u, wt) in enumerate(edges):
            nbr[s, v], w[s, v] = u, wt
    return nbr, w


def random_graph(rng, N, k, n=3, p_blocked=0.2):
    """N nodes in n joints, k random out-edges each (duplicates and self-loops allowed), a share of them blocked."""
    nodes = rng.uniform(-2.0, 2.0, (n, N))
    lists = []
    for v in range(N):
        edges = []
        for _ in range(k):
            u = int(rng.integers(0, N))
            wt = float(np_weights(nodes[:, v], nodes[:, u])) if rng.random() > p_blocked else math.inf
            edges.append((u, wt))
        lists.append(edges)
    nbr, w = _pad_slots(lists, k, N)
    return dict(nodes=nodes, nbr=nbr, w=w)


def ring_graph(N, n=2, weight=0.25):
    """v -> v - 1 only: from node N - 1 to node 0 the distances need N - 1 sweeps."""
    nodes = np.zeros((n, N))
    nodes[0] = weight * np.arange(N)
    nbr, w = _pad_slots([[((v - 1) % N, weight)] for v in range(N)], 1, N)
    w[0, 0] = math.inf  # (no edge 0 -> N - 1: node 0 is the end of the line)
    return dict(nodes=nodes, nbr=nbr, w=w)


def queries_for(rng, graph, Q, ks, kg, p_direct=0.3):
    """Q random queries against a synthetic graph: random start and goal links with random weights."""
    n, N = graph["nodes"].shape
    q = dict(start=rng.uniform(-2.0, 2.0, (n, Q)), goal=rng.uniform(-2.0, 2.0, (n, Q)),
             sidx=rng.integers(0, N, (ks, Q)).astype(np.int32), sw=rng.uniform(0.1, 1.0, (ks, Q)),
             gidx=rng.integers(0, N, (kg, Q)).astype(np.int32), gw=rng.uniform(0.1, 1.0, (kg, Q)),
             direct=np.where(rng.random(Q) < p_direct, rng.uniform(0.5, 6.0, Q), np.inf))
    q["sw"][rng.random((ks, Q)) < 0.2] = np.inf
    q["gw"][rng.random((kg, Q)) < 0.2] = np.inf
    return q


def one_query(n, start_links, goal_links, direct=math.inf, ks=None, kg=None):
    """A single query from lists of (node, weight)."""
    ks, kg = ks or max(1, len(start_links)), kg or max(1, len(goal_links))
    sidx, sw = _pad_slots([start_links], ks, 1)
    gidx, gw = _pad_slots([goal_links], kg, 1)
    return dict(start=np.full((n, 1), -1.0), goal=np.full((n, 1), 9.0), sidx=sidx, sw=sw, gidx=gidx, gw=gw,
                direct=np.array([direct]))


def take_queries(q, cols):
    return {k: np.ascontiguousarray(v[..., cols]) for k, v in q.items()}


def path_cost_backwards(weights):
    """The weights of a route's segments, start first, added from the goal backwards."""
    c = 0.0
    for wt in reversed(list(weights)):
        c = wt + c
    return c


# ---- the wall scene of the end-to-end test ------------------------------------------------------------------------
# A Panda with the 6-sphere model of spheres_along_chain(robot, 0.05, 2) and no self pairs; a wall of 2 cm in the plane
# y = 0 in front of it; start and goal differ in the first joint only, so the straight move sweeps the arm through the
# wall.  (Chosen on the CPU: tests/test_roadmap_host.py asserts that the move is blocked and that the serial reference
# finds a route over WALL_N nodes.)
WALL_START = [-0.9, 0.4, 0.0, -1.8, 0.0, 2.2, 0.7]
WALL_GOAL = [0.9, 0.4, 0.0, -1.8, 0.0, 2.2, 0.7]
WALL_BOX = [0.55, 0.0, 0.45, 0.0, 0.0, 0.0, 1.0, 0.2, 0.01, 0.25]
WALL_N, WALL_K, WALL_H, WALL_FIRST = 128, 8, 0.1, 1


def wall_scene():
    from conftest import ROBOT_SPECS
    from optik_amd import Robot
    from optik_amd.collision import spheres_along_chain
    robot = Robot.from_urdf_file(*ROBOT_SPECS["panda"])
    frames, centers, radii = spheres_along_chain(robot, 0.05, 2)
    return dict(robot=robot, frames=frames, centers=centers, radii=radii, boxes=np.array([WALL_BOX]),
                start=np.array(WALL_START), goal=np.array(WALL_GOAL), N=WALL_N, k=WALL_K, h=WALL_H, first=WALL_FIRST)


def _qmul(a, b):
    ai, aj, ak, aw = (a[..., i] for i in range(4))
    bi, bj, bk, bw = (b[..., i] for i in range(4))
    return np.stack([aw * bi + ai * bw + aj * bk - ak * bj, aw * bj - ai * bk + aj * bw + ak * bi,
                     aw * bk + ai * bj - aj * bi + ak * bw, aw * bw - ai * bi - aj * bj - ak * bk], axis=-1)


def _qrot(q, v):
    u = 2.0 * np.cross(q[..., :3], v)
    return v + q[..., 3:4] * u + np.cross(q[..., :3], u)


def _compose(a, b):
    return np.concatenate([a[..., :3] + _qrot(a[..., 3:], b[..., :3]), _qmul(a[..., 3:], b[..., 3:])], axis=-1)


def np_frames7_batch(tables, q):
    """motion_util.np_frames7 for many configurations at once: q [B, n] -> [B, n + 2, 7]."""
    origins, axes = np.asarray(tables["origins"]).reshape(-1, 7), np.asarray(tables["axes"]).reshape(-1, 3)
    B, n = q.shape
    cur = np.tile(np.array([0.0, 0, 0, 0, 0, 0, 1]), (B, 1))
    out = [cur]
    for j in range(n):
        s, c = np.sin(q[:, j] / 2), np.cos(q[:, j] / 2)
        rot = np.concatenate([np.zeros((B, 3)), axes[j][None] * s[:, None], c[:, None]], axis=1)
        cur = _compose(_compose(cur, np.broadcast_to(origins[j], (B, 7))), rot)
        out.append(cur)
    if len(origins) > n:
        cur = _compose(cur, np.broadcast_to(origins[n], (B, 7)))
    out.append(cur)
    return np.stack(out, axis=1)


def host_checked_weights(scene, motion, qa, qb):
    """What optik_hip_roadmap_edges defines, on the CPU: the weight of qa[b] -> qb[b] ([B, n] each) where the motion
    check of motion_measure.hpp (motion_util's g++ build, over the numpy FK) finds it free, +inf elsewhere."""
    tables = scene["robot"].chain_tables()
    qa, qb = np.atleast_2d(qa), np.atleast_2d(qb)
    wts = np_weights(qa.T, qb.T)
    Ks, frames = [], []
    for a, b, d in zip(qa, qb, wts):
        K = np_steps(d, scene["h"])
        Ks.append(K)
        if K < 1:
            frames.append(None)
            continue
        t = np.arange(K + 1, dtype=np.float64) / np.float64(K)
        s = a[None, :] + t[:, None] * (b - a)[None, :]
        s[0], s[K] = a, b
        frames.append(np_frames7_batch(tables, s))
    _, free, _, _ = motion.reduce(Ks, frames, 0.0, scene["frames"], scene["centers"], scene["radii"],
                                  boxes=scene["boxes"])
    return np.where(free, wts, np.inf)


# ---- the synthetic cases that the host test and the -m gpu test share ----------------------------------------------

def equal_routes_graph():
    """Two routes 3 -> {1, 2} -> 0 of the same cost; node 3 lists node 2 in the slot before node 1."""
    nodes = np.array([[0.0, 1.0, 1.0, 2.0], [0.0, 0.5, -0.5, 0.0]])
    nbr, w = _pad_slots([[], [(0, 0.5)], [(0, 0.5)], [(2, 1.0), (1, 1.0)]], 2, 4)
    return dict(nodes=nodes, nbr=nbr, w=w)


def two_components_graph(rng):
    """Nodes 0 .. 19 and 20 .. 39 with edges inside each half only."""
    halves = [random_graph(rng, 20, 3, n=3, p_blocked=0.0) for _ in range(2)]
    nbr = np.concatenate([halves[0]["nbr"], halves[1]["nbr"] + 20], axis=1)
    return dict(nodes=np.concatenate([h["nodes"] for h in halves], axis=1), nbr=np.ascontiguousarray(nbr),
                w=np.concatenate([h["w"] for h in halves], axis=1))


def synthetic_cases():
    """[(name, graph, queries, Lmax)]: what the host reference is checked on against Dijkstra and the device against
    both.  Deterministic."""
    rng = np.random.default_rng(18)
    cases = []
    for N, k in ((1, 1), (65, 3), (300, 4)):
        g = random_graph(rng, N, k)
        cases.append((f"random{N}", g, queries_for(rng, g, 5, 3, 2), 64))
    ring = ring_graph(130)
    far = one_query(2, [(129, 0.5)], [(0, 0.5)])
    cases.append(("ring130", ring, far, 64))                       # 130 nodes to walk: status 2, the true cost
    cases.append(("ring130_near", ring, one_query(2, [(40, 0.5)], [(0, 0.5)]), 64))  # 41 nodes: found
    two = two_components_graph(rng)
    q = queries_for(rng, two, 4, 2, 2, p_direct=0.0)
    q["sidx"][:, :2] = rng.integers(0, 20, (2, 2)); q["gidx"][:, :2] = rng.integers(20, 40, (2, 2))  # across: no route
    q["sidx"][:, 2:] = rng.integers(20, 40, (2, 2)); q["gidx"][:, 2:] = rng.integers(20, 40, (2, 2))
    cases.append(("two_components", two, q, 64))
    eq = equal_routes_graph()
    cases.append(("equal_routes", eq, one_query(2, [(3, 0.25)], [(0, 0.25)]), 64))
    cases.append(("direct_tie", eq, one_query(2, [(3, 0.25)], [(0, 0.25)], direct=2.0), 64))   # 0.25 + 1.5 + 0.25
    cases.append(("slot_tie", eq, one_query(2, [(2, 1.25), (1, 1.25)], [(0, 0.25)]), 64))
    cases.append(("lmax2_route", eq, one_query(2, [(1, 0.25)], [(0, 0.25)], direct=5.0), 2))     # route better: status 2
    cases.append(("lmax2_direct", eq, one_query(2, [(1, 2.25)], [(0, 3.25)], direct=5.0), 2))    # direct better: found
    nanq = one_query(2, [(3, 0.25)], [(0, 0.25)])
    nanq["start"][1, 0] = math.nan
    cases.append(("nan_start", eq, nanq, 64))
    nanw = one_query(2, [(3, math.nan)], [(0, 0.25)], direct=1.0)
    cases.append(("nan_link", eq, nanw, 64))
    return cases


def dijkstra_cost(graph, queries, j):
    """(d, cost) of query j from the heapq Dijkstra: the first-hop rule over Python floats."""
    N = graph["nodes"].shape[1]
    d = dijkstra(N, graph["nbr"], graph["w"], queries["gidx"][:, j], queries["gw"][:, j])
    best = float(queries["direct"][j])
    for u, wt in zip(queries["sidx"][:, j], queries["sw"][:, j]):
        if 0 <= u < N:
            c = float(wt) + float(d[u])
            if c < best:
                best = c
    return d, best
