// ik_roadmap_goals_lazy.hip -- goal-set planning on lazy roadmaps (roadmap_goals_lazy_measure.hpp: the rules, the
// theorem and the freezing rule): the loop of ik_roadmap_lazy.hip with the goal-set pass of
// ik_roadmap_goals.hip, and every pass after the first run on the queries that can still change only.
// optik_hip_roadmap_lazy_plan_goals / _from_flags (include/optik_hip.h).
//
//   (optik_hip_roadmap_query_goals, ik_roadmap_goals.hip: a pass; it writes each route's nodes and hop slots)
//   goals_lazy_scan_kernel     one thread per query of the pass: lazy_scan_kernel's walk over the query's hop slots --
//                              an UNKNOWN slot is taken once with a vector atomicCAS on its verdict and appended to
//                              the round's list through an atomicAdd counter --, and a query that is still live (the
//                              freezing rule) appends its index to the next pass's live list through a second
//                              counter.  Which query takes a shared slot and the order of both lists vary from run
//                              to run; the sets, the verdicts and every output do not.  Final form: nothing is claimed
//                              or listed, and a query whose route holds an UNKNOWN slot becomes UNSETTLED (status 4,
//                              len 2, which -1, goal 0 behind the start).  No thread waits for another.
//   goals_lazy_gather_kernel   one thread per (live query, element): the query's start, G goals, count, start links,
//                              goal links and direct weights from the caller's [..][Q] arrays into compact [..][Q']
//                              ones in the chain's lazy workspace -- adjacent threads write adjacent words
//   goals_lazy_scatter_kernel  one thread per (live query, element): the compact path [Lmax][Q'][n] and len, cost,
//                              status, which [Q'] back to the caller's [Lmax][Q][n] and [Q]; NULL outputs are skipped
//   (lazydev::check_claimed, ik_roadmap_lazy.hip: the claimed segments gathered, the motion check, the marks)
//
// The loop runs on the host and reads two int32 in one copy per round, the size of the round's list and the live
// count: one stream synchronise a round, none in the last pass once `rounds` checks are made.
#include <algorithm>

#include "roadmap_goals_lazy_measure.hpp"
#include "roadmap_lazy_device.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::colldev;
using namespace optik::lazydev;

namespace {

struct GoalsScanLaunch {
    long long Q, Qp, cap;  // Q: the caller's queries; Qp: those of this pass; cap: the room of `list`
    int N, k, n, Lmax, final_pass;
    const int32_t *route, *hop;  // [Lmax][Qp] (optik_hip_roadmap_query_goals)
    const int32_t *pass_status;  // [Qp]
    const int32_t *live_in;      // [Qp] the caller's index of the pass's query c; null: c itself (Qp == Q)
    int32_t *verdict;            // [k][N]
    int32_t *list;               // [cap] the slots s * N + v claimed in this round
    int32_t *counts;             // [2]: the slots claimed, the live queries
    int32_t *live_out;           // [Qp] the live queries after this pass
    const double *goals;         // [G][n][Q]
    double *path;                // [Lmax][Q][n] or null
    int32_t *len, *status, *which;  // [Q] or null
};

__global__ __launch_bounds__(LAZY_BLOCK) void goals_lazy_scan_kernel(const GoalsScanLaunch a) {
    const long long c = (long long)blockIdx.x * LAZY_BLOCK + threadIdx.x;
    if (c >= a.Qp) return;
    const long long qi = a.live_in ? a.live_in[c] : c;
    if (qi < 0 || qi >= a.Q) return;
    bool unknown = false;
    for (int t = 1; t < a.Lmax - 1; ++t) {
        const int v = a.route[(long long)t * a.Qp + c], s = a.hop[(long long)t * a.Qp + c];
        if (v < 0) break;  // (behind the route; only a FOUND query has one)
        if (s < 0 || s >= a.k || v >= a.N) continue;  // (the route's last node leaves by its goal link)
        const long long e = (long long)s * a.N + v;
        if (a.final_pass) {
            unknown = unknown || a.verdict[e] == roadmap::UNKNOWN;
            continue;
        }
        const int old = atomicCAS(&a.verdict[e], roadmap::UNKNOWN, roadmap::CLAIMED);
        if (old == roadmap::UNKNOWN) {
            const long long pos = atomicAdd(&a.counts[0], 1);
            if (pos < a.cap) a.list[pos] = (int32_t)e;  // (a slot is claimed once: pos < k * N always)
        }
        unknown = unknown || old == roadmap::UNKNOWN || old == roadmap::CLAIMED;
    }
    if (!a.final_pass) {
        if (!roadmap::frozen_after_pass(a.pass_status[c], unknown)) {
            const long long pos = atomicAdd(&a.counts[1], 1);
            if (pos < a.Qp) a.live_out[pos] = (int32_t)qi;  // (a query lists itself once: pos < Qp always)
        }
        return;
    }
    if (!unknown) return;
    if (a.status) a.status[qi] = roadmap::UNSETTLED;
    if (a.len) a.len[qi] = 2;
    if (a.which) a.which[qi] = -1;
    if (a.path)
        for (int t = 1; t < a.Lmax; ++t)
            for (int i = 0; i < a.n; ++i)
                a.path[((long long)t * a.Q + qi) * a.n + i] = a.goals[(long long)i * a.Q + qi];
}

struct CompactLaunch {
    long long Q, Qp;
    int n, G, ks, kg, Lmax;
    const int32_t *live;         // [Qp]
    // the caller's query arrays, [..][Q] ...
    const double *start, *goals, *sw, *gw, *direct;
    const int32_t *gcount, *sidx, *gidx;
    // ... and their compact twins, [..][Qp]
    double *c_start, *c_goals, *c_sw, *c_gw, *c_direct;
    int32_t *c_gcount, *c_sidx, *c_gidx;
    // the compact outputs [Lmax][Qp][n], [Qp] and the caller's [Lmax][Q][n], [Q] (any may be null)
    const double *c_path, *c_cost;
    const int32_t *c_len, *c_status, *c_which;
    double *path, *cost;
    int32_t *len, *status, *which;
};

// rows of Qp words each: start n | goals G n | sw ks | gw G kg | direct G | gcount 1 | sidx ks | gidx G kg
__global__ __launch_bounds__(LAZY_BLOCK) void goals_lazy_gather_kernel(const CompactLaunch a) {
    const long long f = (long long)blockIdx.x * LAZY_BLOCK + threadIdx.x;
    const long long links = (long long)a.G * a.kg;
    const long long rows = a.n + (long long)a.G * a.n + a.ks + links + a.G + 1 + a.ks + links;
    if (f >= rows * a.Qp) return;
    long long row = f / a.Qp;
    const long long c = f % a.Qp, qi = a.live[c];
    if (qi < 0 || qi >= a.Q) return;
    if (row < a.n) { a.c_start[row * a.Qp + c] = a.start[row * a.Q + qi]; return; }
    row -= a.n;
    if (row < (long long)a.G * a.n) { a.c_goals[row * a.Qp + c] = a.goals[row * a.Q + qi]; return; }
    row -= (long long)a.G * a.n;
    if (row < a.ks) { a.c_sw[row * a.Qp + c] = a.sw[row * a.Q + qi]; return; }
    row -= a.ks;
    if (row < links) { a.c_gw[row * a.Qp + c] = a.gw[row * a.Q + qi]; return; }
    row -= links;
    if (row < a.G) { a.c_direct[row * a.Qp + c] = a.direct[row * a.Q + qi]; return; }
    row -= a.G;
    if (row < 1) { a.c_gcount[c] = a.gcount[qi]; return; }
    row -= 1;
    if (row < a.ks) { a.c_sidx[row * a.Qp + c] = a.sidx[row * a.Q + qi]; return; }
    row -= a.ks;
    a.c_gidx[row * a.Qp + c] = a.gidx[row * a.Q + qi];
}

// the path's Lmax * Qp * n words, then four rows of Qp words: len, cost, status, which
__global__ __launch_bounds__(LAZY_BLOCK) void goals_lazy_scatter_kernel(const CompactLaunch a) {
    long long f = (long long)blockIdx.x * LAZY_BLOCK + threadIdx.x;
    const long long row_words = a.Qp * a.n, path_words = (long long)a.Lmax * row_words;
    if (f < path_words) {
        if (!a.path) return;
        const long long t = f / row_words, rem = f % row_words, c = rem / a.n, i = rem % a.n, qi = a.live[c];
        if (qi < 0 || qi >= a.Q) return;
        a.path[(t * a.Q + qi) * a.n + i] = a.c_path[f];
        return;
    }
    f -= path_words;
    if (f >= 4 * a.Qp) return;
    const long long row = f / a.Qp, c = f % a.Qp, qi = a.live[c];
    if (qi < 0 || qi >= a.Q) return;
    if (row == 0) { if (a.len) a.len[qi] = a.c_len[c]; return; }
    if (row == 1) { if (a.cost) a.cost[qi] = a.c_cost[c]; return; }
    if (row == 2) { if (a.status) a.status[qi] = a.c_status[c]; return; }
    if (a.which) a.which[qi] = a.c_which[c];
}

struct GoalsQueryArgs {
    const double *start, *goals;
    const int32_t *gcount;
    int32_t G;
    int64_t Q;
    const int32_t *sidx, *gidx;
    const double *sw, *gw, *direct;
    int32_t ks, kg, Lmax;
    double *path, *cost;
    int32_t *len, *status, *which;
};

// The loop of roadmap_goals_lazy_measure.hpp.  d_edge_free [k][N]: stands for the motion check (the test hook); null:
// the motion check at `resolution`.  skip: every pass after the first runs the live queries only.
int goals_lazy_loop(optik_hip_chain *ch, const double *ee_offset7, const GraphArgs &g, double resolution,
                    const uint8_t *d_edge_free, const GoalsQueryArgs &q, int32_t rounds, bool skip, int32_t *rounds_used,
                    int64_t *checked, hipStream_t stream) {
    if (rounds_used) *rounds_used = 0;
    if (checked) *checked = 0;
    if (q.Q == 0) return 0;
    if (!g.nodes || !g.nbr || !g.verdict || !g.w) return fail(OPTIK_HIP_EINVAL, "bad argument");
    const size_t n = (size_t)ch->n, Q = (size_t)q.Q, cells = (size_t)g.k * (size_t)g.N, L = (size_t)q.Lmax,
                 G = (size_t)q.G, ks = (size_t)q.ks, links = G * (size_t)q.kg;
    const size_t hops = q.Lmax > 3 ? Q * (L - 3) : 0;  // (a route of Lmax waypoints has Lmax - 3 graph hops)
    const size_t cap = std::max<size_t>(1, std::min(cells, hops));
    // the workspace: counters | route | hop | list | two live lists | the pass's status | free flags; with skip the
    // compact inputs and outputs, each with room for Q queries (the live count is not known before the first pass);
    // last the claimed segments
    size_t o = 16;
    auto take = [&o](size_t bytes) { const size_t at = o; o += align16(bytes); return at; };
    const size_t o_route = take(4 * L * Q), o_hop = take(4 * L * Q), o_list = take(4 * cap), o_live0 = take(4 * Q),
                 o_live1 = take(4 * Q), o_status = take(4 * Q), o_free = take(cap);
    const size_t o_len = take(skip ? 4 * Q : 0), o_which = take(skip ? 4 * Q : 0), o_cost = take(skip ? 8 * Q : 0),
                 o_gcount = take(skip ? 4 * Q : 0), o_sidx = take(skip ? 4 * ks * Q : 0),
                 o_gidx = take(skip ? 4 * links * Q : 0), o_start = take(skip ? 8 * n * Q : 0),
                 o_goals = take(skip ? 8 * G * n * Q : 0), o_sw = take(skip ? 8 * ks * Q : 0),
                 o_gw = take(skip ? 8 * links * Q : 0), o_direct = take(skip ? 8 * G * Q : 0),
                 o_path = take(skip && q.path ? 8 * L * Q * n : 0);
    const size_t o_qa = o, bytes = o_qa + (d_edge_free ? 0 : 2 * sizeof(double) * n * cap);
    unsigned char *ws = nullptr;
    if (int rc = reserve_ws(ch, bytes, &ws)) return rc;
    auto ints = [ws](size_t at) { return reinterpret_cast<int32_t *>(ws + at); };
    auto reals = [ws](size_t at) { return reinterpret_cast<double *>(ws + at); };
    int32_t *d_counts = ints(0), *d_route = ints(o_route), *d_hop = ints(o_hop), *d_live[2] = {ints(o_live0), ints(o_live1)};
    // (the first pass writes the caller's status; without one it has the workspace's, which the scan reads)
    int32_t *first_status = q.status ? q.status : ints(o_status);
    GoalsScanLaunch s;
    std::memset(&s, 0, sizeof s);
    s.Q = q.Q; s.Qp = q.Q; s.cap = (long long)cap;
    s.N = g.N; s.k = g.k; s.n = ch->n; s.Lmax = q.Lmax;
    s.route = d_route; s.hop = d_hop;
    s.pass_status = first_status;
    s.verdict = g.verdict;
    s.list = ints(o_list);
    s.counts = d_counts;
    s.goals = q.goals; s.path = q.path; s.len = q.len; s.status = q.status; s.which = q.which;
    CompactLaunch m;
    std::memset(&m, 0, sizeof m);
    m.Q = q.Q;
    m.n = ch->n; m.G = q.G; m.ks = q.ks; m.kg = q.kg; m.Lmax = q.Lmax;
    m.start = q.start; m.goals = q.goals; m.sw = q.sw; m.gw = q.gw; m.direct = q.direct;
    m.gcount = q.gcount; m.sidx = q.sidx; m.gidx = q.gidx;
    m.c_start = reals(o_start); m.c_goals = reals(o_goals); m.c_sw = reals(o_sw); m.c_gw = reals(o_gw);
    m.c_direct = reals(o_direct);
    m.c_gcount = ints(o_gcount); m.c_sidx = ints(o_sidx); m.c_gidx = ints(o_gidx);
    m.c_path = q.path ? reals(o_path) : nullptr; m.c_cost = reals(o_cost);
    m.c_len = ints(o_len); m.c_status = ints(o_status); m.c_which = ints(o_which);
    m.path = q.path; m.cost = q.cost; m.len = q.len; m.status = q.status; m.which = q.which;
    int32_t used = 0;
    int64_t total = 0, Qp = q.Q;
    int out = 0;         // the live list this pass's scan writes; the other one is what the pass reads
    bool compact = false;
    for (;;) {
        if (compact) {
            const long long rows = (long long)(n + G * n + ks + links + G + 1 + ks + links);
            m.Qp = Qp; m.live = d_live[out ^ 1];
            {
                BIND_DEVICE(ch);
                hipLaunchKernelGGL(goals_lazy_gather_kernel, dim3(blocks(rows * Qp)), dim3(LAZY_BLOCK), 0, stream, m);
                HIP_TRY(hipGetLastError());
            }
            if (int rc = optik_hip_roadmap_query_goals(ch, g.nodes, g.N, g.nbr, g.w, g.k, m.c_start, m.c_goals,
                                                       m.c_gcount, q.G, Qp, m.c_sidx, m.c_sw, q.ks, m.c_gidx, m.c_gw,
                                                       q.kg, m.c_direct, q.Lmax, const_cast<double *>(m.c_path),
                                                       const_cast<int32_t *>(m.c_len), const_cast<double *>(m.c_cost),
                                                       const_cast<int32_t *>(m.c_status),
                                                       const_cast<int32_t *>(m.c_which), d_route, d_hop, stream))
                return rc;
            BIND_DEVICE(ch);
            hipLaunchKernelGGL(goals_lazy_scatter_kernel, dim3(blocks((long long)L * Qp * (long long)n + 4 * Qp)),
                               dim3(LAZY_BLOCK), 0, stream, m);
            HIP_TRY(hipGetLastError());
            s.pass_status = m.c_status;
            s.live_in = m.live;
        } else if (int rc = optik_hip_roadmap_query_goals(ch, g.nodes, g.N, g.nbr, g.w, g.k, q.start, q.goals, q.gcount,
                                                          q.G, q.Q, q.sidx, q.sw, q.ks, q.gidx, q.gw, q.kg, q.direct,
                                                          q.Lmax, q.path, q.len, q.cost, first_status, q.which, d_route,
                                                          d_hop, stream))
            return rc;
        s.Qp = Qp;
        s.live_out = d_live[out];
        s.final_pass = used >= rounds ? 1 : 0;
        int32_t h_counts[2] = {0, 0};
        {
            BIND_DEVICE(ch);
            if (!s.final_pass) HIP_TRY(hipMemsetAsync(d_counts, 0, 2 * sizeof(int32_t), stream));
            hipLaunchKernelGGL(goals_lazy_scan_kernel, dim3(blocks(Qp)), dim3(LAZY_BLOCK), 0, stream, s);
            HIP_TRY(hipGetLastError());
            if (s.final_pass) break;
            // (the one synchronise of a round: the host decides whether another pass follows, and on how many queries)
            HIP_TRY(hipMemcpyAsync(h_counts, d_counts, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
        const int32_t count = h_counts[0], live = h_counts[1];
        if (count <= 0) break;
        // (a claimed slot lies on the route of a live query)
        if ((size_t)count > cap || live < 1 || live > Qp)
            return fail(OPTIK_HIP_EINVAL, "roadmap_lazy_plan_goals: the verdicts are not a lazy roadmap's");
        if (int rc = check_claimed(ch, ee_offset7, g, resolution, d_edge_free, s.list, count, ws + o_free, reals(o_qa),
                                   stream))
            return rc;
        used += 1;
        total += count;
        if (skip) {
            compact = true;
            Qp = live;
            out ^= 1;
        }
    }
    if (rounds_used) *rounds_used = used;
    if (checked) *checked = total;
    return 0;
}

// what the two entry points refuse before any device work; 0 to go on
int check_goals_plan(const optik_hip_chain *ch, const GraphArgs &g, const GoalsQueryArgs &q, int32_t rounds) {
    // (Q = 0: what optik_hip_roadmap_query_goals refuses of the chain, N, k, ks, kg, Lmax and G, in its words; a
    // negative Q and one above 2^30 as they are)
    if (int rc = optik_hip_roadmap_query_goals(ch, nullptr, g.N, nullptr, nullptr, g.k, nullptr, nullptr, nullptr, q.G,
                                               q.Q < 0 || q.Q > ((int64_t)1 << 30) ? q.Q : 0, nullptr, nullptr, q.ks,
                                               nullptr, nullptr, q.kg, nullptr, q.Lmax, nullptr, nullptr, nullptr,
                                               nullptr, nullptr, nullptr, nullptr, nullptr))
        return rc;
    if (rounds < 0 || rounds > roadmap::MAX_ROUNDS)
        return fail(OPTIK_HIP_EINVAL,
                    "roadmap_lazy_plan_goals: rounds must be in 0 .. " + std::to_string(roadmap::MAX_ROUNDS));
    if (q.Q > 0 && (!q.start || !q.goals || !q.gcount || !q.sidx || !q.sw || !q.gidx || !q.gw || !q.direct))
        return fail(OPTIK_HIP_EINVAL, "bad argument");
    return 0;
}

}  // namespace

extern "C" {

int optik_hip_roadmap_lazy_plan_goals(optik_hip_chain *ch, const double *ee_offset7, const double *d_nodes, int32_t N,
                                      const int32_t *d_nbr, double *d_w, int32_t *d_verdict, int32_t k,
                                      double resolution, const double *d_start, const double *d_goals,
                                      const int32_t *d_gcount, int32_t G, int64_t Q, const int32_t *d_sidx,
                                      const double *d_sw, int32_t ks, const int32_t *d_gidx, const double *d_gw,
                                      int32_t kg, const double *d_direct, int32_t Lmax, int32_t rounds,
                                      int32_t skip_settled, double *d_path, int32_t *d_len, double *d_cost,
                                      int32_t *d_status, int32_t *d_which, int32_t *rounds_used, int64_t *checked,
                                      void *stream) {
    const GraphArgs g{d_nodes, N, k, d_nbr, nullptr, d_w, d_verdict};
    const GoalsQueryArgs q{d_start, d_goals, d_gcount, G, Q, d_sidx, d_gidx, d_sw, d_gw, d_direct, ks, kg, Lmax,
                           d_path, d_cost, d_len, d_status, d_which};
    if (int rc = check_goals_plan(ch, g, q, rounds)) return rc;
    // (B = 0: the motion check's own refusals -- the resolution, prismatic joints)
    if (int rc = optik_hip_collision_motion_batch(ch, nullptr, nullptr, nullptr, 0, resolution, nullptr, nullptr,
                                                  nullptr, nullptr, nullptr))
        return rc;
    return goals_lazy_loop(ch, ee_offset7, g, resolution, nullptr, q, rounds, skip_settled != 0, rounds_used, checked,
                           (hipStream_t)stream);
}

int optik_hip_roadmap_lazy_plan_goals_from_flags(optik_hip_chain *ch, const double *d_nodes, int32_t N,
                                                 const int32_t *d_nbr, double *d_w0, double *d_w, int32_t *d_verdict,
                                                 int32_t k, const uint8_t *d_edge_free, const uint8_t *d_node_free,
                                                 const double *d_start, const double *d_goals,
                                                 const int32_t *d_gcount, int32_t G, int64_t Q, const int32_t *d_sidx,
                                                 const double *d_sw, int32_t ks, const int32_t *d_gidx,
                                                 const double *d_gw, int32_t kg, const double *d_direct, int32_t Lmax,
                                                 int32_t rounds, int32_t skip_settled, double *d_path, int32_t *d_len,
                                                 double *d_cost, int32_t *d_status, int32_t *d_which,
                                                 int32_t *rounds_used, int64_t *checked, void *stream) {
    const GraphArgs g{d_nodes, N, k, d_nbr, d_w0, d_w, d_verdict};
    const GoalsQueryArgs q{d_start, d_goals, d_gcount, G, Q, d_sidx, d_gidx, d_sw, d_gw, d_direct, ks, kg, Lmax,
                           d_path, d_cost, d_len, d_status, d_which};
    if (int rc = check_goals_plan(ch, g, q, rounds)) return rc;
    if (Q > 0 && !d_edge_free) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (d_node_free)
        if (int rc = reset_launch(ch, nullptr, g, 0, d_node_free, (hipStream_t)stream)) return rc;
    return goals_lazy_loop(ch, nullptr, g, 1.0, d_edge_free, q, rounds, skip_settled != 0, rounds_used, checked,
                           (hipStream_t)stream);
}

}  // extern "C"
