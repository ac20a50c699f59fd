// ik_roadmap_lazy.hip -- lazy roadmaps on the device (roadmap_lazy_measure.hpp: the rules):
// the edges of a roadmap are presumed free and checked only when a shortest route uses them, and the verdicts are kept
// until the world changes.  optik_hip_roadmap_lazy_reset / _lazy_plan / _lazy_plan_from_flags (include/optik_hip.h).
//
//   lazy_length_kernel    one thread per slot: the unchecked weight w0 of v -> nbr[s][v]
//   lazy_reset_kernel     one thread per slot: from node_free, nbr and w0 to the verdict and the working weight w
//   (optik_hip_roadmap_query_route, ik_roadmap.hip: a pass; it writes each route's nodes and hop slots)
//   lazy_scan_kernel      one thread per query: walks the query's hop slots.  Claiming form: an UNKNOWN slot is taken
//                         once with a vector atomicCAS on its verdict (UNKNOWN -> CLAIMED) and appended to the round's
//                         list through an atomicAdd counter; a slot found CLAIMED belongs to the round as well.  Which
//                         query takes a shared slot, and the order of the list, vary from run to run; the set, the
//                         verdicts and every output do not.  Final form: nothing is claimed, and a query whose route
//                         holds an UNKNOWN slot becomes UNSETTLED.  No thread waits for another.
//   lazy_gather_kernel    one thread per claimed slot: the segment node -> neighbour into the chain's workspace, as
//                         the motion check takes its segments (the count is known on the host by then: [n][count])
//   (optik_hip_collision_motion_batch, classify form, on the same stream: the motion check's own code)
//   lazy_mark_kernel      one thread per claimed slot: from the free flag to the verdict and w
//
// The workspace, the reset and the check of a round's claimed slots (gather, motion check, mark) are functions of
// roadmap_lazy_device.hpp: the goal-set loop of ik_roadmap_goals_lazy.hip calls them too.
// The loop runs on the host and reads one int32 per round, the size of the round's list: one stream synchronise a
// round, none in the last pass once `rounds` checks are made.
#include <algorithm>

#include "roadmap_lazy_device.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::colldev;
using namespace optik::lazydev;

static_assert(roadmap::MAX_ROUNDS == OPTIK_HIP_ROADMAP_LAZY_MAX_ROUNDS && roadmap::UNKNOWN == OPTIK_HIP_ROADMAP_UNKNOWN
                  && roadmap::FREE == OPTIK_HIP_ROADMAP_FREE && roadmap::BLOCKED == OPTIK_HIP_ROADMAP_BLOCKED,
              "optik_hip.h states the constants of roadmap_lazy_measure.hpp");

namespace {

struct SlotLaunch {
    const double *nodes;  // [n][N]
    int N, k, n;
    const int32_t *nbr;   // [k][N]
    double *w0;           // [k][N]
    const uint8_t *node_free;  // [N]
    int32_t *verdict;     // [k][N]
    double *w;            // [k][N]
};

__global__ __launch_bounds__(LAZY_BLOCK) void lazy_length_kernel(const SlotLaunch a) {
    const long long e = (long long)blockIdx.x * LAZY_BLOCK + threadIdx.x;
    if (e >= (long long)a.k * a.N) return;
    const int v = (int)(e % a.N), u = a.nbr[e];
    const bool ok = u >= 0 && u < a.N;
    const double wt = ok ? roadmap::edge_weight(a.n, a.nodes + v, a.N, a.nodes + u, a.N) : roadmap::inf();
    a.w0[e] = roadmap::unchecked_weight(wt, u, a.N);
}

__global__ __launch_bounds__(LAZY_BLOCK) void lazy_reset_kernel(const SlotLaunch a) {
    const long long e = (long long)blockIdx.x * LAZY_BLOCK + threadIdx.x;
    if (e >= (long long)a.k * a.N) return;
    const int v = (int)(e % a.N), u = a.nbr[e];
    const bool ok = u >= 0 && u < a.N;
    const double w0 = a.w0[e];
    const int verdict = roadmap::reset_verdict(u, a.N, w0, a.node_free[v] != 0, ok && a.node_free[ok ? u : 0] != 0);
    a.verdict[e] = verdict;
    a.w[e] = verdict == roadmap::BLOCKED ? roadmap::inf() : w0;
}

struct ScanLaunch {
    long long Q, cap;      // cap: the room of `list`
    int N, k, n, Lmax, final_pass;
    const int32_t *route, *hop;  // [Lmax][Q] (optik_hip_roadmap_query_route)
    int32_t *verdict;      // [k][N]
    int32_t *list;         // [cap] the slots s * N + v claimed in this round
    int32_t *count;        // [1]
    uint8_t *unknown;      // [Q]
    const double *goal;    // [n][Q]
    double *path;          // [Lmax][Q][n] or null
    int32_t *len, *status;  // [Q] or null
};

__global__ __launch_bounds__(LAZY_BLOCK) void lazy_scan_kernel(const ScanLaunch a) {
    const long long qi = (long long)blockIdx.x * LAZY_BLOCK + threadIdx.x;
    if (qi >= a.Q) return;
    bool unknown = false;
    for (int t = 1; t < a.Lmax - 1; ++t) {
        const int v = a.route[(long long)t * a.Q + qi], s = a.hop[(long long)t * a.Q + qi];
        if (v < 0) break;  // (behind the route; only a FOUND query has one)
        if (s < 0 || s >= a.k || v >= a.N) continue;  // (the route's last node leaves by the goal link)
        const long long e = (long long)s * a.N + v;
        if (a.final_pass) {
            unknown = unknown || a.verdict[e] == roadmap::UNKNOWN;
            continue;
        }
        const int old = atomicCAS(&a.verdict[e], roadmap::UNKNOWN, roadmap::CLAIMED);
        if (old == roadmap::UNKNOWN) {
            const long long pos = atomicAdd(a.count, 1);
            if (pos < a.cap) a.list[pos] = (int32_t)e;  // (a slot is claimed once: pos < k * N always)
        }
        unknown = unknown || old == roadmap::UNKNOWN || old == roadmap::CLAIMED;
    }
    a.unknown[qi] = unknown ? 1 : 0;
    if (!a.final_pass || !unknown) return;
    if (a.status) a.status[qi] = roadmap::UNSETTLED;
    if (a.len) a.len[qi] = 2;
    if (a.path)
        for (int t = 1; t < a.Lmax; ++t)
            for (int i = 0; i < a.n; ++i)
                a.path[((long long)t * a.Q + qi) * a.n + i] = a.goal[(long long)i * a.Q + qi];
}

struct MarkLaunch {
    long long B;           // the claimed slots
    int N, k, n;
    const int32_t *list;   // [B]
    const int32_t *nbr;    // [k][N]
    const double *nodes;   // [n][N]
    double *qa, *qb;       // [n][B]
    const uint8_t *free_flag;  // [B], or with by_slot [k][N]
    int by_slot;
    int32_t *verdict;      // [k][N]
    double *w;             // [k][N]
};

__global__ __launch_bounds__(LAZY_BLOCK) void lazy_gather_kernel(const MarkLaunch a) {
    const long long b = (long long)blockIdx.x * LAZY_BLOCK + threadIdx.x;
    if (b >= a.B) return;
    const long long e = a.list[b];
    if (e < 0 || e >= (long long)a.k * a.N) return;
    const int v = (int)(e % a.N), u = a.nbr[e];
    const bool ok = u >= 0 && u < a.N;  // (a claimed slot was UNKNOWN: it is not empty)
    for (int i = 0; i < a.n; ++i) {
        const double f = a.nodes[(long long)i * a.N + v];
        a.qa[(long long)i * a.B + b] = f;
        a.qb[(long long)i * a.B + b] = ok ? a.nodes[(long long)i * a.N + u] : f;
    }
}

__global__ __launch_bounds__(LAZY_BLOCK) void lazy_mark_kernel(const MarkLaunch a) {
    const long long b = (long long)blockIdx.x * LAZY_BLOCK + threadIdx.x;
    if (b >= a.B) return;
    const long long e = a.list[b];
    if (e < 0 || e >= (long long)a.k * a.N) return;
    const int verdict = roadmap::mark(a.free_flag[a.by_slot ? e : b] != 0);
    a.verdict[e] = verdict;
    if (verdict == roadmap::BLOCKED) a.w[e] = roadmap::inf();
}

}  // namespace

// (roadmap_lazy_device.hpp: shared with the goal-set loop of ik_roadmap_goals_lazy.hip)
int optik::lazydev::reserve_ws(optik_hip_chain *ch, size_t bytes, unsigned char **out) {
    std::lock_guard<std::mutex> lock(ch->mu);
    BIND_DEVICE(ch);
    HIP_TRY(ch->roadmap_lazy_ws.reserve(bytes));
    *out = ch->roadmap_lazy_ws.get();
    return 0;
}

namespace {

// what reset refuses: the graph as optik_hip_roadmap_query refuses it
int check_lazy_graph(const optik_hip_chain *ch, int32_t N, int32_t k) {
    return optik_hip_roadmap_query_route(ch, nullptr, N, nullptr, nullptr, k, nullptr, nullptr, 0, nullptr, nullptr, 1,
                                         nullptr, nullptr, 1, nullptr, roadmap::MIN_WAYPOINTS, nullptr, nullptr,
                                         nullptr, nullptr, nullptr, nullptr, nullptr);
}

}  // namespace

int optik::lazydev::reset_launch(optik_hip_chain *ch, const double *ee_offset7, const GraphArgs &g, int lengths,
                                 const uint8_t *d_node_free, hipStream_t stream) {
    if (!g.nodes || !g.nbr || !g.w0 || !g.verdict || !g.w) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (!d_node_free) {
        unsigned char *ws = nullptr;
        if (int rc = reserve_ws(ch, (size_t)g.N, &ws)) return rc;
        if (int rc = optik_hip_collision_batch(ch, ee_offset7, g.nodes, g.N, nullptr, ws, stream)) return rc;
        d_node_free = ws;
    }
    SlotLaunch a{g.nodes, g.N, g.k, ch->n, g.nbr, g.w0, d_node_free, g.verdict, g.w};
    BIND_DEVICE(ch);
    const unsigned grid = blocks((long long)g.k * g.N);
    if (lengths) hipLaunchKernelGGL(lazy_length_kernel, dim3(grid), dim3(LAZY_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(lazy_reset_kernel, dim3(grid), dim3(LAZY_BLOCK), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int optik::lazydev::check_claimed(optik_hip_chain *ch, const double *ee_offset7, const GraphArgs &g, double resolution,
                                  const uint8_t *d_edge_free, const int32_t *d_list, int32_t count,
                                  unsigned char *d_free, double *d_qa, hipStream_t stream) {
    MarkLaunch m;
    std::memset(&m, 0, sizeof m);
    m.B = count;
    m.N = g.N; m.k = g.k; m.n = ch->n;
    m.list = d_list; m.nbr = g.nbr; m.nodes = g.nodes;
    m.qa = d_qa;
    m.qb = d_qa ? d_qa + (size_t)ch->n * (size_t)count : nullptr;
    m.free_flag = d_edge_free ? d_edge_free : d_free;
    m.by_slot = d_edge_free ? 1 : 0;
    m.verdict = g.verdict; m.w = g.w;
    if (!d_edge_free) {
        {
            BIND_DEVICE(ch);
            hipLaunchKernelGGL(lazy_gather_kernel, dim3(blocks(count)), dim3(LAZY_BLOCK), 0, stream, m);
            HIP_TRY(hipGetLastError());
        }
        if (int rc = optik_hip_collision_motion_batch(ch, ee_offset7, m.qa, m.qb, count, resolution, nullptr, d_free,
                                                      nullptr, nullptr, stream))
            return rc;
    }
    BIND_DEVICE(ch);
    hipLaunchKernelGGL(lazy_mark_kernel, dim3(blocks(count)), dim3(LAZY_BLOCK), 0, stream, m);
    HIP_TRY(hipGetLastError());
    return 0;
}

namespace {

struct QueryArgs {
    const double *start, *goal;
    int64_t Q;
    const int32_t *sidx, *gidx;
    const double *sw, *gw, *direct;
    int32_t ks, kg, Lmax;
    double *path, *cost;
    int32_t *len, *status;
};

// The loop of roadmap_lazy_measure.hpp, rules 3 to 5.  d_edge_free [k][N]: stands for the motion check (the test
// hook); null: the motion check at `resolution`.
int lazy_loop(optik_hip_chain *ch, const double *ee_offset7, const GraphArgs &g, double resolution,
              const uint8_t *d_edge_free, const QueryArgs &q, int32_t rounds, int32_t *rounds_used, int64_t *checked,
              hipStream_t stream) {
    if (rounds_used) *rounds_used = 0;
    if (checked) *checked = 0;
    if (q.Q == 0) return 0;
    if (!g.nodes || !g.nbr || !g.verdict || !g.w) return fail(OPTIK_HIP_EINVAL, "bad argument");
    const size_t n = (size_t)ch->n, Q = (size_t)q.Q, cells = (size_t)g.k * (size_t)g.N;
    const size_t hops = q.Lmax > 3 ? Q * (size_t)(q.Lmax - 3) : 0;  // (a route of Lmax waypoints has Lmax - 3 graph hops)
    const size_t cap = std::max<size_t>(1, std::min(cells, hops));
    const size_t o_route = 16, o_hop = o_route + align16(4 * (size_t)q.Lmax * Q),
                 o_list = o_hop + align16(4 * (size_t)q.Lmax * Q), o_unknown = o_list + align16(4 * cap),
                 o_free = o_unknown + align16(Q), o_qa = o_free + align16(cap),
                 bytes = o_qa + (d_edge_free ? 0 : 2 * sizeof(double) * n * cap);
    unsigned char *ws = nullptr;
    if (int rc = reserve_ws(ch, bytes, &ws)) return rc;
    int32_t *d_count = reinterpret_cast<int32_t *>(ws);
    ScanLaunch s;
    std::memset(&s, 0, sizeof s);
    s.Q = q.Q; s.cap = (long long)cap;
    s.N = g.N; s.k = g.k; s.n = ch->n; s.Lmax = q.Lmax;
    s.route = reinterpret_cast<int32_t *>(ws + o_route);
    s.hop = reinterpret_cast<int32_t *>(ws + o_hop);
    s.verdict = g.verdict;
    s.list = reinterpret_cast<int32_t *>(ws + o_list);
    s.count = d_count;
    s.unknown = ws + o_unknown;
    s.goal = q.goal; s.path = q.path; s.len = q.len; s.status = q.status;
    int32_t used = 0;
    int64_t total = 0;
    for (;;) {
        if (int rc = optik_hip_roadmap_query_route(ch, g.nodes, g.N, g.nbr, g.w, g.k, q.start, q.goal, q.Q, q.sidx, q.sw,
                                                   q.ks, q.gidx, q.gw, q.kg, q.direct, q.Lmax, q.path, q.len, q.cost,
                                                   q.status, const_cast<int32_t *>(s.route),
                                                   const_cast<int32_t *>(s.hop), stream))
            return rc;
        s.final_pass = used >= rounds ? 1 : 0;
        int32_t count = 0;
        {
            BIND_DEVICE(ch);
            if (!s.final_pass) HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(int32_t), stream));
            hipLaunchKernelGGL(lazy_scan_kernel, dim3(blocks(q.Q)), dim3(LAZY_BLOCK), 0, stream, s);
            HIP_TRY(hipGetLastError());
            if (s.final_pass) break;
            // (the one synchronise of a round: the host decides whether another pass follows)
            HIP_TRY(hipMemcpyAsync(&count, d_count, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
        if (count <= 0) break;
        if ((size_t)count > cap) return fail(OPTIK_HIP_EINVAL, "roadmap_lazy_plan: the verdicts are not a lazy roadmap's");
        if (int rc = check_claimed(ch, ee_offset7, g, resolution, d_edge_free, s.list, count, ws + o_free,
                                   reinterpret_cast<double *>(ws + o_qa), stream))
            return rc;
        used += 1;
        total += count;
    }
    if (rounds_used) *rounds_used = used;
    if (checked) *checked = total;
    return 0;
}

// what the two plan entry points refuse before any device work; 0 to go on
int check_plan(const optik_hip_chain *ch, const GraphArgs &g, const QueryArgs &q, int32_t rounds) {
    if (int rc = optik_hip_roadmap_query_route(ch, nullptr, g.N, nullptr, nullptr, g.k, nullptr, nullptr,
                                               q.Q < 0 ? q.Q : 0, nullptr, nullptr, q.ks, nullptr, nullptr, q.kg,
                                               nullptr, q.Lmax, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               nullptr))
        return rc;
    if (q.Q > ((int64_t)1 << 30)) return fail(OPTIK_HIP_EINVAL, "roadmap_lazy_plan: more than 2^30 queries in one launch");
    if (rounds < 0 || rounds > roadmap::MAX_ROUNDS)
        return fail(OPTIK_HIP_EINVAL, "roadmap_lazy_plan: rounds must be in 0 .. " + std::to_string(roadmap::MAX_ROUNDS));
    if (q.Q > 0 && (!q.start || !q.goal || !q.sidx || !q.sw || !q.gidx || !q.gw || !q.direct))
        return fail(OPTIK_HIP_EINVAL, "bad argument");
    return 0;
}

}  // namespace

extern "C" {

int optik_hip_roadmap_lazy_reset(optik_hip_chain *ch, const double *ee_offset7, const double *d_nodes, int32_t N,
                                 const int32_t *d_nbr, int32_t k, int32_t lengths, double *d_w0,
                                 const uint8_t *d_node_free, int32_t *d_verdict, double *d_w, void *stream) {
    if (int rc = check_lazy_graph(ch, N, k)) return rc;
    const GraphArgs g{d_nodes, N, k, d_nbr, d_w0, d_w, d_verdict};
    return reset_launch(ch, ee_offset7, g, lengths, d_node_free, (hipStream_t)stream);
}

int optik_hip_roadmap_lazy_plan(optik_hip_chain *ch, const double *ee_offset7, const double *d_nodes, int32_t N,
                                const int32_t *d_nbr, double *d_w, int32_t *d_verdict, int32_t k, double resolution,
                                const double *d_start, const double *d_goal, int64_t Q, const int32_t *d_sidx,
                                const double *d_sw, int32_t ks, const int32_t *d_gidx, const double *d_gw, int32_t kg,
                                const double *d_direct, int32_t Lmax, int32_t rounds, double *d_path, int32_t *d_len,
                                double *d_cost, int32_t *d_status, int32_t *rounds_used, int64_t *checked,
                                void *stream) {
    const GraphArgs g{d_nodes, N, k, d_nbr, nullptr, d_w, d_verdict};
    const QueryArgs q{d_start, d_goal, Q, d_sidx, d_gidx, d_sw, d_gw, d_direct, ks, kg, Lmax, d_path, d_cost, d_len,
                      d_status};
    if (int rc = check_plan(ch, g, q, rounds)) return rc;
    // (B = 0: the motion check's own refusals -- the resolution, prismatic joints)
    if (int rc = optik_hip_collision_motion_batch(ch, nullptr, nullptr, nullptr, 0, resolution, nullptr, nullptr,
                                                  nullptr, nullptr, nullptr))
        return rc;
    return lazy_loop(ch, ee_offset7, g, resolution, nullptr, q, rounds, rounds_used, checked, (hipStream_t)stream);
}

int optik_hip_roadmap_lazy_plan_from_flags(optik_hip_chain *ch, const double *d_nodes, int32_t N, const int32_t *d_nbr,
                                           double *d_w0, double *d_w, int32_t *d_verdict, int32_t k,
                                           const uint8_t *d_edge_free, const uint8_t *d_node_free,
                                           const double *d_start, const double *d_goal, int64_t Q,
                                           const int32_t *d_sidx, const double *d_sw, int32_t ks,
                                           const int32_t *d_gidx, const double *d_gw, int32_t kg,
                                           const double *d_direct, int32_t Lmax, int32_t rounds, double *d_path,
                                           int32_t *d_len, double *d_cost, int32_t *d_status, int32_t *rounds_used,
                                           int64_t *checked, void *stream) {
    const GraphArgs g{d_nodes, N, k, d_nbr, d_w0, d_w, d_verdict};
    const QueryArgs q{d_start, d_goal, Q, d_sidx, d_gidx, d_sw, d_gw, d_direct, ks, kg, Lmax, d_path, d_cost, d_len,
                      d_status};
    if (int rc = check_plan(ch, g, q, rounds)) return rc;
    if (Q > 0 && !d_edge_free) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (d_node_free)
        if (int rc = reset_launch(ch, nullptr, g, 0, d_node_free, (hipStream_t)stream)) return rc;
    return lazy_loop(ch, nullptr, g, 1.0, d_edge_free, q, rounds, rounds_used, checked, (hipStream_t)stream);
}

}  // extern "C"
