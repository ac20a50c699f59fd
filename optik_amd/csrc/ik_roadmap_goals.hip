// ik_roadmap_goals.hip -- goal-set planning on the device (roadmap_goals_measure.hpp: the rules and their operation
// order): the cheapest route from a start to any of up to 16 goals over one roadmap, and the
// goal it reaches.  optik_hip_roadmap_query_goals (include/optik_hip.h).
//
//   roadmap_query_goals_kernel<CAP, T>   one block per query, the sizes of roadmap_query_kernel (ik_roadmap.hip): CAP
//                                  1024 (256 threads), 4096 (512) and 8192 (1024).  The shortest-path tree grows from
//                                  the goals, so a goal set only changes where d starts and how a walk ends:
//                                  1. the query's counted goal links (gcount * kg <= 256 pairs of index and weight) and
//                                     direct weights are staged in LDS once, and the counted numbers are looked at
//                                     for NaN by the whole block on the way (one __syncthreads_or);
//                                  2. d starts at +inf; thread e, one per staged link, takes rule 1's minimum for the
//                                     node its link names -- threads whose links name the same node compute and store
//                                     the same value, so nothing is ordered and nothing is atomic;
//                                  3. the Jacobi sweeps of roadmap_query_kernel, unchanged: two [CAP] buffers, one
//                                     __syncthreads_or per sweep;
//                                  4. thread e again: rule 3's goal test of its node against the converged d, into a
//                                     [CAP] byte table -- the walk then asks one LDS byte per node where a scan of
//                                     the staged links would read 256;
//                                  5. thread 0 takes the first hop and walks (at most 62 nodes), looks up the hop
//                                     slots if asked for, and the block writes which, route, hop and the path.
//                                  No atomics, no thread waits for another beyond the block's barriers, no private
//                                  array is indexed dynamically.
#include "collision_device.hpp"
#include "roadmap_goals_measure.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::colldev;

static_assert(roadmap::MAX_GOALS == OPTIK_HIP_ROADMAP_MAX_GOALS && roadmap::K_MAX == OPTIK_HIP_ROADMAP_MAX_K,
              "optik_hip.h states the caps of roadmap_goals_measure.hpp");

namespace {

constexpr int LINKS = roadmap::MAX_GOALS * roadmap::K_MAX;  // staged (index, weight) pairs
constexpr long long MAX_QUERIES = 1ll << 30;

struct GoalsLaunch {
    roadmap::Query y;      // the graph, the start links and the sizes; the query's own members are filled in per block
    const double *nodes;   // [n][N]
    const double *start;   // [n][Q]
    const double *goals;   // [G][n][Q]
    const int32_t *gcount; // [Q]
    long long Q;
    int n, G;
    const int32_t *gidx;   // [G][kg][Q]
    const double *gw;      // [G][kg][Q]
    const double *direct;  // [G][Q]
    double *path;          // [Lmax][Q][n] or null
    int32_t *len;          // [Q] or null
    double *cost;          // [Q] or null
    int32_t *status;       // [Q] or null
    int32_t *which;        // [Q] or null
    int32_t *route, *hop;  // [Lmax][Q] or null: as roadmap_query_kernel writes them
};

template <int CAP, int THREADS>
__global__ __launch_bounds__(THREADS) void roadmap_query_goals_kernel(const GoalsLaunch a) {
    __shared__ double s_d[2][CAP];
    __shared__ double s_gw[LINKS], s_direct[roadmap::MAX_GOALS];
    __shared__ int32_t s_gi[LINKS];
    __shared__ signed char s_goal[CAP];  // rule 3's goal of a node, -1: none
    __shared__ int s_nodes[roadmap::MAX_WAYPOINTS], s_hops[roadmap::MAX_WAYPOINTS];
    __shared__ roadmap::GoalsPlan s_plan;
    static_assert(sizeof(s_d) + sizeof(s_gw) + sizeof(s_direct) + sizeof(s_gi) + sizeof(s_goal) + sizeof(s_nodes)
                          + sizeof(s_hops) + sizeof(s_plan) <= 160 * 1024,
                  "the distance buffers, the staged links and the goal table in one CU's LDS");
    static_assert(THREADS >= LINKS, "one thread per staged link");
    const long long qi = blockIdx.x;
    const int tid = threadIdx.x, N = a.y.N, kg = a.y.kg;
    roadmap::GoalsQuery z;
    z.y = a.y;
    z.y.sidx += qi; z.y.sw += qi;
    z.y.qs = a.Q;
    z.G = a.G;
    z.gcount = roadmap::clamp_count(a.gcount[qi], a.G);
    z.gidx = s_gi; z.gw = s_gw; z.gq = 1; z.gs = kg;
    z.direct = s_direct; z.ds = 1;
    const int links = z.gcount * kg;
    // 1. (goal g's slot s is staged pair g * kg + s; [G][kg][Q] and [G][n][Q] make both offsets e * Q + qi)
    int bad = 0;
    for (int e = tid; e < links; e += THREADS) {
        const double wt = a.gw[(long long)e * a.Q + qi];
        s_gi[e] = a.gidx[(long long)e * a.Q + qi];
        s_gw[e] = wt;
        bad |= wt != wt ? 1 : 0;
    }
    for (int g = tid; g < z.gcount; g += THREADS) {
        const double c = a.direct[(long long)g * a.Q + qi];
        s_direct[g] = c;
        bad |= c != c ? 1 : 0;
    }
    for (int e = tid; e < z.gcount * a.n; e += THREADS) {
        const double x = a.goals[(long long)e * a.Q + qi];
        bad |= x != x ? 1 : 0;
    }
    for (int i = tid; i < a.n; i += THREADS) {
        const double x = a.start[(long long)i * a.Q + qi];
        bad |= x != x ? 1 : 0;
    }
    for (int s = tid; s < z.y.ks; s += THREADS) {
        const double wt = z.y.sw[s * z.y.qs];
        bad |= wt != wt ? 1 : 0;
    }
    for (int v = tid; v < N; v += THREADS) {
        s_d[0][v] = roadmap::inf();
        s_goal[v] = -1;
    }
    const bool has_nan = __syncthreads_or(bad) != 0;
    // 2.
    for (int e = tid; e < links; e += THREADS) {
        const int u = s_gi[e];
        if (roadmap::node_ok(z.y, u)) s_d[0][u] = roadmap::goals_weight(z, u);
    }
    __syncthreads();
    // 3.
    int cur = 0;
    for (int sweep = 0; sweep < N; ++sweep) {
        int changed = 0;
        for (int v = tid; v < N; v += THREADS) {
            const double dv = roadmap::pull(z.y, s_d[cur], v);
            changed |= dv < s_d[cur][v] ? 1 : 0;
            s_d[cur ^ 1][v] = dv;
        }
        // (one barrier per sweep: the sweep after this one reads what this one wrote and overwrites what it read)
        if (!__syncthreads_or(changed)) break;
        cur ^= 1;
    }
    // 4. (a node that no counted link names keeps -1: its own goal-link weights are +inf, which equals d_v only where
    // d_v is +inf, and the walk never stands on such a node -- its first hop and every successor have a finite d)
    for (int e = tid; e < links; e += THREADS) {
        const int u = s_gi[e];
        if (roadmap::node_ok(z.y, u)) s_goal[u] = (signed char)roadmap::goal_of(z, s_d[cur][u], u);
    }
    __syncthreads();
    // 5.
    if (tid == 0) {
        const roadmap::GoalsPlan r = roadmap::plan_goals(z, s_d[cur], has_nan, s_nodes,
                                                         [&](int v) { return (int)s_goal[v]; });
        s_plan = r;
        if (a.len) a.len[qi] = r.p.len;
        if (a.cost) a.cost[qi] = r.p.cost;
        if (a.status) a.status[qi] = r.p.status;
        if (a.which) a.which[qi] = r.which;
        if (a.hop)
            for (int t = 0; t < r.p.len - 2; ++t)
                s_hops[t] = t + 1 < r.p.len - 2 ? roadmap::hop_slot(z.y, s_d[cur], s_nodes[t], s_nodes[t + 1]) : -1;
    }
    __syncthreads();
    const roadmap::GoalsPlan r = s_plan;
    // (waypoint t, 1 <= t < len - 1, is node s_nodes[t - 1]; only a FOUND plan has len > 2)
    if (a.route || a.hop)
        for (int t = tid; t < z.y.Lmax; t += THREADS) {
            const bool node = t >= 1 && t < r.p.len - 1;
            if (a.route) a.route[(long long)t * a.Q + qi] = node ? s_nodes[t - 1] : -1;
            if (a.hop) a.hop[(long long)t * a.Q + qi] = node ? s_hops[t - 1] : -1;
        }
    if (!a.path) return;
    for (int e = tid; e < z.y.Lmax * a.n; e += THREADS) {
        const int t = e / a.n, i = e % a.n;
        a.path[((long long)t * a.Q + qi) * a.n + i] = roadmap::waypoint_value(
            z, r, s_nodes, t, i, a.nodes, a.start + qi, a.Q, a.goals + qi, a.Q, (long long)a.n * a.Q);
    }
}

}  // namespace

extern "C" {

int optik_hip_roadmap_query_goals(const optik_hip_chain *ch, const double *d_nodes, int32_t N, const int32_t *d_nbr,
                                  const double *d_w, int32_t k, const double *d_start, const double *d_goals,
                                  const int32_t *d_gcount, int32_t G, int64_t Q, const int32_t *d_sidx,
                                  const double *d_sw, int32_t ks, const int32_t *d_gidx, const double *d_gw, int32_t kg,
                                  const double *d_direct, int32_t Lmax, double *d_path, int32_t *d_len, double *d_cost,
                                  int32_t *d_status, int32_t *d_which, int32_t *d_route, int32_t *d_hop,
                                  void *stream) {
    if (!ch || Q < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (Q > MAX_QUERIES) return fail(OPTIK_HIP_EINVAL, "roadmap_query_goals: more than 2^30 queries in one launch");
    // (Q = 0: what optik_hip_roadmap_query refuses of N, k, ks, kg, Lmax and the chain, in its words)
    if (int rc = optik_hip_roadmap_query(ch, nullptr, N, nullptr, nullptr, k, nullptr, nullptr, 0, nullptr, nullptr, ks,
                                         nullptr, nullptr, kg, nullptr, Lmax, nullptr, nullptr, nullptr, nullptr,
                                         nullptr))
        return rc;
    if (G < 1 || G > roadmap::MAX_GOALS)
        return fail(OPTIK_HIP_EINVAL,
                    "roadmap_query_goals: G must be in 1 .. " + std::to_string(roadmap::MAX_GOALS) + " goals per query");
    if (Q == 0 || (!d_path && !d_len && !d_cost && !d_status && !d_which && !d_route && !d_hop)) return 0;
    if (!d_nodes || !d_nbr || !d_w || !d_start || !d_goals || !d_gcount || !d_sidx || !d_sw || !d_gidx || !d_gw
        || !d_direct)
        return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    GoalsLaunch a;
    std::memset(&a, 0, sizeof a);
    a.y.N = N; a.y.k = k; a.y.nbr = d_nbr; a.y.w = d_w;
    a.y.ks = ks; a.y.kg = kg;
    a.y.sidx = d_sidx; a.y.sw = d_sw;
    a.y.Lmax = Lmax;
    a.nodes = d_nodes; a.start = d_start; a.goals = d_goals; a.gcount = d_gcount;
    a.Q = Q; a.n = ch->n; a.G = G;
    a.gidx = d_gidx; a.gw = d_gw; a.direct = d_direct;
    a.path = d_path; a.len = d_len; a.cost = d_cost; a.status = d_status; a.which = d_which;
    a.route = d_route; a.hop = d_hop;
    const dim3 grid((unsigned)Q);
    if (N <= 1024)
        hipLaunchKernelGGL((roadmap_query_goals_kernel<1024, 256>), grid, dim3(256), 0, (hipStream_t)stream, a);
    else if (N <= 4096)
        hipLaunchKernelGGL((roadmap_query_goals_kernel<4096, 512>), grid, dim3(512), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((roadmap_query_goals_kernel<8192, 1024>), grid, dim3(1024), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
