// ik_roadmap.hip -- roadmap planning on the device (roadmap_measure.hpp: the arithmetic and its operation order;
// DESIGN.md section 5.18): nearest neighbours in joint space, motion-checked edges, and many shortest-path queries
// over one graph.  optik_hip_roadmap_knn / _edges / _query (include/optik_hip.h).
//
//   roadmap_knn_kernel<N>          one thread per query, one wave per block.  The nodes pass through LDS in tiles of
//                                  256, [N][256] doubles; a lane keeps its query's joints and the 16 best (distance,
//                                  index) pairs in registers and inserts through roadmap::Best's fixed network, so
//                                  nothing is indexed dynamically.  The result is the first k of a total order: it
//                                  does not depend on the tile size or on the order of the visits.
//   roadmap_gather_kernel          one thread per (slot, endpoint): the segment endpoint -> node (or node -> endpoint)
//                                  into the chain's workspace, as the motion check takes its segments
//   (optik_hip_collision_motion_batch, classify form, on the same stream: the motion check's own code)
//   roadmap_weight_kernel          one thread per segment: the weight, +inf unless the motion was free
//   roadmap_query_kernel<CAP, T>   one block per query.  The distances to the goal live in LDS, two [CAP] buffers
//                                  (Jacobi: a sweep reads one and writes the other, one barrier per sweep that also
//                                  ORs the "changed" flags); every node pulls over its own out-list, [k][N] reads
//                                  coalesced over the nodes, no atomics.  Thread 0 then takes the first hop and walks
//                                  the successors (at most 62 nodes), and the block writes the path.  Three sizes:
//                                  CAP 1024 (16 KiB, 256 threads), 4096 (64 KiB, 512) and 8192 (128 KiB, 1024).
//                                  For a lazy roadmap (optik_hip_roadmap_query_route; ik_roadmap_lazy.hip) thread 0
//                                  also looks up the slot of every graph hop while d is still in LDS, and the block
//                                  writes the walked node indices and those slots.
#include "collision_device.hpp"
#include "roadmap_lazy_measure.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::colldev;

static_assert(roadmap::MAX_NODES == OPTIK_HIP_ROADMAP_MAX_NODES && roadmap::K_MAX == OPTIK_HIP_ROADMAP_MAX_K
                  && roadmap::MAX_WAYPOINTS == OPTIK_HIP_PATH_OPTIMIZE_MAX_WAYPOINTS,
              "optik_hip.h states the caps of roadmap_measure.hpp; a plan is a path path_optimize takes");
static_assert(2 * sizeof(double) * roadmap::MAX_NODES <= 160 * 1024 - 1024, "two distance buffers in one CU's LDS");

namespace {

constexpr int KNN_BLOCK = 64, KNN_TILE = 256, EDGE_BLOCK = 256;
constexpr long long MAX_QUERIES = 1ll << 30;

struct KnnLaunch {
    const double *q;      // [n][Q]
    long long Q;
    const double *nodes;  // [n][N]
    int N, k, exclude_self;
    int32_t *idx;         // [k][Q] or null
    double *dist;         // [k][Q] or null
};

template <int NJ>
__global__ __launch_bounds__(KNN_BLOCK) void roadmap_knn_kernel(const KnnLaunch a) {
    __shared__ double s_node[NJ][KNN_TILE];
    const long long qi = (long long)blockIdx.x * KNN_BLOCK + threadIdx.x;
    const bool act = qi < a.Q;
    double q[NJ];
#pragma unroll
    for (int i = 0; i < NJ; ++i) q[i] = act ? a.q[(long long)i * a.Q + qi] : 0.0;
    roadmap::Best best;
    best.clear();
    for (int t0 = 0; t0 < a.N; t0 += KNN_TILE) {
        const int cnt = a.N - t0 < KNN_TILE ? a.N - t0 : KNN_TILE;
        __syncthreads();  // (the tile before is read)
        for (int e = threadIdx.x; e < NJ * KNN_TILE; e += KNN_BLOCK) {
            const int i = e / KNN_TILE, j = e % KNN_TILE;
            if (j < cnt) s_node[i][j] = a.nodes[(long long)i * a.N + t0 + j];
        }
        __syncthreads();
        if (act) {
            for (int j = 0; j < cnt; ++j) {
                double d = 0.0;
#pragma unroll
                for (int i = 0; i < NJ; ++i) d = motion::distance_take(d, fabs(s_node[i][j] - q[i]));
                const int node = t0 + j;
                if (!(a.exclude_self && (long long)node == qi)) best.insert(d, node);
            }
        }
    }
    if (!act) return;
#pragma unroll
    for (int s = 0; s < roadmap::K_MAX; ++s) {
        if (s < a.k) {
            if (a.idx) a.idx[(long long)s * a.Q + qi] = best.i[s];
            if (a.dist) a.dist[(long long)s * a.Q + qi] = best.d[s];
        }
    }
}

struct EdgeLaunch {
    const double *from;   // [n][Q]
    long long Q, B;       // B = k * Q
    const double *nodes;  // [n][N]
    int N, n, reverse;
    const int32_t *idx;   // [k][Q]; null: node q for endpoint q
    double *qa, *qb;      // [n][B] the gathered segments
    const uint8_t *free_flag;  // [B]
    double *w;            // [k][Q]
};

__device__ __forceinline__ int edge_node(const EdgeLaunch &a, long long b) {
    const long long u = a.idx ? (long long)a.idx[b] : b % a.Q;
    return (u >= 0 && u < a.N) ? (int)u : -1;
}

__global__ __launch_bounds__(EDGE_BLOCK) void roadmap_gather_kernel(const EdgeLaunch a) {
    const long long b = (long long)blockIdx.x * EDGE_BLOCK + threadIdx.x;
    if (b >= a.B) return;
    const long long qi = b % a.Q;
    const int u = edge_node(a, b);
    for (int i = 0; i < a.n; ++i) {
        const double f = a.from[(long long)i * a.Q + qi];
        // (an empty slot: a motion of length 0, its weight is +inf whatever the check says)
        const double t = u >= 0 ? a.nodes[(long long)i * a.N + u] : f;
        a.qa[(long long)i * a.B + b] = a.reverse ? t : f;
        a.qb[(long long)i * a.B + b] = a.reverse ? f : t;
    }
}

__global__ __launch_bounds__(EDGE_BLOCK) void roadmap_weight_kernel(const EdgeLaunch a) {
    const long long b = (long long)blockIdx.x * EDGE_BLOCK + threadIdx.x;
    if (b >= a.B) return;
    a.w[b] = roadmap::checked_weight(roadmap::edge_weight(a.n, a.qa + b, a.B, a.qb + b, a.B), edge_node(a, b),
                                     a.free_flag[b] != 0);
}

struct QueryLaunch {
    roadmap::Query y;     // the graph and the sizes; the query's own members are filled in per block
    const double *nodes;  // [n][N]
    const double *start, *goal;  // [n][Q]
    long long Q;
    int n;
    const double *direct;  // [Q]
    double *path;          // [Lmax][Q][n] or null
    int32_t *len;          // [Q] or null
    double *cost;          // [Q] or null
    int32_t *status;       // [Q] or null
    int32_t *route, *hop;  // [Lmax][Q] or null: waypoint t's node, and the slot of the graph hop that leaves it
};

template <int CAP, int THREADS>
__global__ __launch_bounds__(THREADS) void roadmap_query_kernel(const QueryLaunch a) {
    __shared__ double s_d[2][CAP];
    __shared__ int s_nodes[roadmap::MAX_WAYPOINTS], s_hops[roadmap::MAX_WAYPOINTS];
    __shared__ roadmap::Plan s_plan;
    const long long qi = blockIdx.x;
    const int tid = threadIdx.x, N = a.y.N;
    roadmap::Query y = a.y;
    y.sidx += qi; y.sw += qi; y.gidx += qi; y.gw += qi;
    y.qs = a.Q;
    y.direct = a.direct[qi];
    for (int v = tid; v < N; v += THREADS) s_d[0][v] = roadmap::goal_weight(y, v);
    __syncthreads();
    int cur = 0;
    for (int sweep = 0; sweep < N; ++sweep) {
        int changed = 0;
        for (int v = tid; v < N; v += THREADS) {
            const double dv = roadmap::pull(y, s_d[cur], v);
            changed |= dv < s_d[cur][v] ? 1 : 0;
            s_d[cur ^ 1][v] = dv;
        }
        // (one barrier per sweep: the sweep after this one reads what this one wrote and overwrites what it read)
        if (!__syncthreads_or(changed)) break;
        cur ^= 1;
    }
    if (tid == 0) {
        const bool nan = roadmap::query_has_nan(y, a.n, a.start + qi, a.Q, a.goal + qi, a.Q);
        const roadmap::Plan p = roadmap::plan(y, s_d[cur], nan, s_nodes);
        s_plan = p;
        if (a.len) a.len[qi] = p.len;
        if (a.cost) a.cost[qi] = p.cost;
        if (a.status) a.status[qi] = p.status;
        if (a.hop)
            for (int t = 0; t < p.len - 2; ++t)
                s_hops[t] = t + 1 < p.len - 2 ? roadmap::hop_slot(y, s_d[cur], s_nodes[t], s_nodes[t + 1]) : -1;
    }
    __syncthreads();
    const int len = s_plan.len;
    // (waypoint t, 1 <= t < len - 1, is node s_nodes[t - 1]; only a FOUND plan has len > 2)
    if (a.route || a.hop)
        for (int t = tid; t < y.Lmax; t += THREADS) {
            const bool node = t >= 1 && t < len - 1;
            if (a.route) a.route[(long long)t * a.Q + qi] = node ? s_nodes[t - 1] : -1;
            if (a.hop) a.hop[(long long)t * a.Q + qi] = node ? s_hops[t - 1] : -1;
        }
    if (!a.path) return;
    for (int e = tid; e < y.Lmax * a.n; e += THREADS) {
        const int t = e / a.n, i = e % a.n;
        double v = a.goal[(long long)i * a.Q + qi];
        if (t == 0) v = a.start[(long long)i * a.Q + qi];
        else if (t < len - 1) v = a.nodes[(long long)i * N + s_nodes[t - 1]];
        a.path[((long long)t * a.Q + qi) * a.n + i] = v;
    }
}

// what the three entry points refuse alike; 0 to go on
int check_graph(const optik_hip_chain *ch, long long Q, int N, int k, const char *what) {
    if (!ch || Q < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (k < 1 || k > roadmap::K_MAX)
        return fail(OPTIK_HIP_EINVAL, std::string(what) + ": k must be in 1 .. " + std::to_string(roadmap::K_MAX));
    if (N < 1 || N > roadmap::MAX_NODES)
        return fail(OPTIK_HIP_EINVAL, std::string(what) + ": a roadmap has 1 .. " + std::to_string(roadmap::MAX_NODES)
                                          + " nodes");
    if (Q > MAX_QUERIES) return fail(OPTIK_HIP_EINVAL, std::string(what) + ": more than 2^30 queries in one launch");
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, prismatic_msg());
    return 0;
}

}  // namespace

extern "C" {

int optik_hip_roadmap_knn(const optik_hip_chain *ch, const double *d_q, int64_t Q, const double *d_nodes, int32_t N,
                          int32_t k, int32_t exclude_self, int32_t *d_idx, double *d_dist, void *stream) {
    if (int rc = check_graph(ch, Q, N, k, "roadmap_knn")) return rc;
    if (Q == 0 || (!d_idx && !d_dist)) return 0;
    if (!d_q || !d_nodes) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    KnnLaunch a{d_q, Q, d_nodes, N, k, exclude_self ? 1 : 0, d_idx, d_dist};
    const unsigned grid = (unsigned)((Q + KNN_BLOCK - 1) / KNN_BLOCK);
    switch (ch->n) {
#define CASE(NN) \
    case NN: hipLaunchKernelGGL(roadmap_knn_kernel<NN>, dim3(grid), dim3(KNN_BLOCK), 0, (hipStream_t)stream, a); break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
        CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
#undef CASE
    default: return fail(OPTIK_HIP_EUNSUPPORTED, "roadmap_knn: chains of 1 .. 16 joint positions");
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int optik_hip_roadmap_edges(optik_hip_chain *ch, const double *ee_offset7, const double *d_from, int64_t Q,
                            const double *d_nodes, int32_t N, const int32_t *d_idx, int32_t k, double resolution,
                            int32_t reverse, double *d_w, void *stream) {
    if (!ch || Q < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (k < 1 || k > roadmap::K_MAX)
        return fail(OPTIK_HIP_EINVAL, "roadmap_edges: k must be in 1 .. " + std::to_string(roadmap::K_MAX));
    if (N < 1) return fail(OPTIK_HIP_EINVAL, "roadmap_edges: no nodes");
    if (Q > MAX_QUERIES / roadmap::K_MAX)
        return fail(OPTIK_HIP_EINVAL, "roadmap_edges: more than 2^26 endpoints in one launch");
    // (B = 0: the motion check's own refusals -- the resolution, prismatic joints)
    if (int rc = optik_hip_collision_motion_batch(ch, nullptr, nullptr, nullptr, 0, resolution, nullptr, nullptr,
                                                  nullptr, nullptr, nullptr))
        return rc;
    if (Q == 0 || !d_w) return 0;
    if (!d_from || !d_nodes) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (!d_idx && (k != 1 || (int64_t)N != Q))
        return fail(OPTIK_HIP_EINVAL, "roadmap_edges: without d_idx endpoint q is paired with node q (k = 1, N = Q)");
    const long long B = (long long)k * Q;
    const size_t n = (size_t)ch->n;
    EdgeLaunch a;
    std::memset(&a, 0, sizeof a);
    {
        std::lock_guard<std::mutex> lock(ch->mu);
        BIND_DEVICE(ch);
        HIP_TRY(ch->roadmap_ws.reserve((sizeof(double) * 2 * n + 1) * (size_t)B));
        a.qa = reinterpret_cast<double *>(ch->roadmap_ws.get());
    }
    a.qb = a.qa + n * (size_t)B;
    uint8_t *d_free = reinterpret_cast<uint8_t *>(a.qb + n * (size_t)B);
    a.from = d_from; a.Q = Q; a.B = B;
    a.nodes = d_nodes; a.N = N; a.n = ch->n; a.reverse = reverse ? 1 : 0;
    a.idx = d_idx;
    a.free_flag = d_free;
    a.w = d_w;
    const unsigned grid = (unsigned)((B + EDGE_BLOCK - 1) / EDGE_BLOCK);
    {
        BIND_DEVICE(ch);
        hipLaunchKernelGGL(roadmap_gather_kernel, dim3(grid), dim3(EDGE_BLOCK), 0, (hipStream_t)stream, a);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = optik_hip_collision_motion_batch(ch, ee_offset7, a.qa, a.qb, B, resolution, nullptr, d_free, nullptr,
                                                  nullptr, stream))
        return rc;
    BIND_DEVICE(ch);
    hipLaunchKernelGGL(roadmap_weight_kernel, dim3(grid), dim3(EDGE_BLOCK), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int optik_hip_roadmap_query(const optik_hip_chain *ch, const double *d_nodes, int32_t N, const int32_t *d_nbr,
                            const double *d_w, int32_t k, const double *d_start, const double *d_goal, int64_t Q,
                            const int32_t *d_sidx, const double *d_sw, int32_t ks, const int32_t *d_gidx,
                            const double *d_gw, int32_t kg, const double *d_direct, int32_t Lmax, double *d_path,
                            int32_t *d_len, double *d_cost, int32_t *d_status, void *stream) {
    return optik_hip_roadmap_query_route(ch, d_nodes, N, d_nbr, d_w, k, d_start, d_goal, Q, d_sidx, d_sw, ks, d_gidx,
                                         d_gw, kg, d_direct, Lmax, d_path, d_len, d_cost, d_status, nullptr, nullptr,
                                         stream);
}

int optik_hip_roadmap_query_route(const optik_hip_chain *ch, const double *d_nodes, int32_t N, const int32_t *d_nbr,
                                  const double *d_w, int32_t k, const double *d_start, const double *d_goal, int64_t Q,
                                  const int32_t *d_sidx, const double *d_sw, int32_t ks, const int32_t *d_gidx,
                                  const double *d_gw, int32_t kg, const double *d_direct, int32_t Lmax, double *d_path,
                                  int32_t *d_len, double *d_cost, int32_t *d_status, int32_t *d_route, int32_t *d_hop,
                                  void *stream) {
    if (int rc = check_graph(ch, Q, N, k, "roadmap_query")) return rc;
    if (ks < 1 || ks > roadmap::K_MAX || kg < 1 || kg > roadmap::K_MAX)
        return fail(OPTIK_HIP_EINVAL, "roadmap_query: ks and kg must be in 1 .. " + std::to_string(roadmap::K_MAX));
    if (Lmax < roadmap::MIN_WAYPOINTS || Lmax > roadmap::MAX_WAYPOINTS)
        return fail(OPTIK_HIP_EINVAL, "roadmap_query: a path has 2 .. 64 waypoints");
    if (Q == 0 || (!d_path && !d_len && !d_cost && !d_status && !d_route && !d_hop)) return 0;
    if (!d_nodes || !d_nbr || !d_w || !d_start || !d_goal || !d_sidx || !d_sw || !d_gidx || !d_gw || !d_direct)
        return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    QueryLaunch a;
    std::memset(&a, 0, sizeof a);
    a.y.N = N; a.y.k = k; a.y.nbr = d_nbr; a.y.w = d_w;
    a.y.ks = ks; a.y.kg = kg;
    a.y.sidx = d_sidx; a.y.sw = d_sw; a.y.gidx = d_gidx; a.y.gw = d_gw;
    a.y.Lmax = Lmax;
    a.nodes = d_nodes; a.start = d_start; a.goal = d_goal;
    a.Q = Q; a.n = ch->n;
    a.direct = d_direct;
    a.path = d_path; a.len = d_len; a.cost = d_cost; a.status = d_status;
    a.route = d_route; a.hop = d_hop;
    const dim3 grid((unsigned)Q);
    if (N <= 1024)
        hipLaunchKernelGGL((roadmap_query_kernel<1024, 256>), grid, dim3(256), 0, (hipStream_t)stream, a);
    else if (N <= 4096)
        hipLaunchKernelGGL((roadmap_query_kernel<4096, 512>), grid, dim3(512), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((roadmap_query_kernel<8192, 1024>), grid, dim3(1024), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
