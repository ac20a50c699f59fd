// ik_rrt_goals.hip -- the bidirectional tree planner with a goal set per query (rrt_goals_measure.hpp: the rules and
// their operation order): tree 1 has one root per counted goal that is free, and the query ends
// at the first junction with any of them.  optik_hip_rrt_plan_goals (include/optik_hip.h).
//
//   rrt_goals_gather_kernel  one thread per query of the chunk: its clamped goal count; the 1 + G configurations that
//                            rule 0 classifies, [n][(1 + G) Qc] -- the start, then per slot the goal if it is counted
//                            and the start again if it is not --; and the G direct motions in travel direction,
//                            start -> goal g, [n][G Qc] twice -- NaN on both ends for a slot that is not counted, which
//                            the motion check answers "not sampled" without reading a model.  The second of the two
//                            arrays is where the later kernels read a counted goal from.
//   (optik_hip_collision_batch on the 1 + G columns, optik_hip_collision_motion_batch on the G segments, same stream)
//   rrt_goals_begin_kernel   one thread per query: rule 0 -- the roots of tree 1 in ascending g with the root -> goal
//                            table, the nearest free direct motion --, and the count of the queries that go on.  Only
//                            the flags of counted slots are read.
//   (rrtdev::run_iterations: ik_rrt.hip's rrt_step_kernel and the motion check, as optik_hip_rrt_plan runs them -- the
//    per-iteration kernel needs no new rule, a tree 1 with R roots is a tree with R nodes to it)
//   rrt_goals_walk_kernel    one wave per query: rrt_walk_kernel's walk, which follows tree 1's branch to whichever
//                            root it ends in; that root's goal slot is `which`, and the path is padded with that goal.
//
// No kernel waits for another workgroup; every loop's trip count is bounded by a tree's size, n, G or Lmax; no private
// array is indexed dynamically; the one atomic is the begin kernel's vector atomicAdd on the count of running queries,
// as in rrt_begin_kernel (its counterpart, the atomicSub of a query that ends, is rrt_step_kernel's).
#include <algorithm>

#include "rrt_device.hpp"
#include "rrt_goals_measure.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::colldev;
using namespace optik::rrtdev;

static_assert(rrt::MAX_GOALS == OPTIK_HIP_RRT_MAX_GOALS && OPTIK_HIP_RRT_MAX_GOALS == OPTIK_HIP_ROADMAP_MAX_GOALS,
              "optik_hip.h states the cap of rrt_goals_measure.hpp; a goal set is what ik_solutions and the roadmap's "
              "goal-set query take");

namespace {

struct RrtGoalsLaunch {
    RrtLaunch a;              // (a.goal, a.g and a.s are not used: the ends are below)
    int G;
    const double *goals;      // [G][n][Q] the caller's
    const int32_t *gcount;    // [Q] the caller's
    double *cfg;              // [n][(1 + G) Qc] column q: the start; column (1 + g) Qc + q: goal g, or the start
    double *da, *db;          // [n][G Qc] column g Qc + q: start -> goal g, NaN if the slot is not counted
    int32_t *gc;              // [Qc] the clamped counts
    int32_t *root_goal;       // [G][Qc] the goal slot of root r
    int32_t *direct;          // [Qc] rule 0's direct goal, or -1
    const uint8_t *cflags;    // [(1 + G) Qc] cfg's flags
    const uint8_t *mflags;    // [G Qc] the direct motions' flags
    int32_t *which;           // [Q] or null
};

__device__ __forceinline__ double start_joint(const RrtGoalsLaunch &p, long long q, int i) {
    return p.cfg[(long long)i * (1 + p.G) * p.a.Qc + q];
}
// (of a counted goal only: the other slots hold NaN)
__device__ __forceinline__ double goal_joint(const RrtGoalsLaunch &p, long long q, int g, int i) {
    return p.db[(long long)i * p.G * p.a.Qc + (long long)g * p.a.Qc + q];
}

__global__ __launch_bounds__(RRT_BLOCK) void rrt_goals_gather_kernel(const RrtGoalsLaunch p) {
    const long long q = (long long)blockIdx.x * RRT_BLOCK + threadIdx.x, Qc = p.a.Qc;
    if (q >= Qc) return;
    const int n = p.a.n, G = p.G;
    const int gc = rrt::clamp_count(p.gcount[p.a.q0 + q], G);
    p.gc[q] = gc;
    for (int i = 0; i < n; ++i) {
        const double s = p.a.start[(long long)i * p.a.Q + p.a.q0 + q];
        double *cfg = p.cfg + (long long)i * (1 + G) * Qc + q;
        double *da = p.da + (long long)i * G * Qc + q, *db = p.db + (long long)i * G * Qc + q;
        cfg[0] = s;
        for (int g = 0; g < G; ++g) {
            const bool counted = g < gc;
            // (a slot that is not counted is not read at all)
            const double v = counted ? p.goals[((long long)g * n + i) * p.a.Q + p.a.q0 + q] : roadmap::nan_value();
            cfg[(long long)(1 + g) * Qc] = counted ? v : s;
            da[(long long)g * Qc] = counted ? s : roadmap::nan_value();
            db[(long long)g * Qc] = v;
        }
    }
}

__global__ __launch_bounds__(RRT_BLOCK) void rrt_goals_begin_kernel(const RrtGoalsLaunch p) {
    const RrtLaunch &a = p.a;
    const long long q = (long long)blockIdx.x * RRT_BLOCK + threadIdx.x, Qc = a.Qc;
    if (q >= Qc) return;
    const int n = a.n, G = p.G, M = a.M, gc = p.gc[q];
    bool ends_finite = true;
    for (int i = 0; i < n; ++i) ends_finite = ends_finite && rrt::finite(start_joint(p, q, i));
    for (int g = 0; g < gc; ++g)
        for (int i = 0; i < n; ++i) ends_finite = ends_finite && rrt::finite(goal_joint(p, q, g, i));
    const bool start_free = p.cflags[q] != 0;
    // the roots in ascending g and, among those whose direct motion is free, the nearest (a tie: the lower g)
    int R = 0, direct = -1;
    double bd = roadmap::inf();
    for (int g = 0; g < gc; ++g) {
        if (p.cflags[(long long)(1 + g) * Qc + q] == 0) continue;
        if (R < G) p.root_goal[(long long)R * Qc + q] = g;
        R += 1;
        if (p.mflags[(long long)g * Qc + q] == 0) continue;
        const double d = motion::motion_distance(n, p.cfg + q, (1 + G) * Qc, p.db + (long long)g * Qc + q, G * Qc);
        if (rrt::direct_better(d, bd, direct)) { bd = d; direct = g; }
    }
    const int state = rrt::begin_goals(ends_finite, gc, start_free, R, direct);
    const bool run = state == rrt::RUNNING;
    if (run) {
        // (R <= G <= M: the call refuses a max_nodes below G)
        double *c0 = tree_conf(a, q, 0), *c1 = tree_conf(a, q, 1);
        int32_t *par1 = tree_parent(a, q, 1);
        for (int i = 0; i < n; ++i) c0[(size_t)i * M] = start_joint(p, q, i);
        for (int r = 0; r < R && r < M; ++r) {
            const int g = p.root_goal[(long long)r * Qc + q];
            for (int i = 0; i < n; ++i) c1[(size_t)i * M + r] = goal_joint(p, q, g, i);
            par1[r] = -1;
        }
        tree_parent(a, q, 0)[0] = -1;
        atomicAdd(a.unfinished, 1);
    }
    a.count[q] = run ? 1 : 0;
    a.count[Qc + q] = run ? (R < M ? R : M) : 0;
    a.state[q] = state;
    p.direct[q] = state == rrt::FOUND ? direct : -1;
    a.junction[q] = -1;
    a.junction[Qc + q] = -1;
    a.used[q] = 0;
    a.pend[q] = -1;
    a.pend[Qc + q] = -1;
    a.pend[2 * Qc + q] = 0;
    for (int i = 0; i < n; ++i) clear_segments(a, q, i);
}

__global__ __launch_bounds__(RRT_WAVE) void rrt_goals_walk_kernel(const RrtGoalsLaunch p) {
    __shared__ int s_way[roadmap::MAX_WAYPOINTS];  // waypoint t: node v of tree 0, or M + v of tree 1
    __shared__ int s_len, s_pad;                   // s_pad: the goal slot the path is padded with, -1 for the start
    const RrtLaunch &a = p.a;
    const long long q = blockIdx.x, qo = a.q0 + q, Qc = a.Qc;
    const int lane = threadIdx.x, n = a.n, M = a.M, G = p.G;
    if (lane == 0) {
        const int state = a.state[q], j0 = a.junction[q], j1 = a.junction[Qc + q];
        const int c0 = a.count[q], c1 = a.count[Qc + q], gc = p.gc[q], direct = p.direct[q];
        int status = state == rrt::RUNNING ? rrt::NO_ROUTE : state, len = 2, which = -1;
        double cost = roadmap::inf();
        if (state == rrt::QUERY_NAN) cost = roadmap::nan_value();
        if (state == rrt::FOUND && !(j0 >= 0 && j0 < c0 && j1 >= 0 && j1 < c1)) {
            if (direct >= 0 && direct < gc) {
                // the direct motion (rule 0)
                cost = 0.0 + motion::motion_distance(n, p.cfg + q, (1 + G) * Qc, p.db + (long long)direct * Qc + q, G * Qc);
                status = rrt::found_status(2, a.Lmax);
                if (status == rrt::FOUND) which = direct;
            } else {
                status = rrt::NO_ROUTE;  // (rule 0 chose no goal and there is no junction: cannot happen)
            }
        } else if (state == rrt::FOUND) {
            const double *conf0 = tree_conf(a, q, 0), *conf1 = tree_conf(a, q, 1);
            int32_t *par0 = tree_parent(a, q, 0);
            const int32_t *par1 = tree_parent(a, q, 1);
            // tree 0's branch, its links turned round: root -> junction
            int prev = -1, v = j0;
            for (int k = 0; k < c0 && v >= 0 && v < c0; ++k) {
                const int up = par0[v];
                par0[v] = prev;
                prev = v;
                v = up;
            }
            int W = 0;
            cost = 0.0;
            v = prev;  // (the root)
            for (int k = 0; k < c0; ++k) {
                if (W < roadmap::MAX_WAYPOINTS) s_way[W] = v;
                W += 1;
                const int down = par0[v];
                if (down < 0 || down >= c0) break;
                cost = cost + motion::motion_distance(n, conf0 + v, M, conf0 + down, M);
                v = down;
            }
            cost = cost + motion::motion_distance(n, conf0 + v, M, conf1 + j1, M);
            v = j1;
            for (int k = 0; k < c1; ++k) {
                if (W < roadmap::MAX_WAYPOINTS) s_way[W] = M + v;
                W += 1;
                const int up = par1[v];
                if (up < 0 || up >= c1) break;
                cost = cost + motion::motion_distance(n, conf1 + v, M, conf1 + up, M);
                v = up;
            }
            // (v is the root the branch ends in: one of the first R <= G nodes)
            const int g = v >= 0 && v < G ? p.root_goal[(long long)v * Qc + q] : -1;
            status = g >= 0 && g < gc ? rrt::found_status(W, a.Lmax) : rrt::NO_ROUTE;
            if (status == rrt::FOUND) {
                len = W;
                which = g;
            }
            if (status == rrt::NO_ROUTE) cost = roadmap::inf();
        }
        s_len = len;
        s_pad = status == rrt::FOUND ? which : (gc > 0 ? 0 : -1);
        if (a.len) a.len[qo] = len;
        if (a.cost) a.cost[qo] = cost;
        if (a.status) a.status[qo] = status;
        if (a.iters) a.iters[qo] = a.used[q];
        if (a.nodes) {
            a.nodes[qo] = c0;
            a.nodes[a.Q + qo] = c1;
        }
        if (p.which) p.which[qo] = which;
    }
    __syncthreads();
    if (!a.path) return;
    const int len = s_len, pad = s_pad;
    const double *conf = tree_conf(a, q, 0);  // (tree 1 follows tree 0: node M + v)
    for (int e = lane; e < a.Lmax * n; e += RRT_WAVE) {
        const int t = e / n, i = e % n;
        double v = pad >= 0 ? goal_joint(p, q, pad, i) : start_joint(p, q, i);
        if (t == 0) v = start_joint(p, q, i);
        else if (t < len - 1) {
            const int w = s_way[t];
            v = conf[(size_t)(w / M) * n * M + (size_t)i * M + (w % M)];
        }
        a.path[((long long)t * a.Q + qo) * n + i] = v;
    }
}

}  // namespace

extern "C" {

int optik_hip_rrt_plan_goals(optik_hip_chain *ch, const double *ee_offset7, const double *d_start,
                             const double *d_goals, const int32_t *d_gcount, int64_t Q, int32_t G, int32_t iters,
                             double step, double resolution, uint64_t first, int32_t max_nodes, int32_t Lmax,
                             int32_t poll, double *d_path, int32_t *d_len, double *d_cost, int32_t *d_status,
                             int32_t *d_iters, int32_t *d_nodes, int32_t *d_which, void *stream_) {
    if (G < 1 || G > rrt::MAX_GOALS)
        return fail(OPTIK_HIP_EINVAL, "rrt_plan_goals: G must be in 1 .. " + std::to_string(rrt::MAX_GOALS)
                                          + " goals per query");
    if (max_nodes < rrt::min_nodes(G) || max_nodes > rrt::MAX_NODES)
        return fail(OPTIK_HIP_EINVAL, "rrt_plan_goals: max_nodes must be in max(2, G) .. "
                                          + std::to_string(rrt::MAX_NODES) + ": every goal may be a root");
    if (int rc = check_args(ch, Q, iters, step, resolution, max_nodes, Lmax, poll)) return rc;
    if (ch->n < 1 || ch->n > OPTIK_HIP_MAX_DOF)
        return fail(OPTIK_HIP_EUNSUPPORTED, "rrt_plan_goals: chains of 1 .. 16 joint positions");
    if (Q == 0 || (!d_path && !d_len && !d_cost && !d_status && !d_iters && !d_nodes && !d_which)) return 0;
    if (!d_start || !d_goals || !d_gcount) return fail(OPTIK_HIP_EINVAL, "bad argument");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t n = (size_t)ch->n, M = (size_t)max_nodes, I = (size_t)iters, uG = (size_t)G;
    // (the trees are optik_hip_rrt_plan's, so is the chunk)
    const size_t Qc = (size_t)std::min<int64_t>(Q, optik_hip_rrt_chunk(ch, max_nodes));
    const size_t o_samples = 16, o_cfg = o_samples + align16(8 * n * I), o_da = o_cfg + align16(8 * n * (1 + uG) * Qc),
                 o_db = o_da + align16(8 * n * uG * Qc), o_qa = o_db + align16(8 * n * uG * Qc),
                 o_qb = o_qa + align16(8 * n * 3 * Qc), o_flags = o_qb + align16(8 * n * 3 * Qc),
                 o_count = o_flags + align16((1 + 2 * uG) * Qc + 3 * Qc), o_state = o_count + align16(4 * 2 * Qc),
                 o_junction = o_state + align16(4 * Qc), o_used = o_junction + align16(4 * 2 * Qc),
                 o_pend = o_used + align16(4 * Qc), o_gc = o_pend + align16(4 * 3 * Qc), o_direct = o_gc + align16(4 * Qc),
                 o_root = o_direct + align16(4 * Qc), o_parent = o_root + align16(4 * uG * Qc),
                 o_conf = o_parent + align16(4 * 2 * M * Qc), bytes = o_conf + 8 * 2 * n * M * Qc;
    unsigned char *ws = nullptr;
    {
        std::lock_guard<std::mutex> lock(ch->mu);
        BIND_DEVICE(ch);
        HIP_TRY(ch->rrt_ws.reserve(bytes));
        ws = ch->rrt_ws.get();
    }
    RrtGoalsLaunch p;
    std::memset(&p, 0, sizeof p);
    RrtLaunch &a = p.a;
    a.Q = Q; a.n = ch->n; a.M = max_nodes; a.Lmax = Lmax; a.I = iters; a.eta = step;
    a.start = d_start;
    a.lo = ch->wide ? ch->wdev->lb : ch->dev->lb;
    a.hi = ch->wide ? ch->wdev->ub : ch->dev->ub;
    a.unfinished = reinterpret_cast<int32_t *>(ws);
    a.samples = reinterpret_cast<double *>(ws + o_samples);
    a.qa = reinterpret_cast<double *>(ws + o_qa);
    a.count = reinterpret_cast<int32_t *>(ws + o_count);
    a.state = reinterpret_cast<int32_t *>(ws + o_state);
    a.junction = reinterpret_cast<int32_t *>(ws + o_junction);
    a.used = reinterpret_cast<int32_t *>(ws + o_used);
    a.pend = reinterpret_cast<int32_t *>(ws + o_pend);
    a.parent = reinterpret_cast<int32_t *>(ws + o_parent);
    a.conf = reinterpret_cast<double *>(ws + o_conf);
    a.path = d_path; a.len = d_len; a.cost = d_cost; a.status = d_status; a.iters = d_iters; a.nodes = d_nodes;
    p.G = G; p.goals = d_goals; p.gcount = d_gcount; p.which = d_which;
    p.cfg = reinterpret_cast<double *>(ws + o_cfg);
    p.da = reinterpret_cast<double *>(ws + o_da);
    p.db = reinterpret_cast<double *>(ws + o_db);
    p.gc = reinterpret_cast<int32_t *>(ws + o_gc);
    p.direct = reinterpret_cast<int32_t *>(ws + o_direct);
    p.root_goal = reinterpret_cast<int32_t *>(ws + o_root);
    // (the iterations' three flags per query, then rule 0's 1 + 2 G)
    uint8_t *d_flags = ws + o_flags, *d_cflags = d_flags + 3 * Qc;
    a.flags = d_flags;
    if (int rc = optik_hip_seed_batch(ch, first, iters, const_cast<double *>(a.samples), stream)) return rc;
    for (int64_t q0 = 0; q0 < Q; q0 += (int64_t)Qc) {
        const long long L = std::min<int64_t>((int64_t)Qc, Q - q0);
        a.q0 = q0; a.Qc = L;
        // (a chunk's arrays are [..][L]: the offsets above leave room for Qc >= L)
        a.qb = a.qa + n * 3 * (size_t)L;
        p.cflags = d_cflags;
        p.mflags = d_cflags + (1 + uG) * (size_t)L;
        {
            BIND_DEVICE(ch);
            HIP_TRY(hipMemsetAsync(a.unfinished, 0, sizeof(int32_t), stream));
            hipLaunchKernelGGL(rrt_goals_gather_kernel, dim3(blocks(L)), dim3(RRT_BLOCK), 0, stream, p);
            HIP_TRY(hipGetLastError());
        }
        if (int rc = optik_hip_collision_batch(ch, ee_offset7, p.cfg, (1 + G) * L, nullptr, d_cflags, stream)) return rc;
        if (int rc = optik_hip_collision_motion_batch(ch, ee_offset7, p.da, p.db, G * L, resolution, nullptr,
                                                      d_cflags + (1 + uG) * (size_t)L, nullptr, nullptr, stream))
            return rc;
        {
            BIND_DEVICE(ch);
            hipLaunchKernelGGL(rrt_goals_begin_kernel, dim3(blocks(L)), dim3(RRT_BLOCK), 0, stream, p);
            HIP_TRY(hipGetLastError());
        }
        if (int rc = run_iterations(ch, ee_offset7, a, iters, poll, resolution, d_flags, stream)) return rc;
        BIND_DEVICE(ch);
        hipLaunchKernelGGL(rrt_goals_walk_kernel, dim3((unsigned)L), dim3(RRT_WAVE), 0, stream, p);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
