// ik_rrt.hip -- the bidirectional tree planner on the device (rrt_measure.hpp: the rules and their operation order;
// DESIGN.md section 5.26): for the queries a roadmap misses, two trees per query grown from the query's own start and
// goal.  optik_hip_rrt_plan (include/optik_hip.h).
//
//   rrt_gather_kernel   one thread per query of the chunk: its start and goal into the workspace, [n][Qc], as the
//                       collision and motion checks take their configurations
//   (optik_hip_collision_batch on both, optik_hip_collision_motion_batch on start -> goal, same stream)
//   rrt_begin_kernel    one thread per query: rule 0, the two roots, and the count of the queries that go on
//   rrt_step_kernel     one wave per query, both trees in turn (the nearest node of tree b is the nearest to the
//                       candidate that the search in tree a gives, so the two searches of a query cannot overlap).
//                       First it commits the iteration before from the motion check's free flags (append, junction,
//                       freeze), then it runs rules 1 to 4 of this iteration: lanes stride over the nodes of a tree,
//                       [n][M] per (query, tree) so that a wave reads consecutive doubles, each lane keeps its best
//                       (distance, index), and a butterfly of __shfl_xor (ik_argmin.hpp's idiom, with the total order
//                       of rrt::nearer) leaves the winner in every lane.  Lane j < n then steers joint j and writes
//                       the iteration's three segments in travel direction: p - c, c - m and m - e.  A query that is
//                       frozen, and a segment that the rules do not ask for, is NaN: the motion check answers it
//                       "not sampled" without reading a model.
//   (optik_hip_collision_motion_batch, classify form, on the same stream: the motion check's own code, 3 Qc segments)
//   rrt_walk_kernel     one wave per query: lane 0 reverses the parent links of tree 0's branch in place (the trees are
//                       scratch by then), walks start -> junction -> goal adding the cost forwards, and the wave
//                       writes the path.
//
// Two launches of this unit's own per iteration would be one too many: the commit of iteration i and the search of
// iteration i + 1 are one kernel, so an iteration is that kernel and the motion check's five.  No kernel waits for
// another workgroup; every loop's trip count is bounded by a tree's size, n or Lmax.  The loop over the iterations
// runs on the host; every `poll` iterations it reads one int32, the count of the queries that have not ended.
// The launch record and that loop (rrtdev::run_iterations, defined here) are declared in rrt_device.hpp:
// ik_rrt_goals.hip runs the same loop, and so rrt_step_kernel as it is, on trees with several goal roots.
#include <algorithm>

#include "rrt_device.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::colldev;
using namespace optik::rrtdev;

static_assert(rrt::MAX_NODES == OPTIK_HIP_RRT_MAX_NODES && rrt::MAX_ITERS == OPTIK_HIP_RRT_MAX_ITERS
                  && rrt::MAX_POLL == OPTIK_HIP_RRT_MAX_POLL
                  && roadmap::MAX_WAYPOINTS == OPTIK_HIP_PATH_OPTIMIZE_MAX_WAYPOINTS,
              "optik_hip.h states the caps of rrt_measure.hpp; a plan is a path path_optimize takes");

namespace {

// (the launch record RrtLaunch, tree_conf, tree_parent and clear_segments: rrt_device.hpp)

__global__ __launch_bounds__(RRT_BLOCK) void rrt_gather_kernel(const RrtLaunch a) {
    const long long q = (long long)blockIdx.x * RRT_BLOCK + threadIdx.x;
    if (q >= a.Qc) return;
    for (int i = 0; i < a.n; ++i) {
        a.s[(long long)i * a.Qc + q] = a.start[(long long)i * a.Q + a.q0 + q];
        a.g[(long long)i * a.Qc + q] = a.goal[(long long)i * a.Q + a.q0 + q];
    }
}

__global__ __launch_bounds__(RRT_BLOCK) void rrt_begin_kernel(const RrtLaunch a) {
    const long long q = (long long)blockIdx.x * RRT_BLOCK + threadIdx.x;
    if (q >= a.Qc) return;
    bool ends_finite = true;
    for (int i = 0; i < a.n; ++i)
        ends_finite = ends_finite && rrt::finite(a.s[(long long)i * a.Qc + q]) && rrt::finite(a.g[(long long)i * a.Qc + q]);
    const int state = rrt::begin(ends_finite, a.flags[q] != 0, a.flags[a.Qc + q] != 0, a.flags[2 * a.Qc + q] != 0);
    const bool run = state == rrt::RUNNING;
    if (run) {
        double *c0 = tree_conf(a, q, 0), *c1 = tree_conf(a, q, 1);
        for (int i = 0; i < a.n; ++i) {
            c0[(size_t)i * a.M] = a.s[(long long)i * a.Qc + q];
            c1[(size_t)i * a.M] = a.g[(long long)i * a.Qc + q];
        }
        tree_parent(a, q, 0)[0] = -1;
        tree_parent(a, q, 1)[0] = -1;
        atomicAdd(a.unfinished, 1);
    }
    a.count[q] = run ? 1 : 0;
    a.count[a.Qc + q] = run ? 1 : 0;
    a.state[q] = state;
    a.junction[q] = -1;
    a.junction[a.Qc + q] = -1;
    a.used[q] = 0;
    a.pend[q] = -1;
    a.pend[a.Qc + q] = -1;
    a.pend[2 * a.Qc + q] = 0;
    for (int i = 0; i < a.n; ++i) clear_segments(a, q, i);
}

// Rule 1 over one tree: every lane ends with the winner.  conf [n][M], x in LDS.
__device__ __forceinline__ void wave_nearest(const double *conf, int n, int M, int count, const double *s_x, int lane,
                                             double &dist, int &index) {
    double bd = roadmap::inf();
    int bi = -1;
    for (int j = lane; j < count; j += RRT_WAVE) {
        double d = 0.0;
        for (int i = 0; i < n; ++i) d = motion::distance_take(d, fabs(s_x[i] - conf[(size_t)i * M + j]));
        if (rrt::nearer(d, j, bd, bi)) { bd = d; bi = j; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double od = __shfl_xor(bd, off, RRT_WAVE);
        const int oi = __shfl_xor(bi, off, RRT_WAVE);
        if (oi >= 0 && rrt::nearer(od, oi, bd, bi)) { bd = od; bi = oi; }
    }
    dist = bd;
    index = bi;
}

__global__ __launch_bounds__(RRT_WAVE) void rrt_step_kernel(const RrtLaunch a) {
    __shared__ double s_x[OPTIK_HIP_MAX_DOF], s_c[OPTIK_HIP_MAX_DOF];
    const long long q = blockIdx.x;
    const int lane = threadIdx.x, n = a.n, M = a.M;
    if (a.state[q] != rrt::RUNNING) return;  // (frozen: its segments are NaN already)
    const long long B = 3 * a.Qc;
    int cnt0 = a.count[q], cnt1 = a.count[a.Qc + q];
    const bool joint = lane < n;
    // ---- the iteration before: what the motion check said (rules 3 and 4) ----
    if (a.iter > 0) {
        const int pa = (a.iter - 1) & 1, pb = 1 - pa;
        const int p = a.pend[q], m = a.pend[a.Qc + q], back = a.pend[2 * a.Qc + q];
        const bool ok0 = a.flags[q] != 0, ok1 = a.flags[a.Qc + q] != 0, ok2 = a.flags[2 * a.Qc + q] != 0;
        int cnt_a = pa == 0 ? cnt0 : cnt1, cnt_b = pa == 0 ? cnt1 : cnt0;
        if (p >= 0 && p < cnt_a && m >= 0 && m < cnt_b && cnt_a < M && ok0) {
            // (segment 0 is p -> c for tree 0 and c -> p for tree 1)
            if (joint) {
                const double c = (pa == 0 ? a.qb : a.qa)[(long long)lane * B + q];
                tree_conf(a, q, pa)[(size_t)lane * M + cnt_a] = c;
            }
            if (lane == 0) tree_parent(a, q, pa)[cnt_a] = p;
            cnt_a += 1;
            if (ok1) {
                if (lane == 0) {
                    a.junction[pa * a.Qc + q] = cnt_a - 1;
                    a.junction[pb * a.Qc + q] = m;
                    a.count[pa * a.Qc + q] = cnt_a;
                    a.state[q] = rrt::FOUND;
                    a.used[q] = a.iter;
                    atomicSub(a.unfinished, 1);
                }
                if (joint) clear_segments(a, q, lane);
                return;
            }
            if (back && ok2 && cnt_b < M) {
                // (segment 2 is m -> e for tree 0 and e -> m for tree 1)
                if (joint) {
                    const double e = (pb == 0 ? a.qb : a.qa)[(long long)lane * B + 2 * a.Qc + q];
                    tree_conf(a, q, pb)[(size_t)lane * M + cnt_b] = e;
                }
                if (lane == 0) tree_parent(a, q, pb)[cnt_b] = m;
                cnt_b += 1;
            }
            cnt0 = pa == 0 ? cnt_a : cnt_b;
            cnt1 = pa == 0 ? cnt_b : cnt_a;
            if (lane == 0) {
                a.count[q] = cnt0;
                a.count[a.Qc + q] = cnt1;
            }
        }
    }
    if (a.iter >= a.I) {
        // rule 6
        if (lane == 0) {
            a.state[q] = rrt::NO_ROUTE;
            a.used[q] = a.I;
            atomicSub(a.unfinished, 1);
        }
        if (joint) clear_segments(a, q, lane);
        return;
    }
    // ---- this iteration: rules 1 to 4 ----
    const int ta = a.iter & 1, tb = 1 - ta;
    const int cnt_a = ta == 0 ? cnt0 : cnt1, cnt_b = ta == 0 ? cnt1 : cnt0;
    const double *conf_a = tree_conf(a, q, ta), *conf_b = tree_conf(a, q, tb);
    if (joint) s_x[lane] = a.samples[(long long)lane * a.I + a.iter];
    __syncthreads();  // (also: the nodes appended above are visible to every lane)
    double d, dm;
    int p, m;
    wave_nearest(conf_a, n, M, cnt_a, s_x, lane, d, p);
    if (!rrt::steers(d) || cnt_a >= M || p < 0) {
        if (lane == 0) a.pend[q] = -1;
        if (joint) clear_segments(a, q, lane);
        return;
    }
    double pj = 0.0, cj = 0.0, lo = 0.0, hi = 0.0;
    if (joint) {
        pj = conf_a[(size_t)lane * M + p];
        lo = a.lo[lane];
        hi = a.hi[lane];
        cj = rrt::steer_joint(pj, s_x[lane], d, a.eta, lo, hi);
        s_c[lane] = cj;
    }
    __syncthreads();
    wave_nearest(conf_b, n, M, cnt_b, s_c, lane, dm, m);
    if (m < 0) {  // (a tree has its root: cannot happen)
        if (lane == 0) a.pend[q] = -1;
        if (joint) clear_segments(a, q, lane);
        return;
    }
    const bool back = rrt::extends_back(dm, a.eta, cnt_b, M);
    if (joint) {
        const double mj = conf_b[(size_t)lane * M + m];
        const double ej = back ? rrt::steer_joint(mj, cj, dm, a.eta, lo, hi) : roadmap::nan_value();
        const double mb = back ? mj : roadmap::nan_value();
        double *qa = a.qa + (long long)lane * B + q, *qb = a.qb + (long long)lane * B + q;
        // travel direction: tree 0 is walked parent -> child, tree 1 child -> parent, a connection tree 0 -> tree 1
        qa[0] = ta == 0 ? pj : cj;
        qb[0] = ta == 0 ? cj : pj;
        qa[a.Qc] = ta == 0 ? cj : mj;
        qb[a.Qc] = ta == 0 ? mj : cj;
        qa[2 * a.Qc] = tb == 0 ? mb : ej;
        qb[2 * a.Qc] = tb == 0 ? ej : mb;
    }
    if (lane == 0) {
        a.pend[q] = p;
        a.pend[a.Qc + q] = m;
        a.pend[2 * a.Qc + q] = back ? 1 : 0;
    }
}

__global__ __launch_bounds__(RRT_WAVE) void rrt_walk_kernel(const RrtLaunch a) {
    __shared__ int s_way[roadmap::MAX_WAYPOINTS];  // waypoint t: node v of tree 0, or M + v of tree 1
    __shared__ int s_len;
    const long long q = blockIdx.x, qo = a.q0 + q;
    const int lane = threadIdx.x, n = a.n, M = a.M;
    if (lane == 0) {
        const int state = a.state[q], j0 = a.junction[q], j1 = a.junction[a.Qc + q];
        const int c0 = a.count[q], c1 = a.count[a.Qc + q];
        int status = state == rrt::RUNNING ? rrt::NO_ROUTE : state, len = 2;
        double cost = roadmap::inf();
        if (state == rrt::QUERY_NAN) cost = roadmap::nan_value();
        if (state == rrt::FOUND && !(j0 >= 0 && j0 < c0 && j1 >= 0 && j1 < c1)) {
            // the direct motion (rule 0)
            cost = 0.0 + motion::motion_distance(n, a.s + q, a.Qc, a.g + q, a.Qc);
            status = rrt::found_status(2, a.Lmax);
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
            status = rrt::found_status(W, a.Lmax);
            if (status == rrt::FOUND) len = W;
        }
        s_len = len;
        if (a.len) a.len[qo] = len;
        if (a.cost) a.cost[qo] = cost;
        if (a.status) a.status[qo] = status;
        if (a.iters) a.iters[qo] = a.used[q];
        if (a.nodes) {
            a.nodes[qo] = c0;
            a.nodes[a.Q + qo] = c1;
        }
    }
    __syncthreads();
    if (!a.path) return;
    const int len = s_len;
    const double *conf = tree_conf(a, q, 0);  // (tree 1 follows tree 0: node M + v)
    for (int e = lane; e < a.Lmax * n; e += RRT_WAVE) {
        const int t = e / n, i = e % n;
        double v = a.g[(long long)i * a.Qc + q];
        if (t == 0) v = a.s[(long long)i * a.Qc + q];
        else if (t < len - 1) {
            const int w = s_way[t];
            v = conf[(size_t)(w / M) * n * M + (size_t)i * M + (w % M)];
        }
        a.path[((long long)t * a.Q + qo) * n + i] = v;
    }
}

}  // namespace

namespace optik {
namespace rrtdev {

int check_args(const optik_hip_chain *ch, int64_t Q, int32_t iters, double step, double resolution, int32_t max_nodes,
               int32_t Lmax, int32_t poll) {
    if (!ch || Q < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (Q > MAX_QUERIES) return fail(OPTIK_HIP_EINVAL, "rrt_plan: more than 2^30 queries in one launch");
    if (iters < 1 || iters > rrt::MAX_ITERS)
        return fail(OPTIK_HIP_EINVAL, "rrt_plan: iters must be in 1 .. " + std::to_string(rrt::MAX_ITERS));
    if (!(step > 0.0) || !std::isfinite(step)) return fail(OPTIK_HIP_EINVAL, "rrt_plan: step must be finite and > 0");
    if (max_nodes < rrt::MIN_NODES || max_nodes > rrt::MAX_NODES)
        return fail(OPTIK_HIP_EINVAL, "rrt_plan: max_nodes must be in 2 .. " + std::to_string(rrt::MAX_NODES));
    if (Lmax < roadmap::MIN_WAYPOINTS || Lmax > roadmap::MAX_WAYPOINTS)
        return fail(OPTIK_HIP_EINVAL, "rrt_plan: a path has 2 .. 64 waypoints");
    if (poll < 1 || poll > rrt::MAX_POLL)
        return fail(OPTIK_HIP_EINVAL, "rrt_plan: poll must be in 1 .. " + std::to_string(rrt::MAX_POLL));
    // (B = 0: the motion check's own refusals -- the resolution, prismatic joints)
    return optik_hip_collision_motion_batch(const_cast<optik_hip_chain *>(ch), nullptr, nullptr, nullptr, 0, resolution,
                                            nullptr, nullptr, nullptr, nullptr, nullptr);
}

int run_iterations(optik_hip_chain *ch, const double *ee_offset7, RrtLaunch &a, int32_t iters, int32_t poll,
                   double resolution, uint8_t *d_flags, hipStream_t stream) {
    const long long L = a.Qc;
    bool ended = false;
    for (int32_t i = 0; i < iters; ++i) {
        a.iter = i;
        {
            BIND_DEVICE(ch);
            hipLaunchKernelGGL(rrt_step_kernel, dim3((unsigned)L), dim3(RRT_WAVE), 0, stream, a);
            HIP_TRY(hipGetLastError());
            if (i % poll == 0) {
                // (the one synchronise of a poll: the host decides whether the iterations go on)
                int32_t left = 0;
                HIP_TRY(hipMemcpyAsync(&left, a.unfinished, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
                HIP_TRY(hipStreamSynchronize(stream));
                if (left <= 0) { ended = true; break; }
            }
        }
        if (int rc = optik_hip_collision_motion_batch(ch, ee_offset7, a.qa, a.qb, 3 * L, resolution, nullptr, d_flags,
                                                      nullptr, nullptr, stream))
            return rc;
    }
    BIND_DEVICE(ch);
    if (!ended) {
        a.iter = iters;  // (the last iteration's commit, and rule 6)
        hipLaunchKernelGGL(rrt_step_kernel, dim3((unsigned)L), dim3(RRT_WAVE), 0, stream, a);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace rrtdev
}  // namespace optik

extern "C" {

int64_t optik_hip_rrt_chunk(const optik_hip_chain *ch, int32_t max_nodes) {
    if (!ch || max_nodes < 1) return 0;
    const int64_t per = 2 * (int64_t)max_nodes * (8 * (int64_t)ch->n + 4);
    return std::max<int64_t>(1, OPTIK_HIP_RRT_CHUNK_BYTES / per);
}

int optik_hip_rrt_plan(optik_hip_chain *ch, const double *ee_offset7, const double *d_start, const double *d_goal,
                       int64_t Q, int32_t iters, double step, double resolution, uint64_t first, int32_t max_nodes,
                       int32_t Lmax, int32_t poll, double *d_path, int32_t *d_len, double *d_cost, int32_t *d_status,
                       int32_t *d_iters, int32_t *d_nodes, void *stream_) {
    if (int rc = check_args(ch, Q, iters, step, resolution, max_nodes, Lmax, poll)) return rc;
    if (ch->n < 1 || ch->n > OPTIK_HIP_MAX_DOF)
        return fail(OPTIK_HIP_EUNSUPPORTED, "rrt_plan: chains of 1 .. 16 joint positions");
    if (Q == 0 || (!d_path && !d_len && !d_cost && !d_status && !d_iters && !d_nodes)) return 0;
    if (!d_start || !d_goal) return fail(OPTIK_HIP_EINVAL, "bad argument");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t n = (size_t)ch->n, M = (size_t)max_nodes, I = (size_t)iters;
    const size_t Qc = (size_t)std::min<int64_t>(Q, optik_hip_rrt_chunk(ch, max_nodes));
    const size_t o_samples = 16, o_s = o_samples + align16(8 * n * I), o_g = o_s + align16(8 * n * Qc),
                 o_qa = o_g + align16(8 * n * Qc), o_qb = o_qa + align16(8 * n * 3 * Qc),
                 o_flags = o_qb + align16(8 * n * 3 * Qc), o_count = o_flags + align16(3 * Qc),
                 o_state = o_count + align16(4 * 2 * Qc), o_junction = o_state + align16(4 * Qc),
                 o_used = o_junction + align16(4 * 2 * Qc), o_pend = o_used + align16(4 * Qc),
                 o_parent = o_pend + align16(4 * 3 * Qc), o_conf = o_parent + align16(4 * 2 * M * Qc),
                 bytes = o_conf + 8 * 2 * n * M * Qc;
    unsigned char *ws = nullptr;
    {
        std::lock_guard<std::mutex> lock(ch->mu);
        BIND_DEVICE(ch);
        HIP_TRY(ch->rrt_ws.reserve(bytes));
        ws = ch->rrt_ws.get();
    }
    RrtLaunch a;
    std::memset(&a, 0, sizeof a);
    a.Q = Q; a.n = ch->n; a.M = max_nodes; a.Lmax = Lmax; a.I = iters; a.eta = step;
    a.start = d_start; a.goal = d_goal;
    a.lo = ch->wide ? ch->wdev->lb : ch->dev->lb;
    a.hi = ch->wide ? ch->wdev->ub : ch->dev->ub;
    a.unfinished = reinterpret_cast<int32_t *>(ws);
    a.samples = reinterpret_cast<double *>(ws + o_samples);
    a.s = reinterpret_cast<double *>(ws + o_s);
    a.g = reinterpret_cast<double *>(ws + o_g);
    a.qa = reinterpret_cast<double *>(ws + o_qa);
    a.qb = reinterpret_cast<double *>(ws + o_qb);
    a.flags = ws + o_flags;
    a.count = reinterpret_cast<int32_t *>(ws + o_count);
    a.state = reinterpret_cast<int32_t *>(ws + o_state);
    a.junction = reinterpret_cast<int32_t *>(ws + o_junction);
    a.used = reinterpret_cast<int32_t *>(ws + o_used);
    a.pend = reinterpret_cast<int32_t *>(ws + o_pend);
    a.parent = reinterpret_cast<int32_t *>(ws + o_parent);
    a.conf = reinterpret_cast<double *>(ws + o_conf);
    a.path = d_path; a.len = d_len; a.cost = d_cost; a.status = d_status; a.iters = d_iters; a.nodes = d_nodes;
    uint8_t *d_flags = ws + o_flags;
    // (the samples of the whole call: iteration i reads restart seed first + i, whatever the query)
    if (int rc = optik_hip_seed_batch(ch, first, iters, const_cast<double *>(a.samples), stream)) return rc;
    for (int64_t q0 = 0; q0 < Q; q0 += (int64_t)Qc) {
        const long long L = std::min<int64_t>((int64_t)Qc, Q - q0);
        a.q0 = q0; a.Qc = L;
        // (a chunk's arrays are [..][L]: the offsets above leave room for Qc >= L)
        a.qb = a.qa + n * 3 * (size_t)L;
        {
            BIND_DEVICE(ch);
            HIP_TRY(hipMemsetAsync(a.unfinished, 0, sizeof(int32_t), stream));
            hipLaunchKernelGGL(rrt_gather_kernel, dim3(blocks(L)), dim3(RRT_BLOCK), 0, stream, a);
            HIP_TRY(hipGetLastError());
        }
        if (int rc = optik_hip_collision_batch(ch, ee_offset7, a.s, L, nullptr, d_flags, stream)) return rc;
        if (int rc = optik_hip_collision_batch(ch, ee_offset7, a.g, L, nullptr, d_flags + L, stream)) return rc;
        if (int rc = optik_hip_collision_motion_batch(ch, ee_offset7, a.s, a.g, L, resolution, nullptr, d_flags + 2 * L,
                                                      nullptr, nullptr, stream))
            return rc;
        {
            BIND_DEVICE(ch);
            hipLaunchKernelGGL(rrt_begin_kernel, dim3(blocks(L)), dim3(RRT_BLOCK), 0, stream, a);
            HIP_TRY(hipGetLastError());
        }
        if (int rc = run_iterations(ch, ee_offset7, a, iters, poll, resolution, d_flags, stream)) return rc;
        BIND_DEVICE(ch);
        hipLaunchKernelGGL(rrt_walk_kernel, dim3((unsigned)L), dim3(RRT_WAVE), 0, stream, a);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
