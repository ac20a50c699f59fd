// ik_rrt.hip -- the bidirectional tree planner on the device (rrt_measure.hpp and rrt_goals_measure.hpp: the rules and
// their operation order; DESIGN.md sections 5.26 and 5.28): for the queries a roadmap misses, two trees per query,
// tree 0 grown from the query's start and tree 1 from one root per counted goal that is free; the query ends at the
// first junction with any of them.  One set of kernels and one planner body (plan): optik_hip_rrt_plan_goals calls
// it, and optik_hip_rrt_plan is its call with G = 1 and every slot counted -- [G][n][Q] with G = 1 is [n][Q], and the
// rules of rrt_goals_measure.hpp with one counted goal are rrt_measure.hpp's bit for bit (include/optik_hip.h).
//
//   rrt_gather_kernel   one thread per query of the chunk: its clamped goal count (no counts: G); the 1 + G
//                       configurations that rule 0 classifies, [n][(1 + G) Qc] -- the start, then per slot the goal if it
//                       is counted and the start again if it is not --; and the G direct motions in travel direction,
//                       start -> goal g, [n][G Qc] twice -- NaN on both ends for a slot that is not counted, which the
//                       motion check answers "not sampled" without reading a model.  The second of the two arrays is
//                       where the later kernels read a counted goal from.
//   (optik_hip_collision_batch on the 1 + G columns, optik_hip_collision_motion_batch on the G segments, same stream)
//   rrt_begin_kernel    one thread per query: rule 0 -- the roots of tree 1 in ascending g with the root -> goal table,
//                       the nearest free direct motion --, and the count of the queries that go on.  Only the flags of
//                       counted slots are read.
//   rrt_step_kernel     (rrt_step_body without a constraint) one wave per query, both trees in turn (the nearest node of tree b is the nearest to the
//                       candidate that the search in tree a gives, so the two searches of a query cannot overlap).
//                       First it commits the iteration before from the motion check's free flags (append, junction,
//                       freeze), then it runs rules 1 to 4 of this iteration: lanes stride over the nodes of a tree,
//                       [n][M] per (query, tree) so that a wave reads consecutive doubles, each lane keeps its best
//                       (distance, index), and a butterfly of __shfl_xor (ik_argmin.hpp's idiom, with the total order
//                       of rrt::nearer) leaves the winner in every lane.  Lane j < n then steers joint j and writes
//                       the iteration's three segments in travel direction: p - c, c - m and m - e.  A query that is
//                       frozen, and a segment that the rules do not ask for, is NaN: the motion check answers it
//                       "not sampled" without reading a model.  It needs no rule for the goal set: a tree 1 with R
//                       roots is a tree with R nodes to it.
//   (optik_hip_collision_motion_batch, classify form, on the same stream: the motion check's own code, 3 Qc segments)
//   rrt_walk_kernel     one wave per query: lane 0 reverses the parent links of tree 0's branch in place (the trees are
//                       scratch by then), walks start -> junction -> root adding the cost forwards, and the wave
//                       writes the path; the goal slot of the root that tree 1's branch ends in is `which`, and the
//                       path is padded with that goal.
//   rrt_nearest_kernel  (a test hook, optik_hip_rrt_nearest_from_nodes) one wave per query point: wave_nearest and
//                       rrt::steer_joint, the two functions of rrt_step_body, on a tree the caller wrote.
//
// Under a pose constraint (rrt_constrained_measure.hpp; optik_hip_rrt_plan_constrained) the
// same planner body runs with a constraint record (RrtConstraint), which swaps one kernel and adds two:
//   rrt_mask_kernel     one thread per flag of rule 0: a configuration's collision flag is cleared where its violation
//                       (optik_hip_constraint_batch on the same 1 + G columns) is not <= tol, a direct motion's where
//                       optik_hip_constraint_motion_batch's ok byte is 0.  gather and begin stay as they are.
//   rrt_cstep_kernel<CH>  rrt_step_body with the projection inside -- the one body of both step kernels, the constraint's
//                       parts under `if constexpr`, so the commit, rule 6 and the segment write exist once.  CH is
//                       ChainDev or WideChainDev, the chain table staged in LDS (copy_table, ik_launch.hpp; the record's
//                       head and the dispatch on CH are constraint_device.hpp's).  The commit counts a segment only if
//                       the motion check's flag AND constraint_motion's ok byte are set.  After the steer lane 0 runs
//                       constraint::project on the candidate in LDS -- the header's own function, no barrier inside --
//                       and leaves the verdict (rrt::takes) in LDS; every lane reads it after the barrier, so every
//                       early exit stays wave-uniform.  The second search runs against the projected candidate, the
//                       back-extension is projected the same way, and the two counters of d_projected are bumped by
//                       lane 0 (one wave per query and one kernel after the other: no atomics).
//   (optik_hip_constraint_motion_batch after the motion check, on the same 3 Qc segments: seven launches an iteration)
//
// Two launches of this unit's own per iteration would be one too many: the commit of iteration i and the search of
// iteration i + 1 are one kernel, so an iteration is that kernel and the motion check's five.  No kernel waits for
// another workgroup; every loop's trip count is bounded by a tree's size, n, G or Lmax; no private array is indexed
// dynamically; the atomics are vector atomics on the count of running queries, the begin kernel's atomicAdd and the
// atomicSub of a query that ends in rrt_step_kernel.  The loop over the iterations runs on the host (run_iterations);
// every `poll` iterations it reads one int32, the count of the queries that have not ended.
#include <algorithm>
#include <type_traits>

#include "constraint_device.hpp"
#include "rrt_constrained_measure.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::hostparams;
using namespace optik::colldev;
using namespace optik::condev;

static_assert(rrt::MAX_NODES == OPTIK_HIP_RRT_MAX_NODES && rrt::MAX_ITERS == OPTIK_HIP_RRT_MAX_ITERS
                  && rrt::MAX_POLL == OPTIK_HIP_RRT_MAX_POLL
                  && roadmap::MAX_WAYPOINTS == OPTIK_HIP_PATH_OPTIMIZE_MAX_WAYPOINTS,
              "optik_hip.h states the caps of rrt_measure.hpp; a plan is a path path_optimize takes");
static_assert(rrt::MAX_GOALS == OPTIK_HIP_RRT_MAX_GOALS && OPTIK_HIP_RRT_MAX_GOALS == OPTIK_HIP_ROADMAP_MAX_GOALS,
              "optik_hip.h states the cap of rrt_goals_measure.hpp; a goal set is what ik_solutions and the roadmap's "
              "goal-set query take");

static_assert(rrt::PROJECTION_OK == constraint::PROJECTED && constraint::PROJECTED == OPTIK_HIP_CONSTRAINT_PROJECTED,
              "rrt_constrained_measure.hpp names the projection's status without including constraint_measure.hpp");

namespace {

constexpr int RRT_BLOCK = 256, RRT_WAVE = 64;
constexpr long long MAX_QUERIES = 1ll << 30;

struct RrtLaunch {
    long long Q, q0, Qc;         // the call's queries; the chunk's first and its count
    int n, M, Lmax, I, iter, G;
    double eta;
    const double *start;         // [n][Q] the caller's
    const double *goals;         // [G][n][Q] the caller's
    const int32_t *gcount;       // [Q] the caller's, or null: G each
    const double *lo, *hi;       // [n] the joint limits (the chain's table)
    const double *samples;       // [n][I]
    double *cfg;                 // [n][(1 + G) Qc] column q: the start; column (1 + g) Qc + q: goal g, or the start
    double *da, *db;             // [n][G Qc] column g Qc + q: start -> goal g, NaN if the slot is not counted
    int32_t *gc;                 // [Qc] the clamped counts
    int32_t *root_goal;          // [G][Qc] the goal slot of root r
    int32_t *direct;             // [Qc] rule 0's direct goal, or -1
    uint8_t *flags;              // [3][Qc] the motion check's flags of the iteration's segments
    uint8_t *cflags;             // [(1 + G) Qc] optik_hip_collision_batch's flags of cfg
    uint8_t *mflags;             // [G Qc] the motion check's flags of the direct motions
    double *conf;                // [Qc][2][n][M]
    int32_t *parent;             // [Qc][2][M]
    int32_t *count;              // [2][Qc]
    int32_t *state;              // [Qc] rrt::RUNNING or how the query ended
    int32_t *junction;           // [2][Qc]
    int32_t *used;               // [Qc]
    int32_t *pend;               // [3][Qc] the iteration in flight: p (-1: none), m, whether tree b extends
    double *qa, *qb;             // [n][3 Qc] the segments, column s * Qc + q
    int32_t *unfinished;         // [1]
    double *path;                // [Lmax][Q][n] or null
    int32_t *len, *status, *iters, *nodes, *which;  // [Q], nodes [2][Q]; or null
    double *cost;
};

// What a constrained call adds to the launch (kernel arguments of rrt_cstep_kernel and rrt_mask_kernel only: the
// record above, and with it the kernels of the unconstrained planner, stay as they are).
struct RrtConstraint {
    ConstraintDev d;
    ProjectArgs p;
    double tol;                  // the violation rule 0 and a sample of a motion may have
    double *viol;                // [(1 + G) Qc] optik_hip_constraint_batch's violations of cfg
    uint8_t *cok;                // [3][Qc] optik_hip_constraint_motion_batch's ok bytes of the iteration's segments
    uint8_t *cok0;               // [G Qc] and of the direct motions
    int32_t *projected;          // [2][Q] the caller's, or null
};

// The host's side of it: the pointers the constraint entries take.
struct ConstraintCall {
    const double *ref7, *lo6, *hi6;
    RrtConstraint k;
};

__device__ __forceinline__ double *tree_conf(const RrtLaunch &a, long long q, int t) {
    return a.conf + ((size_t)q * 2 + t) * (size_t)a.n * a.M;
}
__device__ __forceinline__ int32_t *tree_parent(const RrtLaunch &a, long long q, int t) {
    return a.parent + ((size_t)q * 2 + t) * (size_t)a.M;
}

// every segment of query q is "not sampled" from here on
__device__ __forceinline__ void clear_segments(const RrtLaunch &a, long long q, int i) {
    const long long B = 3 * a.Qc;
    for (int s = 0; s < 3; ++s) {
        a.qa[(long long)i * B + s * a.Qc + q] = roadmap::nan_value();
        a.qb[(long long)i * B + s * a.Qc + q] = roadmap::nan_value();
    }
}

__device__ __forceinline__ double start_joint(const RrtLaunch &a, long long q, int i) {
    return a.cfg[(long long)i * (1 + a.G) * a.Qc + q];
}
// (of a counted goal only: the other slots hold NaN)
__device__ __forceinline__ double goal_joint(const RrtLaunch &a, long long q, int g, int i) {
    return a.db[(long long)i * a.G * a.Qc + (long long)g * a.Qc + q];
}

inline unsigned blocks(long long work) { return (unsigned)((work + RRT_BLOCK - 1) / RRT_BLOCK); }

__global__ __launch_bounds__(RRT_BLOCK) void rrt_gather_kernel(const RrtLaunch a) {
    const long long q = (long long)blockIdx.x * RRT_BLOCK + threadIdx.x, Qc = a.Qc;
    if (q >= Qc) return;
    const int n = a.n, G = a.G;
    const int gc = rrt::clamp_count(a.gcount ? a.gcount[a.q0 + q] : G, G);
    a.gc[q] = gc;
    for (int i = 0; i < n; ++i) {
        const double s = a.start[(long long)i * a.Q + a.q0 + q];
        double *cfg = a.cfg + (long long)i * (1 + G) * Qc + q;
        double *da = a.da + (long long)i * G * Qc + q, *db = a.db + (long long)i * G * Qc + q;
        cfg[0] = s;
        for (int g = 0; g < G; ++g) {
            const bool counted = g < gc;
            // (a slot that is not counted is not read at all)
            const double v = counted ? a.goals[((long long)g * n + i) * a.Q + a.q0 + q] : roadmap::nan_value();
            cfg[(long long)(1 + g) * Qc] = counted ? v : s;
            da[(long long)g * Qc] = counted ? s : roadmap::nan_value();
            db[(long long)g * Qc] = v;
        }
    }
}

__global__ __launch_bounds__(RRT_BLOCK) void rrt_begin_kernel(const RrtLaunch a) {
    const long long q = (long long)blockIdx.x * RRT_BLOCK + threadIdx.x, Qc = a.Qc;
    if (q >= Qc) return;
    const int n = a.n, G = a.G, M = a.M, gc = a.gc[q];
    bool ends_finite = true;
    for (int i = 0; i < n; ++i) ends_finite = ends_finite && rrt::finite(start_joint(a, q, i));
    for (int g = 0; g < gc; ++g)
        for (int i = 0; i < n; ++i) ends_finite = ends_finite && rrt::finite(goal_joint(a, q, g, i));
    const bool start_free = a.cflags[q] != 0;
    // the roots in ascending g and, among those whose direct motion is free, the nearest (a tie: the lower g)
    int R = 0, direct = -1;
    double bd = roadmap::inf();
    for (int g = 0; g < gc; ++g) {
        if (a.cflags[(long long)(1 + g) * Qc + q] == 0) continue;
        if (R < G) a.root_goal[(long long)R * Qc + q] = g;
        R += 1;
        if (a.mflags[(long long)g * Qc + q] == 0) continue;
        const double d = motion::motion_distance(n, a.cfg + q, (1 + G) * Qc, a.db + (long long)g * Qc + q, G * Qc);
        if (rrt::direct_better(d, bd, direct)) { bd = d; direct = g; }
    }
    const int state = rrt::begin_goals(ends_finite, gc, start_free, R, direct);
    const bool run = state == rrt::RUNNING;
    if (run) {
        // (R <= G <= M: the call refuses a max_nodes below G)
        double *c0 = tree_conf(a, q, 0), *c1 = tree_conf(a, q, 1);
        int32_t *par1 = tree_parent(a, q, 1);
        for (int i = 0; i < n; ++i) c0[(size_t)i * M] = start_joint(a, q, i);
        for (int r = 0; r < R && r < M; ++r) {
            const int g = a.root_goal[(long long)r * Qc + q];
            for (int i = 0; i < n; ++i) c1[(size_t)i * M + r] = goal_joint(a, q, g, i);
            par1[r] = -1;
        }
        tree_parent(a, q, 0)[0] = -1;
        atomicAdd(a.unfinished, 1);
    }
    a.count[q] = run ? 1 : 0;
    a.count[Qc + q] = run ? (R < M ? R : M) : 0;
    a.state[q] = state;
    a.direct[q] = state == rrt::FOUND ? direct : -1;
    a.junction[q] = -1;
    a.junction[Qc + q] = -1;
    a.used[q] = 0;
    a.pend[q] = -1;
    a.pend[Qc + q] = -1;
    a.pend[2 * Qc + q] = 0;
    for (int i = 0; i < n; ++i) clear_segments(a, q, i);
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

// Rule 0 under a constraint: "free" is free AND within the constraint.  (a NaN segment has both flags at 0 already)
__global__ __launch_bounds__(RRT_BLOCK) void rrt_mask_kernel(const RrtLaunch a, const RrtConstraint k) {
    const long long j = (long long)blockIdx.x * RRT_BLOCK + threadIdx.x;
    const long long nc = (1 + a.G) * a.Qc, nm = (long long)a.G * a.Qc;
    if (j < nc) {
        if (!(k.viol[j] <= k.tol)) a.cflags[j] = 0;
    } else if (j < nc + nm) {
        if (k.cok0[j - nc] == 0) a.mflags[j - nc] = 0;
    }
}

// Lane 0: project s_v [n] in place, and whether the result is taken as a node steered from column `from` of conf
// [n][M] (rrt::takes).  s_take[0] = taken, s_take[1] = the projection ended PROJECTED.
template <class CH>
__device__ __forceinline__ void project_candidate(const CH &sch, const RrtConstraint &k, int n, int M,
                                                  const double *conf, int from, double *s_v, int *s_take) {
    const constraint::Projected pr = project(sch, k.d, k.p, n, s_v);
    bool same = true;
    for (int i = 0; i < n; ++i) same = same && s_v[i] == conf[(size_t)i * M + from];
    s_take[0] = rrt::takes(pr.status, pr.iterations, same) ? 1 : 0;
    s_take[1] = pr.status == constraint::PROJECTED ? 1 : 0;
}

__device__ __forceinline__ void count_projections(const RrtLaunch &a, const RrtConstraint &k, long long q,
                                                  int attempted, int ended) {
    if (!k.projected || attempted == 0) return;
    k.projected[a.q0 + q] += attempted;
    k.projected[a.Q + a.q0 + q] += ended;
}

// CH of a step without a constraint: no table, no projection, k is not read.
struct NoChain {};

// The step of both planners: rrt_step_kernel (CH = NoChain) and rrt_cstep_kernel<CH>.
template <class CH>
__device__ __forceinline__ void rrt_step_body(const RrtLaunch &a, const RrtConstraint *k) {
    constexpr bool CON = !std::is_same<CH, NoChain>::value;
    __shared__ double s_x[OPTIK_HIP_MAX_DOF], s_c[OPTIK_HIP_MAX_DOF];
    // (the projections' own: never used without a constraint, and so not allocated)
    __shared__ CH sch;
    __shared__ double s_e[OPTIK_HIP_MAX_DOF];
    __shared__ int s_take[4];
    const long long q = blockIdx.x;
    const int lane = threadIdx.x, n = a.n, M = a.M;
    if (a.state[q] != rrt::RUNNING) return;  // (frozen: its segments are NaN already)
    const long long B = 3 * a.Qc;
    int cnt0 = a.count[q], cnt1 = a.count[a.Qc + q];
    const bool joint = lane < n;
    // ---- the iteration before: what the motion check (and the constraint's) said (rules 3 and 4) ----
    if (a.iter > 0) {
        const int pa = (a.iter - 1) & 1, pb = 1 - pa;
        const int p = a.pend[q], m = a.pend[a.Qc + q], back = a.pend[2 * a.Qc + q];
        bool ok0 = a.flags[q] != 0, ok1 = a.flags[a.Qc + q] != 0, ok2 = a.flags[2 * a.Qc + q] != 0;
        if constexpr (CON) {
            ok0 = ok0 && k->cok[q] != 0;
            ok1 = ok1 && k->cok[a.Qc + q] != 0;
            ok2 = ok2 && k->cok[2 * a.Qc + q] != 0;
        }
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
    if constexpr (CON) copy_table(sch, table_of<CH>(k->d));
    if (joint) s_x[lane] = a.samples[(long long)lane * a.I + a.iter];
    __syncthreads();  // (also: the nodes appended above are visible to every lane)
    int attempted = 0, ended = 0;  // the projections of this step
    // the exit of a step that leaves no segments behind
    auto give_up = [&]() {
        if (lane == 0) {
            a.pend[q] = -1;
            if constexpr (CON) count_projections(a, *k, q, attempted, ended);
        }
        if (joint) clear_segments(a, q, lane);
    };
    double d, dm;
    int p, m;
    wave_nearest(conf_a, n, M, cnt_a, s_x, lane, d, p);
    if (!rrt::steers(d) || cnt_a >= M || p < 0) return give_up();
    double pj = 0.0, cj = 0.0, lo = 0.0, hi = 0.0;
    if (joint) {
        pj = conf_a[(size_t)lane * M + p];
        lo = a.lo[lane];
        hi = a.hi[lane];
        cj = rrt::steer_joint(pj, s_x[lane], d, a.eta, lo, hi);
        s_c[lane] = cj;
    }
    __syncthreads();
    if constexpr (CON) {
        if (lane == 0) project_candidate(sch, *k, n, M, conf_a, p, s_c, s_take);
        __syncthreads();
        // (every lane reads the verdict from LDS before it branches on it)
        attempted = 1;
        ended = s_take[1];
        if (s_take[0] == 0) return give_up();
        if (joint) cj = s_c[lane];
    }
    wave_nearest(conf_b, n, M, cnt_b, s_c, lane, dm, m);
    if (m < 0) return give_up();  // (a tree has its root: cannot happen)
    bool back = rrt::extends_back(dm, a.eta, cnt_b, M);  // (wave-uniform: dm and cnt_b are)
    if constexpr (CON) {
        if (back) {
            if (joint) s_e[lane] = rrt::steer_joint(conf_b[(size_t)lane * M + m], cj, dm, a.eta, lo, hi);
            __syncthreads();
            if (lane == 0) project_candidate(sch, *k, n, M, conf_b, m, s_e, s_take + 2);
            __syncthreads();
            back = s_take[2] != 0;
            attempted += 1;
            ended += s_take[3];
        }
    }
    if (joint) {
        const double mj = conf_b[(size_t)lane * M + m];
        double ej;
        if constexpr (CON) ej = back ? s_e[lane] : roadmap::nan_value();
        else ej = back ? rrt::steer_joint(mj, cj, dm, a.eta, lo, hi) : roadmap::nan_value();
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
        if constexpr (CON) count_projections(a, *k, q, attempted, ended);
    }
}

__global__ __launch_bounds__(RRT_WAVE) void rrt_step_kernel(const RrtLaunch a) { rrt_step_body<NoChain>(a, nullptr); }

template <class CH>
__global__ __launch_bounds__(RRT_WAVE) void rrt_cstep_kernel(const RrtLaunch a, const RrtConstraint k) {
    rrt_step_body<CH>(a, &k);
}

// optik_hip_rrt_nearest_from_nodes: rules 1 and 2 on a tree the caller wrote, one wave per query point -- the step
// body's own wave_nearest and rrt::steer_joint, with the point staged in LDS as the step stages its sample.
struct RrtProbe {
    const double *conf;          // [n][M] the caller's
    const double *x;             // [n][X] the caller's
    const double *lo, *hi;       // [n] the joint limits (the chain's table)
    long long X;
    int n, M, count;
    double eta;
    int32_t *index;              // [X]
    double *dist;                // [X]
    double *cand;                // [n][X]
};

__global__ __launch_bounds__(RRT_WAVE) void rrt_nearest_kernel(const RrtProbe a) {
    __shared__ double s_x[OPTIK_HIP_MAX_DOF];
    const long long q = blockIdx.x;
    const int lane = threadIdx.x, n = a.n, M = a.M;
    const bool joint = lane < n;
    if (joint) s_x[lane] = a.x[(long long)lane * a.X + q];
    __syncthreads();
    double d;
    int p;
    wave_nearest(a.conf, n, M, a.count, s_x, lane, d, p);
    if (lane == 0) {
        a.index[q] = p;
        a.dist[q] = d;
    }
    if (joint) {
        // (no candidate where the step gives up: NaN)
        const bool made = rrt::steers(d) && p >= 0;
        a.cand[(long long)lane * a.X + q] =
            made ? rrt::steer_joint(a.conf[(size_t)lane * M + p], s_x[lane], d, a.eta, a.lo[lane], a.hi[lane])
                 : roadmap::nan_value();
    }
}

__global__ __launch_bounds__(RRT_WAVE) void rrt_walk_kernel(const RrtLaunch a) {
    __shared__ int s_way[roadmap::MAX_WAYPOINTS];  // waypoint t: node v of tree 0, or M + v of tree 1
    __shared__ int s_len, s_pad;                   // s_pad: the goal slot the path is padded with, -1 for the start
    const long long q = blockIdx.x, qo = a.q0 + q, Qc = a.Qc;
    const int lane = threadIdx.x, n = a.n, M = a.M, G = a.G;
    if (lane == 0) {
        const int state = a.state[q], j0 = a.junction[q], j1 = a.junction[Qc + q];
        const int c0 = a.count[q], c1 = a.count[Qc + q], gc = a.gc[q], direct = a.direct[q];
        int status = state == rrt::RUNNING ? rrt::NO_ROUTE : state, len = 2, which = -1;
        double cost = roadmap::inf();
        if (state == rrt::QUERY_NAN) cost = roadmap::nan_value();
        if (state == rrt::FOUND && !(j0 >= 0 && j0 < c0 && j1 >= 0 && j1 < c1)) {
            if (direct >= 0 && direct < gc) {
                // the direct motion (rule 0)
                cost = 0.0 + motion::motion_distance(n, a.cfg + q, (1 + G) * Qc, a.db + (long long)direct * Qc + q, G * Qc);
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
            const int g = v >= 0 && v < G ? a.root_goal[(long long)v * Qc + q] : -1;
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
        if (a.which) a.which[qo] = which;
    }
    __syncthreads();
    if (!a.path) return;
    const int len = s_len, pad = s_pad;
    const double *conf = tree_conf(a, q, 0);  // (tree 1 follows tree 0: node M + v)
    for (int e = lane; e < a.Lmax * n; e += RRT_WAVE) {
        const int t = e / n, i = e % n;
        double v = pad >= 0 ? goal_joint(a, q, pad, i) : start_joint(a, q, i);
        if (t == 0) v = start_joint(a, q, i);
        else if (t < len - 1) {
            const int w = s_way[t];
            v = conf[(size_t)(w / M) * n * M + (size_t)i * M + (w % M)];
        }
        a.path[((long long)t * a.Q + qo) * n + i] = v;
    }
}

// what both calls refuse before any device work, in optik_hip_rrt_plan's words; 0 to go on
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

// The iterations of the chunk a.q0, a.Qc whose begin kernel has run on `stream`: rrt_step_kernel and the motion check
// over the 3 a.Qc segments per iteration, one read of *a.unfinished every `poll` iterations, and the last commit with
// rule 6.  The walk kernel comes next on the stream.
// Under a constraint (cc not null): rrt_cstep_kernel in its place and optik_hip_constraint_motion_batch after the motion check.
int run_iterations(optik_hip_chain *ch, const double *ee_offset7, RrtLaunch &a, const ConstraintCall *cc, int32_t iters,
                   int32_t poll, double resolution, hipStream_t stream) {
    const long long L = a.Qc;
    bool ended = false;
    auto step = [&]() -> int {
        if (cc) {
            CONSTRAINT_LAUNCH(rrt_cstep_kernel, ch, (unsigned)L, RRT_WAVE, stream, a, cc->k);
        } else {
            hipLaunchKernelGGL(rrt_step_kernel, dim3((unsigned)L), dim3(RRT_WAVE), 0, stream, a);
            HIP_TRY(hipGetLastError());
        }
        return 0;
    };
    for (int32_t i = 0; i < iters; ++i) {
        a.iter = i;
        {
            BIND_DEVICE(ch);
            if (int rc = step()) return rc;
            if (i % poll == 0) {
                // (the one synchronise of a poll: the host decides whether the iterations go on)
                int32_t left = 0;
                HIP_TRY(hipMemcpyAsync(&left, a.unfinished, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
                HIP_TRY(hipStreamSynchronize(stream));
                if (left <= 0) { ended = true; break; }
            }
        }
        if (int rc = optik_hip_collision_motion_batch(ch, ee_offset7, a.qa, a.qb, 3 * L, resolution, nullptr, a.flags,
                                                      nullptr, nullptr, stream))
            return rc;
        if (cc)
            if (int rc = optik_hip_constraint_motion_batch(ch, ee_offset7, cc->ref7, cc->lo6, cc->hi6, a.qa, a.qb, 3 * L,
                                                           resolution, cc->k.tol, nullptr, cc->k.cok, nullptr, nullptr,
                                                           stream))
                return rc;
    }
    BIND_DEVICE(ch);
    if (!ended) {
        a.iter = iters;  // (the last iteration's commit, and rule 6)
        if (int rc = step()) return rc;
    }
    return 0;
}

// The arrays of a workspace one after the other, each on a 16-byte boundary.  With base 0 the same sequence of
// take() calls gives the size to reserve.
struct Carve {
    uintptr_t base;
    size_t at = 0;
    template <class T> void take(T *&array, size_t count) {
        array = reinterpret_cast<T *>(base + at);
        at += (sizeof(T) * count + 15) & ~(size_t)15;
    }
};

// The workspace of a call in chunks of Qc queries -- the samples, rule 0's configurations, direct motions and flags,
// the iteration's segments and flags, the per-query state and the trees -- into the record; returns its size.
// (a chunk's arrays are [..][L] with L <= Qc: a later chunk may be shorter, never longer)
// Under a constraint its few bytes per query follow: the violations of rule 0's configurations and the ok bytes.
size_t carve_workspace(RrtLaunch &a, ConstraintCall *cc, unsigned char *ws, size_t Qc) {
    const size_t n = (size_t)a.n, M = (size_t)a.M, I = (size_t)a.I, G = (size_t)a.G;
    Carve c{reinterpret_cast<uintptr_t>(ws)};
    c.take(a.unfinished, 1);
    c.take(a.samples, n * I);
    c.take(a.cfg, n * (1 + G) * Qc);
    c.take(a.da, n * G * Qc);
    c.take(a.db, n * G * Qc);
    c.take(a.qa, n * 3 * Qc);
    c.take(a.qb, n * 3 * Qc);
    c.take(a.flags, 3 * Qc + (1 + 2 * G) * Qc);  // (the iterations' three flags per query, then rule 0's 1 + 2 G)
    a.cflags = a.flags + 3 * Qc;
    c.take(a.count, 2 * Qc);
    c.take(a.state, Qc);
    c.take(a.junction, 2 * Qc);
    c.take(a.used, Qc);
    c.take(a.pend, 3 * Qc);
    c.take(a.gc, Qc);
    c.take(a.direct, Qc);
    c.take(a.root_goal, G * Qc);
    c.take(a.parent, 2 * M * Qc);
    c.take(a.conf, 2 * n * M * Qc);
    if (cc) {
        c.take(cc->k.viol, (1 + G) * Qc);
        c.take(cc->k.cok, 3 * Qc + G * Qc);  // (the iterations' three ok bytes per query, then rule 0's G)
    }
    return c.at;
}

// The planner of all three calls, their arguments checked: d_goals [G][n][Q]; d_gcount null: G each; d_which may be
// null; cc null: no constraint.
int plan(optik_hip_chain *ch, const double *ee_offset7, ConstraintCall *cc, const double *d_start, const double *d_goals,
         const int32_t *d_gcount, int64_t Q, int32_t G, int32_t iters, double step, double resolution, uint64_t first,
         int32_t max_nodes, int32_t Lmax, int32_t poll, double *d_path, int32_t *d_len, double *d_cost,
         int32_t *d_status, int32_t *d_iters, int32_t *d_nodes, int32_t *d_which, hipStream_t stream) {
    const size_t Qc = (size_t)std::min<int64_t>(Q, optik_hip_rrt_chunk(ch, max_nodes)), uG = (size_t)G;
    RrtLaunch a;
    std::memset(&a, 0, sizeof a);
    a.Q = Q; a.n = ch->n; a.M = max_nodes; a.Lmax = Lmax; a.I = iters; a.G = G; a.eta = step;
    a.start = d_start; a.goals = d_goals; a.gcount = d_gcount;
    a.lo = ch->wide ? ch->wdev->lb : ch->dev->lb;
    a.hi = ch->wide ? ch->wdev->ub : ch->dev->ub;
    a.path = d_path; a.len = d_len; a.cost = d_cost; a.status = d_status; a.iters = d_iters; a.nodes = d_nodes;
    a.which = d_which;
    const size_t bytes = carve_workspace(a, cc, nullptr, Qc);
    {
        std::lock_guard<std::mutex> lock(ch->mu);
        BIND_DEVICE(ch);
        HIP_TRY(ch->rrt_ws.reserve(bytes));
        carve_workspace(a, cc, ch->rrt_ws.get(), Qc);
        // (0 where the iterations never begin; rrt_cstep_kernel adds to it)
        if (cc && cc->k.projected) HIP_TRY(hipMemsetAsync(cc->k.projected, 0, sizeof(int32_t) * 2 * (size_t)Q, stream));
    }
    // (the samples of the whole call: iteration i reads restart seed first + i, whatever the query)
    if (int rc = optik_hip_seed_batch(ch, first, iters, const_cast<double *>(a.samples), stream)) return rc;
    for (int64_t q0 = 0; q0 < Q; q0 += (int64_t)Qc) {
        const long long L = std::min<int64_t>((int64_t)Qc, Q - q0);
        a.q0 = q0; a.Qc = L;
        a.qb = a.qa + (size_t)a.n * 3 * (size_t)L;
        a.mflags = a.cflags + (1 + uG) * (size_t)L;
        if (cc) cc->k.cok0 = cc->k.cok + 3 * (size_t)L;
        {
            BIND_DEVICE(ch);
            HIP_TRY(hipMemsetAsync(a.unfinished, 0, sizeof(int32_t), stream));
            hipLaunchKernelGGL(rrt_gather_kernel, dim3(blocks(L)), dim3(RRT_BLOCK), 0, stream, a);
            HIP_TRY(hipGetLastError());
        }
        if (int rc = optik_hip_collision_batch(ch, ee_offset7, a.cfg, (1 + G) * L, nullptr, a.cflags, stream)) return rc;
        if (int rc = optik_hip_collision_motion_batch(ch, ee_offset7, a.da, a.db, G * L, resolution, nullptr, a.mflags,
                                                      nullptr, nullptr, stream))
            return rc;
        if (cc) {
            if (int rc = optik_hip_constraint_batch(ch, ee_offset7, cc->ref7, cc->lo6, cc->hi6, a.cfg, (1 + G) * L, nullptr,
                                                    cc->k.viol, stream))
                return rc;
            if (int rc = optik_hip_constraint_motion_batch(ch, ee_offset7, cc->ref7, cc->lo6, cc->hi6, a.da, a.db, G * L,
                                                           resolution, cc->k.tol, nullptr, cc->k.cok0, nullptr, nullptr,
                                                           stream))
                return rc;
            BIND_DEVICE(ch);
            hipLaunchKernelGGL(rrt_mask_kernel, dim3(blocks((1 + 2 * (long long)G) * L)), dim3(RRT_BLOCK), 0, stream, a,
                               cc->k);
            HIP_TRY(hipGetLastError());
        }
        {
            BIND_DEVICE(ch);
            hipLaunchKernelGGL(rrt_begin_kernel, dim3(blocks(L)), dim3(RRT_BLOCK), 0, stream, a);
            HIP_TRY(hipGetLastError());
        }
        if (int rc = run_iterations(ch, ee_offset7, a, cc, iters, poll, resolution, stream)) return rc;
        BIND_DEVICE(ch);
        hipLaunchKernelGGL(rrt_walk_kernel, dim3((unsigned)L), dim3(RRT_WAVE), 0, stream, a);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" {

int64_t optik_hip_rrt_chunk(const optik_hip_chain *ch, int32_t max_nodes) {
    if (!ch || max_nodes < 1) return 0;
    const int64_t per = 2 * (int64_t)max_nodes * (8 * (int64_t)ch->n + 4);
    return std::max<int64_t>(1, OPTIK_HIP_RRT_CHUNK_BYTES / per);
}

int optik_hip_rrt_nearest_from_nodes(optik_hip_chain *ch, const double *d_conf, int32_t max_nodes, int32_t count,
                                     const double *d_x, int64_t X, double step, int32_t *d_index, double *d_dist,
                                     double *d_cand, void *stream_) {
    if (!ch || X < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (X > MAX_QUERIES) return fail(OPTIK_HIP_EINVAL, "rrt_nearest_from_nodes: more than 2^30 points in one launch");
    if (!(step > 0.0) || !std::isfinite(step))
        return fail(OPTIK_HIP_EINVAL, "rrt_nearest_from_nodes: step must be finite and > 0");
    if (max_nodes < 1 || max_nodes > rrt::MAX_NODES)
        return fail(OPTIK_HIP_EINVAL, "rrt_nearest_from_nodes: max_nodes must be in 1 .. " + std::to_string(rrt::MAX_NODES));
    if (count < 1 || count > max_nodes)
        return fail(OPTIK_HIP_EINVAL, "rrt_nearest_from_nodes: count must be in 1 .. max_nodes");
    if (ch->n < 1 || ch->n > OPTIK_HIP_MAX_DOF)
        return fail(OPTIK_HIP_EUNSUPPORTED, "rrt_nearest_from_nodes: chains of 1 .. 16 joint positions");
    if (X == 0) return 0;
    if (!d_conf || !d_x || !d_index || !d_dist || !d_cand) return fail(OPTIK_HIP_EINVAL, "bad argument");
    RrtProbe a;
    a.conf = d_conf; a.x = d_x; a.X = X; a.n = ch->n; a.M = max_nodes; a.count = count; a.eta = step;
    a.lo = ch->wide ? ch->wdev->lb : ch->dev->lb;
    a.hi = ch->wide ? ch->wdev->ub : ch->dev->ub;
    a.index = d_index; a.dist = d_dist; a.cand = d_cand;
    BIND_DEVICE(ch);
    hipLaunchKernelGGL(rrt_nearest_kernel, dim3((unsigned)X), dim3(RRT_WAVE), 0, (hipStream_t)stream_, a);
    HIP_TRY(hipGetLastError());
    return 0;
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
    // (one goal slot, counted: [G][n][Q] with G = 1 is d_goal's [n][Q])
    return plan(ch, ee_offset7, nullptr, d_start, d_goal, nullptr, Q, 1, iters, step, resolution, first, max_nodes, Lmax, poll,
                d_path, d_len, d_cost, d_status, d_iters, d_nodes, nullptr, (hipStream_t)stream_);
}

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
    if (!d_start || !d_goals) return fail(OPTIK_HIP_EINVAL, "bad argument");  // (d_gcount null: G each)
    return plan(ch, ee_offset7, nullptr, d_start, d_goals, d_gcount, Q, G, iters, step, resolution, first, max_nodes,
                Lmax, poll, d_path, d_len, d_cost, d_status, d_iters, d_nodes, d_which, (hipStream_t)stream_);
}

int optik_hip_rrt_plan_constrained(optik_hip_chain *ch, const double *ee_offset7, const double *ref7, const double *lo6,
                                   const double *hi6, double tol, double ptol, int32_t piters, double damping,
                                   double max_step, const double *d_start, const double *d_goals,
                                   const int32_t *d_gcount, int64_t Q, int32_t G, int32_t iters, double step,
                                   double resolution, uint64_t first, int32_t max_nodes, int32_t Lmax, int32_t poll,
                                   double *d_path, int32_t *d_len, double *d_cost, int32_t *d_status, int32_t *d_iters,
                                   int32_t *d_nodes, int32_t *d_which, int32_t *d_projected, void *stream_) {
    if (G < 1 || G > rrt::MAX_GOALS)
        return fail(OPTIK_HIP_EINVAL, "rrt_plan_constrained: G must be in 1 .. " + std::to_string(rrt::MAX_GOALS)
                                          + " goals per query");
    if (max_nodes < rrt::min_nodes(G) || max_nodes > rrt::MAX_NODES)
        return fail(OPTIK_HIP_EINVAL, "rrt_plan_constrained: max_nodes must be in max(2, G) .. "
                                          + std::to_string(rrt::MAX_NODES) + ": every goal may be a root");
    if (int rc = check_args(ch, Q, iters, step, resolution, max_nodes, Lmax, poll)) return rc;
    // (B = 0: the constraint entries' own refusals -- the reference, the bounds, tol; ptol, piters, damping, max_step)
    if (int rc = optik_hip_constraint_motion_batch(ch, nullptr, ref7, lo6, hi6, nullptr, nullptr, 0, resolution, tol,
                                                   nullptr, nullptr, nullptr, nullptr, nullptr))
        return rc;
    if (int rc = optik_hip_constraint_project_batch(ch, nullptr, ref7, lo6, hi6, nullptr, 0, ptol, piters, damping,
                                                    max_step, nullptr, nullptr, nullptr, nullptr, nullptr))
        return rc;
    if (ch->n < 1 || ch->n > OPTIK_HIP_MAX_DOF)
        return fail(OPTIK_HIP_EUNSUPPORTED, "rrt_plan_constrained: chains of 1 .. 16 joint positions");
    if (Q == 0
        || (!d_path && !d_len && !d_cost && !d_status && !d_iters && !d_nodes && !d_which && !d_projected))
        return 0;
    if (!d_start || !d_goals) return fail(OPTIK_HIP_EINVAL, "bad argument");  // (d_gcount null: G each)
    ConstraintCall cc;
    std::memset(&cc, 0, sizeof cc);
    cc.ref7 = ref7; cc.lo6 = lo6; cc.hi6 = hi6;
    fill_constraint(ch, ee_offset7, ref7, lo6, hi6, cc.k.d);
    cc.k.p = ProjectArgs{ptol, damping, max_step, piters};
    cc.k.tol = tol;
    cc.k.projected = d_projected;
    return plan(ch, ee_offset7, &cc, d_start, d_goals, d_gcount, Q, G, iters, step, resolution, first, max_nodes, Lmax,
                poll, d_path, d_len, d_cost, d_status, d_iters, d_nodes, d_which, (hipStream_t)stream_);
}

}  // extern "C"
