/*
 * optik_hip.h -- C ABI of the MI355X kernel layer for optik's random-restart IK.
 *
 * This is the boundary a host written in the reference's own language binds
 * (Rust `extern "C"` / cgo-style FFI): plain pointers and
 * sizes, integer return codes, no C++ or torch types.  It replaces, behind
 * `Robot::ik` (/root/reference/crates/optik/src/lib.rs:241-415),
 *   - the rayon fan-out over restart indices        lib.rs:297-301, 393-395
 *   - the per-restart NLopt SLSQP solve             lib.rs:302-356, 372 (nlopt crate)
 *   - the ChaCha8 restart seeds                     lib.rs:358-370, 86-91 (rand crates)
 *   - objective / gradient / FK / Jacobian          objective.rs:40-110, kinematics.rs:123-196
 *   - classification and winner selection           lib.rs:376-390, 397-413
 *
 * Conventions: poses are 7 doubles [tx, ty, tz, qi, qj, qk, qw]; `d_` pointers
 * are device (HBM) memory, everything else is host memory; batched per-restart
 * arrays are struct-of-arrays ([component][batch]) so that lane-consecutive
 * accesses coalesce.  All calls are stream-ordered on `stream` (a hipStream_t
 * passed as void*, NULL = default stream) and return 0 on success or a negative
 * OPTIK_HIP_E* code; optik_hip_last_error() describes the last failure of the
 * calling thread.  There is no CPU fallback: without a usable GPU every compute
 * entry point fails with OPTIK_HIP_ENODEVICE.
 */
#ifndef OPTIK_HIP_H
#define OPTIK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OPTIK_HIP_MAX_DOF 16 /* joint positions of a chain (9 .. 16: the general kernels, see below) */

enum {
    OPTIK_HIP_OK = 0,
    OPTIK_HIP_EINVAL = -1,     /* bad argument */
    OPTIK_HIP_EUNSUPPORTED = -2, /* chain shape the kernels do not cover */
    OPTIK_HIP_ENODEVICE = -3,  /* no HIP device / HIP runtime error */
    OPTIK_HIP_ENOMEM = -4
};

/* JointType, kinematics.rs:227-241 */
enum { OPTIK_JOINT_FIXED = 0, OPTIK_JOINT_REVOLUTE = 1, OPTIK_JOINT_PRISMATIC = 2 };

/* Per-restart status = NLopt's nlopt_result for the SLSQP run (lib.rs:372-379). */
enum {
    OPTIK_RES_FAILURE = -1,
    OPTIK_RES_ROUNDOFF_LIMITED = -4,
    OPTIK_RES_FORCED_STOP = -5,   /* abandoned: timeout or a lower index succeeded */
    OPTIK_RES_ITER_CAP = -100,
    OPTIK_RES_NOT_RUN = 0,
    OPTIK_RES_STOPVAL_REACHED = 2,
    OPTIK_RES_FTOL_REACHED = 3,
    OPTIK_RES_XTOL_REACHED = 4
};

/* optik_solver_config.solution_mode.  Quality and Speed are the reference's (config.rs:3-8).  The two extensions
 * rank the successful restarts by the body Jacobian J of their solution (the TRAC-IK solve types Manip1 / Manip2,
 * without TRAC-IK's joint-limit penalty factor; J unscaled, metres and radians as KDL's): Manipulability keeps the
 * largest w = sqrt(det G) = the product of J's min(n, 6) largest singular values, Condition the largest
 * c = sigma_min / sigma_max (G = J^T J for n <= 6, J J^T for n > 6; the operation order: csrc/manip_measure.hpp).
 * Both are scheduled as Quality: every restart of the range runs to its end (no early exit, no FIND_ANY). */
#define OPTIK_MODE_QUALITY 1
#define OPTIK_MODE_SPEED 2
#define OPTIK_MODE_MANIPULABILITY 3
#define OPTIK_MODE_CONDITION 4

/* SolverConfig with the layout of CSolverConfig
 * (crates/optik-cpp/src/lib.rs:10-20; config.rs:22-50): 96 bytes on LP64. */
typedef struct optik_solver_config {
    int32_t solution_mode; /* OPTIK_MODE_*: 1 = Quality, 2 = Speed (config.rs:3-8); 3, 4: extensions */
    int32_t _pad;
    double max_time;       /* seconds, 0 = unlimited */
    uint64_t max_restarts; /* 0 = unlimited */
    double tol_f;
    double tol_df;
    double tol_dx;
    double linear_weight[3];
    double angular_weight[3];
} optik_solver_config;

/* Flat kinematic chain (the output of KinematicChain::from_urdf,
 * kinematics.rs:18-105, uploaded once per robot). */
typedef struct optik_hip_chain optik_hip_chain;

int optik_hip_device_count(void);
const char *optik_hip_last_error(void);

/* origins: n_joints x 7 poses (Joint::origin), axes: n_joints x 3 (unit axis of
 * each chain joint, ignored for fixed), types: OPTIK_JOINT_*, lb/ub: n limits
 * (Robot::joint_limits, lib.rs:78-84).  Supported: 1 <= n <= 16 positional joints plus
 * an optional trailing fixed joint (what from_urdf's folding produces).  n <= 8 runs on the
 * tuned solvers (the lane-per-restart form for n <= 7 from one full load of the chip on, the
 * quad solver otherwise); 9 <= n <= 16 runs on one general kernel per entry point (joint count at run
 * time; the solver keeps one restart per wave in LDS with the wave's 64 lanes working on it
 * together: the same results as the CPU oracle bit for bit, a fraction of the tuned solvers'
 * rate) -- the reference itself has no limit
 * (kinematics.rs:107-110).  Prismatic joints (n <= 8): forward kinematics only (the reference's
 * Jacobian is todo!(), kinematics.rs:185). */
int optik_hip_chain_create(const double *origins, const double *axes, const int32_t *types,
                           int32_t n_joints, const double *lb, const double *ub, int32_t n,
                           optik_hip_chain **out);
void optik_hip_chain_destroy(optik_hip_chain *chain);
int32_t optik_hip_chain_num_positions(const optik_hip_chain *chain);

/* Which rand 0.9.2 code path the restart seeds restate for `rng.random_range(lb..=ub)`
 * (lib.rs:89).  SINGLE_INCLUSIVE (default): UniformFloat::sample_single_inclusive, which is
 * what Rng::random_range dispatches to for a RangeInclusive<f64> -- scale = ub - lb.
 * NEW_INCLUSIVE: Uniform::new_inclusive(lb, ub).sample(rng) -- scale = (ub - lb) / (1 - eps),
 * decreased by ulps until scale * (1 - eps) + lb <= ub.  The two differ in the last bits
 * of every seed; the kernels only see the precomputed scale.  The environment variable
 * OPTIK_RANDOM_RANGE_RULE=new_inclusive selects the second rule for chains created after
 * it is set.  Not to be called while a launch on the chain is in flight. */
enum { OPTIK_HIP_RANGE_SINGLE_INCLUSIVE = 0, OPTIK_HIP_RANGE_NEW_INCLUSIVE = 1 };
int optik_hip_chain_set_range_rule(optik_hip_chain *chain, int32_t rule);
int32_t optik_hip_chain_range_rule(const optik_hip_chain *chain);

/* objective + objective_grad (objective.rs:40-110) for B configurations.
 * d_q [n][B] -> d_f [B], d_g [n][B] (d_g may be NULL).  Only the weights of
 * `cfg` are read.  ee_offset7 may be NULL (identity). */
int optik_hip_eval_batch(const optik_hip_chain *chain, const optik_solver_config *cfg,
                         const double *target7, const double *ee_offset7, const double *d_q,
                         int64_t B, double *d_f, double *d_g, void *stream);

/* forward_kinematics + joint_jacobian (kinematics.rs:123-196) for B
 * configurations: d_pose [7][B] (EE pose), d_jac [6n][B] column-major 6 x n per
 * configuration (may be NULL). */
int optik_hip_fk_batch(const optik_hip_chain *chain, const double *ee_offset7, const double *d_q,
                       int64_t B, double *d_pose, double *d_jac, void *stream);

/* Robot::diff_ik (lib.rs:123-239) for B configurations, each row exactly as optik_robot_diff_ik_ex solves it
 * (the same FK / Jacobian device code and the same LP source, csrc/diff_ik_lp.hpp: the same bits).
 * d_q [n][B]; d_V [6][ld_V] with ld_V >= B, or ld_V = 0 for one twist d_V[6] shared by every row;
 * d_vmax [n][ld_vmax] likewise (0: one limit vector d_vmax[n]) -> d_alpha [B], d_v [n][B], d_status [B]
 * (0 solved; 1 no solution -- some v_max_i < 0 or NaN -- with alpha and v zero).  ee_offset7 may be NULL.
 * One thread per row, no workspace, no allocation.  Refused with OPTIK_HIP_EUNSUPPORTED, also when B = 0 (a
 * call with B = 0 and NULL buffers is how to ask): chains of more than 8 joint positions and chains with
 * prismatic joints, as the single call refuses them.  Otherwise B = 0 is a no-op. */
int optik_hip_diff_ik_batch(const optik_hip_chain *chain, const double *ee_offset7, const double *d_q,
                            const double *d_V, int64_t ld_V, const double *d_vmax, int64_t ld_vmax,
                            int64_t B, double *d_alpha, double *d_v, int32_t *d_status, void *stream);

/* Which way is out (extension; the arithmetic: csrc/collision_gradient.hpp).  For B
 * configurations d_q [n][B] of a chain with a collision model, the witness table of each: one row per frame f of its
 * F = n + 2 frames, the smallest term of the clearance that belongs to frame f (the robot spheres on f against the
 * world spheres, boxes and grid; the self pairs whose higher frame is f; ties to the first in that order).
 * d_dist [F][B] that term's distance (the minimum over f is optik_hip_collision_batch's clearance bit for bit),
 * d_witness [F][3][B] int32 (robot sphere, kind, index) in the numbering the model and world were given in -- kind 0
 * world sphere, 1 box, 2 grid (index 0), 3 self pair (robot sphere a, index of the pair) --, d_grad [F][n][B] the
 * derivative of the distance with respect to the joint positions.  Any output may be NULL.  A row without a term (and
 * every row of a chain without a model): dist +inf, grad 0, witness -1.  A configuration with a NaN frame: dist and
 * grad NaN, witness -1 in every row.  One thread per configuration, no workspace, no allocation.
 * OPTIK_HIP_EUNSUPPORTED, also when B = 0: prismatic joints, and chains of 9 .. 16 joint positions (not in this
 * version). */
int optik_hip_collision_witness_batch(const optik_hip_chain *chain, const double *ee_offset7, const double *d_q,
                                      int64_t B, double *d_dist, double *d_grad, int32_t *d_witness, void *stream);

/* Collision-avoiding diff_ik: optik_hip_diff_ik_batch (same arguments, same layout) with velocity dampers (Faverjon
 * and Tournassoud 1987).  Every witness row with a finite dist < influence adds the half-space
 *     grad . v >= -gain * (dist - safety) / (influence - safety)
 * to the LP -- at most OPTIK_HIP_MAX_DAMPER_ROWS of them, the closest, ties to the lower frame (csrc/diff_ik_lp.hpp:
 * diff_ik_lp_damped).  A term at `influence` may approach at `gain` m/s, a term at `safety` not at all, a term
 * inside `safety` must recede.  d_status: 0 solved; 1 no solution (a bad v_max, a NaN frame of a chain with a model,
 * or dampers that no velocity within the limits satisfies) with alpha and v zero.  A chain without a model, and a row
 * with nothing inside `influence`, gets the bits of optik_hip_diff_ik_batch.  One fused kernel, no workspace, no
 * allocation.
 * OPTIK_HIP_EINVAL unless influence > safety >= 0 and gain > 0, all finite.  OPTIK_HIP_EUNSUPPORTED, also when B = 0:
 * as optik_hip_diff_ik_batch (more than 8 joint positions -- 9 .. 16 are not in this version --, prismatic joints). */
#define OPTIK_HIP_MAX_DAMPER_ROWS 4
int optik_hip_diff_ik_avoid_batch(const optik_hip_chain *chain, const double *ee_offset7, const double *d_q,
                                  const double *d_V, int64_t ld_V, const double *d_vmax, int64_t ld_vmax, int64_t B,
                                  double influence, double safety, double gain, double *d_alpha, double *d_v,
                                  int32_t *d_status, void *stream);

/* Bending paths out of collision (extension; the arithmetic and its operation order:
 * csrc/path_optimize.hpp): covariant gradient smoothing, after CHOMP, of P joint-space paths of L waypoints each,
 * 3 <= L <= OPTIK_HIP_PATH_OPTIMIZE_MAX_WAYPOINTS.  d_q_in [L][P][n] -- the layout optik_hip_ik_path writes its
 * waypoint solutions d_x in, so its output is handed over as it is.  The first and the last waypoint never move.
 * Each of `iters` updates steps every free waypoint by -step * Ainv * g from the same iterate, g the gradient of
 *     U = w_smooth * F_smooth + w_obs * F_obs,
 * F_smooth half the sum of the squared segment lengths, F_obs the sum over the free waypoints and their n + 2 witness
 * rows (optik_hip_collision_witness_batch) of a hinge of dist - safety that reaches zero at `influence`, Ainv the
 * inverse of the first-difference metric; then clamps to the chain's joint limits.  One more evaluation follows the
 * last update: iters + 1 in all; iters = 0 copies the path and reports its costs.
 * d_q_out [L][P][n] the final waypoints (may be d_q_in); d_cost_first, d_cost_last [P][3] = (U, F_smooth, F_obs) at
 * the first and at the last iterate; d_clearance [P] the smallest witness distance over all L waypoints of the last
 * iterate (+inf without a model, NaN with a NaN frame); d_status [P] int32: 0, or 1 when the last cost is NaN.  Any
 * output may be NULL.  A chain without a model has F_obs = 0: the path relaxes towards the straight line.
 * One wave per path, the whole loop in one launch; stream-ordered, no workspace, no allocation.  K updates in one
 * call give the bits of K calls of one update, whatever P is.
 * OPTIK_HIP_EINVAL before any device work: L outside 3 .. 64, P < 0 (P = 0: nothing to do), iters < 0, or unless
 * step > 0, w_smooth >= 0, w_obs >= 0 and influence > safety >= 0, all finite.  OPTIK_HIP_EUNSUPPORTED, also when
 * P = 0: prismatic joints, and chains of 9 .. 16 joint positions (not in this version). */
#define OPTIK_HIP_PATH_OPTIMIZE_MAX_WAYPOINTS 64
int optik_hip_path_optimize(const optik_hip_chain *chain, const double *ee_offset7, const double *d_q_in, int32_t L,
                            int64_t P, int32_t iters, double step, double w_smooth, double w_obs, double influence,
                            double safety, double *d_q_out, double *d_cost_first, double *d_cost_last,
                            double *d_clearance, int32_t *d_status, void *stream);

/* Roadmap planning (extension; the arithmetic and its operation order:
 * csrc/roadmap_measure.hpp): a directed graph over N <= OPTIK_HIP_ROADMAP_MAX_NODES joint-space nodes, every edge a
 * motion checked by optik_hip_collision_motion_batch in the direction it is used in, queried for many (start, goal)
 * pairs at once.  The metric is L-infinity in radians: the weight of a -> b is max_i |b_i - a_i|, the d of the motion
 * check.  Configurations are struct-of-arrays, [n][count], as every batch operator has them.  Any revolute chain of
 * 1 .. 16 joint positions.  All three are stream-ordered with no host synchronisation.  Refused with
 * OPTIK_HIP_EINVAL before any device work: k (ks, kg) outside 1 .. OPTIK_HIP_ROADMAP_MAX_K, N outside 1 ..
 * OPTIK_HIP_ROADMAP_MAX_NODES (optik_hip_roadmap_edges: N < 1), Q < 0 (Q = 0 is a no-op) or above 2^30, Lmax outside
 * 2 .. 64, a resolution that is not finite and > 0; with OPTIK_HIP_EUNSUPPORTED: chains with prismatic joints.
 *
 * optik_hip_roadmap_knn: queries d_q [n][Q] against d_nodes [n][N] -> d_idx [k][Q], d_dist [k][Q] (either may be
 * NULL): the k first nodes of each query in the total order on (distance, index) -- a number before a NaN distance,
 * then the smaller distance, then the smaller index --, best first; slots past the candidates hold index -1 and
 * distance +inf.  exclude_self != 0 skips node j for query j (queries and nodes are the same array).  The result is
 * defined by the order alone: not by the launch shape, the tile size or the order of the visits.
 *
 * optik_hip_roadmap_edges: the Q * k segments d_from[:, q] -> d_nodes[:, d_idx[s][q]] (reverse != 0: node -> from)
 * are gathered, checked at `resolution` by the motion check's own code on the same stream (model, world and
 * ee_offset7 as there; without a model every motion of finite length is free), and d_w [k][Q] receives the weight where the
 * motion is free and +inf where it is not, where it is not sampled, or where the index is outside 0 .. N - 1.  The
 * motion check samples qa + (j / K)(qb - qa), so a segment and its reverse have different samples: an edge holds in
 * the direction it was checked in.  d_idx NULL pairs endpoint q with node q (k = 1, N = Q; N is not capped): the direct
 * start -> goal check of a plan.  The gathered segments (16 n + 1 bytes each) are the chain's workspace, grown on
 * demand, next to the motion check's: one call per chain handle at a time.
 *
 * optik_hip_roadmap_query: the graph d_nbr, d_w [k][N] (the out-edges v -> d_nbr[s][v], checked in that direction);
 * per query its start and goal d_start, d_goal [n][Q], the start links d_sidx, d_sw [ks][Q] (start -> node), the goal
 * links d_gidx, d_gw [kg][Q] (node -> goal, checked with reverse) and the direct weight d_direct [Q].  The distance
 * to the goal d[u] starts as u's goal-link weight (+inf without one) and every node relaxes d[v] = min(d[v], w(v, u) +
 * d[u]) over its own out-list until nothing changes: the values of Dijkstra's algorithm with each route summed from
 * the goal backwards, whatever the sweep order.  A NaN or negative index is no edge; weights are >= 0.  The first hop
 * is the direct edge if its weight is <= every d_sw[s] + d[d_sidx[s]] (ties to the direct edge, then to the lowest
 * slot); the successor of a node is the goal if its goal-link weight equals d[v], else the lowest-index u of its
 * out-list with w(v, u) + d[u] == d[v] exactly.  Outputs (any may be NULL): d_path [Lmax][Q][n] -- the layout
 * optik_hip_path_optimize takes -- holds the start, the nodes walked and the goal, padded with the goal; d_len [Q]
 * the waypoints before the padding; d_cost [Q]; d_status [Q]:
 *   0 found; 1 no route (cost +inf); 2 the route needs more than Lmax waypoints (the true cost); 3 the start, the
 *   goal, the direct weight or a link weight is NaN (cost NaN).  Unless 0: len 2, the start, then the goal repeated.
 * The walk stops at Lmax waypoints whatever the successors say (a zero-weight cycle between duplicate nodes ends
 * there, as status 2).  One workgroup per query, d in LDS -- two buffers of N doubles, which is where the cap on N
 * comes from; a query's result does not depend on Q. */
#define OPTIK_HIP_ROADMAP_MAX_NODES 8192
#define OPTIK_HIP_ROADMAP_MAX_K 16
int optik_hip_roadmap_knn(const optik_hip_chain *chain, const double *d_q, int64_t Q, const double *d_nodes, int32_t N,
                          int32_t k, int32_t exclude_self, int32_t *d_idx, double *d_dist, void *stream);
int optik_hip_roadmap_edges(optik_hip_chain *chain, const double *ee_offset7, const double *d_from, int64_t Q,
                            const double *d_nodes, int32_t N, const int32_t *d_idx, int32_t k, double resolution,
                            int32_t reverse, double *d_w, void *stream);
int optik_hip_roadmap_query(const optik_hip_chain *chain, const double *d_nodes, int32_t N, const int32_t *d_nbr,
                            const double *d_w, int32_t k, const double *d_start, const double *d_goal, int64_t Q,
                            const int32_t *d_sidx, const double *d_sw, int32_t ks, const int32_t *d_gidx,
                            const double *d_gw, int32_t kg, const double *d_direct, int32_t Lmax, double *d_path,
                            int32_t *d_len, double *d_cost, int32_t *d_status, void *stream);

/* Lazy roadmaps (extension; the rules: csrc/roadmap_lazy_measure.hpp): Lazy PRM.  The nodes
 * and the neighbour lists of a roadmap depend on the joint limits alone, so they survive every change of the world.
 * The edges are presumed free and checked -- by optik_hip_collision_motion_batch's own code, in the direction v ->
 * d_nbr[s][v] -- only when a shortest route uses them; a verdict holds until the next reset.  The state, all [k][N]
 * and caller-owned: the unchecked weights d_w0 (the motion's length; +inf for an empty slot or a length that is NaN
 * or infinite), the int32 verdicts d_verdict (OPTIK_HIP_ROADMAP_UNKNOWN / _FREE / _BLOCKED) and the working weights
 * d_w = d_w0 with +inf at the blocked slots: the graph optik_hip_roadmap_query sees.
 *
 * optik_hip_roadmap_query_route: optik_hip_roadmap_query with two more outputs [Lmax][Q] int32 (either may be NULL;
 * both NULL: optik_hip_roadmap_query itself): d_route, the node of waypoint t for 1 <= t < len - 1 and -1 elsewhere;
 * d_hop, the slot s of the graph hop that leaves waypoint t -- the LOWEST s with d_nbr[s][v] == u and d_w[s][v] +
 * d[u] == d[v] --, -1 for the route's last node (it leaves by its goal link) and elsewhere.
 *
 * optik_hip_roadmap_lazy_reset: lengths != 0 first writes d_w0 from d_nodes and d_nbr (otherwise d_w0 is read as it
 * is).  d_node_free [N] uint8 NULL: the nodes are classified by optik_hip_collision_batch against the chain's model
 * and world (clearance >= margin; every node is free without a model).  A slot is BLOCKED if it is empty, if d_w0 is
 * +inf or if either of its nodes is not free -- exactly the edges that the motion check refuses for their end points
 * alone --, every other slot UNKNOWN.  Stream-ordered, no host synchronisation.
 *
 * optik_hip_roadmap_lazy_plan: the query's arguments (links and direct weight checked by the caller, as for
 * optik_hip_roadmap_query) and `rounds` in 0 .. OPTIK_HIP_ROADMAP_LAZY_MAX_ROUNDS.  A pass is
 * optik_hip_roadmap_query_route for all Q queries on d_w.  C is the set of UNKNOWN hop slots over the FOUND routes of
 * the pass, each slot once.  If C is empty, or after `rounds` checks, the call ends; otherwise the motions of C are
 * checked at `resolution`, a free one makes its slot FREE, any other BLOCKED with d_w = +inf, and the next pass
 * follows.  Outputs as optik_hip_roadmap_query (any may be NULL) with one more status:
 *   4 unsettled: the last pass found a route that still holds an UNKNOWN slot.  len 2, the start, then the goal
 *   repeated; the cost is that route's, a lower bound.
 * Status 2 keeps its meaning; its route is not walked, so none of it is checked, and its cost is a lower bound too.
 * For status 0, 1 and 3 the status, len, cost and path are those of optik_hip_roadmap_query over the eagerly checked
 * graph (optik_hip_roadmap_edges on every slot), bit for bit.  *rounds_used (the checks made) and *checked (the sizes
 * of the C sets added up) are host words, may be NULL; like every output they do not depend on the order in which
 * the device claims slots.  rounds = 0 makes one pass and checks nothing.
 * The loop runs on the host: it reads one int32, the size of C, per round -- one synchronise of `stream` per round,
 * none once `rounds` checks are made.  The routes, the claimed slots and their segments are the chain's workspace,
 * grown on demand: one call per chain handle at a time; calls that share d_w and d_verdict must not overlap.
 *
 * optik_hip_roadmap_lazy_plan_from_flags (a test hook, as optik_hip_select_from_keys): the same loop with d_edge_free
 * [k][N] uint8 in place of the motion check; d_node_free [N] uint8 not NULL runs the reset from it first (d_w0 is
 * read), NULL continues with d_w and d_verdict as they are.
 *
 * All four refuse what optik_hip_roadmap_query and optik_hip_roadmap_edges refuse, with the same codes, and rounds
 * outside 0 .. 4096 with OPTIK_HIP_EINVAL, before any device work. */
#define OPTIK_HIP_ROADMAP_UNKNOWN 0
#define OPTIK_HIP_ROADMAP_FREE 1
#define OPTIK_HIP_ROADMAP_BLOCKED 2
#define OPTIK_HIP_ROADMAP_UNSETTLED 4
#define OPTIK_HIP_ROADMAP_LAZY_MAX_ROUNDS 4096
int optik_hip_roadmap_query_route(const optik_hip_chain *chain, const double *d_nodes, int32_t N, const int32_t *d_nbr,
                                  const double *d_w, int32_t k, const double *d_start, const double *d_goal, int64_t Q,
                                  const int32_t *d_sidx, const double *d_sw, int32_t ks, const int32_t *d_gidx,
                                  const double *d_gw, int32_t kg, const double *d_direct, int32_t Lmax, double *d_path,
                                  int32_t *d_len, double *d_cost, int32_t *d_status, int32_t *d_route, int32_t *d_hop,
                                  void *stream);
int optik_hip_roadmap_lazy_reset(optik_hip_chain *chain, const double *ee_offset7, const double *d_nodes, int32_t N,
                                 const int32_t *d_nbr, int32_t k, int32_t lengths, double *d_w0,
                                 const uint8_t *d_node_free, int32_t *d_verdict, double *d_w, void *stream);
int optik_hip_roadmap_lazy_plan(optik_hip_chain *chain, const double *ee_offset7, const double *d_nodes, int32_t N,
                                const int32_t *d_nbr, double *d_w, int32_t *d_verdict, int32_t k, double resolution,
                                const double *d_start, const double *d_goal, int64_t Q, const int32_t *d_sidx,
                                const double *d_sw, int32_t ks, const int32_t *d_gidx, const double *d_gw, int32_t kg,
                                const double *d_direct, int32_t Lmax, int32_t rounds, double *d_path, int32_t *d_len,
                                double *d_cost, int32_t *d_status, int32_t *rounds_used, int64_t *checked,
                                void *stream);
int optik_hip_roadmap_lazy_plan_from_flags(optik_hip_chain *chain, const double *d_nodes, int32_t N,
                                           const int32_t *d_nbr, double *d_w0, double *d_w, int32_t *d_verdict,
                                           int32_t k, const uint8_t *d_edge_free, const uint8_t *d_node_free,
                                           const double *d_start, const double *d_goal, int64_t Q,
                                           const int32_t *d_sidx, const double *d_sw, int32_t ks,
                                           const int32_t *d_gidx, const double *d_gw, int32_t kg,
                                           const double *d_direct, int32_t Lmax, int32_t rounds, double *d_path,
                                           int32_t *d_len, double *d_cost, int32_t *d_status, int32_t *rounds_used,
                                           int64_t *checked, void *stream);

/* Goal-set planning (extension; the rules, the theorem and their operation order:
 * csrc/roadmap_goals_measure.hpp): optik_hip_roadmap_query with G goal slots per query, 1 <= G <=
 * OPTIK_HIP_ROADMAP_MAX_GOALS, in place of the one goal -- the IK solutions of a pose, for one.  d_goals [G][n][Q];
 * d_gcount [Q] int32: only the goals g < gcount exist (a count outside 0 .. G is clamped), and NOTHING of the others is
 * read, so the NaN rows optik_hip_ik_solutions leaves past its count are harmless.  Per goal its goal links d_gidx, d_gw
 * [G][kg][Q] (node -> goal, checked with reverse) and its direct weight d_direct [G][Q]; the start links as before.
 * The shortest-path tree grows from the goals, so d[u] starts as the minimum over the counted goals' link weights of u
 * and one run of the relaxation serves all of them: the cost is the minimum over g < gcount of
 * optik_hip_roadmap_query's cost to goal g, bit for bit, and where one goal alone attains it, status, len and path
 * are that query's too.  Ties: the direct edge of the lowest goal, then the lowest start slot; a node's successor is
 * the lowest goal whose own link weight equals d[v], then the lowest node index.  Outputs (any may be NULL): d_path,
 * d_len, d_cost, d_status as optik_hip_roadmap_query (status 3: a NaN in the start, a start link weight, or a counted
 * goal, its link weights or its direct weight; gcount = 0: status 1); d_which [Q] int32, the goal reached for status 0
 * and -1 otherwise.  A found path ends in goal `which` and is padded with it; any other is the start, then goal 0
 * repeated (the start repeated for gcount = 0).  d_route, d_hop [Lmax][Q] as optik_hip_roadmap_query_route.  With G =
 * 1 and gcount = 1 every output equals optik_hip_roadmap_query_route's, bit for bit.  Refuses what
 * optik_hip_roadmap_query refuses, with the same codes, and G outside 1 .. 16 with OPTIK_HIP_EINVAL, before any device
 * work.  Stream-ordered, no host synchronisation; one workgroup per query, the counted links staged in LDS. */
#define OPTIK_HIP_ROADMAP_MAX_GOALS 16
int optik_hip_roadmap_query_goals(const optik_hip_chain *chain, const double *d_nodes, int32_t N, const int32_t *d_nbr,
                                  const double *d_w, int32_t k, const double *d_start, const double *d_goals,
                                  const int32_t *d_gcount, int32_t G, int64_t Q, const int32_t *d_sidx,
                                  const double *d_sw, int32_t ks, const int32_t *d_gidx, const double *d_gw, int32_t kg,
                                  const double *d_direct, int32_t Lmax, double *d_path, int32_t *d_len, double *d_cost,
                                  int32_t *d_status, int32_t *d_which, int32_t *d_route, int32_t *d_hop, void *stream);

/* Goal-set planning on lazy roadmaps (extension; the rules, the theorem and the freezing rule:
 * csrc/roadmap_goals_lazy_measure.hpp): the loop of optik_hip_roadmap_lazy_plan with optik_hip_roadmap_query_goals as
 * its pass.  The state d_w, d_verdict [k][N] is a lazy roadmap's and optik_hip_roadmap_lazy_reset resets it; the query
 * arguments are optik_hip_roadmap_query_goals' (the start links, the G x kg goal links and the G direct weights
 * checked by the caller); `rounds` as optik_hip_roadmap_lazy_plan.  C is the set of UNKNOWN hop slots over the FOUND
 * routes of a pass; the call ends when C is empty or after `rounds` checks.  Outputs as
 * optik_hip_roadmap_query_goals (any may be NULL) with status 4, unsettled: the last pass found a route that still
 * holds an UNKNOWN slot -- len 2, the start, then goal 0 repeated, which -1, the cost that route's, a lower bound.
 * For status 0, 1 and 3 the status, len, cost, path and which are those of optik_hip_roadmap_query_goals over the
 * eagerly checked graph, bit for bit; for status 2 the cost is a lower bound.  gcount = 0 is status 1.
 * skip_settled = 0 runs every pass on all Q queries, as the rules are written.  skip_settled != 0 runs every pass
 * after the first on the live queries only -- those of status 2, and those of status 0 whose route holds an UNKNOWN
 * slot --: their arguments are gathered into compact arrays, queried, and the results scattered back.  A query that
 * is left out is frozen: every later pass would write what it holds, bit for bit (the proof is in the rules' header),
 * so every output, *rounds_used and *checked are identical in the two forms.
 * The loop runs on the host: it reads two int32 in one copy per round, the size of C and the live count -- one
 * synchronise of `stream` per round, none once `rounds` checks are made.  The routes, the lists, the compact arrays
 * (room for Q queries) and the claimed segments are the chain's lazy workspace, grown on demand: one call per chain
 * handle at a time; calls that share d_w and d_verdict must not overlap.
 * optik_hip_roadmap_lazy_plan_goals_from_flags (a test hook): d_edge_free [k][N] uint8 in place of the motion check,
 * d_node_free [N] uint8 not NULL runs the reset from it first, as optik_hip_roadmap_lazy_plan_from_flags.
 * Both refuse what optik_hip_roadmap_query_goals and optik_hip_roadmap_lazy_plan refuse (rounds outside 0 .. 4096, the
 * resolution, prismatic chains, Q above 2^30), with the same codes, before any device work; Q = 0 is a no-op. */
int optik_hip_roadmap_lazy_plan_goals(optik_hip_chain *chain, const double *ee_offset7, const double *d_nodes,
                                      int32_t N, const int32_t *d_nbr, double *d_w, int32_t *d_verdict, int32_t k,
                                      double resolution, const double *d_start, const double *d_goals,
                                      const int32_t *d_gcount, int32_t G, int64_t Q, const int32_t *d_sidx,
                                      const double *d_sw, int32_t ks, const int32_t *d_gidx, const double *d_gw,
                                      int32_t kg, const double *d_direct, int32_t Lmax, int32_t rounds,
                                      int32_t skip_settled, double *d_path, int32_t *d_len, double *d_cost,
                                      int32_t *d_status, int32_t *d_which, int32_t *rounds_used, int64_t *checked,
                                      void *stream);
int optik_hip_roadmap_lazy_plan_goals_from_flags(optik_hip_chain *chain, const double *d_nodes, int32_t N,
                                                 const int32_t *d_nbr, double *d_w0, double *d_w, int32_t *d_verdict,
                                                 int32_t k, const uint8_t *d_edge_free, const uint8_t *d_node_free,
                                                 const double *d_start, const double *d_goals,
                                                 const int32_t *d_gcount, int32_t G, int64_t Q, const int32_t *d_sidx,
                                                 const double *d_sw, int32_t ks, const int32_t *d_gidx,
                                                 const double *d_gw, int32_t kg, const double *d_direct, int32_t Lmax,
                                                 int32_t rounds, int32_t skip_settled, double *d_path, int32_t *d_len,
                                                 double *d_cost, int32_t *d_status, int32_t *d_which,
                                                 int32_t *rounds_used, int64_t *checked, void *stream);

/* The bidirectional tree planner (extension; the rules and their operation order:
 * csrc/rrt_measure.hpp): RRT-Connect with one extension per tree and iteration, for the queries a roadmap returns as
 * status 1 -- a start or goal in a pocket none of its nodes sees.  It needs no roadmap: each query grows tree 0 from
 * its own start and tree 1 from its own goal, d_start, d_goal [n][Q].  Any revolute chain of 1 .. 16 joint positions;
 * the metric is L-infinity in radians; every motion is checked at `resolution` by optik_hip_collision_motion_batch's
 * own code (classify form, same stream; model, world and ee_offset7 as there) IN THE DIRECTION THE FINAL PATH TRAVELS
 * IT: parent -> child in tree 0, child -> parent in tree 1, tree-0 node -> tree-1 node for a connection.
 *
 * The sample of iteration i is restart seed first + i (optik_hip_seed_batch) for EVERY query; the queries differ by
 * their ends.  A tree holds at most max_nodes nodes, a configuration and a parent index each.
 * Before iteration 0: a NaN or infinite joint in the start or goal gives status 3 (cost NaN); a start or goal that is
 * not free by optik_hip_collision_batch status 1 (cost +inf); a free direct motion start -> goal status 0 with len 2.
 * iters is 0 and the trees are empty (nodes 0) for all three.
 * Iteration i, a = i & 1, b = 1 - a, r = sample i:
 *   nearest  p = the node of tree a first in the total order on (distance to r, index): a number before a NaN, then
 *            the smaller distance, then the smaller index (optik_hip_roadmap_knn's order with k = 1);
 *   steer    d = that distance; nothing happens if d is 0, NaN or infinite; c = r copied if d <= step, otherwise
 *            c_j = p_j + (step / d) * (r_j - p_j), the quotient, the difference, the product and the sum each rounded;
 *            then if (c_j < lo_j) c_j = lo_j; if (c_j > hi_j) c_j = hi_j;
 *   extend   nothing more happens if tree a is full or the motion between p and c is not free (or not sampled);
 *            otherwise c joins tree a with parent p;
 *   connect  m = the nearest node of tree b to c.  If the motion between c and m is free the query is found.  If not,
 *            and the distance of m and c is > step and tree b is not full, e = steer from m towards c joins tree b with
 *            parent m if the motion between m and e is free.
 * A found path is tree 0 from its root to its junction node, then tree 1 from its junction node to its root: W
 * waypoints, the cost the sum of their consecutive distances added from the start forwards.  Outputs (any may be
 * NULL): d_path [Lmax][Q][n] -- the layout optik_hip_path_shortcut, _path_resample and _path_optimize take --,
 * d_len [Q], d_cost [Q], d_status [Q]:
 *   0 found, W <= Lmax: the waypoints padded with the goal; 1 no junction after `iters` iterations (cost +inf);
 *   2 found with W > Lmax (the true cost); 3 as above.  Unless 0: len 2, the start, then the goal repeated.
 * d_iters [Q]: the iterations run before the query ended (i + 1 when iteration i found it, `iters` for status 1);
 * d_nodes [2][Q]: the sizes of the two trees.
 * A query's result does not depend on Q, on how the queries are chunked, on `poll` or on a launch shape, and is bit
 * for bit rrt_measure.hpp's serial reference given the same samples and motion verdicts.
 * The loop over the iterations runs on the host, stream-ordered: per iteration one kernel of its own (one wave per
 * query: the commit of the iteration before, both nearest searches and the steers) and the motion check over 3 Q
 * segments; every `poll` iterations it reads one int32, the number of queries that have not ended, and stops at 0 --
 * one synchronise of `stream` per poll.  Ended queries hand the motion check NaN segments, which it does not sample.
 * The trees are the chain's workspace, grown on demand: 2 * max_nodes * (8 n + 4) bytes per query, the queries in
 * chunks of at most OPTIK_HIP_RRT_CHUNK_BYTES of it (optik_hip_rrt_chunk: that many queries), one after the other on
 * the stream.  One call per chain handle at a time.
 * Refused with OPTIK_HIP_EINVAL before any device work: Q < 0 (Q = 0 is a no-op) or above 2^30, iters outside 1 ..
 * OPTIK_HIP_RRT_MAX_ITERS, a step that is not finite and > 0, max_nodes outside 2 .. OPTIK_HIP_RRT_MAX_NODES, Lmax
 * outside 2 .. 64, poll outside 1 .. OPTIK_HIP_RRT_MAX_POLL, a resolution that is not finite and > 0; with
 * OPTIK_HIP_EUNSUPPORTED, also when Q = 0: chains with prismatic joints. */
#define OPTIK_HIP_RRT_MAX_ITERS 65536
#define OPTIK_HIP_RRT_MAX_NODES 4096
#define OPTIK_HIP_RRT_MAX_POLL 65536
#define OPTIK_HIP_RRT_CHUNK_BYTES (256ll << 20)
int optik_hip_rrt_plan(optik_hip_chain *chain, const double *ee_offset7, const double *d_start, const double *d_goal,
                       int64_t Q, int32_t iters, double step, double resolution, uint64_t first, int32_t max_nodes,
                       int32_t Lmax, int32_t poll, double *d_path, int32_t *d_len, double *d_cost, int32_t *d_status,
                       int32_t *d_iters, int32_t *d_nodes, void *stream);
int64_t optik_hip_rrt_chunk(const optik_hip_chain *chain, int32_t max_nodes);

/* A test hook (a diagnostic, as optik_hip_select_from_keys): `nearest` and `steer` of the tree planner on a tree the
 * caller wrote, with no planner around them -- the wave code that every iteration of optik_hip_rrt_plan, _plan_goals
 * and _plan_constrained runs (the step kernel's own nearest search and rrt_measure.hpp's steer_joint, not copies).
 * d_conf [n][max_nodes]: node j's joint i at i * max_nodes + j, the planner's layout of one tree; only the nodes
 * j < count are read.  d_x [n][X]: X query points, one wave each.  n and the joint limits lo, hi are the chain's;
 * neither a model nor a world is read.  Outputs, none may be NULL:
 *   d_index [X] int32   the node first in the total order on (distance to x, index) -- a number before a NaN, the
 *                       smaller distance, the smaller index; never -1, since count >= 1;
 *   d_dist [X]          that node's L-infinity distance to x (NaN if every node's is);
 *   d_cand [n][X]       the steer from that node towards x with `step`, clamped to lo, hi -- the candidate c of an
 *                       iteration.  Where the planner's iteration ends without a candidate, d_dist 0 (x equals the
 *                       node), NaN or infinite, every joint of the column is NaN.
 * Stream-ordered, no workspace, no lock.  Refused with OPTIK_HIP_EINVAL before any device work: X < 0 (X = 0 is a
 * no-op) or above 2^30, a step that is not finite and > 0, max_nodes outside 1 .. OPTIK_HIP_RRT_MAX_NODES (a tree of
 * one node is a tree here), count outside 1 .. max_nodes, and, where X > 0, a NULL buffer (at X = 0 no buffer is
 * looked at and all may be NULL); with OPTIK_HIP_EUNSUPPORTED, also when X = 0, chains of more than 16 joint
 * positions. */
int optik_hip_rrt_nearest_from_nodes(optik_hip_chain *chain, const double *d_conf, int32_t max_nodes, int32_t count,
                                     const double *d_x, int64_t X, double step, int32_t *d_index, double *d_dist,
                                     double *d_cand, void *stream);

/* The tree planner with a goal set (extension; the rules and their operation order:
 * csrc/rrt_goals_measure.hpp): optik_hip_rrt_plan with G goal slots per query, 1 <= G <= OPTIK_HIP_RRT_MAX_GOALS, in
 * place of the one goal -- the IK solutions of a pose, for one.  d_goals [G][n][Q]; d_gcount [Q] int32: only the goals
 * g < gcount exist (a count outside 0 .. G is clamped), and NOTHING of the others influences any output, so the NaN
 * rows optik_hip_ik_solutions leaves past its count are the normal input.  d_gcount NULL: every query's count is G,
 * all slots exist.  Tree 1 has one root per counted goal that
 * is free, and the query ends at the FIRST junction with any of them: past the direct motions the answer is the goal
 * joined first, not the cheapest one.
 * Before iteration 0, in this order: a NaN or infinite joint in the start or in any counted goal gives status 3 (cost
 * NaN); gcount = 0 status 1; a start that is not free by optik_hip_collision_batch status 1; the counted goals that
 * are free become the roots of tree 1 in ascending g, nodes 0 .. R - 1 with parent -1; R = 0 gives status 1; among the
 * roots whose direct motion start -> goal is free the one with the smallest distance, a tie going to the lower g,
 * gives status 0 with len 2 and which = that g.  iters is 0 and the trees are empty (nodes 0) in all of these.
 * The iterations are optik_hip_rrt_plan's, by the same kernel: nearest, steer, extend, connect and the
 * back-extension.  A tree holds at most max_nodes nodes and the roots count, so a tree 1 full of roots never grows.
 * A found path is tree 0 from its root to its junction node, then tree 1 from its junction node up the parent links to
 * a root; d_which [Q] int32 is the goal slot of that root for status 0 and -1 otherwise (also for status 2, which
 * keeps the cost).  The path is padded with goal `which` for status 0; any other is the start, then goal 0 repeated
 * (the start repeated for gcount = 0), len 2.  The other outputs, the workspace, the chunks (optik_hip_rrt_chunk: the
 * trees are the same size) and the polling are optik_hip_rrt_plan's; any output may be NULL.  With G = 1 and gcount =
 * 1 every output equals optik_hip_rrt_plan's bit for bit, and which is 0 where the status is 0: optik_hip_rrt_plan IS
 * this call with G = 1, d_goals = d_goal ([1][n][Q] is [n][Q]), d_gcount NULL and d_which NULL, behind its own
 * refusals.  A query's result
 * does not depend on Q, on the chunking, on `poll` or on a launch shape, and is bit for bit rrt_goals_measure.hpp's
 * serial reference given the same samples and verdicts.
 * Before iteration 0 the call classifies (1 + G) Q configurations in one optik_hip_collision_batch call -- a slot that
 * is not counted goes in as the start again -- and G Q direct motions in one optik_hip_collision_motion_batch call, a
 * slot that is not counted as a NaN segment, which is not sampled; no flag of such a slot is read.
 * Refused with OPTIK_HIP_EINVAL before any device work: G outside 1 .. 16, max_nodes outside max(2, G) ..
 * OPTIK_HIP_RRT_MAX_NODES, and what optik_hip_rrt_plan refuses; with OPTIK_HIP_EUNSUPPORTED, also when Q = 0: chains
 * with prismatic joints.  Q = 0 is otherwise a no-op.  One call per chain handle at a time. */
#define OPTIK_HIP_RRT_MAX_GOALS 16
int optik_hip_rrt_plan_goals(optik_hip_chain *chain, const double *ee_offset7, const double *d_start,
                             const double *d_goals, const int32_t *d_gcount, int64_t Q, int32_t G, int32_t iters,
                             double step, double resolution, uint64_t first, int32_t max_nodes, int32_t Lmax,
                             int32_t poll, double *d_path, int32_t *d_len, double *d_cost, int32_t *d_status,
                             int32_t *d_iters, int32_t *d_nodes, int32_t *d_which, void *stream);

/* The tree planner under a pose constraint (extension; the rules and their operation order:
 * csrc/rrt_constrained_measure.hpp): optik_hip_rrt_plan_goals with every node projected onto the pose constraint
 * (ref7, lo6, hi6: the constraint calls' below) before it joins a tree, and every motion judged by
 * optik_hip_collision_motion_batch AND by optik_hip_constraint_motion_batch at tol, in the direction the path travels
 * it -- a constrained bidirectional RRT, the fallback of a constrained roadmap's status-1 rows.  The rules are
 * optik_hip_rrt_plan_goals' with these changes and no others:
 *  - Before iteration 0 a configuration is free if it is free by optik_hip_collision_batch and its violation
 *    (optik_hip_constraint_batch) is <= tol; a direct motion is free if both motion checks pass.  So a start that
 *    violates the constraint gives status 1 and a counted goal that violates it is not a root; the order of the cases
 *    is unchanged.
 *  - The steered, clamped candidate c is projected: optik_hip_constraint_project_batch's method with tol = ptol,
 *    iters = piters, damping, max_step.  The iteration does nothing if the status is not
 *    OPTIK_HIP_CONSTRAINT_PROJECTED, or if the projection ran at least one iteration and its result equals the node p
 *    it was steered from in every joint.  Otherwise the projected c' replaces c everywhere: the motion p - c' must pass
 *    both checks, m is the nearest node of the other tree to c', a connection c' - m that passes both ends the query.
 *  - The back-extension e = steer(m, c'), under optik_hip_rrt_plan's conditions on the distance of m and c', is
 *    projected the same way; a projection that is not taken means no back-extension; the motion m - e' must pass both.
 *  - The samples are the restart seeds first + i, not projected; route, status and padding are unchanged.
 * d_projected [2][Q] int32: the projections attempted and those that ended OPTIK_HIP_CONSTRAINT_PROJECTED, candidates
 * and back-extensions together, 0 where the iterations never began.  The other outputs are
 * optik_hip_rrt_plan_goals'; any may be NULL.  The single-goal call is this one with G = 1, d_gcount NULL and d_which
 * NULL.  With a box that is free on all six axes (lo = -inf, hi = +inf) every projection returns its input after 0
 * iterations and every constraint verdict is ok wherever the motion is sampled: every shared output equals
 * optik_hip_rrt_plan_goals' bit for bit.  Every node but the roots has violation <= ptol and lies inside the joint
 * limits; between the nodes holds what the motion check found at its samples with tol -- edge interiors are not
 * projected, so tol is the caller's statement and has no default.  OPTIK_HIP_RRT_PROJECT_ITERS is the default piters
 * of the layers above (the table).
 * An iteration is seven launches: this planner's step kernel with the projection inside, the motion check's five and
 * optik_hip_constraint_motion_batch's one on the same 3 Q segments.  The extra workspace is a few bytes per query;
 * optik_hip_rrt_chunk keeps its meaning.  A query's result does not depend on Q, on the chunking, on `poll` or on a
 * launch shape, and is bit for bit rrt_constrained_measure.hpp's serial reference given the same samples, verdicts
 * and projections.
 * Refused before any device work: what optik_hip_rrt_plan_goals refuses; what the constraint calls refuse of the
 * reference, the bounds and tol; ptol not finite and >= 0; piters outside 0 .. OPTIK_HIP_CONSTRAINT_MAX_ITERS; damping
 * not finite and >= 0; max_step not finite and > 0; with OPTIK_HIP_EUNSUPPORTED, also when Q = 0: chains with prismatic
 * joints.  Q = 0 is otherwise a no-op.  One call per chain handle at a time. */
#define OPTIK_HIP_RRT_PROJECT_ITERS 16
int optik_hip_rrt_plan_constrained(optik_hip_chain *chain, const double *ee_offset7, const double *ref7,
                                   const double *lo6, const double *hi6, double tol, double ptol, int32_t piters,
                                   double damping, double max_step, const double *d_start, const double *d_goals,
                                   const int32_t *d_gcount, int64_t Q, int32_t G, int32_t iters, double step,
                                   double resolution, uint64_t first, int32_t max_nodes, int32_t Lmax, int32_t poll,
                                   double *d_path, int32_t *d_len, double *d_cost, int32_t *d_status, int32_t *d_iters,
                                   int32_t *d_nodes, int32_t *d_which, int32_t *d_projected, void *stream);

/* Path shortcutting and equal-spacing resampling (extension; the arithmetic and its operation
 * order: csrc/shortcut_measure.hpp).  Paths are d_path [Lin][P][n] -- the layout optik_hip_roadmap_query writes and
 * optik_hip_path_optimize reads --, path p having d_len[p] waypoints (d_len NULL: Lin each) and padding behind them
 * that is not looked at.  Any revolute chain of 1 .. 16 joint positions; the metric is L-infinity in radians.
 *
 * optik_hip_path_shortcut: each path's polyline is subdivided into at most V vertices -- its own waypoints, bit for
 * bit, plus interior points of the motion check's interpolation at a spacing of about length / (V - len) --, EVERY
 * pair i < j of them is checked as the motion vertex i -> vertex j at `resolution` by the motion check's own code
 * (classify form, same stream; model, world and ee_offset7 as there; without a model every finite motion is free), and
 * the route 0 -> last that minimises the sum of (length + hop_penalty) per hop over that visibility graph is walked: the
 * optimum over all vertex shortcuts, deterministic.  Exact ties go to the hop that reaches furthest.  hop_penalty >= 0,
 * in radians, keeps a detour through a collinear vertex -- equal to the direct hop up to one rounding in this metric
 * -- from deciding the waypoint count.  Outputs, any may be NULL: d_out [Lout][P][n] the route's vertices padded with
 * the goal; d_len_out [P] the waypoints before the padding; d_cost [P] the route's pure length summed from the goal
 * backwards, without penalties; d_cost_in [P] the same for the input; d_status [P]:
 *   0 route found (every hop a motion checked free in the direction of travel);
 *   1 no route through the visibility graph (the input itself is blocked, or a piece's own samples find what its
 *     parent segment's missed);
 *   2 d_len[p] outside 2 .. min(Lin, V), or the route has more than Lout vertices (d_cost is then its true cost);
 *   3 a NaN or an infinity among the path's waypoints.
 * Unless 0 the input comes back: its waypoints (d_len[p] clamped into 2 .. Lin) padded with the goal if they fit Lout,
 * else the start, then the goal repeated (len 2); d_cost = d_cost_in.  cost <= cost_in is not promised bit for bit
 * (the sums round differently); the route minimises the objective above.
 * Workspace: V (V - 1) / 2 segments per path at 16 n + 1 bytes each, the chain's, grown on demand, next to the motion
 * check's 24 bytes per segment; the paths are processed in chunks of at most OPTIK_HIP_PATH_SHORTCUT_CHUNK_BYTES of
 * it (optik_hip_path_shortcut_chunk: that many paths), back to back on the stream with no host synchronisation.  A
 * path's result does not depend on P, on the chunking or on the launch shape.  One call per chain handle at a time.
 *
 * optik_hip_path_resample: Lout waypoints at equal arc length along each polyline: waypoint j at j / (Lout - 1) of the
 * total length, on the segment that holds it; the ends are copied.  d_out [Lout][P][n]; d_status [P] (may be NULL): 0;
 * 2 for d_len[p] outside 2 .. Lin (resampled as clamped); 3 for a NaN or infinite length (the start, then the goal
 * repeated).  The new waypoints lie on the input, the new segments cut its corners: they are NOT checked.  One thread
 * per (path, waypoint), no workspace.
 *
 * Both refuse with OPTIK_HIP_EINVAL before any device work: V, Lin or Lout outside 2 .. 64, P < 0 (P = 0 is a no-op)
 * or above 2^30, a resolution that is not finite and > 0, a hop_penalty that is NaN, negative or infinite; with
 * OPTIK_HIP_EUNSUPPORTED, also when P = 0: chains with prismatic joints. */
#define OPTIK_HIP_PATH_SHORTCUT_MAX_VERTICES 64
#define OPTIK_HIP_PATH_SHORTCUT_CHUNK_BYTES (256ll << 20)
int optik_hip_path_shortcut(optik_hip_chain *chain, const double *ee_offset7, const double *d_path,
                            const int32_t *d_len, int32_t Lin, int64_t P, int32_t V, double resolution,
                            double hop_penalty, int32_t Lout, double *d_out, int32_t *d_len_out, double *d_cost,
                            double *d_cost_in, int32_t *d_status, void *stream);
int optik_hip_path_resample(const optik_hip_chain *chain, const double *d_path, const int32_t *d_len, int32_t Lin,
                            int64_t P, int32_t Lout, double *d_out, int32_t *d_status, void *stream);
int64_t optik_hip_path_shortcut_chunk(const optik_hip_chain *chain, int32_t V);

/* Shortcutting and resampling that keep a pose constraint (extension; the rules and their
 * operation order: csrc/shortcut_constrained_measure.hpp).  The constraint is ref7, lo6, hi6 as optik_hip_constraint_batch
 * takes it and travels with the call; paths, lengths and outputs are optik_hip_path_shortcut's and _path_resample's.
 *
 * optik_hip_path_shortcut_constrained: optik_hip_path_shortcut with every subdivision vertex that is not one of the
 * input's own waypoints projected onto the constraint (optik_hip_constraint_project_batch's method at ptol, piters,
 * damping, max_step; one vertex per lane) -- a vertex whose projection does not end OPTIK_HIP_CONSTRAINT_PROJECTED is
 * dead: NaN, in no pair, on no route -- and every pair i < j open only where the motion vertex i -> vertex j is free
 * by the motion check AND ok by optik_hip_constraint_motion_batch's rule at `resolution`, tol.  The input's waypoints,
 * the start and the goal among them, are copied bit for bit and never move.  So on a route of status 0 every vertex
 * that is not an input waypoint has violation <= ptol and lies within the joint limits, and every hop has passed both
 * checks in the direction of travel, at the samples; hop interiors are not projected, tol says how far they may leave
 * the constraint.  d_cost may exceed d_cost_in: projected vertices leave the polyline.  d_projected [2][P] (may be
 * NULL): the projections attempted and those that ended projected, both 0 for the statuses 2 and 3 of a bad input.
 * With a box that is free on all six axes and paths within the joint limits every shared output equals
 * optik_hip_path_shortcut's bit for bit.
 * Per chunk, back to back on the stream with no host synchronisation: a gather kernel that builds and projects the
 * vertices, stores them ([n][Pc V] doubles of the workspace) and writes the pair segments; the motion check (classify
 * form); optik_hip_constraint_motion_mask on the same segments and flags; a route kernel that reads the stored
 * vertices -- nothing is projected twice.  Workspace: optik_hip_path_shortcut's plus 8 n V bytes per path
 * (optik_hip_path_shortcut_constrained_chunk: the paths per chunk).  A path's result does not depend on P, on the
 * chunking or on the launch shape.  One call per chain handle at a time.
 *
 * optik_hip_path_resample_constrained: optik_hip_path_resample with every waypoint 0 < j < Lout - 1 projected the same
 * way; one wave per path, lane j = waypoint j.  A projection that does not end projected leaves the interpolated
 * waypoint and gives the path status 4 (OPTIK_HIP_PATH_RESAMPLE_UNPROJECTED), which ranks below 2 and 3; a path of
 * status 3 is not projected.  The spacing is equal before the projection and only approximately equal after it; the
 * new segments are NOT checked.  d_projected [2][P] as above.
 *
 * optik_hip_constraint_motion_mask: d_flag [B] in and out: a segment whose flag is 0 is not sampled and stays 0; every
 * other flag becomes optik_hip_constraint_motion_batch's ok byte for d_qa -> d_qb ([n][B]).  One segment per lane,
 * grid-stride, no atomics.
 *
 * Refusals, before any device work and also when P = 0: optik_hip_path_shortcut's / _path_resample's, then
 * optik_hip_constraint_motion_batch's for the constraint, tol (shortcut and mask only) and the chain, then
 * optik_hip_constraint_project_batch's for ptol, piters, damping and max_step. */
#define OPTIK_HIP_PATH_RESAMPLE_UNPROJECTED 4
int optik_hip_path_shortcut_constrained(optik_hip_chain *chain, const double *ee_offset7, const double *d_path,
                                        const int32_t *d_len, int32_t Lin, int64_t P, int32_t V, double resolution,
                                        double hop_penalty, int32_t Lout, const double *ref7, const double *lo6,
                                        const double *hi6, double tol, double ptol, int32_t piters, double damping,
                                        double max_step, double *d_out, int32_t *d_len_out, double *d_cost,
                                        double *d_cost_in, int32_t *d_status, int32_t *d_projected, void *stream);
int optik_hip_path_resample_constrained(const optik_hip_chain *chain, const double *ee_offset7, const double *d_path,
                                        const int32_t *d_len, int32_t Lin, int64_t P, int32_t Lout, const double *ref7,
                                        const double *lo6, const double *hi6, double ptol, int32_t piters,
                                        double damping, double max_step, double *d_out, int32_t *d_status,
                                        int32_t *d_projected, void *stream);
int optik_hip_constraint_motion_mask(const optik_hip_chain *chain, const double *ee_offset7, const double *ref7,
                                     const double *lo6, const double *hi6, const double *d_qa, const double *d_qb,
                                     int64_t B, double resolution, double tol, uint8_t *d_flag, void *stream);
int64_t optik_hip_path_shortcut_constrained_chunk(const optik_hip_chain *chain, int32_t V);

/* Path optimisation that keeps a pose constraint (extension; the rule and its operation order:
 * csrc/path_optimize.hpp step 7 on top of csrc/constraint_measure.hpp).  optik_hip_path_optimize with the constraint
 * ref7, lo6, hi6 of optik_hip_constraint_batch: projected covariant gradient smoothing.  Each of the `iters` updates is
 * optik_hip_path_optimize's update, the clamp included, and then every interior waypoint on its own is projected back
 * onto the constraint with optik_hip_constraint_project_batch's method at ptol (at most piters iterations, damping,
 * max_step).  A projection that does not end OPTIK_HIP_CONSTRAINT_PROJECTED leaves the waypoint at its value of the
 * previous iterate, bit for bit: an interior waypoint that satisfies the constraint at ptol on input satisfies it in
 * every iterate.  The two ends never move and are never projected.  It is projection after the step, not a projection
 * in the metric; the segments between the waypoints are not looked at (optik_hip_constraint_motion_batch checks them).
 * With a box that is free on all six axes nothing is projected and the shared outputs are optik_hip_path_optimize's,
 * bit for bit.
 * Outputs as there, plus d_violation [P]: the largest violation (optik_hip_constraint_batch's) over all L waypoints of
 * the last iterate, the two ends included, NaN if one of them is; and d_projected [2][P] int32: the projections
 * attempted over all updates, then those that ended projected.  Any output may be NULL.
 * One wave per path, the whole loop in one launch, the projections one waypoint per lane; stream-ordered, no
 * workspace, no allocation.  K updates in one call give the bits of K calls of one update (the counters add up),
 * whatever P is.
 * Refusals, before any device work and also when P = 0: optik_hip_path_optimize's, then
 * optik_hip_constraint_project_batch's for the reference, the bounds, ptol, piters, damping and max_step. */
int optik_hip_path_optimize_constrained(const optik_hip_chain *chain, const double *ee_offset7, const double *d_q_in,
                                        int32_t L, int64_t P, int32_t iters, double step, double w_smooth, double w_obs,
                                        double influence, double safety, const double *ref7, const double *lo6,
                                        const double *hi6, double ptol, int32_t piters, double damping, double max_step,
                                        double *d_q_out, double *d_cost_first, double *d_cost_last, double *d_clearance,
                                        int32_t *d_status, double *d_violation, int32_t *d_projected, void *stream);

/* Collision repair (extension; the rules and their operation order: csrc/repair_measure.hpp on
 * top of csrc/collision_gradient.hpp and csrc/constraint_measure.hpp).  Every column of d_x [n][B] on its own is pushed
 * out of collision: while its clearance (optik_hip_collision_batch's number: the margin is not in it) is below `safety`
 * it steps by `step` down the gradient of optik_hip_path_optimize's hinge of its witness rows (influence, safety),
 * clamped to the joint limits, and -- with a pose box ref7, lo6, hi6 of optik_hip_constraint_batch -- is projected back
 * onto the box with optik_hip_constraint_project_batch's method at ptol (piters, damping, project_max_step); at most
 * `iters` (0 .. OPTIK_HIP_REPAIR_MAX_ITERS) steps.  ref7, lo6 and hi6 all NULL: no box (ptol .. project_max_step are
 * then ignored).  max_move (>= 0, +inf: no bound) bounds the L-infinity distance from the input.  A fixed step without
 * a line search; step-then-project, not a step in the constraint's null space.
 * d_status [B]:
 *   OPTIK_HIP_REPAIR_FREE   the returned x has clearance >= safety.  With d_iterations > 0 it also lies within the
 *                           joint limits and satisfies the box at ptol; with d_iterations == 0 the input was free
 *                           already and is returned bit for bit, d_moved 0
 *   OPTIK_HIP_REPAIR_LIMIT  `iters` steps were not enough
 *   OPTIK_HIP_REPAIR_STUCK  the gradient vanished, a projection did not end OPTIK_HIP_CONSTRAINT_PROJECTED, or the step
 *                           would have left max_move: x is the last accepted iterate
 *   OPTIK_HIP_REPAIR_NAN    the clearance is NaN (a NaN or infinite joint)
 * and, of the returned x whatever the status: d_x [n][B] (may be the input buffer), d_clearance [B], d_violation [B]
 * (optik_hip_constraint_batch's; 0.0 without a box or with a box free on all six axes), d_moved [B] (max_i |x_i -
 * input_i|), d_iterations [B] (accepted steps).  Any output pointer may be NULL.
 * One configuration per lane, the whole loop in one launch; stream-ordered, no workspace, no allocation; the result of
 * a column does not depend on B or on the launch shape.  Revolute chains of 1 .. 8 joints.
 * Refusals, before any device work and also when B = 0: OPTIK_HIP_EUNSUPPORTED for chains of 9 .. 16 joint positions
 * and prismatic chains; OPTIK_HIP_EINVAL for parameters outside influence > safety >= 0, step > 0 (all finite), iters
 * in 0 .. 4096, max_move >= 0; what optik_hip_constraint_project_batch refuses of a box and its projection's
 * arguments; a chain without a collision model. */
#define OPTIK_HIP_REPAIR_MAX_ITERS 4096
#define OPTIK_HIP_REPAIR_FREE 0
#define OPTIK_HIP_REPAIR_LIMIT 1
#define OPTIK_HIP_REPAIR_STUCK 2
#define OPTIK_HIP_REPAIR_NAN 3
typedef struct optik_hip_collision_repair_outputs {
    double *d_x;             /* [n][B] */
    double *d_clearance;     /* [B] */
    double *d_violation;     /* [B] */
    double *d_moved;         /* [B] */
    int32_t *d_status;       /* [B] */
    int32_t *d_iterations;   /* [B] */
} optik_hip_collision_repair_outputs;
int optik_hip_collision_repair_batch(const optik_hip_chain *chain, const double *ee_offset7, const double *d_x,
                                     int64_t B, double influence, double safety, double step, int32_t iters,
                                     double max_move, const double *ref7, const double *lo6, const double *hi6,
                                     double ptol, int32_t piters, double damping, double project_max_step,
                                     const optik_hip_collision_repair_outputs *out, void *stream);

/* Timing of joint paths under velocity and acceleration limits, and the sampling of the timed trajectory (extension;
 * DESIGN.md section 5.20; the arithmetic and its operation order: csrc/time_measure.hpp).  Paths are d_path [L][P][n]
 * as above, path p having d_len[p] waypoints (d_len NULL: L each), 3 <= d_len[p] <= L <= 64.  Any revolute chain of
 * 1 .. 16 joint positions.
 *
 * optik_hip_path_time: time-optimal path parameterisation by reachability analysis (TOPP-RA) in its collocation form
 * on the path's own waypoints, rest to rest, under d_vmax [n] (> 0, may be +inf) and d_amax [n] (finite, > 0), both
 * in device memory.  One backward pass gives the largest admissible squared path speed per waypoint in closed form,
 * one greedy forward pass the profile: always feasible, optimal where the path is dense and gently curved (every
 * |second difference| <= |first difference| / 2); elsewhere it is longer than the optimum, stops at sharp corners,
 * and on a jagged path two neighbouring stops give status 1 (about a third of unbiased random walks; time_measure.hpp).
 * The grid step is the waypoint index, so evenly spaced input -- optik_hip_path_resample's -- is what it is
 * meant for.  Outputs, any may be NULL: d_t [L][P] the time of each waypoint from t = 0; d_qd and d_qdd [L][P][n] the
 * joint velocities and accelerations there; d_x [L][P] the squared path speed; d_duration [P]; d_status [P]:
 *   0 timed (behind the path's own waypoints: the duration, zero velocity, acceleration and x);
 *   1 a segment whose two ends both have x = 0, or a duration that is not finite;
 *   2 d_len[p] outside 3 .. L, or a stage that bounds nothing (a waypoint repeated three times, or twice at the start);
 *   3 a NaN or an infinity among the path's waypoints.
 * Unless 0 every time and the duration are NaN; status 1 still writes its x, velocities and accelerations (they satisfy
 * every limit, the profile just never leaves a waypoint), 2 and 3 write 0 for them.  One wave per path, no workspace; a path's
 * result does not depend on P or on the launch shape and is bit for bit time_measure.hpp's serial reference.
 *
 * optik_hip_trajectory_sample: Tout samples of each timed path at tau = k * dt, k = 0 .. Tout - 1, by cubic Hermite
 * interpolation in time over the waypoints' (time, position, velocity): d_q and d_qd_out [Tout][P][n].  tau >= the
 * duration gives the goal with zero velocity; a path whose status is not 0 gives its start with zero velocity.  The
 * curve leaves the polyline between waypoints: it is NOT checked here.  One thread per (path, sample).
 *
 * Both refuse with OPTIK_HIP_EINVAL before any device work: L outside 3 .. 64, P < 0 (P = 0 is a no-op) or above
 * 2^30, a dt that is not finite and > 0, Tout outside 1 .. OPTIK_HIP_TRAJECTORY_MAX_SAMPLES; with
 * OPTIK_HIP_EUNSUPPORTED, also when P = 0: chains with prismatic joints, whose limits are not radians. */
#define OPTIK_HIP_PATH_TIME_MAX_WAYPOINTS 64
#define OPTIK_HIP_TRAJECTORY_MAX_SAMPLES 65536
int optik_hip_path_time(const optik_hip_chain *chain, const double *d_path, const int32_t *d_len, int32_t L, int64_t P,
                        const double *d_vmax, const double *d_amax, double *d_t, double *d_qd, double *d_qdd,
                        double *d_x, double *d_duration, int32_t *d_status, void *stream);
int optik_hip_trajectory_sample(const optik_hip_chain *chain, const double *d_path, const int32_t *d_len, int32_t L,
                                int64_t P, const double *d_t, const double *d_qd, const int32_t *d_status, double dt,
                                int32_t Tout, double *d_q, double *d_qd_out, void *stream);

/* optik_hip_path_time with limits on the tool as well (extension; the arithmetic and its
 * operation order: csrc/time_tool_measure.hpp).  tool_limits4, in HOST memory: the speed of the tool centre point
 * (m/s), its tangential and its normal acceleration (m/s^2) and the end effector's angular speed (rad/s), each > 0 and
 * +inf for "no limit".  The tool is the pose fk_batch returns, with ee_offset7 (host memory, may be NULL).  The path
 * derivative of that pose, by the same differences over the waypoint index as the joints', gives one more row of each
 * stage (the tangential acceleration) and three more bounds on the squared path speed (speed, normal acceleration,
 * angular speed).  Guaranteed at the waypoints: tool speed <= v, |tangential| <= a_t, normal <= a_n, angular speed <= w,
 * hence |tool acceleration| <= sqrt(a_t^2 + a_n^2).  Not bounded: the angular acceleration and anything between
 * waypoints.  Everything optik_hip_path_time says of its arguments, outputs and statuses holds; three more outputs, any
 * may be NULL: d_tool_speed [L][P], d_tool_accel [L][P][2] (tangential, normal) and d_tool_wspeed [L][P] at the
 * waypoints, 0 wherever the velocities are.  With all four limits +inf the shared outputs are optik_hip_path_time's
 * bit for bit.  One wave per path, the forward kinematics of waypoint i on lane i; no workspace; bit for bit
 * time_tool_measure.hpp's serial reference.  Refusals: optik_hip_path_time's, and OPTIK_HIP_EINVAL for tool_limits4
 * NULL or a tool limit that is NaN or <= 0. */
int optik_hip_path_time_tool(const optik_hip_chain *chain, const double *d_path, const int32_t *d_len, int32_t L,
                             int64_t P, const double *d_vmax, const double *d_amax, const double *tool_limits4,
                             const double *ee_offset7, double *d_t, double *d_qd, double *d_qdd, double *d_x,
                             double *d_duration, int32_t *d_status, double *d_tool_speed, double *d_tool_accel,
                             double *d_tool_wspeed, void *stream);

/* Spline retiming: the stage between optik_hip_path_time / _path_time_tool and optik_hip_trajectory_sample (extension;
 * DESIGN.md section 5.36; the arithmetic and its operation order: csrc/time_spline_measure.hpp).  d_path, d_len, L, P
 * as optik_hip_path_time takes them; d_t_in [L][P] and d_status_in [P] (may be NULL: all 0) are its d_t and d_status.
 * The result is the clamped (rest to rest) C2 cubic spline through the waypoints at the times k * d_t_in, k >= 1 the
 * least factor at which |velocity| <= d_vmax, |acceleration| <= d_amax and |jerk| <= d_jmax [n] (device memory; each
 * > 0, +inf for "no limit") hold along the whole curve, not only at the waypoints; k = 1 returns the input times bit
 * for bit.  Outputs, any may be NULL: d_t [L][P] the new times, d_qd and d_qdd [L][P][n] the spline's velocity and
 * acceleration at the waypoints, d_duration [P], d_factor [P] (k), d_ratios [P][3] (the final peak velocity,
 * acceleration and jerk over their limits, the largest over the joints), d_status [P]: 0; 1 the input status was
 * neither 0 nor 4, or the times do not increase strictly from 0, or k is not finite; 2 a length outside 3 .. min(L,
 * 64); 3 a waypoint or a time that is not finite; 4 a final ratio still above 1 -- the products k * t round the knot
 * times, which moves the jerk ratio by up to a few 1e-12 at 64 waypoints, in rare cases more than the headroom of
 * 3e-12.  A result with status 4 carries valid times: passed in again as d_t_in and d_status_in it is retimed once
 * more (by about 1 + 2e-12) and ends at 0.  For 1 .. 3 the times and the duration are NaN and everything else 0; the
 * waypoints behind a path's own hold the duration and zeros.  A C2 cubic spline is the cubic
 * Hermite curve of its own knot velocities: (d_t, d_qd, d_status) goes into optik_hip_trajectory_sample as it is (a
 * path with status 4 is sampled as its start, like every status other than 0).  The jerk is bounded on the open
 * interval: the motion starts and stops with a finite acceleration step.  One wave per path, striding when the grid is
 * capped; no workspace; bit for bit time_spline_measure.hpp's serial reference.  Refusals: optik_hip_path_time's. */
int optik_hip_path_time_spline(const optik_hip_chain *chain, const double *d_path, const int32_t *d_len, int32_t L,
                               int64_t P, const double *d_t_in, const int32_t *d_status_in, const double *d_vmax,
                               const double *d_amax, const double *d_jmax, double *d_t, double *d_qd, double *d_qdd,
                               double *d_duration, double *d_factor, double *d_ratios, int32_t *d_status,
                               void *stream);

/* The measures of solution modes 3 and 4 for B configurations d_q [n][B] (any chain of 1 .. 16 revolute joint
 * positions): d_w [B] manipulability w = sqrt(det G), d_c [B] condition c = sigma_min / sigma_max, both of the body
 * Jacobian fk_batch returns (ee_offset7 may be NULL).  Either output may be NULL.  A G that is not numerically
 * positive definite (an LDL^T pivot <= 0) gives w = c = 0 exactly.  One thread per configuration, no workspace.
 * Refused with OPTIK_HIP_EUNSUPPORTED: chains with prismatic joints. */
int optik_hip_manip_batch(const optik_hip_chain *chain, const double *ee_offset7, const double *d_q, int64_t B,
                          double *d_w, double *d_c, void *stream);

/* The collision filter (extension; the arithmetic: csrc/collision_measure.hpp).
 * A chain with n joint positions has n + 2 frames: 0 the base (identity), k = 1 .. n the pose after joint k's motion,
 * n + 1 the end effector (the pose fk_batch returns, with the call's ee_offset7).  The model: S robot spheres, each
 * (frame index, centre in that frame, radius >= 0), S <= OPTIK_HIP_MAX_COLLISION_SPHERES; P self pairs (a, b), a != b,
 * P <= OPTIK_HIP_MAX_COLLISION_PAIRS; a margin >= 0.  The world, in the base frame: spheres4 [Ms][4] (centre,
 * radius) and boxes10 [Mb][10] (t, unit quaternion i, j, k, w, half extents), up to OPTIK_HIP_MAX_WORLD_OBSTACLES
 * of each.  The clearance of a configuration is the minimum of every (robot sphere, obstacle) signed distance and
 * every self-pair distance: +inf with nothing to check, NaN for a NaN configuration.  It is free iff
 * clearance >= margin.
 *
 * The filter is active exactly while the chain has a model with S >= 1 (S = 0 clears it).  Then every solver launch
 * (optik_hip_ik_batch, optik_hip_ik_host, optik_hip_ik_solutions, optik_hip_ik_path) runs a key kernel after the
 * solver (and after the key pass of modes 3 and 4), on the same stream, before any selection: each success that
 * is not free gets the key +inf and is never chosen.  Speed is scheduled as Quality (EARLY_EXIT, FIND_ANY and the
 * single-call claim have no effect; every restart runs to its end) with Speed's keys: its winner is the lowest-index
 * free success.  d_status and d_x are left as the solver wrote them, so a rejected restart still shows a success
 * status; optik_hip_collision_batch on d_x gives the reason.  Without a model nothing of this runs.
 *
 * set_collision_model / set_world take host arrays, wait for the chain's device to finish the work in flight and
 * replace the whole model / world (Ms = Mb = 0: an empty world).  Refused with OPTIK_HIP_EINVAL, before any device
 * work: a frame index outside 0 .. n + 1, a non-finite centre, a NaN or negative radius or half extent, a pair index
 * out of range or a == b, a NaN, infinite or negative margin, a box quaternion with |q|^2 more than 1e-9 from 1,
 * counts over the limits; with OPTIK_HIP_EUNSUPPORTED: a model (S >= 1) on a chain with prismatic joints. */
#define OPTIK_HIP_MAX_COLLISION_SPHERES 256
#define OPTIK_HIP_MAX_COLLISION_PAIRS 4096
#define OPTIK_HIP_MAX_WORLD_OBSTACLES 65536
int optik_hip_chain_set_collision_model(optik_hip_chain *chain, const int32_t *frames, const double *centers3,
                                        const double *radii, int32_t S, const int32_t *pairs2, int32_t P,
                                        double margin);
int optik_hip_chain_set_world(optik_hip_chain *chain, const double *spheres4, int32_t Ms, const double *boxes10,
                              int32_t Mb);
/* All n + 2 frames of B configurations d_q [n][B] -> d_frames [B][n + 2][7] (pose7: t, quaternion i, j, k, w);
 * frame n + 1 equals fk_batch's pose bit for bit.  Revolute chains of 1 .. 16 joint positions (prismatic:
 * OPTIK_HIP_EUNSUPPORTED).  Stream-ordered. */
int optik_hip_link_frames_batch(const optik_hip_chain *chain, const double *ee_offset7, const double *d_q, int64_t B,
                                double *d_frames, void *stream);
/* The clearance d_clearance [B] of B configurations d_q [n][B] against the chain's model and world, and the free flag
 * d_free [B] (1 iff clearance >= margin); either may be NULL.  Without a model: clearance +inf (NaN for a NaN
 * configuration), free 1 unless NaN.  Stream-ordered; refused as optik_hip_link_frames_batch. */
int optik_hip_collision_batch(const optik_hip_chain *chain, const double *ee_offset7, const double *d_q, int64_t B,
                              double *d_clearance, uint8_t *d_free, void *stream);

/* The distance-field world (extension; the arithmetic: csrc/collision_measure.hpp, steps
 * 5 - 7): a third obstacle kind next to the spheres and boxes, a sampled signed distance field (an ESDF / TSDF voxel
 * grid) that is axis-aligned in the base frame.  Node (i, j, k) sits at origin3 + voxel * (i, j, k); values is float32
 * [nx][ny][nz] in C order (z fastest).  Each robot sphere inside the grid contributes the trilinearly interpolated
 * value at its centre minus its radius to the clearance minimum; a sphere whose centre lies outside [origin, origin +
 * voxel * (n - 1)] on any axis contributes nothing.  Every consumer of the world reads the grid: collision_batch, the
 * collision key pass of the solver launches, collision_motion_batch and ik_path's motion key pass.  The interpolated
 * field approximates the true distance to within sqrt(3) * voxel (for a 1-Lipschitz field) plus f32 rounding: a
 * caller who needs a conservative answer adds that to the margin.
 *
 * optik_hip_chain_set_world_grid takes host arrays, waits for the chain's device as set_world does and replaces the
 * whole grid; values == NULL with nx = ny = nz = 0 clears it.  set_world leaves the grid alone and this call leaves
 * the spheres and boxes alone.  Refused with OPTIK_HIP_EINVAL before any device work: a dimension outside 2 ..
 * OPTIK_HIP_MAX_GRID_DIM, more than OPTIK_HIP_MAX_GRID_NODES nodes, a voxel that is zero, negative, NaN or infinite,
 * a non-finite origin, a NaN or infinite value.
 *
 * optik_hip_world_grid_bake writes (float)(the signed distance of the chain's current spheres and boxes at the
 * node) for every node of the given grid to d_values_out (device memory, nx * ny * nz floats).  Stream-ordered; it
 * installs nothing.  Refused as above, and for a world without spheres and boxes. */
#define OPTIK_HIP_MAX_GRID_DIM 1024
#define OPTIK_HIP_MAX_GRID_NODES (1 << 24)
int optik_hip_chain_set_world_grid(optik_hip_chain *chain, const double *origin3, double voxel, int32_t nx, int32_t ny,
                                   int32_t nz, const float *values);
int optik_hip_world_grid_bake(const optik_hip_chain *chain, const double *origin3, double voxel, int32_t nx,
                              int32_t ny, int32_t nz, float *d_values_out, void *stream);

/* From sensor data to a distance-field world (extension; the arithmetic:
 * csrc/collision_measure.hpp, steps 8 and 9).  Both calls take device buffers, are stream-ordered and install nothing:
 * hand the values to optik_hip_chain_set_world_grid.  An occupancy grid is uint8 [nx][ny][nz] on the nodes of a grid
 * as above (z fastest), non-zero = occupied.
 *
 * optik_hip_world_grid_from_occupancy writes the signed field of d_occupied to d_values_out (nx * ny * nz floats) by
 * an exact Euclidean distance transform: voxel * (distance in voxels to the nearest occupied node - 0.5) at a free
 * node, minus voxel * (distance to the nearest free node - 0.5) at an occupied one, clamped to +-max_distance; a grid
 * without occupied (free) nodes is +max_distance (-max_distance) everywhere.  The zero level lies midway between a
 * free node and an occupied neighbour.  The field takes an occupied voxel for its node: it exceeds the distance to
 * the voxel cubes by up to (sqrt(3) - 1) / 2 * voxel, on top of the interpolation bound above; a conservative caller
 * adds both to the margin.  The chain owns the workspace (16 bytes per node, 256 MiB at the 2^24 nodes a grid may
 * have); it grows on demand, which waits for the device, and is freed with the chain.  One call per chain at a time.
 *
 * optik_hip_occupancy_from_points sets d_occupied[node] = 1 at the nearest node (halves up) of each of the N points of
 * d_points3 ([N][3] doubles, base frame) that lies within half a voxel of the grid and in none of the E exclusion
 * spheres of d_exclude4 ([E][4]: centre, radius; the self-filter: the robot's own spheres, optik_amd.collision.
 * spheres_at).  NaN and infinite points are skipped and a NaN sphere excludes nothing.  It only marks and never
 * clears: clouds accumulate, and the caller zeroes the buffer.  N = 0 does nothing.
 *
 * Refused with OPTIK_HIP_EINVAL before any device work: a grid that set_world_grid would refuse for its geometry, a
 * max_distance that is zero, negative, NaN or infinite, N < 0, E outside 0 .. OPTIK_HIP_MAX_EXCLUDE_SPHERES, a null
 * buffer that is needed. */
#define OPTIK_HIP_MAX_EXCLUDE_SPHERES 1024
int optik_hip_world_grid_from_occupancy(optik_hip_chain *chain, double voxel, int32_t nx, int32_t ny, int32_t nz,
                                        const uint8_t *d_occupied, double max_distance, float *d_values_out,
                                        void *stream);
int optik_hip_occupancy_from_points(const optik_hip_chain *chain, const double *origin3, double voxel, int32_t nx,
                                    int32_t ny, int32_t nz, const double *d_points3, int64_t N,
                                    const double *d_exclude4, int32_t E, uint8_t *d_occupied, void *stream);

/* Depth-image worlds: a persistent evidence map with free-space carving (extension; the
 * arithmetic: csrc/depth_measure.hpp).  The map is int16 [nx][ny][nz] in device memory on the nodes of a grid as above
 * (z fastest), owned by the caller: OPTIK_HIP_MAP_UNKNOWN at a node that was never observed (a new map is all that),
 * evidence in [e_min, e_max] elsewhere.  Both calls are stream-ordered and install nothing.
 *
 * optik_hip_depth_integrate applies F depth images (d_depth: [F][H][W] floats in device memory, z-depth in metres
 * along the optical axis, pixel centres at integer coordinates, rectified) to d_map in place, in order.  intrinsics4
 * ([F][4]: fx, fy, cx, cy) and poses16 ([F][16]: the camera in the base frame as a column-major 4x4, x right, y down,
 * z forward) are HOST arrays, read before the call returns.  Every node is projected into each image and gathers the
 * nearest pixel: a node in front of the surface by more than `band` loses `miss` (carved free; floor e_min), a node
 * within `band` of it gains `hit` (ceiling e_max), a node behind it, outside the image, outside (z_near, z_far] or
 * under an invalid pixel (NaN, infinite, <= z_near) keeps its value; a pixel beyond z_far carves up to z_far and marks
 * nothing.  A pixel whose point lies in one of the E exclusion spheres of d_exclude4 ([E][4] doubles in device memory,
 * base frame: the self-filter) carves in front of itself and marks nothing.  A call with F frames leaves the bits
 * that F calls with one frame leave.  The cleaned images live in a workspace the chain owns (4 bytes per pixel of up
 * to 8 frames, at most 256 MiB); it grows on demand, which waits for the device, and is freed with the chain.  One
 * call per chain at a time.
 *
 * optik_hip_occupancy_from_map writes d_occupied[node] = unknown_occupied (as 0 / 1) where the map is unknown and
 * (e >= threshold) elsewhere; with accumulate != 0 it ORs that into what d_occupied holds, so that a map and a point
 * cloud (optik_hip_occupancy_from_points) feed one distance transform.
 *
 * Refused with OPTIK_HIP_EINVAL before any device work: a grid that set_world_grid would refuse for its geometry, F
 * outside 1 .. OPTIK_HIP_MAX_DEPTH_FRAMES, H or W outside 1 .. OPTIK_HIP_MAX_DEPTH_DIM, E outside 0 ..
 * OPTIK_HIP_MAX_EXCLUDE_SPHERES, unless 0 < z_near < z_far and band >= 0, all finite, hit or miss outside 1 .. 1024,
 * e_min outside -32767 .. 0, e_max outside 0 .. 32767, intrinsics that are not finite with fx, fy > 0, a pose that is
 * not finite, a threshold outside -32767 .. 32767, a null buffer that is needed. */
#define OPTIK_HIP_MAP_UNKNOWN (-32768)
#define OPTIK_HIP_MAX_DEPTH_FRAMES 64
#define OPTIK_HIP_MAX_DEPTH_DIM 4096
int optik_hip_depth_integrate(optik_hip_chain *chain, const double *origin3, double voxel, int32_t nx, int32_t ny,
                              int32_t nz, int16_t *d_map, const float *d_depth, int32_t F, int32_t H, int32_t W,
                              const double *intrinsics4, const double *poses16, const double *d_exclude4, int32_t E,
                              double z_near, double z_far, double band, int32_t hit, int32_t miss, int32_t e_min,
                              int32_t e_max, void *stream);
int optik_hip_occupancy_from_map(const optik_hip_chain *chain, int32_t nx, int32_t ny, int32_t nz, const int16_t *d_map,
                                 int32_t threshold, int32_t unknown_occupied, int32_t accumulate, uint8_t *d_occupied,
                                 void *stream);

/* From a triangle mesh to a distance-field world (extension; the arithmetic:
 * csrc/mesh_measure.hpp).  d_tris9 is a triangle soup in device memory, [M][9] doubles: the vertices a, b, c of each
 * triangle in the base frame; no connectivity, welding or closedness is needed.
 *
 * optik_hip_world_grid_from_mesh writes to d_values_out (nx * ny * nz floats, device memory) the signed distance of
 * every node of the grid to the mesh: the exact point-to-triangle distance, minimised over the triangles, negative
 * where the generalized winding number has magnitude >= 1/2 (so inward-oriented files work, and an open sheet reads
 * as unsigned), clamped to +-max_distance.  This is the true distance: the only error of the resulting world is the
 * sqrt(3) * voxel of the grid's interpolation.  Stream-ordered; it installs nothing: hand the values to
 * optik_hip_chain_set_world_grid.  There is no culling: the cost is nx * ny * nz * M pair evaluations, issued as
 * stream-ordered launches of a bounded number of pairs each.  Finite coordinates are the caller's promise here (the
 * robot-level entry of optik.h checks its host arrays): a NaN or infinite coordinate gives NaN-free but meaningless
 * values.
 *
 * Refused with OPTIK_HIP_EINVAL before any device work: a grid that set_world_grid would refuse for its geometry, M
 * outside 1 .. OPTIK_HIP_MAX_MESH_TRIANGLES, a max_distance that is zero, negative, NaN or infinite, a null buffer.
 *
 * optik_hip_mesh_tile returns the number of triangles the kernel stages at a time.  optik_hip_mesh_pairs_per_launch is
 * a test hook: pairs > 0 sets the launch bound for the process, 0 restores the built-in one, a negative value only
 * asks; it returns the bound in force.  Neither changes a bit of any result. */
#define OPTIK_HIP_MAX_MESH_TRIANGLES (1 << 20)
int optik_hip_world_grid_from_mesh(const optik_hip_chain *chain, const double *origin3, double voxel, int32_t nx,
                                   int32_t ny, int32_t nz, const double *d_tris9, int32_t M, double max_distance,
                                   float *d_values_out, void *stream);
int32_t optik_hip_mesh_tile(void);
int64_t optik_hip_mesh_pairs_per_launch(int64_t pairs);

/* From a solid to a sphere model: a greedy sphere cover (extension; the arithmetic and the
 * guarantee: csrc/spherefit_measure.hpp).  d_values is a signed distance field of the solid on a grid as above
 * (nx * ny * nz floats in device memory, negative inside: what optik_hip_world_grid_from_mesh writes), d_points3 are P
 * points sampled on its surface ([P][3] doubles in device memory, the grid's frame).
 *
 * Every node c of the grid is a candidate sphere: centre at the node, radius r = pad - value[c], a candidate iff
 * r > slack and the value is finite; such a sphere reaches at most `pad` beyond the solid.  It covers a point that
 * lies at least `slack` inside it.  K rounds: each picks the candidate that covers the most points not covered yet
 * (ties: the lower node index) and marks them covered; from the first round whose best gain is 0 on, nothing is chosen.
 * Outputs, device memory: d_chosen int32 [K] the node indices (-1 past the count), d_centers3 [K][3] and d_radii [K]
 * (NaN past the count), d_gains int32 [K] the points each pick newly covered (0 past the count), d_count_uncovered
 * int32 [2]: the number of spheres chosen and the points left uncovered.  With the grid around the points' bounding
 * box and pad >= sqrt(3) * voxel + slack every point can be covered, so a K that is large enough leaves none.
 * Everything decided is an integer: the result does not depend on the launch shape.
 *
 * Stream-ordered, no host synchronisation, and it allocates nothing: d_workspace is device memory of the caller's, at
 * least optik_hip_sphere_fit_workspace_bytes(nx, ny, nz, P) bytes (4 bytes per node, 8 per point and 2 KiB), 4-byte
 * aligned, in use until the call's work has run.  The cost is about 2 * nx * ny * nz * P pair tests, issued as
 * stream-ordered launches of a bounded number of pairs each, and 4 short launches per round.  Finite coordinates are
 * the caller's promise here (the robot-level entry of optik.h checks its host arrays): a NaN point is covered by
 * nothing.  The fit does not read the chain's joints: any chain is accepted, it names the device.
 *
 * Refused with OPTIK_HIP_EINVAL before any device work: a grid that set_world_grid would refuse for its geometry, K
 * outside 1 .. OPTIK_HIP_MAX_FIT_SPHERES, P outside 1 .. OPTIK_HIP_MAX_FIT_POINTS, a pad that is zero, negative, NaN
 * or infinite, a slack that is negative, NaN or not below pad, a null buffer, a workspace that is too small.
 *
 * optik_hip_fit_tile returns the number of points the kernels stage at a time.  optik_hip_fit_pairs_per_launch is a
 * test hook: pairs > 0 sets the launch bound for the process, 0 restores the built-in one, a negative value only asks;
 * it returns the bound in force.  Neither changes an integer of any result. */
#define OPTIK_HIP_MAX_FIT_SPHERES 256
#define OPTIK_HIP_MAX_FIT_POINTS (1 << 20)
int optik_hip_sphere_fit(const optik_hip_chain *chain, const double *origin3, double voxel, int32_t nx, int32_t ny,
                         int32_t nz, const float *d_values, const double *d_points3, int64_t P, double pad,
                         double slack, int32_t K, int32_t *d_chosen, double *d_centers3, double *d_radii,
                         int32_t *d_gains, int32_t *d_count_uncovered, void *d_workspace, int64_t workspace_bytes,
                         void *stream);
int64_t optik_hip_sphere_fit_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int64_t P);
int32_t optik_hip_fit_tile(void);
int64_t optik_hip_fit_pairs_per_launch(int64_t pairs);

/* The motion check (extension; the arithmetic: csrc/motion_measure.hpp): is the straight
 * joint-space segment qa -> qb free at a resolution h > 0 (L-infinity, radians)?  With d = max_i |qb_i - qa_i| the
 * segment has K = max(1, (int)ceil(d / h)) steps and K + 1 samples: sample 0 is qa and sample K is qb, copied, and
 * sample k between them is qa_i + ((double)k / (double)K) * (qb_i - qa_i).  The motion clearance is the minimum of
 * the samples' clearances (optik_hip_collision_batch's, with the same model, world and ee_offset7), NaN if any is NaN;
 * the motion is free iff every sample is free; first is the lowest k whose sample is not free, -1 for a free motion;
 * steps is K.  A segment with d NaN or infinite or with K > OPTIK_HIP_MAX_MOTION_STEPS is not sampled: clearance
 * NaN, free 0, first -1, steps -1.  Without a model: clearance +inf and free 1 (NaN and 0 if a sample is NaN).  The
 * results do not depend on the launch shape or on the order the samples are visited in.
 *
 * optik_hip_collision_motion_batch: B segments d_qa, d_qb [n][B] -> d_clearance [B], d_free [B], d_first [B],
 * d_steps [B]; any output may be NULL.  With d_clearance NULL the call only classifies and skips the samples above a
 * non-free one it has found; free, first and steps are the same.  Stream-ordered, no host synchronisation; its
 * workspace (24 bytes per segment) belongs to the chain and grows on demand, so one call per chain handle at a time,
 * as for the solver launches.  Revolute chains of 1 .. 16 joint positions.  Refused with OPTIK_HIP_EINVAL before any
 * device work: a NaN, infinite, zero or negative resolution, B < 0 (B = 0 is a no-op), more than 2^30 segments; with
 * OPTIK_HIP_EUNSUPPORTED: chains with prismatic joints.
 *
 * optik_hip_chain_set_motion_resolution: the resolution h of optik_hip_ik_path's motion key pass; 0 (the default)
 * switches it off; NaN, negative or infinite: OPTIK_HIP_EINVAL.  Waits for the chain's device as set_world does.
 * The pass is active exactly while h > 0 and the chain has a collision model with S >= 1.  Then every waypoint
 * launch of optik_hip_ik_path runs it after the solver, the key pass of modes 3 and 4 and the collision key pass, on
 * the same stream, before the selection: for each restart with a finite key whose L-infinity distance to the path's
 * carried seed is <= max_step, the motion seed -> x is checked at resolution h (the seed is read on the device: no
 * host synchronisation between waypoints), and the key becomes +inf if that motion is not free (a motion that is
 * not sampled is not free).  Successes beyond max_step are left alone: the selection rejects them.  A path whose
 * seed is itself in collision (a start configuration, say) has no free motion from it: every waypoint of it reports
 * no solution until the caller gives it a free start.  optik_hip_ik_batch, optik_hip_ik_host and
 * optik_hip_ik_solutions ignore the setting; with h = 0 or without a model nothing extra is launched. */
#define OPTIK_HIP_MAX_MOTION_STEPS 4096
int optik_hip_collision_motion_batch(optik_hip_chain *chain, const double *ee_offset7, const double *d_qa,
                                     const double *d_qb, int64_t B, double resolution, double *d_clearance,
                                     uint8_t *d_free, int32_t *d_first, int32_t *d_steps, void *stream);
int optik_hip_chain_set_motion_resolution(optik_hip_chain *chain, double h);

/* The certified motion check (extension; the arithmetic: csrc/advance_measure.hpp).  The
 * sampled check above says "free at the samples"; this one walks the segment q(t) = qa + t (qb - qa), t in [0, 1], by
 * conservative advancement: at every sample each distance term of the clearance gives the largest step of t after
 * which it can still not be below margin - tol, from bounds on how fast it can shrink (the chain's fixed translations
 * bound the speed of every robot sphere per radian of every joint; sphere and box distances are 1-Lipschitz, the grid
 * term is grid_lipschitz-Lipschitz), and the walk advances by the smallest of them.
 *
 * Per segment: status (OPTIK_HIP_CERTIFY_*), steps = the samples evaluated, t_stop, and clearance = the minimum of the
 * evaluated samples' clearances (optik_hip_collision_batch's bits for those configurations; +inf without a model).
 *   FREE     for every t in [0, 1] the clearance is >= margin - tol, and >= margin at the evaluated samples; t_stop 1
 *   BLOCKED  q(t_stop) is not free (clearance < margin there)
 *   LIMIT    max_steps samples were evaluated and t_stop < 1: nothing is said (a long grazing motion with a small
 *            tol; or, with a grid installed, a sphere outside the grid creeping up to a boundary behind which the
 *            field is low)
 *   NAN      a NaN frame at t_stop (clearance NaN); or a NaN or infinite joint in qa or qb: steps 0, t_stop NaN
 * A motion whose true minimum clearance is below margin - tol never comes back FREE, one whose minimum is >= margin
 * never comes back BLOCKED; in between either answer is right.  The statement is about the library's clearance
 * function: with a grid world it inherits the trilinear field's sqrt(3) * voxel, it is only as true as grid_lipschitz
 * (sqrt(3) is valid for every grid whose neighbouring nodes differ by at most one voxel, as those of a true distance
 * field do), and the floating-point rounding of the bounds is not accounted for (tol is meant to be many orders
 * above 1e-16).  A free segment takes at most about max(1, grid_lipschitz) * lam_max / tol samples, lam_max the
 * largest speed bound of a robot sphere per unit of t.
 *
 * optik_hip_collision_motion_certify_batch: B segments d_qa, d_qb [n][B] -> d_status [B], d_steps [B], d_t_stop [B],
 * d_clearance [B]; any output may be NULL.  One wave per segment; stream-ordered, no host synchronisation, no
 * workspace.  Revolute chains of 1 .. 16 joint positions.  Refused with OPTIK_HIP_EINVAL before any device work
 * unless tol is finite and > 0, grid_lipschitz is finite and > 0, 2 <= max_steps <= OPTIK_HIP_CERTIFY_MAX_STEPS and
 * 0 <= B <= 2^30 (B = 0 is a no-op); with OPTIK_HIP_EUNSUPPORTED: chains with prismatic joints. */
#define OPTIK_HIP_CERTIFY_FREE 0
#define OPTIK_HIP_CERTIFY_BLOCKED 1
#define OPTIK_HIP_CERTIFY_LIMIT 2
#define OPTIK_HIP_CERTIFY_NAN 3
#define OPTIK_HIP_CERTIFY_MAX_STEPS 65536
int optik_hip_collision_motion_certify_batch(const optik_hip_chain *chain, const double *ee_offset7,
                                             const double *d_qa, const double *d_qb, int64_t B, double tol,
                                             double grid_lipschitz, int32_t max_steps, int32_t *d_status,
                                             int32_t *d_steps, double *d_t_stop, double *d_clearance, void *stream);

/* Pose constraints (extension; csrc/constraint_measure.hpp states the arithmetic line by line).
 *
 * A pose constraint is a reference pose ref7 (t, quaternion i j k w) and a box lo6, hi6 on the pose error
 * e(x) = (se3 log linear xyz, so3 log xyz) of X = ref^-1 * FK(x) * ee_offset -- the six numbers the IK objective forms
 * before it weights them, with ref in the place of the target.  The residual is r_i = e_i - min(max(e_i, lo_i), hi_i),
 * the violation max_i |r_i| (NaN if any e_i is NaN); lo_i = -inf and hi_i = +inf free an axis; x satisfies the
 * constraint at tol >= 0 iff its violation is <= tol.  The constraint is an argument of every call (host pointers, read
 * before the call returns); the chain keeps nothing of it.
 *
 * optik_hip_constraint_batch: d_q [n][B] -> d_residual [6][B], d_violation [B].
 * optik_hip_constraint_project_batch: damped Gauss-Newton onto the constraint set from d_q [n][B], at most `iters`
 *   steps of at most max_step (L-infinity, radians) each, every iterate clamped to the joint limits -> d_x [n][B],
 *   d_violation [B] (at d_x), d_status [B] (OPTIK_HIP_CONSTRAINT_*: 0 projected -- the violation is <= tol and d_x lies
 *   within the limits --, 1 the iterations are spent, 2 a NaN or infinite joint -- the row comes back as it went in --
 *   or a failed factorisation), d_iterations [B] (steps taken; a row that satisfies the constraint comes back unchanged
 *   after 0).  OPTIK_HIP_CONSTRAINT_ITERS, _DAMPING and _MAX_STEP are the defaults of the layers above (DESIGN.md
 *   section 5.29 has the table they were read from).
 * optik_hip_constraint_motion_batch: the segments d_qa, d_qb [n][B] sampled as optik_hip_collision_motion_batch samples
 *   them at `resolution` -> d_violation [B] (the maximum over the samples, NaN if any sample's is), d_ok [B] (every
 *   sample <= tol), d_first [B] (the lowest violating sample, -1: none), d_steps [B]; a motion that is not sampled gives
 *   NaN, 0, -1, -1.  Nothing is projected: it says what holds at the samples.
 *
 * Any output may be NULL.  One row per lane, grid-stride, stream-ordered, no host synchronisation, no workspace, no
 * atomics.  Revolute chains of 1 .. 16 joint positions.  Refused with OPTIK_HIP_EINVAL before any device work, also
 * when B = 0: a NULL or non-finite ref7, a quaternion whose squared norm is further than 100 machine epsilons from 1,
 * lo_i <= hi_i false on an axis (a NaN included), tol not finite and >= 0, B < 0, iters outside 0 ..
 * OPTIK_HIP_CONSTRAINT_MAX_ITERS, damping not finite and >= 0, max_step or resolution not finite and > 0; with
 * OPTIK_HIP_EUNSUPPORTED, also when B = 0: chains with prismatic joints (the motion check's message). */
#define OPTIK_HIP_CONSTRAINT_PROJECTED 0
#define OPTIK_HIP_CONSTRAINT_BUDGET 1
#define OPTIK_HIP_CONSTRAINT_FAILED 2
#define OPTIK_HIP_CONSTRAINT_MAX_ITERS 4096
#define OPTIK_HIP_CONSTRAINT_ITERS 256
#define OPTIK_HIP_CONSTRAINT_DAMPING 1e-6
#define OPTIK_HIP_CONSTRAINT_MAX_STEP 0.5
int optik_hip_constraint_batch(const optik_hip_chain *chain, const double *ee_offset7, const double *ref7,
                               const double *lo6, const double *hi6, const double *d_q, int64_t B,
                               double *d_residual, double *d_violation, void *stream);
int optik_hip_constraint_project_batch(const optik_hip_chain *chain, const double *ee_offset7, const double *ref7,
                                       const double *lo6, const double *hi6, const double *d_q, int64_t B, double tol,
                                       int32_t iters, double damping, double max_step, double *d_x,
                                       double *d_violation, int32_t *d_status, int32_t *d_iterations, void *stream);
int optik_hip_constraint_motion_batch(const optik_hip_chain *chain, const double *ee_offset7, const double *ref7,
                                      const double *lo6, const double *hi6, const double *d_qa, const double *d_qb,
                                      int64_t B, double resolution, double tol, double *d_violation, uint8_t *d_ok,
                                      int32_t *d_first, int32_t *d_steps, void *stream);

/* Restart seeds: ChaCha8Rng::seed_from_u64(42), set_stream(i), one uniform draw
 * per joint (lib.rs:358-370, 86-91) for i = first .. first+count-1 -> d_q [n][count]. */
int optik_hip_seed_batch(const optik_hip_chain *chain, uint64_t first, int64_t count, double *d_q,
                         void *stream);

/* flags of optik_hip_ik_batch */
#define OPTIK_HIP_IK_EARLY_EXIT 1u /* Speed: abandon restarts above a known success (lib.rs:382-384) */
/* With EARLY_EXIT: abandon every other restart of a target as soon as ANY restart of it has
 * succeeded -- the reference's behaviour with more than one rayon thread (find_any, lib.rs:409-412;
 * README.md:17, 96: "non-deterministic").  The winner is then the lowest index among the restarts
 * that happened to finish successfully: a valid solution -- its x / f are what that restart
 * returns on its own, bit for bit -- but which one depends on timing.  Without it (the default)
 * only restarts ABOVE a success are abandoned and the answer is the reference's 1-thread one. */
#define OPTIK_HIP_IK_FIND_ANY 2u
/* optik_hip_ik_batch / _ik_host with T > 1 targets: hand the (target, restart) work items out
 * restart-major (every target's restart 0, then every target's restart 1, ...) instead of
 * target-major; with EARLY_EXIT about eight restarts per target are kept in flight and most
 * higher indices are never started.  Scheduling only: per-restart results and winners are the
 * same (an abandoned restart's status is FORCED_STOP either way). */
#define OPTIK_HIP_IK_RESTART_MAJOR 4u
/* Outputs of optik_hip_ik_batch; any pointer may be NULL to skip that output.
 * R = restart_end - restart_begin. */
typedef struct optik_hip_ik_outputs {
    /* per restart, struct-of-arrays over T*R columns, column = t*R + (i - restart_begin) */
    double *d_x;        /* [n][T*R] returned point (NLopt's best-so-far x)   */
    double *d_f;        /* [T*R]    returned objective value                  */
    int32_t *d_status;  /* [T*R]    OPTIK_RES_*                               */
    int32_t *d_evals;   /* [T*R]    objective evaluations (NLopt's count)     */
    /* per target: the selection of lib.rs:397-413 */
    double *d_win_x;      /* [T][n]                                           */
    double *d_win_f;      /* [T]                                              */
    uint64_t *d_win_idx;  /* [T] winning restart index, UINT64_MAX if none    */
    double *d_win_key;    /* [T] Quality: ||x - x0||_2 ; Speed: (double)index ; Manipulability: -w ; Condition: -c ;
                           *     +inf if none (d_win_x and d_win_f are NaN then), as optik_hip_ik_path's d_key */
} optik_hip_ik_outputs;

/* The hot path: for each of T targets run restarts restart_begin..restart_end-1
 * (index 0 = the caller's seed x0, index i > 0 = ChaCha8 stream i), classify
 * (lib.rs:376-379) and select (Speed: lowest successful index = the reference's
 * 1-thread order; Quality: min ||x - x0||_2, ties to the lower index).
 * d_targets [T][7], d_x0 [T][n].  deadline_s > 0 abandons restarts still running
 * that many seconds after the kernel starts (max_time, lib.rs:260-264, 308).
 * OPTIK_MODE_MANIPULABILITY / _CONDITION: scheduled as Quality (EARLY_EXIT and FIND_ANY have no effect); after the
 * solver, on the same stream, a key kernel replaces the key of every successful restart by -w / -c of its x (with
 * ee_offset7, as optik_hip_manip_batch computes them); failed restarts keep +inf.  The selection is unchanged --
 * minimum (key, index), ties to the lower index -- so the winner is the most manipulable / best conditioned success.
 * The per-restart x is kept in the chain's workspace when d_x is NULL.  The same holds for optik_hip_ik_solutions
 * (best first) and optik_hip_ik_path (the best within max_step).  Chains with prismatic joints are refused. */
int optik_hip_ik_batch(optik_hip_chain *chain, const optik_solver_config *cfg,
                       const double *d_targets, const double *d_x0, int32_t T,
                       const double *ee_offset7, uint64_t restart_begin, uint64_t restart_end,
                       uint32_t flags, double deadline_s, const optik_hip_ik_outputs *out,
                       void *stream);

/* Up to K distinct solutions per target, from one launch of restarts restart_begin..restart_end-1 run to their end
 * (no early exit, Speed as well as Quality; deadline_s as in optik_hip_ik_batch).  The candidates of a target are
 * its successful restarts (lib.rs:376-379), in the order of (key, restart index) -- key = ||x - x0||_2 summed left
 * to right for Quality, (double)index for Speed, as in optik_hip_ik_batch.  They are taken greedily: a candidate is
 * accepted if max_i |x_i - a_i| > min_dist for every solution a accepted before it (no angle wrapping; min_dist = 0
 * merges exact duplicates only), until K are accepted.  On a redundant arm the successes form a continuum and
 * min_dist sets the spacing of the returned samples.  With K = 1 the one solution is optik_hip_ik_batch's winner
 * without early exit.  The set does not depend on the solver that ran or on the launch size.
 * Outputs, slot order = acceptance order; any pointer may be NULL.  Slots past count: x and f NaN, idx UINT64_MAX,
 * key +inf.  Refused as optik_hip_ik_batch refuses (prismatic chains, infinite limits with random restarts, a bad
 * solution_mode, too many selection tiles), and for K outside 1..OPTIK_HIP_MAX_SOLUTIONS or a NaN or negative
 * min_dist.  Stream-ordered; uses the chain's launch workspace like optik_hip_ik_batch. */
#define OPTIK_HIP_MAX_SOLUTIONS 256
typedef struct optik_hip_ik_solutions_outputs {
    int32_t *d_count; /* [T]                                        */
    double *d_x;      /* [T][K][n]  NaN past count                  */
    double *d_f;      /* [T][K]     the restart's returned objective */
    uint64_t *d_idx;  /* [T][K]     UINT64_MAX past count           */
    double *d_key;    /* [T][K]     +inf past count                 */
} optik_hip_ik_solutions_outputs;
int optik_hip_ik_solutions(optik_hip_chain *chain, const optik_solver_config *cfg,
                           const double *d_targets, const double *d_x0, int32_t T, const double *ee_offset7,
                           uint64_t restart_begin, uint64_t restart_end, double deadline_s,
                           int32_t K, double min_dist, const optik_hip_ik_solutions_outputs *out, void *stream);

/* P independent paths of L waypoints, each waypoint solved from the previous one's solution (warm start).  Path p
 * carries a seed c_p, first d_x0[p].  Waypoint l of path p runs restarts restart_begin..restart_end-1 with seed c_p
 * (restart 0 = c_p; Quality's key = ||x - c_p||_2).  The candidates are its successful restarts (lib.rs:376-379)
 * whose max_i |x_i - c_i| (no angle wrapping) is <= max_step (+inf: every success); the accepted solution is their
 * (key, restart index) minimum, as in optik_hip_ik_batch.  c_p then becomes the accepted solution; a waypoint with no
 * candidate leaves c_p unchanged and its outputs x, f, step NaN, idx UINT64_MAX, key +inf.
 * Schedule: Speed with max_step = +inf runs with early exit under the deterministic rule, and every waypoint equals
 * optik_hip_ik_batch(EARLY_EXIT) with d_x0 = c, bit for bit; Speed with a finite max_step and Quality run every
 * restart to its end.  The result does not depend on the solver, the launch size or timing (deadline_s excepted: it
 * applies to each waypoint's launch, as in optik_hip_ik_batch).
 * d_targets [L][P][7] (waypoint-major); d_x0 [P][n].  flags: 0 or OPTIK_HIP_IK_RESTART_MAJOR (hand-out order only).
 * Refused: R = restart_end - restart_begin outside 1..OPTIK_HIP_PATH_MAX_RESTARTS (one selection block per path;
 * warm-started paths need few restarts), other flags, a NaN or negative max_step, P or L < 1, and whatever
 * optik_hip_ik_batch refuses.  Stream-ordered, with no host synchronisation between waypoints: per waypoint one
 * solver launch and one selection kernel; holds the chain for the whole call and uses its launch workspace. */
#define OPTIK_HIP_PATH_MAX_RESTARTS 4096
typedef struct optik_hip_ik_path_outputs {
    double *d_x;      /* [L][P][n]  NaN where no solution           */
    double *d_f;      /* [L][P]     the restart's returned objective */
    uint64_t *d_idx;  /* [L][P]     UINT64_MAX where no solution    */
    double *d_key;    /* [L][P]     +inf where no solution          */
    double *d_step;   /* [L][P]     max_i |x_i - c_i|; NaN where no solution */
    double *d_last;   /* [P][n]     each path's final seed c_p       */
} optik_hip_ik_path_outputs;
int optik_hip_ik_path(optik_hip_chain *chain, const optik_solver_config *cfg, const double *d_targets,
                      const double *d_x0, int32_t P, int32_t L, const double *ee_offset7, uint64_t restart_begin,
                      uint64_t restart_end, uint32_t flags, double deadline_s, double max_step,
                      const optik_hip_ik_path_outputs *out, void *stream);

/* Up to K distinct configurations per pose REGION (csrc/region_measure.hpp): optik_hip_ik_solutions
 * with a box on the pose error in the place of the exact pose, and the projection of
 * optik_hip_constraint_project_batch in the place of the SLSQP solver.  d_regions [T][19] is DEVICE data, per region
 * ref[7] (t, quaternion i j k w), lo[6], hi[6]; it is not validated here: by the header's rules a NaN in a reference
 * yields OPTIK_HIP_CONSTRAINT_FAILED rows (key +inf, count 0), and a NaN bound bounds nothing on its side (the
 * residual's comparisons are false).  The host API (optik_robot_ik_region) validates every region.  d_x0 [T][n].
 * Restart i of region t (column t*R + (i - restart_begin), R = restart_end - restart_begin) starts at d_x0[t] for
 * i = 0 and at the restart seed of ChaCha stream i otherwise (optik_hip_seed_batch's row, the same for every region),
 * is projected onto the region at tol (at most iters steps, damping, max_step: optik_hip_constraint_project_batch's
 * method and its outputs x, violation, status, iterations), and gets the key +inf unless it ended
 * OPTIK_HIP_CONSTRAINT_PROJECTED, else (double)i for OPTIK_MODE_SPEED and ||x - x0[t]||_2 (squares summed left to
 * right) for every other mode.  keep_ref7 / keep_lo6 / keep_hi6 (host pointers, all NULL: none) name a second box that
 * is only measured: the key becomes +inf where the violation of the projected x against it is not <= keep_tol.
 * Then, stream-ordered and without host synchronisation, what optik_hip_ik_solutions runs behind its solver: the key
 * pass of modes OPTIK_MODE_MANIPULABILITY / _CONDITION, the collision filter when a model is installed, and the
 * greedy selection of up to K rows more than min_dist (L-infinity) apart in (key, index) order.  Every returned row
 * satisfies the region at tol, lies within the joint limits and is free when a model is installed.  Nothing is promised
 * about how well the rows cover the region's solution manifold.
 * Outputs, any pointer may be NULL; the per-restart arrays the selection needs live in the chain's launch workspace
 * when they are.  Refused before any device work, at T = 0 too (a T = 0 call that passes returns 0): a null chain or
 * out, T < 0, an empty restart range, random restarts with infinite joint limits, mode outside 1..4, what
 * optik_hip_constraint_project_batch refuses for tol, iters, damping and max_step, what optik_hip_ik_solutions refuses
 * for K, min_dist and the selection tiles, a keep box given in part or one optik_hip_constraint_batch would refuse, a
 * keep_tol that is not finite and >= 0, and chains with prismatic joints.  Uses the chain's launch workspace like
 * optik_hip_ik_solutions. */
#define OPTIK_HIP_REGION_DOUBLES 19
typedef struct optik_hip_ik_region_outputs {
    double *d_x;              /* [n][T*R]   per restart: the projected configuration */
    double *d_violation;      /* [T*R]      its violation of the region             */
    int32_t *d_status;        /* [T*R]      OPTIK_HIP_CONSTRAINT_*                  */
    int32_t *d_iterations;    /* [T*R]                                              */
    double *d_key;            /* [T*R]      after the key passes, before selection  */
    int32_t *d_count;         /* [T]                                                */
    double *d_sol_x;          /* [T][K][n]  NaN past count                          */
    double *d_sol_violation;  /* [T][K]     NaN past count                          */
    uint64_t *d_sol_idx;      /* [T][K]     UINT64_MAX past count                   */
    double *d_sol_key;        /* [T][K]     +inf past count                         */
} optik_hip_ik_region_outputs;
int optik_hip_ik_region(optik_hip_chain *chain, const double *ee_offset7, const double *d_regions, const double *d_x0,
                        int32_t T, uint64_t restart_begin, uint64_t restart_end, double tol, int32_t iters,
                        double damping, double max_step, int32_t mode, const double *keep_ref7, const double *keep_lo6,
                        const double *keep_hi6, double keep_tol, int32_t K, double min_dist,
                        const optik_hip_ik_region_outputs *out, void *stream);

/* optik_hip_ik_region with collision repair.  repair NULL: optik_hip_ik_region itself, bit for
 * bit and with not one launch more.  Otherwise optik_hip_collision_repair_batch's loop (influence, safety, step, iters,
 * max_move) runs on the same stream between the region kernel and the key passes, on every column whose key is finite,
 * with the column's own region as the box and ptol = tol (piters = iters, damping, max_step: the projection's).  A
 * column that ends OPTIK_HIP_REPAIR_FREE after at least one step takes the repaired x and violation; its key is
 * recomputed by the region kernel's rule from the new x (OPTIK_MODE_SPEED keeps the index, every other mode
 * ||x - x0[t]||_2 in the same summation order) and re-measured against the keep box.  Every other column is left bit for
 * bit, and the collision filter then drops it as before.  The manipulability / condition pass, the filter and the
 * selection follow unchanged.  d_repaired [T] (may be NULL): the columns of each region that took a repaired x.  The
 * per-restart d_status and d_iterations stay the projection's.
 * Refusals as optik_hip_ik_region, and, at T = 0 too: OPTIK_HIP_EUNSUPPORTED for chains of 9 .. 16 joint positions,
 * OPTIK_HIP_EINVAL for what optik_hip_collision_repair_batch refuses of the five parameters and for a chain without a
 * collision model. */
typedef struct optik_hip_region_repair {
    double influence, safety, step, max_move;
    int32_t iters;
    int32_t *d_repaired;      /* [T] or NULL */
} optik_hip_region_repair;
int optik_hip_ik_region_repair(optik_hip_chain *chain, const double *ee_offset7, const double *d_regions,
                               const double *d_x0, int32_t T, uint64_t restart_begin, uint64_t restart_end, double tol,
                               int32_t iters, double damping, double max_step, int32_t mode, const double *keep_ref7,
                               const double *keep_lo6, const double *keep_hi6, double keep_tol, int32_t K,
                               double min_dist, const optik_hip_region_repair *repair,
                               const optik_hip_ik_region_outputs *out, void *stream);

/* Test hooks: the selection stage of the three entry points above on the caller's own per-restart arrays, with no
 * solve in front -- what optik_hip_ik_batch, optik_hip_ik_solutions and one waypoint of optik_hip_ik_path launch behind
 * their solver, from the same launch code and tile plan.  d_key [T*R] (+inf or NaN: no candidate), d_x [n][T*R],
 * d_f [T*R], column t*R + (i - restart_begin); n is the chain's.  The selection order is (key, index): the smaller key,
 * ties to the smaller index; -0.0 == +0.0 is a tie.  Stream-ordered; they take the chain's launch mutex and use its
 * tile workspace, and leave its work-item counter and first-success words alone.
 *   _select_from_keys     reads only the d_win_* fields of `out`; d_x / d_f may be NULL if d_win_x / d_win_f are.
 *   _solutions_from_keys  d_key is scratch: eliminated candidates' keys become +inf (the multi-tile form, R > 4096).
 *   _path_select_from_keys  d_seed [P][n]; out is one waypoint's (L = 1: [P][n], [P]; d_last a copy of d_carry);
 *                           d_carry [P][n], not NULL, receives the next seeds and may be d_seed itself.
 * Refused as the entry points refuse: T or P < 1, R < 1 or restart_begin + R above UINT64_MAX, 2^24 or more selection
 * tiles, K outside 1..OPTIK_HIP_MAX_SOLUTIONS, a NaN, negative or infinite min_dist, R above
 * OPTIK_HIP_PATH_MAX_RESTARTS or a NaN or negative max_step for the path form -- all before the chain is touched. */
int optik_hip_select_from_keys(optik_hip_chain *chain, const double *d_key, const double *d_x, const double *d_f,
                               int32_t T, uint64_t restart_begin, uint64_t R, const optik_hip_ik_outputs *out,
                               void *stream);
int optik_hip_solutions_from_keys(optik_hip_chain *chain, double *d_key, const double *d_x, const double *d_f,
                                  int32_t T, uint64_t restart_begin, uint64_t R, int32_t K, double min_dist,
                                  const optik_hip_ik_solutions_outputs *out, void *stream);
int optik_hip_path_select_from_keys(optik_hip_chain *chain, const double *d_key, const double *d_x, const double *d_f,
                                    const double *d_seed, int32_t P, uint64_t restart_begin, uint64_t R,
                                    double max_step, const optik_hip_ik_path_outputs *out, double *d_carry,
                                    void *stream);

/* Tuning options of the kernel layer (diagnostics: tests and tools; the defaults are what the product runs with).
 * Each option's default comes from the environment variable named with it, read ONCE when the library first needs
 * an option; afterwards only this call changes it.  Not synchronised with calls in flight.
 *   solve_kernel        OPTIK_SOLVE_KERNEL = quad | lane64 | general   0 auto (by launch size), 1 quad solver
 *                                                                       (ik_quad.hpp), 2 lane-per-restart form
 *                                                                       (ik_lane64.hpp), 3 general solver (ik_wide.hpp)
 *   wide_form           OPTIK_WIDE_FORM = lds | hbm   form of the general solver (0 lds, 1 hbm)
 *   range_rule          OPTIK_RANDOM_RANGE_RULE = new_inclusive   OPTIK_HIP_RANGE_* of chains created afterwards
 *   stop_x_legacy       (none)                   1: nlopt_stop_x of NLopt 2.5 (no zero-step rule)
 *   grid_cap            (none)                   a test hook: v >= 1 launches every grid-stride kernel (the batch
 *                                                operators, the motion check, trajectory_sample; not the solvers) with
 *                                                at most v blocks, so that a few hundred rows take the later trips of
 *                                                its loop; 0 (the default) the device's own cap.  No result depends on
 *                                                it.  A negative value is refused with OPTIK_HIP_EINVAL
 * The host layer (optik.h) reads OPTIK_HOST_THREADS and OPTIK_DEVICES; nothing else in the library reads the
 * environment.  Returns 0, or OPTIK_HIP_EINVAL for an unknown name; optik_hip_get_option returns -1 for one. */
int optik_hip_set_option(const char *name, long long value);
long long optik_hip_get_option(const char *name);

/* Host-buffer convenience over optik_hip_ik_batch (what Robot::ik calls): copies
 * targets/x0 in, runs, synchronises, copies the per-target winners out.
 * win_x [T][n], win_f [T], win_idx [T] (UINT64_MAX = no solution), win_key [T]
 * (the selection key; any of them may be NULL).  Calls on one chain are serialised.
 * optik_hip_ik_batch itself is stream-ordered and keeps its launch workspace in the
 * chain handle: use one stream per chain handle. */
int optik_hip_ik_host(optik_hip_chain *chain, const optik_solver_config *cfg,
                      const double *targets, const double *x0, int32_t T, const double *ee_offset7,
                      uint64_t restart_begin, uint64_t restart_end, uint32_t flags,
                      double deadline_s, double *win_x, double *win_f, uint64_t *win_idx,
                      double *win_key);

/* Test hook: elementary functions the kernels use, evaluated on the device.
 * op 0: a/b, 1: sqrt(a), 2: sin(a), 3: cos(a), 4: atan2(a, b) for a > 0, b >= 0. */
int optik_hip_probe(int32_t op, const double *a, const double *b, int64_t count, double *out);
/* Test hook: the math.rs functions one at a time on the device (the reference pins them with golden
 * vectors, crates/optik/tests/test_math.rs:14-61).  poses7 = count x {t[3], quat[i,j,k,w]}; row-major
 * results, `count` x: op 0 so3::log (3), 1 so3::right_jacobian(so3::log(q)) (9), 2 se3::log (6: linear,
 * angular), 3 se3::right_jacobian (36). */
int optik_hip_probe_math(int32_t op, const double *poses7, int64_t count, double *out);

/* Last launch geometry / timing of optik_hip_ik_batch on this chain (for bench.py). */
typedef struct optik_hip_launch_info {
    int32_t grid, block, lds_bytes, tiles;
    float kernel_ms; /* HIP-event time of the solve kernel when timing is enabled */
} optik_hip_launch_info;
/* Enabling timing records a HIP event pair around every solve-kernel launch on the
 * launch stream (and resets the recorded set); optik_hip_timing_mean synchronises
 * on them and returns the mean kernel duration over the launches recorded since
 * (at most 256 are kept). */
void optik_hip_set_timing(optik_hip_chain *chain, int32_t enabled);
int optik_hip_last_launch(const optik_hip_chain *chain, optik_hip_launch_info *info);
int optik_hip_timing_mean(optik_hip_chain *chain, double *mean_ms, int32_t *count);
/* Diagnostic builds (-DOPTIK_PROFILE) accumulate s_memtime cycles per solver phase:
 * out8 = {refill, eval, update, publish, bfgs, lsq, nnls, trips}; all zero in normal builds. */
int optik_hip_phase_profile(optik_hip_chain *chain, unsigned long long *out8);

#ifdef __cplusplus
}
#endif
#endif
