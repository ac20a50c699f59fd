/*
 * optik.h -- the reference's C ABI (crates/optik-cpp/src/lib.rs:26-183), exported by
 * liboptik_amd.so so that the reference's C++ wrapper (crates/optik-cpp/src/lib.cpp,
 * include/optik.hpp) and any other binding of `liboptikcpp` can link against the
 * MI355X implementation unchanged.  All compute goes through the HIP kernels of
 * include/optik_hip.h; there is no CPU fallback.
 *
 * Ownership (as in the reference): a `robot*` is released only by optik_robot_free;
 * every returned `double*` is a malloc'ed buffer the caller releases with free()
 * (lib.cpp:72, 87, 100, 115, 129).  Matrices are column-major.  Invalid input
 * aborts the process with the reference's panic message on stderr (a Rust panic
 * across `extern "C"` aborts too); "no solution" is NULL.
 */
#ifndef OPTIK_H
#define OPTIK_H

#include <stdint.h>

#include "optik_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct optik_robot optik_robot;           /* Box<Robot>, optik-cpp/src/lib.rs:27-57 */
typedef optik_solver_config CSolverConfig;        /* optik-cpp/src/lib.rs:10-20 */

/* ---- the 11 symbols of the reference ------------------------------------------ */
optik_robot *optik_robot_from_urdf_file(const char *path, const char *base_link,
                                        const char *ee_link);                 /* lib.rs:27-37 */
optik_robot *optik_robot_from_urdf_str(const char *urdf, const char *base_link,
                                       const char *ee_link);                  /* lib.rs:40-50 */
void optik_robot_free(optik_robot *robot);                                    /* lib.rs:53-57 */
void optik_robot_set_parallelism(optik_robot *robot, unsigned int n);         /* lib.rs:60-65 */
unsigned int optik_robot_num_positions(const optik_robot *robot);             /* lib.rs:68-73 */
const double *optik_robot_joint_limits(const optik_robot *robot);             /* lib.rs:76-88: [lb.., ub..] */
const double *optik_robot_joint_jacobian(const optik_robot *robot, const double *x); /* lib.rs:91-104: 6 x n */
const double *optik_robot_fk(const optik_robot *robot, const double *x);      /* lib.rs:107-116: 4 x 4 */
const double *optik_robot_random_configuration(const optik_robot *robot);     /* lib.rs:119-125 */
const double *optik_robot_ik(const optik_robot *robot, const CSolverConfig *config,
                             const double *target, const double *x0);         /* lib.rs:128-162 */
/* Differential IK (optik-cpp lib.rs:165-183; Robot::diff_ik, lib.rs:123-239): the joint
 * velocities v_n[n] realising alpha * V_WE for the largest feasible 0 <= alpha <= 1 under
 * |v_i| <= v_max_i.  The LP (<= 9 unknowns) is solved exactly on the host; FK and the Jacobian
 * come from the HIP kernels.  NULL = no solution.  Chains of more than 8 joint positions are
 * refused (the reference's own diff_ik only runs for n = 6: lib.rs:196-197). */
const double *optik_robot_diff_ik(const optik_robot *robot, const double *x0, const double *V_WE,
                                  const double *v_max);

/* ---- extensions used by the Python front end and bench.py --------------------- */
/* Error-returning constructors / solver: 0 on success, negative on failure with the
 * message in optik_robot_last_error() (what a pyo3-style binding turns into an
 * exception instead of aborting). */
int optik_robot_try_from_urdf_str(const char *urdf, const char *base_link, const char *ee_link,
                                  optik_robot **out);
const char *optik_robot_last_error(void);
/* Robot::ik with the full signature of lib.rs:241-247: ee_offset (4x4 col-major, NULL
 * = identity), returns x and the residual c.  rc 0 = solution, 1 = none, < 0 = error. */
int optik_robot_ik_ex(const optik_robot *robot, const CSolverConfig *config, const double *target16,
                      const double *x0, const double *ee_offset16, double *x_out, double *f_out,
                      uint64_t *winner_out);
/* How a 4x4 target becomes the (translation, unit quaternion) pose Robot::ik takes.  The reference has two readings:
 * its C path (optik-cpp/src/lib.rs:137-144) runs nalgebra's ITERATIVE UnitQuaternion::from_matrix on the 3x3 block,
 * its Python path (optik-py/src/lib.rs:8-15) nalgebra's try_convert = the closed-form from_rotation_matrix.  Both give
 * the same rotation for a rotation matrix, last bits apart -- and last bits decide which restart wins (DESIGN.md
 * section 2).  optik_robot_ik (the reference's C symbol) uses the iterative form, as liboptikcpp does;
 * optik_robot_ik_ex (what the Python front end calls; ee_offset only exists there) the closed form;
 * optik_robot_ik_pose takes the choice as a flag: OPTIK_POSE_FROM_MATRIX = the iterative form.
 * optik_pose_from_matrix: the conversion alone (host code, no GPU): m16 column-major -> pose7 [t, qi, qj, qk, qw]. */
#define OPTIK_POSE_FROM_MATRIX 4u
int optik_robot_ik_pose(const optik_robot *robot, const CSolverConfig *config, const double *target16,
                        uint32_t flags, const double *x0, const double *ee_offset16, double *x_out,
                        double *f_out, uint64_t *winner_out);
int optik_pose_from_matrix(const double *m16, uint32_t flags, double *pose7);
/* T independent ik() calls with one SolverConfig: targets16 [T][16] (4x4 col-major each),
 * x0 [T][n] -> x_out [T][n], f_out [T], found_out [T] (0/1).  Every target gets Robot::ik's
 * semantics (config 5 of BASELINE.json: many targets x a few hundred restarts).  Scheduling
 * (robot_host.cpp:ik_batch_on_device): every round is ONE launch of optik_hip_ik_batch over the
 * targets still unsolved.  Speed: a first round of 128 restart indices per target, restart-major
 * with early exit (64 when the round would exceed ~4 M work items, down to 8 for batches of more
 * than 65 536 targets); what it leaves unsolved runs in rounds four times as long each.  Quality:
 * every restart of every target, as many indices per round as ~4 M work items allow, on the
 * lane-per-restart form.
 * rc 0 = ran, < 0 = error. */
int optik_robot_ik_batch_ex(const optik_robot *robot, const CSolverConfig *config, int32_t T,
                            const double *targets16, const double *x0, const double *ee_offset16,
                            double *x_out, double *f_out, int32_t *found_out);
/* The same with the targets as the Python binding receives them: OPTIK_BATCH_ROW_MAJOR = each
 * 4x4 is row-major (optik-py/src/lib.rs:8-15 reads nested rows), OPTIK_BATCH_VALIDATE_POSES =
 * apply parse_pose's isometry test to every target (bottom row exactly 0 0 0 1, R'R = I within
 * 100 * DBL_EPSILON per entry, det R > 0) and return -3 with "invalid target transform
 * specified" before any GPU work if one fails; OPTIK_POSE_FROM_MATRIX = convert every target with the iterative
 * UnitQuaternion::from_matrix (the C path's reading; optik_robot_ik_batch_ex passes it, the Python front end does
 * not). */
#define OPTIK_BATCH_ROW_MAJOR 1u
#define OPTIK_BATCH_VALIDATE_POSES 2u
int optik_robot_ik_batch_poses(const optik_robot *robot, const CSolverConfig *config, int32_t T,
                               const double *targets16, uint32_t flags, const double *x0,
                               const double *ee_offset16, double *x_out, double *f_out,
                               int32_t *found_out);
/* Up to K distinct solutions per target (extension; optik_hip_ik_solutions): every restart index in
 * [0, config->max_restarts) of every target runs to its end, Speed as well as Quality, and the successes are taken
 * in (key, index) order -- Quality: distance to the seed, Speed: the index -- keeping one only if its largest joint
 * difference to every solution kept before it is > min_dist.  On a redundant arm the successes form a continuum and
 * min_dist sets the spacing of the returned samples.  With K = 1 the solution is what ik() returns for the target
 * (Quality with max_time = 0; Speed after set_parallelism(1)).  targets16 [T][16], flags and x0 [T][n] as in
 * optik_robot_ik_batch_poses (rc -3: invalid transform, -2: seed outside the limits) -> count_out [T] (0..K),
 * x_out [T][K][n], f_out [T][K], idx_out [T][K] in acceptance order; slots past the count: NaN, idx UINT64_MAX.  Any
 * output may be NULL.  max_restarts = 0 (unlimited) and max_restarts > OPTIK_ROBOT_MAX_SOLUTION_RESTARTS are refused
 * (-1) before any GPU work, as are K outside 1..256 and a NaN or negative min_dist.  The targets are cut into one
 * contiguous part per device and each part into launches of about 4 M (target, restart) items; a target never spans
 * two launches, so the result does not depend on either.  max_time: the time left is each launch's deadline; a launch
 * that would start after it is not run and its targets keep count 0. */
#define OPTIK_ROBOT_MAX_SOLUTION_RESTARTS (1ull << 22)
int optik_robot_ik_solutions(const optik_robot *robot, const CSolverConfig *config, int32_t T,
                             const double *targets16, uint32_t flags, const double *x0, const double *ee16,
                             int32_t K, double min_dist, int32_t *count_out, double *x_out /* [T][K][n] */,
                             double *f_out /* [T][K] */, uint64_t *idx_out /* [T][K] */);
/* Warm-started IK along P paths of L waypoints each (extension; optik_hip_ik_path): waypoint l of path p is solved
 * over restarts [0, config->max_restarts) from the path's current configuration c_p (first x0[p], then the last
 * accepted solution).  The accepted solution is the best success -- Quality: nearest to c_p, Speed: lowest index --
 * among those with max_i |x_i - c_i| <= max_step (+inf: every success; no angle wrapping).  A waypoint without one
 * keeps c_p and gives x and f NaN, idx UINT64_MAX, step NaN, found 0.  Speed with max_step = +inf equals a host loop
 * of ik() seeded from the previous result (set_parallelism(1), max_time = 0).  targets16 [P][L][16], flags as in
 * optik_robot_ik_batch_poses (rc -3: invalid transform; -2: a start configuration outside the limits), x0 [P][n] ->
 * path-major x_out [P][L][n], f_out, idx_out, step_out (max_i |x_i - c_i| against the configuration the waypoint was
 * solved from), found_out [P][L]; any output may be NULL.  Refused (-1) before any GPU work: max_restarts = 0
 * (unlimited) or above OPTIK_HIP_PATH_MAX_RESTARTS (4096), a NaN or negative max_step.  max_time, if set, is each
 * waypoint launch's deadline (not a budget for the call).  The paths are cut into one contiguous part per device
 * and each part into chunks of whole paths (a waypoint launch of about 4 M items at most): one upload, one
 * optik_hip_ik_path over every waypoint and one download per chunk.  The result depends on neither. */
int optik_robot_ik_path(const optik_robot *robot, const CSolverConfig *config, int32_t P, int32_t L,
                        const double *targets16 /* [P][L][16] */, uint32_t flags, const double *x0 /* [P][n] */,
                        const double *ee16, double max_step, double *x_out /* [P][L][n] */,
                        double *f_out /* [P][L] */, uint64_t *idx_out /* [P][L] */, double *step_out /* [P][L] */,
                        int32_t *found_out /* [P][L] */);
/* GPUs of this node the robot spreads its work over (restarts shard trivially: lib.rs:297-300
 * hands the same index range to rayon workers).  optik_robot_ik / _ik_ex: after the
 * latency-sized first launch every round's restart range is cut into one contiguous part per
 * GPU and the host keeps the minimum of the per-GPU (key, index) records -- the 16-byte
 * reduction SURVEY 8e calls for; _ik_batch_ex: the targets are cut into one contiguous part
 * per GPU, no reduction.  Results do not depend on the device list.  Must be called before
 * the robot's first GPU call; count = 0 restores the default (the HIP device current at first
 * use); the environment variable OPTIK_DEVICES ("all", a count, or "0,1,...") sets the list
 * for robots created after it.  A device may be listed more than once. */
int optik_robot_set_devices(optik_robot *robot, const int32_t *device_ids, int32_t count);
int32_t optik_robot_num_devices(const optik_robot *robot);
/* Over how many of the robot's devices the last _ik / _ik_batch call was actually cut (its widest round): 1 for a
 * call that ended with its latency-sized first launch or whose range was too short to be worth cutting. */
int32_t optik_robot_last_parts(const optik_robot *robot);
/* Robot::diff_ik with its full signature: ee_offset and alpha.  rc 0 = solved, 1 = none. */
int optik_robot_diff_ik_ex(const optik_robot *robot, const double *x0, const double *V_WE6,
                           const double *v_max, const double *ee_offset16, double *alpha_out,
                           double *v_out);
/* Many diff_ik calls at once (extension): row b returns what optik_robot_diff_ik_ex(robot, x0[b], V[b], v_max[b],
 * ee_offset16) returns, bit for bit.  Host buffers, row-major: x0 [B][n], V [B][6], v_max [B][n] ->
 * alpha_out [B], v_out [B][n], status_out [B] (0 solved, 1 no solution: alpha and v zero); any output may be
 * NULL.  One kernel launch per 262 144 rows on the robot's first device (staged through pinned memory kept
 * with the robot).  rc 0, or -1 with the single call's message: null argument, more than 8 joint positions,
 * prismatic joints. */
int optik_robot_diff_ik_batch(const optik_robot *robot, int64_t B, const double *x0, const double *V_WE6,
                              const double *v_max, const double *ee_offset16, double *alpha_out,
                              double *v_out, int32_t *status_out);
/* The measures of solution modes 3 and 4 (extension; include/optik_hip.h: OPTIK_MODE_*, optik_hip_manip_batch) for
 * B configurations: x [B][n] row-major -> w_out [B] manipulability, c_out [B] condition; either may be NULL.
 * ee_offset16 may be NULL.  One kernel launch per 262 144 rows on the robot's first device, as
 * optik_robot_diff_ik_batch.  rc 0, or -1: null argument, prismatic joints.  The modes themselves are valid for
 * optik_robot_ik*, optik_robot_ik_solutions and optik_robot_ik_path, and are scheduled there as Quality. */
int optik_robot_manipulability_batch(const optik_robot *robot, int64_t B, const double *x, const double *ee_offset16,
                                     double *w_out, double *c_out);
/* The collision filter (extension; include/optik_hip.h: optik_hip_chain_set_collision_model and what follows it).
 * Host arrays, checked before any device work (rc -1 and the reason in optik_robot_last_error: the refusals of
 * optik_hip_chain_set_collision_model / _set_world, and a model on a chain with prismatic joints), kept with the
 * robot and applied to every device chain it has or creates later (optik_robot_set_devices included).  While a model
 * with S >= 1 is set, every IK entry point returns free successes only: Speed runs every restart of a launch and
 * returns the lowest-index free success (set_parallelism has no effect on it), Quality and modes 3 and 4 the best
 * free success, ik_solutions free successes only, ik_path free waypoints only.  S = 0 clears the model. */
int optik_robot_set_collision_model(optik_robot *robot, const int32_t *frames, const double *centers3,
                                    const double *radii, int32_t S, const int32_t *pairs2, int32_t P, double margin);
int optik_robot_set_world(optik_robot *robot, const double *spheres4, int32_t Ms, const double *boxes10, int32_t Mb);
/* The distance-field world (extension; include/optik_hip.h: optik_hip_chain_set_world_grid and what precedes it).
 * Host arrays; the grid is kept with the robot and applied to every device chain it has or creates later
 * (optik_robot_set_devices included), as the model and the world are.  values == NULL with zero dims clears it.
 * optik_robot_world_grid_bake bakes the robot's current spheres and boxes on its first device into values_out
 * (host, nx * ny * nz floats) and installs nothing.  rc 0, or -1 with the refusal of the kernel layer. */
int optik_robot_set_world_grid(optik_robot *robot, const double *origin3, double voxel, int32_t nx, int32_t ny,
                               int32_t nz, const float *values);
int optik_robot_world_grid_bake(const optik_robot *robot, const double *origin3, double voxel, int32_t nx, int32_t ny,
                                int32_t nz, float *values_out);
/* From sensor data to that grid (extension; include/optik_hip.h: optik_hip_world_grid_from_occupancy and
 * optik_hip_occupancy_from_points).  Host arrays, on the robot's first device; both install nothing.
 * optik_robot_world_grid_from_occupancy: occupied (nx * ny * nz bytes, non-zero = occupied) -> values_out (floats), the
 * signed field of an exact Euclidean distance transform, clamped to +-max_distance.
 * optik_robot_occupancy_from_points: marks in `occupied` (read, then written back: clouds accumulate) the nodes of the
 * N points3 that none of the E exclude4 spheres (centre, radius; all finite here) holds.  rc 0, or -1. */
int optik_robot_world_grid_from_occupancy(const optik_robot *robot, double voxel, int32_t nx, int32_t ny, int32_t nz,
                                          const uint8_t *occupied, double max_distance, float *values_out);
int optik_robot_occupancy_from_points(const optik_robot *robot, const double *origin3, double voxel, int32_t nx,
                                      int32_t ny, int32_t nz, const double *points3, int64_t N,
                                      const double *exclude4, int32_t E, uint8_t *occupied);
/* Depth-image worlds (extension; include/optik_hip.h: optik_hip_depth_integrate and optik_hip_occupancy_from_map;
 * DESIGN.md section 5.23).  Host arrays, on the robot's first device; both install nothing and keep nothing: the
 * caller owns the map.  optik_robot_depth_integrate: `map` (nx * ny * nz int16, OPTIK_HIP_MAP_UNKNOWN = -32768 where
 * never observed; read, then written back) takes the evidence of the F images of `depth` ([F][H][W] floats, z-depth in
 * metres) seen with intrinsics4 [F][4] (fx, fy, cx, cy) from poses16 [F][16] (column-major 4x4 each, as
 * optik_robot_fk_ex writes them; x right, y down, z forward); pixels on the E exclude4 spheres carve and do not mark.
 * optik_robot_occupancy_from_map: occupied (nx * ny * nz bytes) = unknown_occupied where the map is unknown, (e >=
 * threshold) elsewhere; accumulate != 0 ORs that into what `occupied` holds.  rc 0, or -1: the refusals of the kernel
 * layer, and a non-finite exclusion sphere. */
int optik_robot_depth_integrate(const optik_robot *robot, const double *origin3, double voxel, int32_t nx, int32_t ny,
                                int32_t nz, int16_t *map, const float *depth, int32_t F, int32_t H, int32_t W,
                                const double *intrinsics4, const double *poses16, const double *exclude4, int32_t E,
                                double z_near, double z_far, double band, int32_t hit, int32_t miss, int32_t e_min,
                                int32_t e_max);
int optik_robot_occupancy_from_map(const optik_robot *robot, int32_t nx, int32_t ny, int32_t nz, const int16_t *map,
                                   int32_t threshold, int32_t unknown_occupied, int32_t accumulate, uint8_t *occupied);
/* From a triangle mesh to that grid (extension; include/optik_hip.h: optik_hip_world_grid_from_mesh).  Host arrays,
 * on the robot's first device; installs nothing.  tris9 [M][9]: the vertices a, b, c of each triangle in the base
 * frame -> values_out (nx * ny * nz floats): the signed distance to the mesh, clamped to +-max_distance.  rc 0, or -1:
 * the refusals of the kernel layer, and a NaN or infinite coordinate. */
int optik_robot_world_grid_from_mesh(const optik_robot *robot, const double *origin3, double voxel, int32_t nx,
                                     int32_t ny, int32_t nz, const double *tris9, int32_t M, double max_distance,
                                     float *values_out);
/* From a solid to a sphere model (extension; include/optik_hip.h: optik_hip_sphere_fit).  Host arrays, on the robot's
 * first device; installs nothing.  values (nx * ny * nz floats: a signed distance field of the solid, negative inside)
 * and points3 [P][3] on its surface -> chosen_out int32 [K], centers_out [K][3], radii_out [K], gains_out int32 [K],
 * count_uncovered_out int32 [2] (the spheres chosen, the points left uncovered); entries past the count are -1, NaN,
 * NaN and 0.  rc 0, or -1: the refusals of the kernel layer, and a NaN or infinite point. */
int optik_robot_sphere_fit(const optik_robot *robot, const double *origin3, double voxel, int32_t nx, int32_t ny,
                           int32_t nz, const float *values, const double *points3, int64_t P, double pad, double slack,
                           int32_t K, int32_t *chosen_out, double *centers_out, double *radii_out, int32_t *gains_out,
                           int32_t *count_uncovered_out);
/* x [B][n] -> frames16_out [B][n + 2][16]: every frame as a column-major 4x4 (as optik_robot_fk_ex writes it; frame
 * n + 1 is fk's pose).  ee_offset16 may be NULL.  On the robot's first device; rc 0 or -1. */
int optik_robot_link_frames_batch(const optik_robot *robot, int64_t B, const double *x, const double *ee_offset16,
                                  double *frames16_out);
/* x [B][n] -> clearance_out [B], free_out [B] (1 iff clearance >= margin); either may be NULL.  rc 0 or -1. */
int optik_robot_collision_batch(const optik_robot *robot, int64_t B, const double *x, const double *ee_offset16,
                                double *clearance_out, uint8_t *free_out);
/* Which way is out (extension; include/optik_hip.h: optik_hip_collision_witness_batch).  x [B][n] -> per
 * configuration the F = n + 2 witness rows, row-major: dist_out [B][F], grad_out [B][F][n], witness_out [B][F][3]
 * (robot sphere, kind, index); any may be NULL.  On the robot's first device; rc 0, or -1: null argument, more than
 * 8 joint positions, prismatic joints. */
int optik_robot_collision_witness_batch(const optik_robot *robot, int64_t B, const double *x,
                                        const double *ee_offset16, double *dist_out, double *grad_out,
                                        int32_t *witness_out);
/* Collision-avoiding diff_ik (extension; include/optik_hip.h: optik_hip_diff_ik_avoid_batch): optik_robot_diff_ik_ex
 * with a velocity damper for each of the (up to 4) closest frames within `influence` of an obstacle or of another
 * link.  rc 0 = solved, 1 = none (also: the dampers cannot be met within v_max; alpha and v are then zero), -1 =
 * refused: what optik_robot_diff_ik_ex refuses, and unless influence > safety >= 0 and gain > 0, all finite.
 * The single call is the batch with B = 1 (one launch of the fused kernel on the robot's first device), so row b of
 * optik_robot_diff_ik_avoid_batch returns its bits.  Without a collision model both return what
 * optik_robot_diff_ik_ex / _batch return, bit for bit. */
int optik_robot_diff_ik_avoid(const optik_robot *robot, const double *x0, const double *V_WE6, const double *v_max,
                              double influence, double safety, double gain, const double *ee_offset16,
                              double *alpha_out, double *v_out);
int optik_robot_diff_ik_avoid_batch(const optik_robot *robot, int64_t B, const double *x0, const double *V_WE6,
                                    const double *v_max, double influence, double safety, double gain,
                                    const double *ee_offset16, double *alpha_out, double *v_out,
                                    int32_t *status_out);
/* Bending paths out of collision (extension; include/optik_hip.h: optik_hip_path_optimize).  paths [P][L][n]
 * row-major, 3 <= L <= 64 -> paths_out [P][L][n] (may be `paths`), cost_first_out and cost_last_out [P][3] = (U,
 * F_smooth, F_obs), clearance_out [P], status_out [P] (0, or 1: the last cost is NaN); any output may be NULL.  On the
 * robot's first device; rc 0, or -1: null argument, what optik_hip_path_optimize refuses. */
int optik_robot_path_optimize(const optik_robot *robot, int64_t P, int32_t L, const double *paths, int32_t iters,
                              double step, double w_smooth, double w_obs, double influence, double safety,
                              const double *ee_offset16, double *paths_out, double *cost_first_out,
                              double *cost_last_out, double *clearance_out, int32_t *status_out);
/* Roadmap planning (extension; include/optik_hip.h: optik_hip_roadmap_knn and what follows it; DESIGN.md section
 * 5.18): a way round what the motion check refuses.
 * optik_robot_roadmap_build: N nodes (1 .. 8192) -- the seeds of restart indices first .. first + N - 1, the generator
 * of the IK restarts, uniform inside the joint limits --, each node's k (1 .. 16) nearest others (L-infinity) and the
 * motion node -> neighbour checked at `resolution` against the robot's model and world.  Nodes in collision are
 * kept: they have no free edge.  The roadmap lives in the robot handle, on its first device, and replaces the one
 * before.  Returns the number of free edges, or -1 (what the kernel layer refuses: N, k, the resolution, prismatic
 * joints, infinite joint limits).
 * optik_robot_roadmap_plan: starts, goals [Q][n] row-major -> paths_out [Q][Lmax][n], 2 <= Lmax <= 64 (start, the
 * nodes of the route, goal, padded with the goal: what optik_robot_path_optimize takes), len_out [Q] the waypoints
 * before the padding, cost_out [Q] the L-infinity length of the route, status_out [Q]: 0 found; 1 no route (cost +inf);
 * 2 the route needs more than Lmax waypoints (the true cost); 3 a NaN in the query (cost NaN); unless 0 the path is
 * the start, then the goal repeated.  Any output may be NULL.  Each start and goal is linked to its k nearest nodes
 * and the direct motion start -> goal is checked too, all at the roadmap's resolution; ties go to the direct motion.
 * rc 0, or -1: no roadmap; a stale roadmap -- optik_robot_set_collision_model, _set_world and _set_world_grid each
 * make it stale, so a plan is never checked against a world that is gone: build it again --; a bad Lmax. */
int64_t optik_robot_roadmap_build(optik_robot *robot, int32_t N, int32_t k, double resolution, uint64_t first);
int optik_robot_roadmap_plan(const optik_robot *robot, const double *starts, const double *goals, int64_t Q,
                             int32_t Lmax, double *paths_out, int32_t *len_out, double *cost_out,
                             int32_t *status_out);
/* Lazy roadmaps (extension; include/optik_hip.h: optik_hip_roadmap_lazy_plan): a roadmap
 * that follows a changing world.  Its nodes and neighbour lists survive every optik_robot_set_world* and
 * optik_robot_set_collision_model call; its edges are presumed free and checked only when a shortest route uses them,
 * and the verdicts are forgotten when the world changes.  A lazy roadmap is never stale.
 * optik_robot_roadmap_build_lazy: the nodes of optik_robot_roadmap_build (the same seeds) and their k nearest others;
 * nothing is checked but the nodes themselves.  Replaces the robot's roadmap, eager or lazy.  Returns the number of
 * slots that are not blocked (neither empty nor touching a node in collision), or -1.
 * optik_robot_roadmap_plan_lazy: optik_robot_roadmap_plan's arguments and outputs, and `rounds` in 0 .. 4096: at most
 * that many rounds of checking the unknown edges of the current routes.  With enough rounds every plan of status 0,
 * 1 or 3 equals optik_robot_roadmap_plan over an eager roadmap of the same N, k, resolution, first and world, bit
 * for bit.  Status 4: unsettled -- the route found last still holds an unchecked edge; len 2, the start, then the
 * goal repeated, the cost a lower bound (as is the cost of status 2 here).  If the world changed since the last
 * plan, the verdicts are reset first.  Queries run in chunks of 4 096 against the shared verdicts;
 * *rounds_used_out and *checked_out (may be NULL) are the rounds made and the edges checked, added up over the
 * chunks.  Concurrent callers are serialised.  rc 0, or -1.
 * optik_robot_roadmap_plan on a lazy roadmap and optik_robot_roadmap_plan_lazy on an eager one fail, each naming the
 * other. */
int64_t optik_robot_roadmap_build_lazy(optik_robot *robot, int32_t N, int32_t k, double resolution, uint64_t first);
int optik_robot_roadmap_plan_lazy(const optik_robot *robot, const double *starts, const double *goals, int64_t Q,
                                  int32_t Lmax, int32_t rounds, double *paths_out, int32_t *len_out, double *cost_out,
                                  int32_t *status_out, int32_t *rounds_used_out, int64_t *checked_out);
/* Goal-set planning (extension; include/optik_hip.h: optik_hip_roadmap_query_goals): the
 * cheapest route to any of several goals -- the IK solutions of a pose, for one -- in one pass over the roadmap.
 * optik_robot_roadmap_plan_goals: optik_robot_roadmap_plan with goals [Q][G][n] row-major, 1 <= G <= 16, and counts
 * [Q] (NULL: G each): query q has the goals g < counts[q] only, nothing of the others is read (the NaN rows of
 * optik_robot_ik_solutions past its count are harmless), and counts[q] = 0 is status 1.  Outputs as there, for the
 * cheapest route over the counted goals (its cost is the minimum of optik_robot_roadmap_plan's costs to each, bit for
 * bit), and goal_out [Q]: the goal reached for status 0, -1 otherwise.  A found path ends in that goal; any other is
 * the start, then goal 0 repeated (the start repeated without goals).  Ties go to the direct motion to the lowest goal.
 * Queries run in chunks of 4 096.  rc 0, or -1: what optik_robot_roadmap_plan refuses, G out of range, and a lazy
 * roadmap -- this call plans over eager roadmaps only; optik_robot_roadmap_plan_goals_lazy plans goal sets over lazy
 * ones. */
int optik_robot_roadmap_plan_goals(const optik_robot *robot, const double *starts, const double *goals,
                                   const int32_t *counts, int32_t G, int64_t Q, int32_t Lmax, double *paths_out,
                                   int32_t *len_out, double *cost_out, int32_t *status_out, int32_t *goal_out);
/* Goal sets on lazy roadmaps (extension; include/optik_hip.h: optik_hip_roadmap_lazy_plan_goals; DESIGN.md section
 * 5.34): "the world just changed, now plan to this pose".  optik_robot_roadmap_plan_goals_lazy takes
 * optik_robot_roadmap_plan_goals' arguments and outputs over the roadmap of optik_robot_roadmap_build_lazy, with
 * `rounds`, rounds_used_out and checked_out as optik_robot_roadmap_plan_lazy has them: a world that changed since the
 * last call resets the verdicts first, the chunks of 4 096 queries share the verdicts, and the two counters are
 * added up over the chunks.  One more status, 4: the route found last still holds an unchecked edge -- len 2, the
 * start, then goal 0 repeated, goal -1, the cost a lower bound.  A plan of status 0, 1 or 3 equals
 * optik_robot_roadmap_plan_goals over an eager roadmap of the same N, k, resolution, first and world, bit for bit.
 * rc 0, or -1: null argument, G, Lmax or rounds out of range, no roadmap, and an eager roadmap (the message names
 * optik_robot_roadmap_plan_goals). */
int optik_robot_roadmap_plan_goals_lazy(const optik_robot *robot, const double *starts, const double *goals,
                                        const int32_t *counts, int32_t G, int64_t Q, int32_t Lmax, int32_t rounds,
                                        double *paths_out, int32_t *len_out, double *cost_out, int32_t *status_out,
                                        int32_t *goal_out, int32_t *rounds_used_out, int64_t *checked_out);
/* The bidirectional tree planner (extension; include/optik_hip.h: optik_hip_rrt_plan): what to
 * run on the rows that optik_robot_roadmap_plan returns as status 1.  It reads no roadmap and keeps no state in the
 * robot: starts, goals [Q][n] row-major; two trees per query of at most max_nodes (2 .. 4096) nodes grow from the
 * query's own start and goal for at most iters (1 .. 65 536) iterations with steps of at most `step` radians
 * (L-infinity) towards the restart seeds first, first + 1, ..., every motion checked at `resolution` in the direction
 * the path travels it.  paths_out [Q][Lmax][n], 2 <= Lmax <= 64, len_out [Q], cost_out [Q], status_out [Q] as
 * optik_robot_roadmap_plan writes them (0 found; 1 not found, or a start or goal in collision; 2 found with more than
 * Lmax waypoints; 3 a NaN or an infinity in the query); iters_out [Q] the iterations run; nodes_out [Q][2] the sizes of
 * the trees.  Any output may be NULL.  poll (1 .. 65 536): the iterations between two looks at the number of unfinished
 * queries.  Queries run in chunks of 4 096; a query's result does not depend on the others.  On the robot's first
 * device.  rc 0, or -1: null argument, what the kernel layer refuses. */
int optik_robot_rrt_plan(const optik_robot *robot, const double *starts, const double *goals, int64_t Q, int32_t iters,
                         double step, double resolution, uint64_t first, int32_t max_nodes, int32_t Lmax, int32_t poll,
                         const double *ee_offset16, double *paths_out, int32_t *len_out, double *cost_out,
                         int32_t *status_out, int32_t *iters_out, int32_t *nodes_out);
/* The tree planner with a goal set (extension; include/optik_hip.h: optik_hip_rrt_plan_goals):
 * optik_robot_rrt_plan with goals [Q][G][n] row-major, 1 <= G <= 16, and counts [Q] (NULL: G each): query q has the
 * goals g < counts[q] only, nothing of the others influences an output (the NaN rows of optik_robot_ik_solutions past
 * its count are the normal input), and counts[q] = 0 is status 1.  Tree 1 has one root per counted goal that is free;
 * the query ends at the first junction with any of them -- past the direct motions, where the nearest free one wins and
 * a tie goes to the lower goal, the answer is the goal joined first, not the cheapest.  max_nodes in max(2, G) ..
 * 4096.  Outputs as optik_robot_rrt_plan's, and goal_out [Q]: the goal reached for status 0, -1 otherwise.  A found
 * path ends in that goal; any other is the start, then goal 0 repeated (the start repeated without goals).  It reads no
 * roadmap and keeps no state in the robot.  Queries run in chunks of 4 096.  rc 0, or -1: null argument, G out of
 * range, what the kernel layer refuses. */
int optik_robot_rrt_plan_goals(const optik_robot *robot, const double *starts, const double *goals,
                               const int32_t *counts, int32_t G, int64_t Q, int32_t iters, double step,
                               double resolution, uint64_t first, int32_t max_nodes, int32_t Lmax, int32_t poll,
                               const double *ee_offset16, double *paths_out, int32_t *len_out, double *cost_out,
                               int32_t *status_out, int32_t *iters_out, int32_t *nodes_out, int32_t *goal_out);
/* The tree planner under a pose constraint (extension; include/optik_hip.h: optik_hip_rrt_plan_constrained; DESIGN.md
 * section 5.30): optik_robot_rrt_plan_goals with every tree node projected onto the pose constraint (ref7, lo6, hi6:
 * optik_robot_constraint_batch's) at ptol within piters iterations (damping, max_step: the projection's), and every
 * motion checked against the collision model and against the constraint at tol, in the direction of travel.  A start
 * that violates the constraint at tol gives status 1; a goal that does is not a root.  Outputs as
 * optik_robot_rrt_plan_goals', and projected_out [Q][2]: the projections attempted and the ones that ended projected.
 * One goal per query: G = 1, counts NULL.  rc 0, or -1: null argument, what the kernel layer refuses. */
int optik_robot_rrt_plan_constrained(const optik_robot *robot, const double *starts, const double *goals,
                                     const int32_t *counts, int32_t G, int64_t Q, const double *ref7, const double *lo6,
                                     const double *hi6, double tol, double ptol, int32_t piters, double damping,
                                     double max_step, int32_t iters, double step, double resolution, uint64_t first,
                                     int32_t max_nodes, int32_t Lmax, int32_t poll, const double *ee_offset16,
                                     double *paths_out, int32_t *len_out, double *cost_out, int32_t *status_out,
                                     int32_t *iters_out, int32_t *nodes_out, int32_t *goal_out,
                                     int32_t *projected_out);
/* Shortcutting and resampling planned paths (extension; include/optik_hip.h: optik_hip_path_shortcut and
 * optik_hip_path_resample).  paths [P][L][n] row-major with lens [P] waypoints each (NULL: L
 * each), 2 <= L <= 64 -- optik_robot_roadmap_plan's paths_out and len_out as they are.
 * optik_robot_path_shortcut: at most `vertices` (2 .. 64) vertices per path, every pair of them checked at
 * `resolution`, the route of least length + hop_penalty per hop walked -> paths_out [P][Lout][n] padded with the goal,
 * len_out [P], cost_out [P], cost_in_out [P], status_out [P]: 0 found; 1 no route; 2 a length outside 2 .. min(L,
 * vertices) or a route of more than Lout waypoints; 3 a NaN or an infinity in the path; unless 0 the input comes back.
 * optik_robot_path_resample: Lout (2 .. 64) waypoints at equal L-infinity arc length -> paths_out [P][Lout][n],
 * status_out [P] (0; 2 a bad length; 3 a length that is NaN or infinite).  The resampled segments are not checked.
 * Any output may be NULL.  On the robot's first device; neither reads the robot's roadmap.  rc 0, or -1: null
 * argument, what the kernel layer refuses. */
int optik_robot_path_shortcut(const optik_robot *robot, int64_t P, int32_t L, const double *paths, const int32_t *lens,
                              int32_t vertices, double resolution, double hop_penalty, int32_t Lout,
                              const double *ee_offset16, double *paths_out, int32_t *len_out, double *cost_out,
                              double *cost_in_out, int32_t *status_out);
int optik_robot_path_resample(const optik_robot *robot, int64_t P, int32_t L, const double *paths, const int32_t *lens,
                              int32_t Lout, double *paths_out, int32_t *status_out);
/* Shortcutting and resampling that keep a pose constraint (extension; include/optik_hip.h:
 * optik_hip_path_shortcut_constrained and optik_hip_path_resample_constrained).  The two entries
 * above with the constraint ref7 (t, quaternion i j k w), lo6, hi6: every new vertex / interior waypoint is projected
 * onto it at ptol (at most piters iterations, damping, max_step), the input's own waypoints and the two ends never
 * move, and a shortcut's pairs must pass the motion check AND the constraint's check along the motion at tol.
 * projected_out [P][2]: the projections attempted and those that ended projected.  optik_robot_path_resample_constrained's
 * status_out adds 4: an interior waypoint could not be projected and kept its interpolated value.  Any output may be
 * NULL.  rc 0, or -1: null argument, what the kernel layer refuses. */
int optik_robot_path_shortcut_constrained(const optik_robot *robot, int64_t P, int32_t L, const double *paths,
                                          const int32_t *lens, int32_t vertices, double resolution, double hop_penalty,
                                          int32_t Lout, const double *ref7, const double *lo6, const double *hi6,
                                          double tol, double ptol, int32_t piters, double damping, double max_step,
                                          const double *ee_offset16, double *paths_out, int32_t *len_out,
                                          double *cost_out, double *cost_in_out, int32_t *status_out,
                                          int32_t *projected_out);
int optik_robot_path_resample_constrained(const optik_robot *robot, int64_t P, int32_t L, const double *paths,
                                          const int32_t *lens, int32_t Lout, const double *ref7, const double *lo6,
                                          const double *hi6, double ptol, int32_t piters, double damping,
                                          double max_step, const double *ee_offset16, double *paths_out,
                                          int32_t *status_out, int32_t *projected_out);
/* Path optimisation that keeps a pose constraint (extension; include/optik_hip.h: optik_hip_path_optimize_constrained;
 * DESIGN.md section 5.32).  optik_robot_path_optimize with the constraint ref7, lo6, hi6: after every update each
 * interior waypoint is projected back onto it at ptol (at most piters iterations, damping, max_step) and keeps its old
 * value where that fails.  violation_out [P]: the largest violation over the waypoints of the result; projected_out
 * [P][2]: the projections attempted and those that ended projected.  Any output may be NULL.  rc 0, or -1: null
 * argument, what the kernel layer refuses. */
int optik_robot_path_optimize_constrained(const optik_robot *robot, int64_t P, int32_t L, const double *paths,
                                          int32_t iters, double step, double w_smooth, double w_obs, double influence,
                                          double safety, const double *ref7, const double *lo6, const double *hi6,
                                          double ptol, int32_t piters, double damping, double max_step,
                                          const double *ee_offset16, double *paths_out, double *cost_first_out,
                                          double *cost_last_out, double *clearance_out, int32_t *status_out,
                                          double *violation_out, int32_t *projected_out);
/* Collision repair (extension; include/optik_hip.h: optik_hip_collision_repair_batch).  B rows
 * x [B][n] row-major, each pushed out of collision on its own along the gradient of its clearance until the clearance
 * is >= safety, with ref7, lo6, hi6 (all NULL: no box) projected back onto that pose box at ptol after every step.
 * x_out [B][n], clearance_out, violation_out, moved_out [B], status_out [B] (0 free, 1 iters spent, 2 stuck, 3 NaN),
 * iterations_out [B]; any output may be NULL.  rc 0, or -1: null argument, what the kernel layer refuses. */
int optik_robot_collision_repair_batch(const optik_robot *robot, int64_t B, const double *x, double influence,
                                       double safety, double step, int32_t iters, double max_move, const double *ref7,
                                       const double *lo6, const double *hi6, double ptol, int32_t piters,
                                       double damping, double project_max_step, const double *ee_offset16,
                                       double *x_out, double *clearance_out, double *violation_out, double *moved_out,
                                       int32_t *status_out, int32_t *iterations_out);
/* Timing planned paths and sampling the trajectory (extension; include/optik_hip.h: optik_hip_path_time and
 * optik_hip_trajectory_sample).  paths [P][L][n] row-major with lens [P] waypoints each (NULL: L
 * each), 3 <= L <= 64 -- optik_robot_path_resample's paths_out as it is.
 * optik_robot_path_time: rest-to-rest timing under v_max [n] (> 0, may be +inf) and a_max [n] (finite, > 0) ->
 * times_out [P][L], vel_out [P][L][n], acc_out [P][L][n], duration_out [P], status_out [P]: 0 timed; 1 stalled (a
 * segment with zero speed at both ends); 2 a length outside 3 .. L or a stage that bounds nothing; 3 a NaN or an
 * infinity in the path; unless 0 the times and the duration are NaN.
 * optik_robot_trajectory_sample: T (1 .. 65 536) samples per path at k * dt by cubic Hermite interpolation over what
 * optik_robot_path_time returned -> q_out [P][T][n], qd_out [P][T][n]; past the duration the goal at rest, for a status
 * other than 0 the start at rest.  The samples are not checked for collision.
 * optik_robot_velocity_limits: the URDF's <limit velocity=> of the n articulated joints, +inf where it is absent, 0
 * or negative; a malloc'ed array of n doubles the caller frees.
 * Any output may be NULL.  On the robot's first device.  rc 0, or -1: null argument, what the kernel layer refuses. */
int optik_robot_path_time(const optik_robot *robot, int64_t P, int32_t L, const double *paths, const int32_t *lens,
                          const double *v_max, const double *a_max, double *times_out, double *vel_out,
                          double *acc_out, double *duration_out, int32_t *status_out);
int optik_robot_trajectory_sample(const optik_robot *robot, int64_t P, int32_t L, const double *paths,
                                  const int32_t *lens, const double *times, const double *velocities,
                                  const int32_t *status, double dt, int32_t T, double *q_out, double *qd_out);
const double *optik_robot_velocity_limits(const optik_robot *robot);
/* optik_robot_path_time with limits on the tool as well (extension; include/optik_hip.h: optik_hip_path_time_tool;
 * DESIGN.md section 5.35).  tool_limits4: the tool centre point's speed, its tangential and its normal acceleration and
 * the end effector's angular speed, each > 0, +inf for "no limit"; the tool is the end effector with ee_offset16 (may
 * be NULL).  Beside optik_robot_path_time's outputs: tool_speed_out [P][L], tool_accel_out [P][L][2] (tangential,
 * normal), tool_wspeed_out [P][L] at the waypoints.  Any output may be NULL.  rc 0, or -1: null argument, what the
 * kernel layer refuses (a tool limit that is NaN or <= 0 among it). */
int optik_robot_path_time_tool(const optik_robot *robot, int64_t P, int32_t L, const double *paths,
                               const int32_t *lens, const double *v_max, const double *a_max,
                               const double *tool_limits4, const double *ee_offset16, double *times_out,
                               double *vel_out, double *acc_out, double *duration_out, int32_t *status_out,
                               double *tool_speed_out, double *tool_accel_out, double *tool_wspeed_out);
/* Spline retiming of timed paths (extension; include/optik_hip.h: optik_hip_path_time_spline):
 * paths [P][L][n], lens (may be NULL), times [P][L] and status [P] (may be NULL: all 0) as optik_robot_path_time
 * returned them; v_max, a_max, j_max [n], each > 0, +inf for "no limit".  Outputs, any may be NULL: times_out [P][L],
 * vel_out and acc_out [P][L][n], duration_out [P], factor_out [P], ratios_out [P][3], status_out [P].  rc 0, or -1:
 * null argument, what the kernel layer refuses. */
int optik_robot_path_time_spline(const optik_robot *robot, int64_t P, int32_t L, const double *paths,
                                 const int32_t *lens, const double *times, const int32_t *status,
                                 const double *v_max, const double *a_max, const double *j_max, double *times_out,
                                 double *vel_out, double *acc_out, double *duration_out, double *factor_out,
                                 double *ratios_out, int32_t *status_out);
/* The motion check (extension; include/optik_hip.h: optik_hip_collision_motion_batch and what precedes it).  B segments
 * xa, xb [B][n] row-major at `resolution` (finite, > 0) -> clearance_out [B], free_out [B], first_out [B], steps_out
 * [B]; any may be NULL (clearance_out NULL: the call only classifies).  On the robot's first device, 65 536 segments
 * per launch.  rc 0, or -1: null argument, B < 0, a bad resolution, prismatic joints. */
int optik_robot_collision_motion_batch(const optik_robot *robot, int64_t B, const double *xa, const double *xb,
                                       double resolution, const double *ee_offset16, double *clearance_out,
                                       uint8_t *free_out, int32_t *first_out, int32_t *steps_out);
/* The resolution h of the motion check of optik_robot_ik_path between a path's seed and each candidate (include/
 * optik_hip.h: optik_hip_chain_set_motion_resolution): 0 (the default) is off; it acts while a collision model is
 * set.  Kept with the robot and applied to every device chain it has or creates later (optik_robot_set_devices
 * included).  The other IK entry points ignore it.  rc 0, or -1 for a NaN, negative or infinite h. */
int optik_robot_set_motion_resolution(optik_robot *robot, double h);
/* The certified motion check (extension; include/optik_hip.h: optik_hip_collision_motion_certify_batch and what
 * precedes it).  B segments xa, xb [B][n] row-major -> status_out [B] (OPTIK_HIP_CERTIFY_*:
 * 0 free along the whole segment down to margin - tol, 1 blocked at t_stop, 2 max_steps reached, 3 NaN), steps_out
 * [B], t_stop_out [B], clearance_out [B]; any may be NULL.  On the robot's first device, 65 536 segments per launch.
 * rc 0, or -1: null argument, B < 0, tol or grid_lipschitz not finite and > 0, max_steps outside 2 .. 65 536,
 * prismatic joints. */
int optik_robot_collision_motion_certify_batch(const optik_robot *robot, int64_t B, const double *xa,
                                               const double *xb, double tol, double grid_lipschitz,
                                               int32_t max_steps, const double *ee_offset16, int32_t *status_out,
                                               int32_t *steps_out, double *t_stop_out, double *clearance_out);
/* Pose constraints (extension; include/optik_hip.h: optik_hip_constraint_batch and what precedes it; DESIGN.md section
 * 5.29).  The constraint is ref7 (t, quaternion i j k w), lo6, hi6 with every call; rows x, xa, xb [B][n] row-major.
 * optik_robot_constraint_batch -> residual_out [B][6], violation_out [B]; optik_robot_constraint_project_batch ->
 * x_out [B][n], violation_out [B], status_out [B] (OPTIK_HIP_CONSTRAINT_*), iterations_out [B];
 * optik_robot_constraint_motion_batch -> violation_out [B], ok_out [B], first_out [B], steps_out [B].  Any output may
 * be NULL.  On the robot's first device through the staging loop of the other row batches, 262 144 rows (65 536
 * segments) per launch.  rc 0, or -1: null argument, B < 0, and what the kernel layer refuses -- a reference that is
 * not finite or whose quaternion is not of unit norm, lo <= hi false on an axis, tol not finite and >= 0, iters
 * outside 0 .. 4096, damping < 0, max_step or resolution not finite and > 0, prismatic joints. */
int optik_robot_constraint_batch(const optik_robot *robot, int64_t B, const double *x, const double *ref7,
                                 const double *lo6, const double *hi6, const double *ee_offset16,
                                 double *residual_out, double *violation_out);
int optik_robot_constraint_project_batch(const optik_robot *robot, int64_t B, const double *x, const double *ref7,
                                         const double *lo6, const double *hi6, double tol, int32_t iters,
                                         double damping, double max_step, const double *ee_offset16, double *x_out,
                                         double *violation_out, int32_t *status_out, int32_t *iterations_out);
int optik_robot_constraint_motion_batch(const optik_robot *robot, int64_t B, const double *xa, const double *xb,
                                        double resolution, const double *ref7, const double *lo6, const double *hi6,
                                        double tol, const double *ee_offset16, double *violation_out, uint8_t *ok_out,
                                        int32_t *first_out, int32_t *steps_out);
/* Up to K distinct configurations per pose region (extension; include/optik_hip.h: optik_hip_ik_region; DESIGN.md
 * section 5.33).  regions19 [T][19] row-major, per region ref[7] (t, quaternion i j k w), lo[6], hi[6]; x0 [T][n].
 * Every restart index in [0, restarts) runs (1 .. 2^22); tol, iters, damping, max_step as
 * optik_robot_constraint_project_batch; mode an OPTIK_MODE_*; keep_ref7 / keep_lo6 / keep_hi6 / keep_tol a second box
 * that every returned row must satisfy (all NULL: none).  Outputs, any may be NULL: count_out [T], x_out [T][K][n] (NaN
 * past count), violation_out [T][K] (NaN), idx_out [T][K] (UINT64_MAX), key_out [T][K] (+inf).  On the robot's first
 * device, whole regions of about 4 M restarts per launch.  rc 0, or -1: null argument, T < 0, restarts out of range,
 * a region that is not valid -- a reference that is not finite or whose quaternion is not of unit norm, lo <= hi false
 * on an axis; the message names the row --, and what the kernel layer refuses. */
int optik_robot_ik_region(const optik_robot *robot, int32_t T, const double *regions19, const double *x0,
                          uint64_t restarts, double tol, int32_t iters, double damping, double max_step, int32_t mode,
                          const double *keep_ref7, const double *keep_lo6, const double *keep_hi6, double keep_tol,
                          int32_t K, double min_dist, const double *ee_offset16, int32_t *count_out, double *x_out,
                          double *violation_out, uint64_t *idx_out, double *key_out);
/* optik_robot_ik_region with collision repair (include/optik_hip.h: optik_hip_ik_region_repair; DESIGN.md section
 * 5.37).  repair5 = influence, safety, step, iters, max_move (NULL: optik_robot_ik_region itself); repaired_out [T] (may
 * be NULL): the restarts of each region that took a repaired configuration. */
int optik_robot_ik_region_repair(const optik_robot *robot, int32_t T, const double *regions19, const double *x0,
                                 uint64_t restarts, double tol, int32_t iters, double damping, double max_step,
                                 int32_t mode, const double *keep_ref7, const double *keep_lo6, const double *keep_hi6,
                                 double keep_tol, int32_t K, double min_dist, const double *repair5,
                                 const double *ee_offset16, int32_t *count_out, double *x_out, double *violation_out,
                                 uint64_t *idx_out, double *key_out, int32_t *repaired_out);
int optik_robot_fk_ex(const optik_robot *robot, const double *x, const double *ee_offset16,
                      double *pose16_out);
int optik_robot_joint_jacobian_ex(const optik_robot *robot, const double *x,
                                  const double *ee_offset16, double *jac6n_out);
/* Flat chain table (what KinematicChain::from_urdf produced): n_joints poses, axes, types.
 * optik_robot_chain_tables: *n_joints is IN/OUT -- with non-NULL buffers it holds their capacity in joints on
 * entry (x 7 / x 3 / x 1 elements each; OPTIK_MAX_JOINTS covers every chain of at most 8 joint positions) and the
 * chain's joint count on return; fewer than the chain has: error, nothing is written.  With NULL buffers it just
 * reports the count.  optik_robot_chain_tables_n: the same with the capacity as its own argument. */
#define OPTIK_MAX_JOINTS 9
int optik_robot_chain_tables(const optik_robot *robot, int32_t *n_joints, double *origins7,
                             double *axes3, int32_t *types);
int optik_robot_chain_tables_n(const optik_robot *robot, int32_t capacity, int32_t *n_joints,
                               double *origins7, double *axes3, int32_t *types);
/* The device-side chain of this robot on the current HIP device (created on first
 * use; owned by the robot). */
optik_hip_chain *optik_robot_hip_chain(const optik_robot *robot);

#ifdef __cplusplus
}
#endif
#endif
