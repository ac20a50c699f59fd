// ik_host.hpp -- what the host-side translation units of the kernel layer share: the chain handle, the tuning
// options, error reporting and the (n, trailing fixed joint) dispatch.
//
//   ik_capi.hip        chains, options, optik_hip_ik_batch / optik_hip_ik_host, timing (the C ABI of optik_hip.h)
//   ik_launch_plan.hpp which solver a restart launch runs on and its grid: plan_launch, plain C++ (the one place)
//   ik_select.hip      the selection of lib.rs:397-413 over the per-restart keys
//   ik_solutions.hip   up to K distinct solutions per target over the same keys (optik_hip_ik_solutions)
//   ik_path.hip        the per-waypoint selection of warm-started paths (optik_hip_ik_path)
//   ik_manip.hip       the manipulability / condition keys of solution modes 3 and 4, optik_hip_manip_batch
//   ik_collision.hip   the collision filter: model and world, its key pass, link frames and clearance batches
//   ik_motion.hip      the motion check: segments between configurations, the motion key pass of optik_hip_ik_path
//   ik_advance.hip     the certified motion check: conservative advancement, one wave per segment
//   ik_avoid.hip       clearance witnesses and gradients, collision-avoiding diff_ik (velocity dampers)
//   ik_path_optimize.hip  covariant gradient smoothing of joint paths against the same witnesses
//   ik_roadmap.hip     roadmap planning: nearest neighbours, motion-checked edges, shortest-path queries
//   ik_roadmap_lazy.hip  lazy roadmaps: edges checked only when a route uses them, verdicts kept across plans
//   ik_rrt.hip         the bidirectional tree planner: two trees per query, for the queries a roadmap misses; tree 1
//                      rooted at the goal, or at every free goal of a goal set (the IK solutions of a pose)
//   ik_shortcut.hip    path shortcutting over all-pairs visibility, equal-spacing resampling
//   ik_time.hip        timing of joint paths under velocity and acceleration limits, trajectory sampling
//   ik_occupancy.hip   occupancy grids and point clouds into distance-field worlds (distance transform, voxelize)
//   ik_mesh.hip        triangle meshes into distance-field worlds (exact distance, generalized winding number)
//   ik_batch_ops.hip   objective / gradient, FK / Jacobian and seed batches, the test probes
//   ik_lane_kernel.hip, ik_quad_kernel.hip, ik_wide_kernel.hip    the restart solvers (one restart loop each)
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <string>

#include "../../include/optik_hip.h"
#include "device_buf.hpp"
#include "device_scope.hpp"
#include "ik_grid.hpp"
#include "ik_host_params.hpp"
#include "ik_launch.hpp"
#include "ik_launch_plan.hpp"
#include "ik_wide_launch.hpp"

namespace optik {
namespace coll {
struct ModelDev;  // collision_model.hpp
}  // namespace coll
namespace host {

static_assert(PLAN_EARLY_EXIT == OPTIK_HIP_IK_EARLY_EXIT && PLAN_FIND_ANY == OPTIK_HIP_IK_FIND_ANY
                  && PLAN_RESTART_MAJOR == OPTIK_HIP_IK_RESTART_MAJOR && PLAN_MODE_SPEED == OPTIK_MODE_SPEED,
              "ik_launch_plan.hpp reads the flags and modes of optik_hip.h");

// ---- selection (ik_select.hip) -----------------------------------------------------------------------------
struct TileRec {
    unsigned long long idx;  // winning restart index in the tile, ~0 if none
    double key;
};

struct SelectLaunch {
    const double *out_key;   // [T*R] selection key, +inf unless the restart succeeded
    const double *out_x;     // [n][T*R]
    const double *out_f;     // [T*R]
    TileRec *tile_recs;      // [T][tiles_per_target]
    int tiles_per_target;
    int tile;                // restarts per tile
    int n;
    int pad;
    unsigned long long restart_begin;
    unsigned long long n_restarts;
    size_t ld;               // T * R
    double *win_x;           // [T][n]
    double *win_f;
    unsigned long long *win_idx;
    double *win_key;
    // the launch's work-item counter and first-success words, put back to their initial values by the last
    // kernel of the launch so that the next launch needs no fill commands in front of it (null: leave them)
    unsigned long long *reset_queue;
    unsigned long long *reset_fs;  // [T]
};
static_assert(OPTIK_HIP_PATH_MAX_RESTARTS <= SEL_TILE, "ik_path selects each path's restarts in one block");
// per-tile argmin + per-target reduction (one kernel when a target has a single tile); T blocks publish the winners
hipError_t select_launch(const SelectLaunch &s, int T, hipStream_t stream);

// ---- the solution sets of optik_hip_ik_solutions (ik_solutions.hip) --------------------------------------------
struct SolutionsLaunch {
    double *out_key;         // [T*R] the launch's keys (chain scratch): a candidate that is eliminated goes to +inf
    const double *out_x;     // [n][ld]
    const double *out_f;     // [ld] (null when no f is wanted)
    TileRec *tile_recs;      // [T][tiles_per_target]
    unsigned long long *pick;  // [T] column of the solution the last round accepted, ~0 if none (multi-tile form)
    int tiles_per_target;
    int tile;                // restarts per tile (SEL_TILE)
    int n;
    int K;
    double min_dist;
    unsigned long long restart_begin;
    unsigned long long n_restarts;
    size_t ld;               // T * R
    int32_t *count;          // [T]
    double *x;               // [T][K][n]
    double *f;               // [T][K]
    unsigned long long *idx;  // [T][K]
    double *key;             // [T][K]
    unsigned long long *reset_queue;  // the launch's work-item counter, put back to 0 by the last kernel
};
// K rounds of (argmin of the surviving candidates, elimination of those within min_dist of it): one kernel when a
// target has a single tile, otherwise a tile kernel and a per-target kernel per round
hipError_t solutions_launch(const SolutionsLaunch &s, int T, hipStream_t stream);

// ---- one waypoint of the paths of optik_hip_ik_path (ik_path.hip) ----------------------------------------------
struct PathSelectLaunch {
    const double *out_key;   // [P*R] the waypoint launch's keys, +inf unless the restart succeeded
    const double *out_x;     // [n][ld]
    const double *out_f;     // [ld] (null when no f is wanted)
    const double *seed;      // [P][n] the seeds the waypoint was solved from
    double *carry;           // [P][n] the next waypoint's seeds (may be `seed` itself)
    double *last;            // [P][n] a copy of `carry` (the last waypoint only; may be null)
    int n;
    int filter;              // max_step < +inf: candidates must lie within max_step of the seed
    double max_step;
    unsigned long long restart_begin;
    unsigned long long n_restarts;  // <= SEL_TILE
    size_t ld;               // P * R
    double *x;               // [P][n] this waypoint's outputs; any may be null
    double *f;               // [P]
    unsigned long long *idx;  // [P]
    double *key;             // [P]
    double *step;            // [P]
    unsigned long long *reset_queue;  // the launch's work-item counter, put back to 0
    unsigned long long *reset_fs;     // [P] the first-success words, put back to ~0 (null: launch without early exit)
};
// one 256-thread block per path: the filtered (key, index) argmin, the waypoint's outputs and the next seed
hipError_t path_select_launch(const PathSelectLaunch &s, int P, hipStream_t stream);

// ---- the keys of solution modes 3 and 4 (ik_manip.hip) -------------------------------------------------------
// Overwrites every key < +inf of a solver launch (x [n][cols], key [cols]) with -w (OPTIK_MODE_MANIPULABILITY) or -c
// (OPTIK_MODE_CONDITION) of that restart's x; one kernel on `stream`.  0 or a fail() code.
int manip_key_launch(const optik_hip_chain *ch, int mode, const double *ee_offset7, const double *x, double *key,
                     size_t cols, hipStream_t stream);

// ---- the collision filter (ik_collision.hip) ---------------------------------------------------------------
// Sets to +inf every key < +inf of a solver launch (x [n][cols], key [cols]) whose x is not free against the chain's
// model and world; one kernel on `stream`, after the key pass of modes 3 and 4.  Only while ch->coll_S > 0.
int collision_key_launch(const optik_hip_chain *ch, const double *ee_offset7, const double *x, double *key,
                         size_t cols, hipStream_t stream);

// ---- the motion check (ik_motion.hip) ------------------------------------------------------------------------
// The workspace of a motion launch over `segments` segments, grown on demand (under ch->mu, before the solver launch).
int motion_reserve(optik_hip_chain *ch, long long segments);
// One waypoint of optik_hip_ik_path, behind the collision key pass and before the selection: every success (key < +inf)
// of path p's R restarts (x [n][P * R]) within max_step of the path's seed (seed [P][n], read on the device) whose
// motion seed -> x is not free at the chain's resolution gets key +inf.  Only while ch->motion_h > 0 and ch->coll_S > 0.
int motion_key_launch(const optik_hip_chain *ch, const double *ee_offset7, const double *seed, const double *x,
                      double *key, int P, size_t R, int filter, double max_step, hipStream_t stream);

// ---- pose constraints (ik_constraint.hip) ----------------------------------------------------------------------
// The mask form of the check along a motion, for a caller that has validated its arguments: of the B segments qa -> qb
// ([n][B] each) every one whose flag is not 0 already is sampled at `resolution` against the box (ref7, lo6, hi6), and
// its flag becomes whether every sample's violation is <= tol; one kernel on `stream`.  0 or a fail() code.
int constraint_mask_launch(const optik_hip_chain *ch, const double *ee_offset7, const double *ref7, const double *lo6,
                           const double *hi6, const double *qa, const double *qb, long long B, double resolution,
                           double tol, uint8_t *flag, hipStream_t stream);

// ---- options ---------------------------------------------------------------------------------------------
// Every tuning option of the kernel layer, in one place.  The defaults come from the environment ONCE, at the
// first use (the OPTIK_* names below); tests and tools change them through optik_hip_set_option (optik_hip.h).
// Nothing else in this library reads the environment (robot_host.hpp: OPTIK_HOST_THREADS, robot_host.cpp: OPTIK_DEVICES).
struct Options {
    int solve_kernel = SK_AUTO;      // OPTIK_SOLVE_KERNEL = quad | lane64 | general: which single-launch solver (auto: by size)
    int wide_form = WF_LDS;              // OPTIK_WIDE_FORM = lds | hbm: the general solver's form (9 .. 16 joints); 2: one-lane LDS form
    int range_rule = OPTIK_HIP_RANGE_SINGLE_INCLUSIVE;  // OPTIK_RANDOM_RANGE_RULE = new_inclusive: rand 0.9.2 reading of new chains
    int stop_x_legacy = 0;           // (no environment name) nlopt_stop_x of NLopt 2.5: no zero-step rule
    int grid_cap = 0;                // (no environment name) >= 1: at most this many blocks per grid-stride launch (tests); 0: the device's cap
};
Options &opt();  // (ik_capi.hip)

// ---- errors ----------------------------------------------------------------------------------------------
extern thread_local std::string g_err;  // optik_hip_last_error() of the calling thread (ik_capi.hip)
inline int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return ::optik::host::fail(OPTIK_HIP_ENODEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

inline int ensure_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(OPTIK_HIP_ENODEVICE, std::string("no HIP device available: ")
                                             + (e == hipSuccess ? "device count is 0" : hipGetErrorString(e)));
    return 0;
}

// A chain lives on the device that was current when it was created; its entry points make that
// device current for the calling thread for the duration of the call and restore the caller's
// device on every exit path (device_scope.hpp) -- a host that also drives torch / RCCL on the
// thread finds its own device current again.
#define BIND_DEVICE(CH)                                                                 \
    optik::DeviceScope dev_scope_((CH)->device_id);                                     \
    if (!dev_scope_.ok()) return ::optik::host::fail(OPTIK_HIP_ENODEVICE, "hipSetDevice(" + std::to_string((CH)->device_id) + ") failed")

// Dispatch on (n, trailing fixed joint): kernels are instantiated for 1 <= n <= 8 revolute joints, each with and
// without a trailing fixed joint.
#define OPTIK_N_RANGE_MSG "this kernel is built for 1 <= n <= 8 revolute joints"
#define OPTIK_DISPATCH_ONE(NN, CALL)                                                   \
    if (!done_ && n_ == NN) {                                                          \
        if (tip_) { CALL(NN, true); } else { CALL(NN, false); }                        \
        done_ = true;                                                                  \
    }
#define OPTIK_DISPATCH(CH, CALL)                                                       \
    do {                                                                               \
        const int n_ = (CH)->n;                                                        \
        const bool tip_ = (CH)->tip;                                                   \
        bool done_ = false;                                                            \
        OPTIK_DISPATCH_ONE(1, CALL)                                                     \
        OPTIK_DISPATCH_ONE(2, CALL) OPTIK_DISPATCH_ONE(3, CALL) OPTIK_DISPATCH_ONE(4, CALL) \
        OPTIK_DISPATCH_ONE(5, CALL) OPTIK_DISPATCH_ONE(6, CALL) OPTIK_DISPATCH_ONE(7, CALL) \
        OPTIK_DISPATCH_ONE(8, CALL)                                                     \
        if (!done_) return ::optik::host::fail(OPTIK_HIP_EUNSUPPORTED, OPTIK_N_RANGE_MSG); \
    } while (0)

}  // namespace host
}  // namespace optik

// ---- the chain handle ---------------------------------------------------------------------------------------
struct optik_hip_chain {
    optik::ChainDev host;
    optik::ChainDev *dev = nullptr;
    int n = 0;
    bool tip = false;
    uint32_t key[8];
    double scale[optik::WIDE_MAX_DOF];
    int range_rule = 0;  // OPTIK_HIP_RANGE_*: how `scale` was formed
    // a chain with 9 .. 16 joint positions (ik_wide.hpp): its own table, the general kernels
    bool wide = false;
    optik::WideChainDev whost;
    optik::WideChainDev *wdev = nullptr;
    optik::DeviceBuf<double> wide_ws;  // restart workspace of the resident waves (wide_ws_doubles_per_wave() each)
    int device_id = 0;   // the HIP device the chain lives on (the current device at creation)
    // a chain with prismatic joints: FK only (as in the reference); the joint table for fk_general_kernel
    bool prismatic = false;
    int n_joints = 0;
    int32_t types[optik::MAX_JOINTS] = {};
    double axis_all[optik::MAX_JOINTS][3] = {};
    // launch workspace (grown on demand; one in-flight ik call per chain handle)
    std::mutex mu;
    std::mutex host_mu;  // serialises optik_hip_ik_host calls (they share the staging blocks below)
    // (the grow-only buffers below free themselves when the chain is deleted: optik_hip_chain_destroy binds the device)
    optik::DeviceBuf<optik::host::TileRec> tile_recs;
    optik::DeviceBuf<unsigned long long> first_success;
    optik::DeviceBuf<unsigned long long> sol_pick;  // optik_hip_ik_solutions: per target, the last accepted column
    optik::DeviceBuf<double> path_carry;            // optik_hip_ik_path: [P][n] the seeds of the next waypoint
    // the collision filter (ik_collision.hip): active while coll_S > 0; the model as the kernels stage it, the world
    // as spheres [world_Ms][4] then boxes [world_Mb][10]
    int coll_S = 0, coll_P = 0, coll_groups = 0;
    double coll_margin = 0.0;
    optik::coll::ModelDev *coll_dev = nullptr;
    // [coll_S + coll_P]: the caller's sphere / pair index of each slot of coll_dev (ik_avoid.hip)
    optik::DeviceBuf<uint16_t> coll_orig;
    optik::DeviceBuf<double> world_dev;
    int world_Ms = 0, world_Mb = 0;
    // the distance-field world (optik_hip_chain_set_world_grid): float32 [nx][ny][nz]; null: no grid
    optik::DeviceBuf<float> grid_dev;
    int grid_n[3] = {0, 0, 0};
    double grid_origin[3] = {0.0, 0.0, 0.0};
    double grid_inv = 0.0;
    // the motion check (ik_motion.hip): the resolution of ik_path's motion key pass (0: off) and the workspace of a
    // motion launch (prefix of the sample counts, the segments' reduction words)
    double motion_h = 0.0;
    optik::DeviceBuf<unsigned char> motion_ws;  // bytes
    // optik_hip_roadmap_edges (ik_roadmap.hip): the gathered segments [n][B] twice and their free flags [B]
    optik::DeviceBuf<unsigned char> roadmap_ws;  // bytes
    // optik_hip_roadmap_lazy_plan (ik_roadmap_lazy.hip): the round's counter, the routes' nodes and hop slots
    // [Lmax][Q] twice, the claimed slots, their segments [n][B] twice and free flags; _lazy_reset: the nodes' free flags
    optik::DeviceBuf<unsigned char> roadmap_lazy_ws;  // bytes
    // optik_hip_rrt_plan (ik_rrt.hip): the samples, one chunk's ends, segments, flags, per-query state and trees
    optik::DeviceBuf<unsigned char> rrt_ws;  // bytes
    // optik_hip_path_shortcut (ik_shortcut.hip): one chunk's vertex pairs as segments [n][B] twice, their free flags [B]
    optik::DeviceBuf<unsigned char> shortcut_ws;  // bytes
    // (what the last launch's selection kernel left behind: the work-item counter at 0, this many leading
    // first-success words at ~0 -- a launch that finds them so skips its fill commands)
    // (host-side knowledge that holds for launches ORDERED behind that selection kernel: the stream it ran on is kept
    // with it, a launch on any other stream fills the words itself)
    bool queue_clean = false;
    size_t fs_clean = 0;
    hipStream_t clean_stream = nullptr;
    // scratch per-restart buffers when the caller does not provide them
    // (tmp_key's capacity is the columns; tmp_x and tmp_f follow it, allocated only when a launch needs them)
    optik::DeviceBuf<double> tmp_x, tmp_f, tmp_key;
    unsigned long long *queue = nullptr;  // work-item counter of the in-flight launch
    unsigned long long *prof = nullptr;   // phase timers (OPTIK_PROFILE builds)
    optik::DeviceBuf<double> hw_dev;  // optik_hip_ik_host: the device block ...
    optik::PinnedBuf<double> hw_pin;  // ... and its pinned staging, two blocks of the device block's size
    // optik_hip_ik_host, one target under the first-success rule: the block the first successful restart writes its
    // answer to (WorkQueue::claim; pinned, host-coherent) and the sequence number of the last launch that used it
    unsigned long long *hw_claim = nullptr;
    hipEvent_t claim_done = nullptr;  // recorded behind such a launch: what the polling host also looks at
    unsigned long long claim_seq = 0;
    // such a launch may still be running on the null stream (set, under `mu`, in the critical section that queues it;
    // cleared by whoever has waited for the null stream)
    bool claim_pending = false;
    unsigned hw_flip = 0;  // which half of the pinned block the next zero-copy call uses
    // timing
    int timing = 0;
    static constexpr int EV_POOL = 256;  // event pairs recorded round-robin around the solve kernel
    hipEvent_t ev0[EV_POOL] = {}, ev1[EV_POOL] = {};
    int ev_count = 0;                    // launches recorded since the last reset
    optik_hip_launch_info last{};
    int num_cus = 0;
    int wall_clock_khz = 0;
    // the distance transform (ik_occupancy.hip): the two ping-pong buffers of optik_hip_world_grid_from_occupancy, 16
    // bytes per node (256 MiB at 2^24 nodes); grown on demand
    optik::DeviceBuf<unsigned char> edt_ws;  // bytes
    // the evidence map (ik_depth.hip): the cleaned images of one launch of optik_hip_depth_integrate, 4 bytes per
    // pixel of up to 8 frames; grown on demand
    optik::DeviceBuf<float> depth_ws;
};

namespace optik {
namespace host {

// The grid of a grid-stride launch over `work` items: per_cu blocks per CU fill the device (ik_grid.hpp).
inline int grid_for(const optik_hip_chain *ch, long long work, int block, int per_cu) {
    const long long cap = (long long)(ch->num_cus > 0 ? ch->num_cus : 256) * per_cu;
    return stride_grid(work > 0 ? (unsigned long long)work : 0ull, block, cap, opt().grid_cap);
}

// The per-restart arrays a selection stage reads: key [cols], x [n][cols], f [cols] with cols = T * R, column
// t * R + (i - restart_begin).  A solver launch's, a caller's own (the optik_hip_*_from_keys hooks) or those of
// optik_hip_ik_region (ik_region.hip).
struct SelectionIn {
    double *key;
    const double *x, *f;
    uint64_t restart_begin, R;
    uint64_t tiles_per_target;  // of plan_selection_tiles
    size_t cols;
};
// The launch struct of the solution-set selection, filled in one place (ik_capi.hip): optik_hip_ik_solutions, its test
// hook and optik_hip_ik_region launch what it returns.  reset_queue: the work-item counter the last kernel puts back
// (null: none).
SolutionsLaunch make_solutions_launch(optik_hip_chain *ch, const SelectionIn &in, int32_t K, double min_dist,
                                      const optik_hip_ik_solutions_outputs *out, unsigned long long *reset_queue);

}  // namespace host
}  // namespace optik
