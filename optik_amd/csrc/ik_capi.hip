// ik_capi.hip -- the C ABI of include/optik_hip.h: chains, tuning options, the restart launch (optik_hip_ik_batch),
// its host-buffer form (optik_hip_ik_host), the solution sets (optik_hip_ik_solutions), warm-started paths
// (optik_hip_ik_path), timing.
//
// The solvers are launched from here and defined in their own translation units: the lane-per-restart form
// (ik_lane_kernel.hip), the quad solver (ik_quad_kernel.hip), the general run-time-n solver (ik_wide_kernel.hip);
// which one a launch gets, and its grid, is plan_launch's decision (ik_launch_plan.hpp).  The key pass of solution modes 3 and 4: ik_manip.hip;
// that of the collision filter: ik_collision.hip.
// The selection kernels: ik_select.hip,
// ik_solutions.hip and ik_path.hip; the batch operators: ik_batch_ops.hip.  No CPU fallback exists: every entry point fails loudly without a device.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ik_host.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::hostparams;

namespace optik {
namespace host {

thread_local std::string g_err;

static int solve_kernel_from(const char *e) {
    if (!e) return SK_AUTO;
    if (!std::strcmp(e, "quad")) return SK_QUAD;
    if (!std::strcmp(e, "lane64")) return SK_LANE64;
    if (!std::strcmp(e, "general")) return SK_GENERAL;
    return SK_AUTO;
}
Options &opt() {
    static Options o = [] {
        Options v;
        v.solve_kernel = solve_kernel_from(std::getenv("OPTIK_SOLVE_KERNEL"));
        if (const char *e = std::getenv("OPTIK_WIDE_FORM")) v.wide_form = std::strcmp(e, "hbm") == 0 ? 1 : 0;
        if (const char *e = std::getenv("OPTIK_RANDOM_RANGE_RULE"))
            if (std::strcmp(e, "new_inclusive") == 0 || std::strcmp(e, "1") == 0) v.range_rule = OPTIK_HIP_RANGE_NEW_INCLUSIVE;
        return v;
    }();
    return o;
}

}  // namespace host
}  // namespace optik

namespace {

int default_range_rule() { return opt().range_rule; }

// ch->scale under `rule` (a wide chain's table holds a copy: fill_wide_chain)
void set_chain_scales(optik_hip_chain *ch, const double *lb, const double *ub, int rule) {
    ch->range_rule = rule;
    // infinite limits (continuous joints) make random_range panic in the
    // reference (quirk Q5); restarts > 0 are refused at launch time instead.
    for (int k = 0; k < ch->n; ++k)
        ch->scale[k] = (std::isfinite(lb[k]) && std::isfinite(ub[k])) ? uniform_scale(lb[k], ub[k], rule) : NAN;
}

// The chain table of either layout (ChainDev: n <= 8, the tuned solvers; WideChainDev: the general kernels) from
// origins [n + tip][7], axes [n][3] and the limits [n].
template <class Table>
void fill_chain_table(Table &t, const double *origins, const double *axes, const double *lb, const double *ub, int n,
                      bool tip) {
    std::memset(&t, 0, sizeof t);
    t.n_pos = n;
    t.has_tip = tip;
    std::memcpy(t.origin, origins, sizeof(double) * 7 * (size_t)(n + (tip ? 1 : 0)));
    std::memcpy(t.axis, axes, sizeof(double) * 3 * (size_t)n);
    std::memcpy(t.lb, lb, sizeof(double) * (size_t)n);
    std::memcpy(t.ub, ub, sizeof(double) * (size_t)n);
}
// the general kernels' table: the restart scales are part of it
void fill_wide_chain(WideChainDev &w, const double *origins, const double *axes, const double *lb, const double *ub,
                     int n, bool tip, const double *scales) {
    fill_chain_table(w, origins, axes, lb, ub, n, tip);
    std::memcpy(w.scale, scales, sizeof(double) * (size_t)n);
}
// a table to its device block, allocated at the first upload
template <class Table>
hipError_t upload_table(Table **dev, const Table &host) {
    hipError_t e = *dev ? hipSuccess : hipMalloc(dev, sizeof(Table));
    return e == hipSuccess ? hipMemcpy(*dev, &host, sizeof(Table), hipMemcpyHostToDevice) : e;
}

}  // namespace

extern "C" {

int optik_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *optik_hip_last_error(void) { return g_err.c_str(); }

int optik_hip_chain_create(const double *origins, const double *axes, const int32_t *types,
                           int32_t n_joints, const double *lb, const double *ub, int32_t n,
                           optik_hip_chain **out) {
    if (!origins || !axes || !types || !lb || !ub || !out) return fail(OPTIK_HIP_EINVAL, "null argument");
    if (n < 1 || n > WIDE_MAX_DOF) return fail(OPTIK_HIP_EUNSUPPORTED, "num_positions must be in 1..16");
    if (n_joints != n && n_joints != n + 1)
        return fail(OPTIK_HIP_EUNSUPPORTED, "chain must be n revolute joints plus an optional trailing fixed joint");
    bool prismatic = false;
    for (int j = 0; j < n; ++j) {
        if (types[j] == OPTIK_JOINT_PRISMATIC) prismatic = true;
        else if (types[j] != OPTIK_JOINT_REVOLUTE)
            return fail(OPTIK_HIP_EUNSUPPORTED, "the first n joints of the chain must be revolute or prismatic");
    }
    if (n_joints == n + 1 && types[n] != OPTIK_JOINT_FIXED)
        return fail(OPTIK_HIP_EUNSUPPORTED, "joint after the last revolute joint must be fixed");
    if (prismatic && n > MAX_DOF)
        return fail(OPTIK_HIP_EUNSUPPORTED, "prismatic joints are supported for chains of at most 8 joint positions");
    if (int rc = ensure_device()) return rc;

    auto *ch = new optik_hip_chain();
    std::memset(&ch->host, 0, sizeof ch->host);
    std::memset(&ch->whost, 0, sizeof ch->whost);
    ch->n = n;
    ch->n_joints = n_joints;
    ch->tip = (n_joints == n + 1);
    set_chain_scales(ch, lb, ub, default_range_rule());
    seed_from_u64(42, ch->key);  // RNG_SEED, lib.rs:360
    hipError_t e;
    if (n > MAX_DOF) {
        // 9 .. 16 joint positions: the general kernels of ik_wide.hpp (one table, joint count at run time)
        ch->wide = true;
        fill_wide_chain(ch->whost, origins, axes, lb, ub, n, ch->tip, ch->scale);
        e = upload_table(&ch->wdev, ch->whost);
    } else {
        ch->prismatic = prismatic;
        for (int j = 0; j < n_joints; ++j) {
            ch->types[j] = types[j];
            for (int k = 0; k < 3; ++k) ch->axis_all[j][k] = axes[j * 3 + k];
        }
        fill_chain_table(ch->host, origins, axes, lb, ub, n, ch->tip);
        e = upload_table(&ch->dev, ch->host);
    }
    if (e != hipSuccess) {
        if (ch->dev) (void)hipFree(ch->dev);
        if (ch->wdev) (void)hipFree(ch->wdev);
        delete ch;
        return fail(OPTIK_HIP_ENODEVICE, std::string("chain upload: ") + hipGetErrorString(e));
    }
    int dev = 0;
    hipGetDevice(&dev);
    ch->device_id = dev;
    hipDeviceGetAttribute(&ch->num_cus, hipDeviceAttributeMultiprocessorCount, dev);
    hipDeviceGetAttribute(&ch->wall_clock_khz, hipDeviceAttributeWallClockRate, dev);
    *out = ch;
    return 0;
}

void optik_hip_chain_destroy(optik_hip_chain *ch) {
    if (!ch) return;
    optik::DeviceScope dev_scope(ch->device_id);  // (the frees run on the chain's device)
    if (ch->claim_pending) (void)hipStreamSynchronize(nullptr);
    if (ch->dev) hipFree(ch->dev);
    if (ch->wdev) hipFree(ch->wdev);
    if (ch->coll_dev) hipFree(ch->coll_dev);
    if (ch->queue) hipFree(ch->queue);
    if (ch->hw_claim) hipHostFree(ch->hw_claim);
    if (ch->claim_done) hipEventDestroy(ch->claim_done);
    for (int i = 0; i < optik_hip_chain::EV_POOL; ++i) {
        if (ch->ev0[i]) hipEventDestroy(ch->ev0[i]);
        if (ch->ev1[i]) hipEventDestroy(ch->ev1[i]);
    }
    delete ch;  // (the grow-only buffers free themselves, under dev_scope)
}

int32_t optik_hip_chain_num_positions(const optik_hip_chain *ch) { return ch ? ch->n : 0; }

int optik_hip_chain_set_range_rule(optik_hip_chain *ch, int32_t rule) {
    if (!ch || (rule != OPTIK_HIP_RANGE_SINGLE_INCLUSIVE && rule != OPTIK_HIP_RANGE_NEW_INCLUSIVE))
        return fail(OPTIK_HIP_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(ch->mu);
    set_chain_scales(ch, ch->wide ? ch->whost.lb : ch->host.lb, ch->wide ? ch->whost.ub : ch->host.ub, rule);
    if (ch->wide) {  // (the scales of a wide chain are part of its device table)
        BIND_DEVICE(ch);
        std::memcpy(ch->whost.scale, ch->scale, sizeof(double) * (size_t)ch->n);
        HIP_TRY(upload_table(&ch->wdev, ch->whost));
    }
    return 0;
}

int32_t optik_hip_chain_range_rule(const optik_hip_chain *ch) { return ch ? ch->range_rule : -1; }

}  // extern "C"

// What the solver half of a launch (solve_locked) leaves for the selection stage behind it.
struct SolvedLaunch {
    double *px, *pf, *pk;     // per-restart x [n][cols], f [cols], key [cols] (the caller's buffers or chain scratch)
    uint64_t R;
    uint64_t tiles_per_target;  // selection tiles of SEL_TILE restarts
    size_t cols;              // T * R
    size_t fs_clean_after;    // ch->fs_clean once the launch's last kernel has put the first-success words back
    bool early;               // the launch used the first-success words
};

// The launch's selection kernel has put the work-item counter and the first-success words back: what a launch queued
// behind it on `stream` may rely on.
static void words_put_back(optik_hip_chain *ch, const SolvedLaunch &sl, hipStream_t stream) {
    ch->queue_clean = true;
    ch->fs_clean = sl.fs_clean_after;
    ch->clean_stream = stream;
}

// The solver half of optik_hip_ik_batch and optik_hip_ik_solutions, with the chain's launch mutex held: argument
// checks, workspace, the solver choice and its launch.  want_sel: a selection stage follows (the per-restart keys go
// to scratch; need_x / need_f: it reads x / f, scratch for what the caller does not provide).  The selection stage
// has to put the work-item counter (and, with sl->early, the first-success words) back and then say so: words_put_back.
static int solve_locked(optik_hip_chain *ch, const optik_solver_config *cfg, const double *d_targets,
                        const double *d_x0, int32_t T, const double *ee_offset7, uint64_t restart_begin,
                        uint64_t restart_end, uint32_t flags, double deadline_s, const optik_hip_ik_outputs *out,
                        bool want_sel, bool need_x, bool need_f, hipStream_t stream, bool claim_request,
                        bool *claim_armed, SolvedLaunch *sl) {
    if (!ch || !cfg || !d_targets || !d_x0 || !out || T < 1) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (restart_end <= restart_begin) return fail(OPTIK_HIP_EINVAL, "empty restart range");
    const int mode = cfg->solution_mode;
    if (mode < OPTIK_MODE_QUALITY || mode > OPTIK_MODE_CONDITION)
        return fail(OPTIK_HIP_EINVAL,
                    "solution_mode must be 1 (Quality), 2 (Speed), 3 (Manipulability) or 4 (Condition)");
    // Manipulability and Condition: scheduled as Quality, then a key pass over the successes (ik_manip.hip)
    const bool manip = mode == OPTIK_MODE_MANIPULABILITY || mode == OPTIK_MODE_CONDITION;
    // the collision filter: Speed is scheduled as Quality (no early exit, no claim; Speed's keys), and a key pass
    // after the solver rejects the successes that are not free (ik_collision.hip)
    const bool coll = ch && ch->coll_S > 0;
    const uint64_t R = restart_end - restart_begin;
    if (restart_end > 1 || restart_begin > 0)
        for (int k = 0; k < ch->n; ++k)
            if (std::isnan(ch->scale[k]))
                return fail(OPTIK_HIP_EINVAL, "random restarts need finite joint limits (reference: random_range panics)");
    if (ch->prismatic)
        return fail(OPTIK_HIP_EUNSUPPORTED,
                    "prismatic joints: only forward kinematics is available (the reference's Jacobian panics, kinematics.rs:185)");

    // the plan: which solver, how many restarts per wave and in flight, the grid (ik_launch_plan.hpp)
    PlanIn in{};
    in.n = ch->n; in.wide = ch->wide; in.cus = ch->num_cus;
    in.T = T; in.R = R; in.flags = flags; in.mode = mode; in.coll = coll;
    in.solve_kernel = opt().solve_kernel; in.wide_form = opt().wide_form;
    in.claim_request = claim_request; in.have_claim_block = ch->hw_claim != nullptr;
    in.lane_waves = lane_solve_waves_per_cu(); in.quad_waves = quad_solve_waves_per_cu(ch->n);
    in.latency_waves = 4; in.wide_waves = 8;  // one wave per SIMD; two
    const LaunchPlan plan = plan_launch(in);
    if (plan.error == PLAN_TOO_MANY_TILES)
        return fail(OPTIK_HIP_EINVAL, "too many restarts / targets in one launch (2^24 or more selection tiles)");
    const bool early = plan.early, wide_lds = plan.solver == WIDE_LDS, widek = wide_lds || plan.solver == WIDE_HBM;
    const size_t cols = (size_t)plan.cols;

    // the workspace
    BIND_DEVICE(ch);
    // (a single call that returned on its first success may have left its launch running on the null stream: a
    // launch on another stream shares the chain's workspace with it and waits; on the null stream it queues behind)
    // (on the null stream the flag stays: optik_hip_ik_host's staged path still has to know)
    if (ch->claim_pending && stream != nullptr) { HIP_TRY(hipStreamSynchronize(nullptr)); ch->claim_pending = false; }
    HIP_TRY(ch->tile_recs.reserve((size_t)plan.n_tiles));
    if (!ch->queue) { HIP_TRY(hipMalloc(&ch->queue, sizeof(unsigned long long))); ch->queue_clean = false; }
    // (the words are only known to be clean to a launch queued behind the selection kernel that cleaned them)
    if (stream != ch->clean_stream) { ch->queue_clean = false; ch->fs_clean = 0; }
    if (!ch->queue_clean) HIP_TRY(hipMemsetAsync(ch->queue, 0, sizeof(unsigned long long), stream));
    ch->queue_clean = false;  // (until this launch's selection kernel has put it back)
    size_t fs_clean_after = ch->fs_clean;  // (a launch without early exit leaves the words alone)
    if (early) {
        if ((size_t)T > ch->first_success.capacity()) ch->fs_clean = 0;  // (a new block: no word of it is clean)
        HIP_TRY(ch->first_success.reserve((size_t)T));
        if (ch->fs_clean < (size_t)T)
            HIP_TRY(hipMemsetAsync(ch->first_success.get(), 0xff, sizeof(unsigned long long) * (size_t)T, stream));
        fs_clean_after = std::max(ch->fs_clean, (size_t)T);  // once the selection kernel has put words [0, T) back
        ch->fs_clean = 0;
    }
    // the selection needs the per-restart x / f / key: scratch if the caller skips them (the key passes of modes 3
    // and 4 and of the collision filter read x: grown here, before the launch -- nothing is allocated between the
    // solve and the selection)
    double *px = out->d_x, *pf = out->d_f, *pk = nullptr;
    need_x = need_x || (want_sel && (manip || coll));
    if (want_sel) {
        const bool need_xf = (!px || !pf) && (need_x || need_f);
        if (cols > ch->tmp_key.capacity()) {  // (x and f go with the old key block; they come back below if wanted)
            HIP_TRY(ch->tmp_x.reset());
            HIP_TRY(ch->tmp_f.reset());
            HIP_TRY(ch->tmp_key.reserve(cols));
        }
        if (need_xf) {
            HIP_TRY(ch->tmp_x.reserve(ch->tmp_key.capacity() * (size_t)ch->n));
            HIP_TRY(ch->tmp_f.reserve(ch->tmp_key.capacity()));
        }
        pk = ch->tmp_key.get();
        if (!px && need_x) px = ch->tmp_x.get();
        if (!pf && need_f) pf = ch->tmp_f.get();
    }

    if (widek && !ch->wide) {
        // the chain's table in the general kernels' layout (uploaded per call: a test path)
        fill_wide_chain(ch->whost, &ch->host.origin[0][0], &ch->host.axis[0][0], ch->host.lb, ch->host.ub, ch->n, ch->tip,
                        ch->scale);
        HIP_TRY(upload_table(&ch->wdev, ch->whost));
    }
    // (the general solver's HBM form: every resident wave with its own block of the restart workspace, ik_wide.hpp)
    if (plan.solver == WIDE_HBM) HIP_TRY(ch->wide_ws.reserve(wide_ws_doubles_per_wave() * (size_t)plan.grid));

    // the launch
    SolveLaunch a;
    std::memset(&a, 0, sizeof a);
    a.chain = ch->dev;  // (null for a wide chain: its launch takes ch->wdev)
    make_eval_params(cfg->linear_weight, cfg->angular_weight, ee_offset7, a.ep);
    fill_solve_params(cfg, a.sp, opt().stop_x_legacy != 0);
    std::memcpy(a.key, ch->key, sizeof a.key);
    std::memcpy(a.scale, ch->scale, sizeof a.scale);  // (n <= 8; a wide chain's scales are in its table)
    a.wq.next_item = ch->queue;
    a.wq.total_items = (unsigned long long)cols;
    a.wq.n_restarts = R;
    a.wq.restart_begin = restart_begin;
    a.wq.targets = d_targets;
    a.wq.x0 = d_x0;
    a.wq.first_success = early ? ch->first_success.get() : nullptr;
    a.wq.find_any = plan.find_any ? 1 : 0;
    a.wq.restart_major = plan.restart_major ? 1 : 0;
    a.wq.n_targets = (unsigned long long)T;
    a.wq.quality = plan.quality;
    a.wq.lanes = plan.lanes;
    a.wq.out_x = px;
    a.wq.out_f = pf;
    a.wq.out_key = pk;
    a.wq.out_status = out->d_status;
    a.wq.out_evals = out->d_evals;
#ifdef OPTIK_PROFILE
    if (!ch->prof) HIP_TRY(hipMalloc(&ch->prof, 8 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(ch->prof, 0, 8 * sizeof(unsigned long long), stream));
    a.wq.prof = ch->prof;
#endif
    if (deadline_s > 0.0) {
        const double khz = ch->wall_clock_khz > 0 ? (double)ch->wall_clock_khz : 100000.0;
        a.deadline_ticks = (unsigned long long)(deadline_s * khz * 1e3);
        if (a.deadline_ticks == 0) a.deadline_ticks = 1;
    }
    if (plan.arm_claim) {
        a.wq.claim = ch->hw_claim;
        a.wq.claim_seq = ++ch->claim_seq;
        if (claim_armed) *claim_armed = true;
        if (stream == nullptr) ch->claim_pending = true;  // (the caller may return before this launch has ended)
    }
    const int ev_slot = ch->ev_count % optik_hip_chain::EV_POOL;
    if (ch->timing) {
        if (!ch->ev0[ev_slot]) { HIP_TRY(hipEventCreate(&ch->ev0[ev_slot])); HIP_TRY(hipEventCreate(&ch->ev1[ev_slot])); }
        HIP_TRY(hipEventRecord(ch->ev0[ev_slot], stream));
    }
    int lds = 0;
    if (widek) {
        // the general kernel, eight waves per CU: one restart per wave with its arrays in the wave's LDS -- a single
        // ik() call's rounds --, or one per lane on the HBM workspace
        WideSolveLaunch w;
        std::memset(&w, 0, sizeof w);
        w.chain = ch->wdev;
        w.ep = a.ep; w.sp = a.sp; w.wq = a.wq;
        std::memcpy(w.key, ch->key, sizeof w.key);
        w.deadline_ticks = a.deadline_ticks;
        w.ws = ch->wide_ws.get();
        lds = wide_lds ? wide_lds_bytes() : (int)sizeof(WideChainDev);
        HIP_TRY(wide_solve_launch(plan.grid, stream, w, wide_lds, opt().wide_form != 2));
    } else if (plan.solver == LANE) {
        HIP_TRY(lane_solve_launch(ch->n, ch->tip, plan.grid, stream, a, &lds));
    } else {
        HIP_TRY(quad_solve_launch(ch->n, ch->tip, plan.grid, stream, a, &lds, plan.solver == QUAD_LATENCY));
    }
    HIP_TRY(hipGetLastError());
    if (ch->timing) { HIP_TRY(hipEventRecord(ch->ev1[ev_slot], stream)); ch->ev_count += 1; }
    // modes 3 and 4: the successes' keys become -w / -c, on the same stream, before any selection kernel
    if (manip && pk)
        if (int rc = manip_key_launch(ch, mode, ee_offset7, px, pk, cols, stream)) return rc;
    // the collision filter: the successes that are not free get key +inf, behind the key pass above
    if (coll && pk)
        if (int rc = collision_key_launch(ch, ee_offset7, px, pk, cols, stream)) return rc;
    ch->last.grid = plan.grid; ch->last.block = WAVE; ch->last.lds_bytes = lds; ch->last.tiles = plan.n_tiles;

    sl->px = px; sl->pf = pf; sl->pk = pk;
    sl->R = R;
    sl->tiles_per_target = plan.tiles_per_target;
    sl->cols = cols;
    sl->fs_clean_after = fs_clean_after;
    sl->early = early;
    return 0;
}

static SelectionIn selection_in(const SolvedLaunch &sl, uint64_t restart_begin) {
    return SelectionIn{sl.pk, sl.px, sl.pf, restart_begin, sl.R, sl.tiles_per_target, sl.cols};
}

// The launch structs of the three selection stages, filled in one place each: the product's entry points and the test
// hooks below both launch what these return.  reset_queue / reset_fs: the work-item counter and first-success words
// the stage's last kernel puts back (null: none).
static SelectLaunch make_select_launch(optik_hip_chain *ch, const SelectionIn &in, const optik_hip_ik_outputs *out,
                                       unsigned long long *reset_queue, unsigned long long *reset_fs) {
    SelectLaunch s;
    std::memset(&s, 0, sizeof s);
    s.out_key = in.key; s.out_x = in.x; s.out_f = in.f;
    s.tile_recs = ch->tile_recs.get();
    s.tiles_per_target = (int)in.tiles_per_target;
    s.tile = SEL_TILE;
    s.n = ch->n;
    s.restart_begin = in.restart_begin;
    s.n_restarts = in.R;
    s.ld = in.cols;
    s.win_x = out->d_win_x; s.win_f = out->d_win_f;
    s.win_idx = (unsigned long long *)out->d_win_idx; s.win_key = out->d_win_key;
    s.reset_queue = reset_queue;
    s.reset_fs = reset_fs;
    return s;
}

SolutionsLaunch optik::host::make_solutions_launch(optik_hip_chain *ch, const SelectionIn &in, int32_t K, double min_dist,
                                             const optik_hip_ik_solutions_outputs *out,
                                             unsigned long long *reset_queue) {
    SolutionsLaunch s;
    std::memset(&s, 0, sizeof s);
    s.out_key = in.key; s.out_x = in.x; s.out_f = in.f;
    s.tile_recs = ch->tile_recs.get();
    s.pick = ch->sol_pick.get();
    s.tiles_per_target = (int)in.tiles_per_target;
    s.tile = SEL_TILE;
    s.n = ch->n;
    s.K = K;
    s.min_dist = min_dist;
    s.restart_begin = in.restart_begin;
    s.n_restarts = in.R;
    s.ld = in.cols;
    s.count = out->d_count; s.x = out->d_x; s.f = out->d_f;
    s.idx = (unsigned long long *)out->d_idx; s.key = out->d_key;
    s.reset_queue = reset_queue;
    return s;
}

// One waypoint: `w` = its first slot in the [L][P] outputs, `last` = its seeds also go to out->d_last.
static PathSelectLaunch make_path_select_launch(optik_hip_chain *ch, const SelectionIn &in, const double *seed,
                                                double *carry, double max_step, const optik_hip_ik_path_outputs *out,
                                                size_t w, bool last, unsigned long long *reset_queue,
                                                unsigned long long *reset_fs) {
    const size_t n = (size_t)ch->n;
    PathSelectLaunch s;
    std::memset(&s, 0, sizeof s);
    s.out_key = in.key; s.out_x = in.x; s.out_f = in.f;
    s.seed = seed;
    s.carry = carry;
    s.last = last ? out->d_last : nullptr;
    s.n = ch->n;
    s.filter = max_step < __builtin_huge_val() ? 1 : 0;
    s.max_step = max_step;
    s.restart_begin = in.restart_begin;
    s.n_restarts = in.R;
    s.ld = in.cols;
    s.x = out->d_x ? out->d_x + w * n : nullptr;
    s.f = out->d_f ? out->d_f + w : nullptr;
    s.idx = out->d_idx ? (unsigned long long *)out->d_idx + w : nullptr;
    s.key = out->d_key ? out->d_key + w : nullptr;
    s.step = out->d_step ? out->d_step + w : nullptr;
    s.reset_queue = reset_queue;
    s.reset_fs = reset_fs;
    return s;
}

// The argument rules optik_hip_ik_solutions and optik_hip_ik_path add to optik_hip_ik_batch's (0 or a fail() code).
static int check_solutions_args(int32_t K, double min_dist) {
    if (K < 1 || K > OPTIK_HIP_MAX_SOLUTIONS) return fail(OPTIK_HIP_EINVAL, "K must be in 1..256");
    if (!(min_dist >= 0.0) || !std::isfinite(min_dist))
        return fail(OPTIK_HIP_EINVAL, "min_dist must be finite and >= 0");
    return 0;
}
static int check_path_args(uint64_t R, double max_step) {
    if (R > (uint64_t)OPTIK_HIP_PATH_MAX_RESTARTS)
        return fail(OPTIK_HIP_EINVAL, "ik_path: at most 4096 restarts per waypoint (one selection block per path)");
    if (!(max_step >= 0.0)) return fail(OPTIK_HIP_EINVAL, "ik_path: max_step must be >= 0 (+inf: no limit)");
    return 0;
}

// optik_hip_ik_batch with the chain's launch mutex already held.
static int ik_batch_locked(optik_hip_chain *ch, const optik_solver_config *cfg, const double *d_targets,
                           const double *d_x0, int32_t T, const double *ee_offset7, uint64_t restart_begin,
                           uint64_t restart_end, uint32_t flags, double deadline_s, const optik_hip_ik_outputs *out,
                           void *stream_v, bool claim_request = false, bool *claim_armed = nullptr) {
    if (claim_armed) *claim_armed = false;
    if (!out) return fail(OPTIK_HIP_EINVAL, "bad argument");
    hipStream_t stream = (hipStream_t)stream_v;
    const bool want_win = out->d_win_x || out->d_win_f || out->d_win_idx || out->d_win_key;
    SolvedLaunch sl;
    if (int rc = solve_locked(ch, cfg, d_targets, d_x0, T, ee_offset7, restart_begin, restart_end, flags, deadline_s,
                              out, want_win, out->d_win_x != nullptr, out->d_win_f != nullptr, stream, claim_request,
                              claim_armed, &sl))
        return rc;
    BIND_DEVICE(ch);
    if (want_win) {
        const SelectLaunch s = make_select_launch(ch, selection_in(sl, restart_begin), out, ch->queue,
                                                  sl.early ? ch->first_success.get() : nullptr);
        HIP_TRY(select_launch(s, T, stream));
        words_put_back(ch, sl, stream);
    }
    return 0;
}

extern "C" {

int optik_hip_ik_batch(optik_hip_chain *ch, const optik_solver_config *cfg, const double *d_targets,
                       const double *d_x0, int32_t T, const double *ee_offset7, uint64_t restart_begin,
                       uint64_t restart_end, uint32_t flags, double deadline_s, const optik_hip_ik_outputs *out,
                       void *stream_v) {
    if (!ch) return fail(OPTIK_HIP_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(ch->mu);
    return ik_batch_locked(ch, cfg, d_targets, d_x0, T, ee_offset7, restart_begin, restart_end, flags, deadline_s, out,
                           stream_v);
}

int optik_hip_ik_solutions(optik_hip_chain *ch, const optik_solver_config *cfg, const double *d_targets,
                           const double *d_x0, int32_t T, const double *ee_offset7, uint64_t restart_begin,
                           uint64_t restart_end, double deadline_s, int32_t K, double min_dist,
                           const optik_hip_ik_solutions_outputs *out, void *stream_v) {
    if (!ch || !out) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (int rc = check_solutions_args(K, min_dist)) return rc;
    std::lock_guard<std::mutex> lock(ch->mu);
    hipStream_t stream = (hipStream_t)stream_v;
    // every restart runs to its end: no flags (no early exit, so the first-success words stay as they are)
    optik_hip_ik_outputs none;
    std::memset(&none, 0, sizeof none);
    SolvedLaunch sl;
    if (int rc = solve_locked(ch, cfg, d_targets, d_x0, T, ee_offset7, restart_begin, restart_end, 0u, deadline_s,
                              &none, true, true, out->d_f != nullptr, stream, false, nullptr, &sl))
        return rc;
    BIND_DEVICE(ch);
    if (sl.tiles_per_target > 1) HIP_TRY(ch->sol_pick.reserve((size_t)T));  // (the multi-tile form's round-to-round acceptances)
    const SolutionsLaunch s = make_solutions_launch(ch, selection_in(sl, restart_begin), K, min_dist, out, ch->queue);
    HIP_TRY(solutions_launch(s, T, stream));
    words_put_back(ch, sl, stream);
    return 0;
}

int optik_hip_ik_path(optik_hip_chain *ch, const optik_solver_config *cfg, const double *d_targets,
                      const double *d_x0, int32_t P, int32_t L, const double *ee_offset7, uint64_t restart_begin,
                      uint64_t restart_end, uint32_t flags, double deadline_s, double max_step,
                      const optik_hip_ik_path_outputs *out, void *stream_v) {
    if (!ch || !cfg || !d_targets || !d_x0 || !out || P < 1 || L < 1) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (restart_end <= restart_begin) return fail(OPTIK_HIP_EINVAL, "empty restart range");
    if (int rc = check_path_args(restart_end - restart_begin, max_step)) return rc;
    if (flags & ~(uint32_t)OPTIK_HIP_IK_RESTART_MAJOR)
        return fail(OPTIK_HIP_EINVAL, "ik_path: flags may only hold OPTIK_HIP_IK_RESTART_MAJOR");
    std::lock_guard<std::mutex> lock(ch->mu);
    hipStream_t stream = (hipStream_t)stream_v;
    const int n = ch->n;
    const bool filter = max_step < __builtin_huge_val();
    // Speed without a step limit: the deterministic early exit, whose winner is the lowest successful index -- the
    // filter cannot reject it.  With a limit (and in Quality) every restart runs to its end: early exit could abandon
    // the one restart that passes the filter.
    const uint32_t solve_flags = flags | ((cfg->solution_mode == OPTIK_MODE_SPEED && !filter) ? OPTIK_HIP_IK_EARLY_EXIT : 0u);
    {
        BIND_DEVICE(ch);
        HIP_TRY(ch->path_carry.reserve((size_t)P * (size_t)n));
    }
    // the motion check between waypoints (ik_motion.hip): one more key pass per waypoint, in front of the selection
    const bool motion = ch->motion_h > 0.0 && ch->coll_S > 0;
    if (motion) {
        BIND_DEVICE(ch);
        if (int rc = motion_reserve(ch, (long long)P * (long long)(restart_end - restart_begin))) return rc;
    }
    optik_hip_ik_outputs none;
    std::memset(&none, 0, sizeof none);
    for (int32_t l = 0; l < L; ++l) {
        const double *seed = l == 0 ? d_x0 : ch->path_carry.get();
        SolvedLaunch sl;
        if (int rc = solve_locked(ch, cfg, d_targets + (size_t)l * (size_t)P * 7, seed, P, ee_offset7, restart_begin,
                                  restart_end, solve_flags, deadline_s, &none, true, true, out->d_f != nullptr, stream,
                                  false, nullptr, &sl))
            return rc;
        BIND_DEVICE(ch);
        if (motion)
            if (int rc = motion_key_launch(ch, ee_offset7, seed, sl.px, sl.pk, P, (size_t)sl.R, filter ? 1 : 0, max_step,
                                           stream))
                return rc;
        const PathSelectLaunch s =
            make_path_select_launch(ch, selection_in(sl, restart_begin), seed, ch->path_carry.get(), max_step, out,
                                    (size_t)l * (size_t)P, l + 1 == L, ch->queue,
                                    sl.early ? ch->first_success.get() : nullptr);
        HIP_TRY(path_select_launch(s, P, stream));
        words_put_back(ch, sl, stream);
    }
    return 0;
}

/* Test hooks: the three selection stages on the caller's own keys, x and f, with no solve in front (optik_hip.h).
 * Each fills its launch struct where the product does (make_*_launch) and plans its tiles with plan_selection_tiles;
 * the work-item counter, the first-success words and what the chain knows of them (queue_clean, fs_clean) stay as they
 * are. */
// The rules the three share, checked before the chain is touched; the plan's tiles_per_target, n_tiles and cols.
static int from_keys_plan(const optik_hip_chain *ch, const void *d_key, const void *out, int32_t T,
                          uint64_t restart_begin, uint64_t R, LaunchPlan *plan) {
    if (!d_key || !out || T < 1) return fail(OPTIK_HIP_EINVAL, "bad argument");
    // (the indices restart_begin .. restart_begin + R - 1 stay below ~0, "none")
    if (R < 1 || R > UINT64_MAX - restart_begin) return fail(OPTIK_HIP_EINVAL, "empty restart range");
    if (plan_selection_tiles(T, R, *plan) != PLAN_OK)
        return fail(OPTIK_HIP_EINVAL, "too many restarts / targets in one launch (2^24 or more selection tiles)");
    if (!ch) return fail(OPTIK_HIP_EINVAL, "bad argument");
    return 0;
}
// The selection workspace, as solve_locked reserves it (launch mutex held, device bound).
static int from_keys_workspace(optik_hip_chain *ch, const LaunchPlan &plan, hipStream_t stream) {
    if (ch->claim_pending && stream != nullptr) { HIP_TRY(hipStreamSynchronize(nullptr)); ch->claim_pending = false; }
    HIP_TRY(ch->tile_recs.reserve((size_t)plan.n_tiles));
    return 0;
}

int optik_hip_select_from_keys(optik_hip_chain *ch, const double *d_key, const double *d_x, const double *d_f,
                               int32_t T, uint64_t restart_begin, uint64_t R, const optik_hip_ik_outputs *out,
                               void *stream_v) {
    LaunchPlan plan{};
    if (int rc = from_keys_plan(ch, d_key, out, T, restart_begin, R, &plan)) return rc;
    if ((out->d_win_x && !d_x) || (out->d_win_f && !d_f)) return fail(OPTIK_HIP_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(ch->mu);
    hipStream_t stream = (hipStream_t)stream_v;
    BIND_DEVICE(ch);
    if (int rc = from_keys_workspace(ch, plan, stream)) return rc;
    const SelectionIn in{const_cast<double *>(d_key), d_x, d_f, restart_begin, R, plan.tiles_per_target, (size_t)plan.cols};
    HIP_TRY(select_launch(make_select_launch(ch, in, out, nullptr, nullptr), T, stream));
    return 0;
}

int optik_hip_solutions_from_keys(optik_hip_chain *ch, double *d_key, const double *d_x, const double *d_f, int32_t T,
                                  uint64_t restart_begin, uint64_t R, int32_t K, double min_dist,
                                  const optik_hip_ik_solutions_outputs *out, void *stream_v) {
    if (int rc = check_solutions_args(K, min_dist)) return rc;
    LaunchPlan plan{};
    if (int rc = from_keys_plan(ch, d_key, out, T, restart_begin, R, &plan)) return rc;
    if (!d_x || (out->d_f && !d_f)) return fail(OPTIK_HIP_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(ch->mu);
    hipStream_t stream = (hipStream_t)stream_v;
    BIND_DEVICE(ch);
    if (int rc = from_keys_workspace(ch, plan, stream)) return rc;
    if (plan.tiles_per_target > 1) HIP_TRY(ch->sol_pick.reserve((size_t)T));
    const SelectionIn in{d_key, d_x, d_f, restart_begin, R, plan.tiles_per_target, (size_t)plan.cols};
    HIP_TRY(solutions_launch(make_solutions_launch(ch, in, K, min_dist, out, nullptr), T, stream));
    return 0;
}

int optik_hip_path_select_from_keys(optik_hip_chain *ch, const double *d_key, const double *d_x, const double *d_f,
                                    const double *d_seed, int32_t P, uint64_t restart_begin, uint64_t R,
                                    double max_step, const optik_hip_ik_path_outputs *out, double *d_carry,
                                    void *stream_v) {
    if (int rc = check_path_args(R, max_step)) return rc;
    LaunchPlan plan{};
    if (int rc = from_keys_plan(ch, d_key, out, P, restart_begin, R, &plan)) return rc;
    if (!d_x || !d_seed || !d_carry) return fail(OPTIK_HIP_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(ch->mu);
    hipStream_t stream = (hipStream_t)stream_v;
    BIND_DEVICE(ch);
    if (int rc = from_keys_workspace(ch, plan, stream)) return rc;
    const SelectionIn in{const_cast<double *>(d_key), d_x, d_f, restart_begin, R, plan.tiles_per_target, (size_t)plan.cols};
    HIP_TRY(path_select_launch(make_path_select_launch(ch, in, d_seed, d_carry, max_step, out, 0, true, nullptr, nullptr),
                               P, stream));
    return 0;
}

/* Tuning options (tests, tools): see `struct Options` (ik_host.hpp).  Names: solve_kernel (0 auto, 1 quad, 2 lane64,
 * 3 general), wide_form (0 lds, 1 hbm), range_rule (of chains created afterwards), stop_x_legacy, grid_cap (0 the
 * device's cap, v >= 1 at most v blocks per grid-stride launch; a negative value is refused).  Not synchronised with
 * calls in flight. */
static int *option_slot(const char *name) {
    Options &o = opt();
    if (!name) return nullptr;
    if (!std::strcmp(name, "solve_kernel")) return &o.solve_kernel;
    if (!std::strcmp(name, "wide_form")) return &o.wide_form;
    if (!std::strcmp(name, "range_rule")) return &o.range_rule;
    if (!std::strcmp(name, "stop_x_legacy")) return &o.stop_x_legacy;
    if (!std::strcmp(name, "grid_cap")) return &o.grid_cap;
    return nullptr;
}
int optik_hip_set_option(const char *name, long long value) {
    int *slot = option_slot(name);
    if (!slot) return fail(OPTIK_HIP_EINVAL, "unknown option");
    if (slot == &opt().grid_cap && (value < 0 || value > 0x7fffffffll))
        return fail(OPTIK_HIP_EINVAL, "grid_cap must be >= 0 (0: the device's cap)");
    *slot = (int)value;
    return 0;
}
long long optik_hip_get_option(const char *name) {
    const int *slot = option_slot(name);
    return slot ? (long long)*slot : -1;
}

int optik_hip_ik_host(optik_hip_chain *ch, const optik_solver_config *cfg, const double *targets,
                      const double *x0, int32_t T, const double *ee_offset7, uint64_t restart_begin,
                      uint64_t restart_end, uint32_t flags, double deadline_s, double *win_x, double *win_f,
                      uint64_t *win_idx, double *win_key) {
    if (!ch || !cfg || !targets || !x0 || T < 1) return fail(OPTIK_HIP_EINVAL, "bad argument");  // (cfg is read below, before ik_batch_locked's own check)
    // the launch workspace of the chain is in use until the copies below are done
    std::lock_guard<std::mutex> host_lock(ch->host_mu);
    BIND_DEVICE(ch);
    const int n = ch->n;
    // one device block and one pinned staging block, kept with the chain (a call used to pay
    // six hipMalloc / hipFree pairs and six copies): in = targets [T][7], x0 [T][n];
    // out = win_x [T][n], win_f [T], win_key [T], win_idx [T]
    const size_t n_in = (size_t)(7 + n) * (size_t)T, n_out = (size_t)(n + 3) * (size_t)T;
    // (`mu` from here to the launch: the claim state and the staging blocks belong to the launch workspace)
    std::unique_lock<std::mutex> launch_lock(ch->mu);
    if (n_in + n_out > ch->hw_dev.capacity() || 2 * (n_in + n_out) > ch->hw_pin.capacity()) {
        if (ch->claim_pending) { (void)hipStreamSynchronize(nullptr); ch->claim_pending = false; }  // (its launch reads the block about to go)
        HIP_TRY(ch->hw_dev.reserve(n_in + n_out));
        HIP_TRY(ch->hw_pin.reserve(2 * (n_in + n_out)));  // (two blocks, see below)
    }
    // A few targets (Robot::ik: one): the kernels read the inputs from and write the winners to the
    // pinned block directly -- no copy commands around the launch.  (Two such blocks, used in turn: a call
    // that returned on the first success -- below -- leaves a launch behind whose last restarts still read theirs.)
    const bool zero_copy = T <= 16;
    double *pin = ch->hw_pin.get();
    if (zero_copy) {
        pin += (ch->hw_flip & 1u) * (ch->hw_pin.capacity() / 2);
        ch->hw_flip ^= 1u;
    } else if (ch->claim_pending) {
        // The staged path always uses block 0.  A launch that a first-success call left running may have been given
        // that block: its selection kernel still writes its winner there -- inside the region the targets are about
        // to be staged in -- so it has to end first (the two-block flip only protects the zero-copy calls).
        HIP_TRY(hipStreamSynchronize(nullptr));
        ch->claim_pending = false;
    }
    double *io = zero_copy ? pin : ch->hw_dev.get();
    double *d_t = io, *d_x0 = d_t + (size_t)7 * T;
    double *d_wx = io + n_in, *d_wf = d_wx + (size_t)n * T, *d_wk = d_wf + T;
    uint64_t *d_wi = reinterpret_cast<uint64_t *>(d_wk + T);
    std::memcpy(pin, targets, sizeof(double) * 7 * (size_t)T);
    std::memcpy(pin + (size_t)7 * T, x0, sizeof(double) * (size_t)n * (size_t)T);
    if (!zero_copy)
        HIP_TRY(hipMemcpyAsync(ch->hw_dev.get(), pin, sizeof(double) * n_in, hipMemcpyHostToDevice, nullptr));
    optik_hip_ik_outputs o;
    std::memset(&o, 0, sizeof o);
    o.d_win_x = d_wx; o.d_win_f = d_wf; o.d_win_idx = d_wi; o.d_win_key = d_wk;
    // One target under the first-success rule (lib.rs:409-412, the reference's default): the first restart to
    // succeed writes its answer to a host-coherent block and the call returns as soon as it is there; the launch's
    // other restarts notice the flag at their next evaluation and the launch ends behind the caller's back (the
    // next launch of the chain queues behind it).  Without a success the call ends with the launch, as before.
    // (not under the collision filter: the first success may not be free)
    const bool claim = T == 1 && (flags & OPTIK_HIP_IK_FIND_ANY) && (flags & OPTIK_HIP_IK_EARLY_EXIT)
                       && cfg->solution_mode == OPTIK_MODE_SPEED && ch->coll_S == 0;
    if (claim && !ch->hw_claim) {
        HIP_TRY(hipHostMalloc(&ch->hw_claim, sizeof(unsigned long long) * (3 + MAX_DOF), hipHostMallocCoherent));
        std::memset(ch->hw_claim, 0, sizeof(unsigned long long) * (3 + MAX_DOF));
        HIP_TRY(hipEventCreateWithFlags(&ch->claim_done, hipEventDisableTiming));
    }
    bool armed = false;
    unsigned long long seq = 0;
    int rc = ik_batch_locked(ch, cfg, d_t, d_x0, T, ee_offset7, restart_begin, restart_end, flags, deadline_s, &o, nullptr,
                             claim, &armed);
    seq = ch->claim_seq;
    // (the end of THIS launch, not of the null stream: other chains' calls may keep that one busy)
    if (!rc && armed && hipEventRecord(ch->claim_done, nullptr) != hipSuccess) rc = fail(OPTIK_HIP_ENODEVICE, "hipEventRecord failed");
    launch_lock.unlock();
    if (rc) return rc;
    double *h_out = pin + n_in;
    if (!zero_copy) HIP_TRY(hipMemcpyAsync(h_out, d_wx, sizeof(double) * n_out, hipMemcpyDeviceToHost, nullptr));
    if (armed) {
        // this launch's first success is in the claim block: it goes to the caller's win_*
        auto claimed = [&]() {
            if (__atomic_load_n(ch->hw_claim, __ATOMIC_ACQUIRE) != seq) return false;
            volatile unsigned long long *cw = ch->hw_claim;
            if (win_x) std::memcpy(win_x, (const void *)(cw + 3), sizeof(double) * (size_t)n);
            if (win_f) std::memcpy(win_f, (const void *)(cw + 2), sizeof(double));
            if (win_idx) *win_idx = cw[1];
            if (win_key) *win_key = (double)cw[1];
            return true;
        };
        for (unsigned spin = 1;; ++spin) {
            if (claimed()) return 0;  // (claim_pending stays set: the launch ends behind the caller's back)
            if ((spin & 63u) == 0) {
                const hipError_t q = hipEventQuery(ch->claim_done);
                if (q == hipSuccess) break;  // the launch is over and nobody succeeded (or the word is about to land)
                if (q != hipErrorNotReady) HIP_TRY(q);
            }
        }
        if (claimed()) return 0;
    }
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (armed) {
        // (nothing of this call is left on the null stream -- unless a later launch of the chain armed a claim meanwhile)
        std::lock_guard<std::mutex> relock(ch->mu);
        if (ch->claim_seq == seq) ch->claim_pending = false;
    }
    if (win_x) std::memcpy(win_x, h_out, sizeof(double) * (size_t)n * (size_t)T);
    if (win_f) std::memcpy(win_f, h_out + (size_t)n * T, sizeof(double) * (size_t)T);
    if (win_key) std::memcpy(win_key, h_out + (size_t)(n + 1) * T, sizeof(double) * (size_t)T);
    if (win_idx) std::memcpy(win_idx, h_out + (size_t)(n + 2) * T, sizeof(uint64_t) * (size_t)T);
    return 0;
}

void optik_hip_set_timing(optik_hip_chain *ch, int32_t enabled) {
    if (!ch) return;
    std::lock_guard<std::mutex> lock(ch->mu);
    ch->timing = enabled;
    ch->ev_count = 0;
}

/* OPTIK_PROFILE builds: phase cycle totals of the last solve launch (8 words:
 * refill, eval, update, publish, bfgs, lsq, nnls, trips); zeros otherwise. */
int optik_hip_phase_profile(optik_hip_chain *ch, unsigned long long *out8) {
    if (!ch || !out8) return fail(OPTIK_HIP_EINVAL, "bad argument");
    std::memset(out8, 0, 8 * sizeof(unsigned long long));
    if (!ch->prof) return 0;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out8, ch->prof, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}

int optik_hip_timing_mean(optik_hip_chain *ch, double *mean_ms, int32_t *count) {
    if (!ch || !mean_ms || !count) return fail(OPTIK_HIP_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(ch->mu);
    const int n = ch->ev_count < optik_hip_chain::EV_POOL ? ch->ev_count : optik_hip_chain::EV_POOL;
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        HIP_TRY(hipEventSynchronize(ch->ev1[i]));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, ch->ev0[i], ch->ev1[i]));
        sum += ms;
    }
    *mean_ms = n ? sum / n : 0.0;
    *count = n;
    return 0;
}

int optik_hip_last_launch(const optik_hip_chain *ch, optik_hip_launch_info *info) {
    if (!ch || !info) return fail(OPTIK_HIP_EINVAL, "bad argument");
    *info = ch->last;
    info->kernel_ms = 0.0f;
    if (ch->timing && ch->ev_count > 0) {
        const int slot = (ch->ev_count - 1) % optik_hip_chain::EV_POOL;
        HIP_TRY(hipEventSynchronize(ch->ev1[slot]));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, ch->ev0[slot], ch->ev1[slot]));
        info->kernel_ms = ms;
    }
    return 0;
}

}  // extern "C"
