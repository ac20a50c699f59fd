// wide_emu.cpp -- TEST INFRASTRUCTURE: runs the general solver of optik_amd/csrc/ik_wide.hpp (chains of 9 .. 16 joint
// positions, and shorter ones under solve_kernel = general) on the HOST, one thread per emulated lane
// (tests/emu/lane_emu.hpp), so that tests/test_wide_emulation*.py can compare every restart with the C oracle bit for
// bit without a GPU.  ik_wide.hpp is compiled as it is, with -ffp-contract=off like the kernels, in its three forms:
//
//   WPG  a restart per lane, the lane-strided workspace of ik_wide_kernel.hip's wide_solve_kernel: `lanes` emulated
//        lanes (a multiple of 4), wq.lanes = lanes, SLOTS * 64 doubles (the stride of 64 is fixed in the type)
//   WPL  a restart per wave, one lane working: wq.lanes = 1 on a 4-lane wave, lanes 1 .. 3 idle through wave_any as
//        lanes 1 .. 63 do on the device
//   WPC  a restart per wave, the 64 lanes cooperating: all 64 lanes, each on its own copy of the SLOTS doubles, the
//        copies merged at every __syncthreads() (lane_emu.hpp says why)
//
// Built twice from this one source: libwide_emu.so, and libwide_emu_general_lsi.so with -DOPTIK_WIDE_GENERAL_LSI.
// Not part of the product: nothing under optik_amd/ or bench.py builds, loads or calls this.
#define OPTIK_LANE_EMU 1
#include <thread>
#include <vector>

#include "ik_jacobian.hpp"
#include "ik_wide.hpp"
#include "ik_host_params.hpp"

using namespace optik;

namespace {

enum { FORM_WPG = 0, FORM_WPL = 1, FORM_WPC = 2 };

void fill_chain(WideChainDev &ch, const double *origins, const double *axes, int n, int n_joints, const double *lb,
                const double *ub, int range_rule) {
    std::memset(&ch, 0, sizeof ch);
    ch.n_pos = n;
    ch.has_tip = n_joints == n + 1;
    for (int j = 0; j < n_joints; ++j)
        for (int c = 0; c < 7; ++c) ch.origin[j][c] = origins[j * 7 + c];
    for (int j = 0; j < n; ++j) {
        for (int c = 0; c < 3; ++c) ch.axis[j][c] = axes[j * 3 + c];
        ch.lb[j] = lb[j];
        ch.ub[j] = ub[j];
        ch.scale[j] = hostparams::uniform_scale(lb[j], ub[j], range_rule);
    }
}

template <class F>
void run_lanes(optik_emu::Wave &wave, F &&body) {
    std::vector<std::thread> th;
    for (int lane = 0; lane < wave.lanes; ++lane) {
        th.emplace_back([&, lane]() {
            optik_emu::t_wave = &wave;
            threadIdx.x = (unsigned)lane;
            body(lane);
        });
    }
    for (auto &t : th) t.join();
}

}  // namespace

extern "C" {

// origins [J][7] (t, quat ijkw), axes [n][3], J = n or n + 1; restarts [begin, end) of ONE target.
// out_x [n][R], out_f / out_key [R], out_status / out_evals [R].  form: 0 WPG on `lanes` lanes, 1 WPL, 2 WPC.
int wide_emu_solve(const double *origins, const double *axes, int n, int n_joints, const double *lb, const double *ub,
                   const optik_solver_config *cfg, const double *target7, const double *x0, const double *ee_offset7,
                   uint64_t restart_begin, uint64_t restart_end, int form, int lanes, int range_rule, double *out_x,
                   double *out_f, double *out_key, int32_t *out_status, int32_t *out_evals) {
    if (n < 1 || n > WIDE_MAX_DOF || (n_joints != n && n_joints != n + 1) || restart_end <= restart_begin) return -1;
    if (form == FORM_WPG && (lanes < 4 || lanes > 64 || lanes % 4)) return -1;
    if (form < FORM_WPG || form > FORM_WPC) return -1;
    WideChainDev ch;
    fill_chain(ch, origins, axes, n, n_joints, lb, ub, range_rule);
    EvalParams ep;
    hostparams::make_eval_params(cfg->linear_weight, cfg->angular_weight, ee_offset7, ep);
    SolveParams sp;
    hostparams::fill_solve_params(cfg, sp);
    uint32_t key[8];
    hostparams::seed_from_u64(42, key);

    unsigned long long counter = 0;
    WorkQueue wq;
    std::memset(&wq, 0, sizeof wq);
    const uint64_t R = restart_end - restart_begin;
    wq.next_item = &counter;
    wq.total_items = R;
    wq.n_restarts = R;
    wq.restart_begin = restart_begin;
    wq.targets = target7;
    wq.x0 = x0;
    wq.first_success = nullptr;
    wq.n_targets = 1;
    wq.quality = cfg->solution_mode == 1;
    wq.lanes = form == FORM_WPG ? lanes : 1;
    wq.out_x = out_x;
    wq.out_f = out_f;
    wq.out_key = out_key;
    wq.out_status = out_status;
    wq.out_evals = out_evals;

    optik_emu::Wave wave;
    if (form == FORM_WPG) {
        wave.lanes = lanes;
        std::vector<double> ws((size_t)wide_ws::SLOTS * 64, 0.0);
        run_lanes(wave, [&](int lane) { wide_solve_wave(ch, ep, sp, key, wq, WPG{ws.data() + lane}); });
    } else if (form == FORM_WPL) {
        wave.lanes = 4;
        std::vector<double> ws((size_t)wide_ws::SLOTS, 0.0);
        run_lanes(wave, [&](int) { wide_solve_wave(ch, ep, sp, key, wq, WPL{(lds_double *)ws.data()}); });
    } else {
        wave.lanes = 64;
        std::vector<double> ws((size_t)wide_ws::SLOTS * 64, 0.0);  // a copy per lane
        double *copies[64];
        for (int i = 0; i < 64; ++i) copies[i] = ws.data() + (size_t)i * wide_ws::SLOTS;
        wave.share(copies, (size_t)wide_ws::SLOTS);
        run_lanes(wave, [&](int lane) { wide_solve_wave(ch, ep, sp, key, wq, WPC{(lds_double *)copies[lane]}); });
    }
    return 0;
}

// What the wide eval_batch, fk_batch and seed_batch kernels (ik_wide_kernel.hip) run per configuration, on plain
// arrays, one configuration after another on one thread.  q [B][n]; any output may be null.
//   f [B], g [B][n]          wide_eval_fg against target7 under the config's weights and the ee offset
//   pose [B][7], jac [B][6n] wide_forward and wide_jacobian_column (column-major 6 x n per configuration)
//   seeds [n_seeds][n]       wide_restart_seed of indices first, first + 1, ...
int wide_emu_ops(const double *origins, const double *axes, int n, int n_joints, const double *lb, const double *ub,
                 const optik_solver_config *cfg, const double *target7, const double *ee_offset7, int range_rule,
                 const double *q, long long B, double *f, double *g, double *pose, double *jac, uint64_t first,
                 long long n_seeds, double *seeds) {
    if (n < 1 || n > WIDE_MAX_DOF || (n_joints != n && n_joints != n + 1)) return -1;
    WideChainDev ch;
    fill_chain(ch, origins, axes, n, n_joints, lb, ub, range_rule);
    EvalParams ep;
    hostparams::make_eval_params(cfg->linear_weight, cfg->angular_weight, ee_offset7, ep);
    uint32_t key[8];
    hostparams::seed_from_u64(42, key);
    const Pose target = load_pose(target7);
    for (long long b = 0; b < B; ++b) {
        double qq[WIDE_MAX_DOF], gg[WIDE_MAX_DOF], tf[7 * WIDE_MAX_DOF];
        for (int i = 0; i < n; ++i) qq[i] = q[b * n + i];
        if (f) {
            f[b] = wide_eval_fg(ch, ep, target, n, qq, tf, gg);
            if (g)
                for (int i = 0; i < n; ++i) g[b * n + i] = gg[i];
        }
        if (pose) {
            const Pose ee = wide_forward(ch, ep, n, qq, tf);
            const double p[7] = {ee.t.x, ee.t.y, ee.t.z, ee.q.i, ee.q.j, ee.q.k, ee.q.w};
            for (int i = 0; i < 7; ++i) pose[b * 7 + i] = p[i];
            if (jac) {
                const Q4 eeqc = qconj(ee.q);
                for (int k = 0; k < n; ++k) {
                    double c6[6];
                    wide_jacobian_column(ch, tf, ee, eeqc, k, c6);
                    for (int r = 0; r < 6; ++r) jac[b * 6 * n + k * 6 + r] = c6[r];
                }
            }
        }
    }
    for (long long b = 0; b < n_seeds; ++b) {
        double qq[WIDE_MAX_DOF];
        wide_restart_seed(key, ch.lb, ch.scale, first + (uint64_t)b, n, qq);
        for (int i = 0; i < n; ++i) seeds[b * n + i] = qq[i];
    }
    return 0;
}

}  // extern "C"
