// ik_launch_plan.hpp -- the ONE place where a restart launch's solver and grid are chosen: plan_launch, a pure
// function of the launch's sizes, flags and options, the chip's CU count and the kernels' resident-wave figures.
// solve_locked (ik_capi.hip) calls it once per launch and then does only what needs a device.  Plain C++ (no HIP
// header: tests/test_launch_plan_host.py compiles it with g++ and pins the crossovers; tests/test_gpu_launch_plan.py
// compares the grids it plans with the grids that were launched).
#pragma once

#include <algorithm>
#include <cstdint>

namespace optik {
namespace host {

constexpr int WAVE = 64;
constexpr int QUADS_PER_WAVE_HOST = 16;  // restarts a wave of the quad solver holds
constexpr int SEL_TILE = 4096;           // restarts per 256-thread selection block

// option solve_kernel; option wide_form (2: the LDS form's one-lane build, planned as the LDS form)
enum : int { SK_AUTO = 0, SK_QUAD = 1, SK_LANE64 = 2, SK_GENERAL = 3 };
enum : int { WF_LDS = 0, WF_HBM = 1 };
// what plan_launch reads of optik_hip.h: OPTIK_HIP_IK_* and OPTIK_MODE_SPEED (ik_host.hpp asserts that they agree)
constexpr uint32_t PLAN_EARLY_EXIT = 1u, PLAN_FIND_ANY = 2u, PLAN_RESTART_MAJOR = 4u;
constexpr int PLAN_MODE_SPEED = 2;

struct PlanIn {
    int n;               // joint positions
    bool wide;           // the chain has 9 .. 16 of them (its only solver is the general one)
    int cus;             // compute units of the chain's device (<= 0: unknown, planned as 256)
    int32_t T;           // targets
    uint64_t R;          // restarts per target
    uint32_t flags;      // OPTIK_HIP_IK_*
    int mode;            // OPTIK_MODE_*
    bool coll;           // a collision model is set: Speed is scheduled as Quality (no early exit, no claim)
    int solve_kernel;    // SK_*
    int wide_form;       // WF_*
    bool claim_request;  // the caller would take the first success from the host-coherent claim block ...
    bool have_claim_block;  // ... and the chain has one
    // resident single-wave workgroups per CU of the solvers as built: lane_solve_waves_per_cu(),
    // quad_solve_waves_per_cu(n), the quad solver's latency form (one per SIMD), the general solver (two per SIMD)
    int lane_waves, quad_waves, latency_waves, wide_waves;
};

enum PlanSolver : int { QUAD_LATENCY, QUAD, LANE, WIDE_LDS, WIDE_HBM };
enum PlanError : int { PLAN_OK = 0, PLAN_TOO_MANY_TILES };

struct LaunchPlan {
    PlanError error;
    PlanSolver solver;
    bool early;          // the launch uses the first-success words
    bool find_any;       // ... under the first-success rule
    bool quality;        // Quality's keys (modes 3 and 4 too: replaced by their key pass)
    bool restart_major;
    bool arm_claim;      // the first success goes to the host at once
    int lanes;           // restarts a wave holds
    long long resident;  // restarts in flight
    int grid;            // single-wave workgroups
    uint64_t tiles_per_target;  // selection tiles of SEL_TILE restarts
    int n_tiles;
    uint64_t cols;       // T * R
};

// The selection tiles of T targets with R restarts each: 4096 restarts per 256-thread block.  Fills tiles_per_target,
// n_tiles and cols of `p`; PLAN_TOO_MANY_TILES (nothing filled) for 2^24 tiles or more.  What plan_launch plans with,
// and all that the selection stage on its own (the optik_hip_*_from_keys test hooks) needs of a plan.
inline PlanError plan_selection_tiles(int32_t T, uint64_t R, LaunchPlan &p) {
    // (R beyond 2^36 is 2^24 tiles for one target already: refused before the sums below can wrap)
    if (R > (1ull << 36)) return PLAN_TOO_MANY_TILES;
    const uint64_t tiles_per_target = (R + SEL_TILE - 1) / SEL_TILE;
    const uint64_t n_tiles64 = tiles_per_target * (uint64_t)T;
    // (HIP rejects a launch whose grid.x * block.x reaches 2^32: 256-thread tile blocks cap the tiles at 2^24 - 1)
    if (n_tiles64 * 256ull >= (1ull << 32)) return PLAN_TOO_MANY_TILES;
    p.tiles_per_target = tiles_per_target;
    p.n_tiles = (int)n_tiles64;
    p.cols = (uint64_t)T * R;
    return PLAN_OK;
}

inline LaunchPlan plan_launch(const PlanIn &in) {
    LaunchPlan p{};
    p.error = plan_selection_tiles(in.T, in.R, p);
    if (p.error != PLAN_OK) return p;
    const long long cols = (long long)p.cols, T = in.T;

    p.early = (in.flags & PLAN_EARLY_EXIT) && in.mode == PLAN_MODE_SPEED && !in.coll;
    p.find_any = p.early && (in.flags & PLAN_FIND_ANY);
    p.restart_major = (in.flags & PLAN_RESTART_MAJOR) != 0;
    p.quality = in.mode != PLAN_MODE_SPEED;
    const bool early_rm = p.early && p.restart_major;

    // Which solver (option solve_kernel; same results, bit for bit): the quad solver of ik_quad.hpp (a restart per
    // quad of lanes, its state spread over the quad, NNLS matrix in LDS; n <= 8), from one full load of the chip
    // on the lane-per-restart form of ik_lane64.hpp (n <= 7), or -- `general` -- the run-time-n solver of
    // ik_wide.hpp on a chain of at most 8 joints too: a third, independently written device solver for the parity
    // tests; chains of 9 .. 16 joints always run on it.
    const bool widek = in.wide || in.solve_kernel == SK_GENERAL;
    const bool lane_able = !widek && in.n <= 7 && in.solve_kernel != SK_QUAD;
    const bool lane_forced = lane_able && in.solve_kernel == SK_LANE64;
    // Persistent waves, each pulling work items until the queue is dry: as many as a CU holds, times the CU count.
    const long long cus = in.cus > 0 ? in.cus : 256;
    // (quad solver: a launch with no more work items than the chip has SIMDs runs one restart per wave on the
    // one-wave-per-SIMD build -- no scratch, the lowest latency per iteration; anything bigger on the
    // two-waves-per-SIMD build)
    const bool quad_latency = !widek && cols <= cus * in.latency_waves && !lane_forced;
    // the throughput form for n <= 7: one restart per lane, bounded sub-problems in class order (ik_lane64.hpp)
    // (the default from one full load of the chip on -- 64 restarts for each of its four waves per CU: below that a
    // launch is as long as its longest restart, and the quad solver's trip is the shorter one; lane_vs_quad_probe.py
    // (a rounds 3-5 tool: git history))
    // (not for a Speed batch's latency-sized rounds: restart-major hand-out with early exit keeps a few restarts per
    // target in flight and abandons most of the rest -- the quad solver's shorter trip wins there)
    const bool lanek = lane_able && !quad_latency && (lane_forced || (cols >= cus * in.lane_waves * WAVE && !early_rm));
    // The general solver's two forms (ik_wide.hpp): one restart per wave with its arrays in LDS and the wave's 64
    // lanes working on it together, or a restart per lane with the HBM workspace.  The first has the short
    // dependent chain and no HBM traffic, the second 64 times the restarts in flight -- and the first wins at
    // every size and joint count measured (wide_chain_bench.py (a rounds 3-5 tool: git history), 262 144 restarts:
    // 1.31 / 0.88 / 0.83 / 1.26 M restarts/s at 9 / 10 / 12 / 16 joints against 1.05 / 0.66 / 0.42 / 0.40 M; a launch
    // on the HBM form takes 50 - 100 ms however small it is).  Option wide_form = hbm selects the HBM form (tests,
    // comparisons).
    p.solver = widek ? (in.wide_form != WF_HBM ? WIDE_LDS : WIDE_HBM) : lanek ? LANE : quad_latency ? QUAD_LATENCY : QUAD;
    const long long cap = cus * (widek ? in.wide_waves : lanek ? in.lane_waves : quad_latency ? in.latency_waves : in.quad_waves);
    const long long per_wave_max = (widek || lanek) ? WAVE : QUADS_PER_WAVE_HOST;

    // fewer work items than the chip holds: one restart per wave (or as few as fit).  A restart-major Speed batch
    // keeps about eight restarts per target in flight: the waves pull the higher indices of the targets still
    // unsolved as they go
    // (but never fewer than one restart per resident wave: a small batch has the chip to itself, and the more of a
    // target's restarts run at once the sooner its first success comes)
    // (a few targets have the chip to themselves: two restarts per resident wave at least, 32 per target up to 256
    // targets -- measured: 64 targets 1.01 -> 0.79 ms, 256: 1.66 -> 1.47 ms, and the few hundred targets a big
    // batch's first round leaves over 8 ms sooner)
    const long long inflight = 8;  // restarts per target in flight
    p.resident = cols;
    if (early_rm && p.resident > T * inflight)
        p.resident = std::max(T * inflight, std::min(p.resident, std::max(2 * cap, T * 32)));
    // (the general solver's LDS form: one restart per wave)
    const long long lanes = p.solver == WIDE_LDS ? 1 : std::clamp((p.resident + cap - 1) / cap, 1ll, per_wave_max);
    p.lanes = (int)lanes;
    p.grid = (int)std::min((p.resident + lanes - 1) / lanes, cap);
    // a single call under the first-success rule on the quad solver: the first success goes to the host at once
    p.arm_claim = in.claim_request && in.have_claim_block && (p.solver == QUAD || p.solver == QUAD_LATENCY) && p.find_any
                  && in.T == 1;
    return p;
}

}  // namespace host
}  // namespace optik
