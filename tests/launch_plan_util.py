"""plan_launch of optik_amd/csrc/ik_launch_plan.hpp compiled with g++ as plain C++ (no HIP runtime), for the host test
of the plan and the -m gpu test that compares it with what was launched."""
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optik_amd", "csrc")

# the values of include/optik_hip.h and of the options (optik_amd/_native.py)
EARLY, FIND_ANY, RM = 1, 2, 4
QUALITY, SPEED, MANIPULABILITY, CONDITION = 1, 2, 3, 4
SK = {"auto": 0, "quad": 1, "lane64": 2, "general": 3}
WF = {"lds": 0, "hbm": 1}
SOLVERS = ["QUAD_LATENCY", "QUAD", "LANE", "WIDE_LDS", "WIDE_HBM"]

IN_FIELDS = ["n", "wide", "cus", "T", "R", "flags", "mode", "coll", "solve_kernel", "wide_form", "claim_request",
             "have_claim_block", "lane_waves", "quad_waves", "latency_waves", "wide_waves"]
OUT_FIELDS = ["error", "solver", "early", "find_any", "quality", "restart_major", "arm_claim", "lanes", "resident",
              "grid", "tiles_per_target", "n_tiles", "cols"]

DRIVER = r"""
#include <cstdio>
#include "ik_launch_plan.hpp"

using namespace optik::host;

// one plan per input line (the fields of PlanIn in order), one output line each (the fields of LaunchPlan in order)
int main() {
    static_assert(QUAD_LATENCY == 0 && QUAD == 1 && LANE == 2 && WIDE_LDS == 3 && WIDE_HBM == 4, "solver names");
    static_assert(WAVE == 64 && QUADS_PER_WAVE_HOST == 16 && SEL_TILE == 4096, "the constants the kernels are built to");
    long long v[16];
    for (;;) {
        for (int i = 0; i < 16; ++i)
            if (std::scanf("%lld", &v[i]) != 1) return i == 0 ? 0 : 2;
        PlanIn in{};
        in.n = (int)v[0]; in.wide = v[1] != 0; in.cus = (int)v[2]; in.T = (int32_t)v[3]; in.R = (uint64_t)v[4];
        in.flags = (uint32_t)v[5]; in.mode = (int)v[6]; in.coll = v[7] != 0; in.solve_kernel = (int)v[8];
        in.wide_form = (int)v[9]; in.claim_request = v[10] != 0; in.have_claim_block = v[11] != 0;
        in.lane_waves = (int)v[12]; in.quad_waves = (int)v[13]; in.latency_waves = (int)v[14]; in.wide_waves = (int)v[15];
        const LaunchPlan p = plan_launch(in);
        std::printf("%d %d %d %d %d %d %d %d %lld %d %llu %d %llu\n", (int)p.error, (int)p.solver, (int)p.early,
                    (int)p.find_any, (int)p.quality, (int)p.restart_major, (int)p.arm_claim, p.lanes, p.resident, p.grid,
                    (unsigned long long)p.tiles_per_target, p.n_tiles, (unsigned long long)p.cols);
    }
}
"""


def plan_inputs(n, T, R, flags=0, mode=SPEED, coll=False, solve_kernel="auto", wide_form="lds", cus=256,
                claim_request=False, have_claim_block=False):
    """The PlanIn of a launch on the library as built: resident waves per CU of lane 4, quad 8 (n <= 7) or 6 (n = 8),
    latency 4, general 8."""
    return dict(n=n, wide=int(n > 8), cus=cus, T=T, R=R, flags=flags, mode=mode, coll=int(coll),
                solve_kernel=SK[solve_kernel], wide_form=WF[wide_form], claim_request=int(claim_request),
                have_claim_block=int(have_claim_block), lane_waves=4, quad_waves=8 if n <= 7 else 6, latency_waves=4,
                wide_waves=8)


def build_planner(workdir=None):
    """Compile the driver; returns plan(list of PlanIn dicts) -> list of LaunchPlan dicts (`solver` as its name; after
    an error only `error` is meaningful)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the launch plan on its own"
    d = workdir or tempfile.mkdtemp(prefix="launch_plan_")
    src, exe = os.path.join(d, "driver.cpp"), os.path.join(d, "driver")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe], check=True)

    def plan(inputs):
        text = "".join(" ".join(str(int(i[k])) for k in IN_FIELDS) + "\n" for i in inputs)
        res = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
        rows = [dict(zip(OUT_FIELDS, map(int, ln.split()))) for ln in res.stdout.splitlines()]
        assert len(rows) == len(inputs)
        for r in rows:
            r["solver"] = SOLVERS[r["solver"]]
        return rows

    return plan
