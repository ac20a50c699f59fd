"""What a launch runs on is what plan_launch (optik_amd/csrc/ik_launch_plan.hpp) planned: the grid optik_hip_last_launch
reports equals the grid the g++-built pure function returns for the device's CU count, and the static LDS of the kernel
that ran names the planned solver.  No number of its own: tests/test_launch_plan_host.py pins the plan."""
import numpy as np
import pytest
import torch

from gpu_util import make_targets
from launch_plan_util import EARLY, QUALITY, RM, SPEED, build_planner, plan_inputs

pytestmark = pytest.mark.gpu

# (chain, T, R, keywords of plan_inputs): the sizes around every crossover the chain can reach
LAUNCHES = [
    ("panda", 1, 1, {}), ("panda", 1, 1024, {}), ("panda", 1, 1025, {}), ("panda", 1, 65535, {}),
    ("panda", 1, 65536, {}), ("panda", 64, 1024, dict(flags=EARLY | RM)),
    ("panda", 64, 1024, dict(flags=EARLY | RM, mode=QUALITY)),
    ("panda", 1, 10, dict(solve_kernel="lane64")), ("panda", 1, 10, dict(solve_kernel="quad")),
    ("panda", 1, 5000, dict(solve_kernel="general", wide_form="lds")),
    ("panda", 1, 5000, dict(solve_kernel="general", wide_form="hbm")),
    ("arm8", 1, 1, {}), ("arm8", 1, 1025, {}), ("arm8", 1, 65536, {}), ("arm8", 64, 1024, dict(flags=EARLY | RM)),
    ("arm8", 1, 10, dict(solve_kernel="lane64")),
    ("arm12", 1, 1, {}), ("arm12", 1, 5000, dict(wide_form="lds")), ("arm12", 1, 5000, dict(wide_form="hbm")),
]


def test_the_launch_is_the_plan(oracle, chains):
    from optik_amd import _native as nat
    from optik_amd import device
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    plans = build_planner()([plan_inputs(len(chains[c][0]["lb"]), T, R, cus=cus, **kw) for c, T, R, kw in LAUNCHES])
    rng = np.random.default_rng(3)
    hip, seen = {}, set()
    for (c, T, R, kw), p in zip(LAUNCHES, plans):
        d, ch = chains[c]
        hc = hip.setdefault(c, device.HipChain(**d))
        tg, x0 = make_targets(oracle, d, ch, rng, T)
        cfg = nat.make_config(solution_mode="quality" if kw.get("mode", SPEED) == QUALITY else "speed")
        with nat.options(solve_kernel=kw.get("solve_kernel", "auto"), wide_form=kw.get("wide_form", "lds")):
            hc.ik_batch(cfg, torch.tensor(tg, device="cuda"), torch.tensor(x0, device="cuda"), 0, R,
                        flags=kw.get("flags", 0), per_restart=False)
            torch.cuda.synchronize()
        info = hc.last_launch()
        what = (c, T, R, kw, p, info)
        print(c, T, R, kw, p["solver"], "planned grid", p["grid"], "launched", info["grid"], "lds", info["lds_bytes"])
        assert p["error"] == 0, what
        assert info["grid"] == p["grid"] and info["tiles"] == p["n_tiles"] and info["block"] == 64, what
        # the solver, as far as the kernel's static LDS tells: the lane-per-restart form above 30 000 bytes, the quad
        # solver below; the general solver's LDS form above 8 192, its HBM form the chain table alone
        if p["solver"] in ("WIDE_LDS", "WIDE_HBM"):
            assert (info["lds_bytes"] > 8192) == (p["solver"] == "WIDE_LDS"), what
        else:
            assert (info["lds_bytes"] > 30000) == (p["solver"] == "LANE"), what
        seen.add(p["solver"])
    assert seen == {"QUAD_LATENCY", "QUAD", "LANE", "WIDE_LDS", "WIDE_HBM"}
