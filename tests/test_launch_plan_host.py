"""The solver launch plan (optik_amd/csrc/ik_launch_plan.hpp: plan_launch) as a pure function, compiled with g++: which
solver a launch runs on, how many restarts a wave holds and how many are resident, the grid, the first-success claim and
the selection-tile refusal -- no GPU.  tests/test_gpu_launch_plan.py ties the same function to what is launched."""
import pytest

from launch_plan_util import EARLY, FIND_ANY, QUALITY, RM, SPEED, build_planner, plan_inputs


@pytest.fixture(scope="module")
def plan():
    return build_planner()


# 256 CUs; resident waves per CU: lane 4, quad 8 (n <= 7) or 6 (n = 8), latency 4, general 8.  Derived by hand from the
# launch code as it was before the plan became a function.
#        n, T,    R,     keywords                                      solver          lanes resident grid  early
TABLE = [
    (7, 1, 1, {}, "QUAD_LATENCY", 1, 1, 1, False),
    (7, 1, 1024, {}, "QUAD_LATENCY", 1, 1024, 1024, False),               # one restart per SIMD: the last latency size
    (7, 1, 1025, {}, "QUAD", 1, 1025, 1025, False),
    (7, 1, 65535, {}, "QUAD", 16, 65535, 2048, False),                    # one short of a full load of the lane form
    (7, 1, 65536, {}, "LANE", 64, 65536, 1024, False),
    (8, 1, 65536, {}, "QUAD", 16, 65536, 1536, False),                    # n = 8 has no lane form
    (7, 64, 1024, dict(flags=EARLY | RM), "QUAD", 2, 4096, 2048, True),   # floor: two restarts per resident wave
    (7, 1000, 100, dict(flags=EARLY | RM), "QUAD", 16, 32000, 2000, True),  # floor: 32 restarts per target
    (7, 64, 1024, dict(flags=EARLY | RM, mode=QUALITY), "LANE", 64, 65536, 1024, False),
    (7, 64, 1024, dict(flags=EARLY | RM, coll=True), "LANE", 64, 65536, 1024, False),
    (7, 1, 10, dict(solve_kernel="lane64"), "LANE", 1, 10, 10, False),
    (8, 1, 10, dict(solve_kernel="lane64"), "QUAD_LATENCY", 1, 10, 10, False),
    (7, 1, 10, dict(solve_kernel="quad"), "QUAD_LATENCY", 1, 10, 10, False),
    (12, 1, 5000, dict(wide_form="lds"), "WIDE_LDS", 1, 5000, 2048, False),
    (12, 1, 5000, dict(wide_form="hbm"), "WIDE_HBM", 3, 5000, 1667, False),
    (6, 1, 5000, dict(solve_kernel="general"), "WIDE_LDS", 1, 5000, 2048, False),
]


def test_the_plan_table(plan):
    got = plan([plan_inputs(n, T, R, **kw) for n, T, R, kw, *_ in TABLE])
    for (n, T, R, kw, solver, lanes, resident, grid, early), p in zip(TABLE, got):
        row = (n, T, R, kw)
        assert p["error"] == 0, row
        assert (p["solver"], p["lanes"], p["resident"], p["grid"]) == (solver, lanes, resident, grid), (row, p)
        assert p["early"] == early, (row, p)
        assert p["cols"] == T * R and p["tiles_per_target"] == -(-R // 4096) and p["n_tiles"] == T * -(-R // 4096), (row, p)
        flags, mode = kw.get("flags", 0), kw.get("mode", SPEED)
        assert p["restart_major"] == bool(flags & RM) and p["quality"] == (mode != SPEED), (row, p)
        assert p["find_any"] == 0 and p["arm_claim"] == 0, (row, p)


def test_the_claim_is_armed_exactly_when_every_condition_holds(plan):
    """A single call under the first-success rule on the quad solver, with a claim block to write to."""
    base = dict(n=7, T=1, R=1024, flags=EARLY | FIND_ANY, mode=SPEED, claim_request=True, have_claim_block=True)
    flips = [dict(claim_request=False), dict(have_claim_block=False), dict(T=2), dict(flags=FIND_ANY),
             dict(flags=EARLY), dict(mode=QUALITY), dict(coll=True),
             dict(solve_kernel="lane64"), dict(R=65536), dict(solve_kernel="general")]
    holds = [base, dict(base, R=2000), dict(base, n=8, R=65536), dict(base, flags=EARLY | FIND_ANY | RM)]
    got = plan([plan_inputs(**kw) for kw in holds] + [plan_inputs(**dict(base, **f)) for f in flips])
    assert [p["solver"] for p in got[:len(holds)]] == ["QUAD_LATENCY", "QUAD", "QUAD", "QUAD_LATENCY"]
    for kw, p in zip(holds, got):
        assert p["arm_claim"] == 1 and p["early"] == 1 and p["find_any"] == 1, (kw, p)
    for f, p in zip(flips, got[len(holds):]):
        assert p["error"] == 0 and p["arm_claim"] == 0, (f, p)
    # (the last three flips are flips of the solver)
    assert [p["solver"] for p in got[-3:]] == ["LANE", "LANE", "WIDE_LDS"]


def test_the_tile_refusal(plan):
    """2^24 or more selection tiles (tiles_per_target * T * 256 >= 2^32) are refused, one tile fewer is planned."""
    full = 1 << 24
    cases = [(1, (full - 1) * 4096, 0), (1, (full - 1) * 4096 + 1, 1), (1, full * 4096, 1),
             (4095, 4096 * 4096, 0), (4096, 4096 * 4096 - 4096, 0), (4096, 4096 * 4096 - 4095, 1), (4096, 4096 * 4096, 1)]
    got = plan([plan_inputs(7, T, R) for T, R, _ in cases])
    for (T, R, refused), p in zip(cases, got):
        assert p["error"] == refused, (T, R, p)
        if not refused:
            assert p["n_tiles"] == T * -(-R // 4096) == full - (1 if T == 1 else 4096) and p["cols"] == T * R, (T, R, p)


def test_an_unknown_cu_count_plans_as_256(plan):
    sizes = [(7, 1, 1024, {}), (7, 1, 1025, {}), (7, 1, 65536, {}), (8, 1, 65536, {}),
             (7, 64, 1024, dict(flags=EARLY | RM)), (12, 1, 5000, dict(wide_form="hbm"))]
    want = plan([plan_inputs(n, T, R, cus=256, **kw) for n, T, R, kw in sizes])
    for cus in (0, -1):
        assert plan([plan_inputs(n, T, R, cus=cus, **kw) for n, T, R, kw in sizes]) == want
    # (and the CU count is read: another chip, other crossovers)
    small = plan([plan_inputs(7, 1, 1024, cus=64), plan_inputs(7, 1, 16384, cus=64)])
    assert [p["solver"] for p in small] == ["QUAD", "LANE"] and [p["grid"] for p in small] == [512, 256]
