"""The solver-edge scenario table (tests/golden/generated/solver_edge_scenarios.json) through the host emulation of
the tuned solvers (tests/emu: ik_quad.hpp + ik_nnls_quad.hpp, and ik_lane64.hpp) against the C oracle, bit for bit:
the endings a reachable target never takes -- failed LSQ sub-problems (FAILURE, ROUNDOFF_LIMITED), five Hessian
resets and the relaxed mode-8 tests, the zero-step XTOL, NNLS rejecting a column, the repaired t of the negative LDL'
update -- which tests/test_oracle_solver_edge_census.py shows the restarts compared here (the first EMU_RESTARTS of
every entry) reach.  A mismatch here localises a fault without a GPU.  The evaluation cap and the line search's
non-finite branch are exercised here and nowhere else: nothing that reaches the cap is launched on a GPU."""
import numpy as np
import pytest

import solver_edge_util as u
from test_quad_emulation import _assert_same, emu  # noqa: F401

SCENARIOS = {s["name"]: s for s in u.load_scenarios()}
EMU_RESTARTS = u.EMU_RESTARTS  # of each scenario's range, from its begin


def _run(emu, oracle, chains, sc, quads, lane64, R=EMU_RESTARTS):
    from optik_amd import _native as nat
    d, ch = chains[sc["robot"]]
    begin = sc["restart_begin"]
    end = min(sc["restart_end"], begin + R)
    got = emu.solve(d, nat.make_config(**u.config_kw(sc)), np.array(sc["target"]), np.array(sc["x0"]), begin, end,
                    quads=quads, ee_offset7=sc["ee_offset"], lane64=lane64)
    ref = u.oracle_run(oracle, ch, sc, begin, end)
    _assert_same(got, ref, len(d["lb"]))
    return ref


@pytest.mark.parametrize("quads", [1, 2])
@pytest.mark.parametrize("name", [k for k, s in SCENARIOS.items() if s["n"] <= 8 and s["gpu"]])
def test_quad_form_bit_equal_to_the_oracle(emu, oracle, chains, name, quads):
    _run(emu, oracle, chains, SCENARIOS[name], quads, lane64=False)


@pytest.mark.parametrize("name", [k for k, s in SCENARIOS.items() if s["n"] <= 7 and s["gpu"]])
def test_lane_per_restart_form_bit_equal_to_the_oracle(emu, oracle, chains, name):
    _run(emu, oracle, chains, SCENARIOS[name], quads=2, lane64=True)


def test_the_scenarios_end_in_every_way_within_the_emulated_restarts(oracle, chains):
    """The first EMU_RESTARTS restarts of the n <= 7 and of the n = 8 entries already hold every status."""
    for lo, hi in ((1, 7), (8, 8)):
        seen = set()
        for s in SCENARIOS.values():
            if lo <= s["n"] <= hi and s["gpu"]:
                b = s["restart_begin"]
                seen.update(u.oracle_run(oracle, chains[s["robot"]][1], s, b, b + EMU_RESTARTS)["status"].tolist())
        assert {-1, -4, 2, 3, 4} <= seen, seen


@pytest.mark.parametrize("lane64", [False, True])
def test_evaluation_cap(emu, oracle, chains, lane64):
    """tol_f = tol_df = 0, tol_dx = -1 on the UR10: only an exactly zero step can end a restart, and some never make
    one.  They return RES_ITER_CAP after 100000 evaluations with the best point seen."""
    sc = SCENARIOS["ur10-cap-speed"]
    ref = _run(emu, oracle, chains, sc, quads=2, lane64=lane64, R=sc["restart_end"] - sc["restart_begin"])
    capped = ref["status"] == oracle.RES_ITER_CAP
    assert 1 <= capped.sum() <= 4
    assert (ref["evals"][capped] == 100000).all() and (ref["evals"][~capped] < 100000).all()


NONFINITE = [(k, quads, lane64) for k, s in SCENARIOS.items() if s["n"] <= 8 and s["cls"] == "nonfinite"
             for quads, lane64 in ((1, False), (2, False), (2, True)) if not lane64 or s["n"] <= 7]


@pytest.mark.parametrize("name,quads,lane64", NONFINITE)
def test_nonfinite_line_search(emu, oracle, chains, name, quads, lane64):
    """Weights 1e153: f overflows at a trial point of a few restarts, the line search halves alpha on its non-finite
    branch (the census counts ~100000 passes) and the merit value never recovers: they return RES_ITER_CAP after
    100000 evaluations with the best point seen.  Quad form at 1 and 2 quads, lane-per-restart form for n <= 7."""
    sc = SCENARIOS[name]
    ref = _run(emu, oracle, chains, sc, quads=quads, lane64=lane64, R=sc["restart_end"] - sc["restart_begin"])
    capped = ref["status"] == oracle.RES_ITER_CAP
    assert 1 <= capped.sum() <= 4
    assert (ref["evals"][capped] == 100000).all() and (ref["evals"][~capped] < 100000).all()


FIFTH_RESET = ("arm8-corner_lb-speed", 192, 208, 199)


def test_a_fifth_reset_that_follows_progress(emu, oracle, chains, tmp_path):
    """Restart 199 of arm8-corner_lb-speed makes progress between its Hessian resets, so the count at which SLSQP
    gives up (ireset > 5) decides where it ends (of the table's gpu restarts only this one and restart 78 of
    arm10-far_tols-quality tell `> 5` from `> 4`; everywhere else the resets come back to back and the count is not
    observable).  That claim is checked first: an oracle compiled with `> 4` ends that restart elsewhere."""
    from optik_amd import _native as nat
    name, b, e, which = FIFTH_RESET
    sc = SCENARIOS[name]
    d, ch = chains[sc["robot"]]
    ref = u.oracle_run(oracle, ch, sc, b, e)
    mutant = u.run_mutant_oracle(str(tmp_path), "if (st->ireset > 5) goto L255;", "if (st->ireset > 4) goto L255;",
                                 name, b, e)
    differ = [b + i for i in range(e - b) if (mutant["status"][i], mutant["evals"][i]) !=
              (int(ref["status"][i]), int(ref["evals"][i]))]
    assert which in differ, f"restarts {b}..{e} no longer tell ireset > 5 from > 4 (only {differ} differ)"
    got = emu.solve(d, nat.make_config(**u.config_kw(sc)), np.array(sc["target"]), np.array(sc["x0"]), b, e, quads=2)
    _assert_same(got, ref, len(d["lb"]))
