"""The solver-edge scenario table (tests/golden/generated/solver_edge_scenarios.json) through the host emulation of
the general solver (tests/emu/wide_emu.cpp: optik_amd/csrc/ik_wide.hpp in its three forms) against the C oracle, bit
for bit: the endings a reachable target never takes, which tests/test_oracle_solver_edge_census.py shows the windows
compared here reach (its `n>=9 emu` column).  The evaluation cap and the line search's non-finite branch of the wide
solver are compared here and nowhere else: nothing that reaches the cap is launched on a GPU.

WPG and WPL run every window in full.  The cooperative form (WPC: 64 host threads, about 0.15 s per evaluation) runs,
of every n >= 9 window, the longest prefix that the oracle solves within WPC_WINDOW_EVALS evaluations (at least one
restart), restart 78 alone of the reset-count window, and not the evaluation-cap scenario (a million barriers per
capped restart): the cooperative form does not take the non-finite line search and the cap under comparison.  Its
w_slsqpb and driver are the same text as the one-lane forms'."""
import os

import numpy as np
import pytest

import solver_edge_util as u
from test_wide_emulation import assert_same_with_key, emu  # noqa: F401

SCENARIOS = {s["name"]: s for s in u.load_scenarios()}
WIDE_RESTARTS = u.EMU_RESTARTS  # of each scenario's range, from its begin
WPC_WINDOW_EVALS = 100          # oracle evaluations of the prefix of a window that the cooperative form runs
WPC_RUNS_THE_CAP = False
WIDE_GPU = [k for k, s in SCENARIOS.items() if s["n"] >= 9 and s["gpu"]]
TUNED_GPU = [k for k, s in SCENARIOS.items() if s["n"] <= 8 and s["gpu"]]
FORMS = [("WPG", 4), ("WPG", 8), ("WPL", 4), ("WPC", 64)]
FORM_IDS = ["WPG-4", "WPG-8", "WPL", "WPC"]


@pytest.fixture(scope="module")
def windows(oracle, chains):
    """name -> the oracle's records of the scenario's window (every entry; the gpu: false ones whole): computed once."""
    out = {}
    for name, sc in SCENARIOS.items():
        b, e = u.emu_window(sc) if sc["gpu"] else (sc["restart_begin"], sc["restart_end"])
        out[name] = u.oracle_run(oracle, chains[sc["robot"]][1], sc, b, e)
    return out


def _head(ref, R):
    full = len(ref["status"])
    return {k: (v[:R] if isinstance(v, np.ndarray) and v.shape[:1] == (full,) else v) for k, v in ref.items()}


def _wpc_prefix(ref):
    return max(1, int(np.searchsorted(np.cumsum(ref["evals"]), WPC_WINDOW_EVALS, side="right")))


def _run(emu, chains, sc, ref, form, lanes, R=None, begin=None, **kw):
    from optik_amd import _native as nat
    d, _ = chains[sc["robot"]]
    begin = sc["restart_begin"] if begin is None else begin
    R = len(ref["status"]) if R is None else R
    got = emu.wide_solve(d, nat.make_config(**u.config_kw(sc)), np.array(sc["target"]), np.array(sc["x0"]), begin,
                         begin + R, form=form, lanes=lanes, ee_offset7=sc["ee_offset"], **kw)
    assert_same_with_key(got, _head(ref, R), len(d["lb"]), sc["x0"], begin, sc["config"]["solution_mode"] == "quality")
    return got


@pytest.mark.parametrize("form,lanes", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("name", WIDE_GPU)
def test_wide_entries_bit_equal_to_the_oracle(emu, chains, windows, name, form, lanes):
    ref = windows[name]
    _run(emu, chains, SCENARIOS[name], ref, form, lanes, R=_wpc_prefix(ref) if form == "WPC" else None)


@pytest.mark.parametrize("name", TUNED_GPU)
def test_tuned_range_entries_on_the_one_lane_lds_form(emu, chains, windows, name):
    """solve_kernel = general serves the chains of at most 8 joints too: every n <= 8 entry's window on WPL."""
    _run(emu, chains, SCENARIOS[name], windows[name], "WPL", 4)


def test_the_wide_windows_end_in_every_way(windows):
    """The windows of the n >= 9 entries hold every status (and the cooperative form's prefixes more than one)."""
    seen, coop = set(), set()
    for name in WIDE_GPU:
        seen.update(windows[name]["status"].tolist())
        coop.update(windows[name]["status"][:_wpc_prefix(windows[name])].tolist())
    assert {-1, -4, 2, 3, 4} <= seen, seen
    assert {-1, -4, 2, 3} <= coop, coop


@pytest.mark.parametrize("name", WIDE_GPU)
def test_general_lsi_build_gives_the_same_bits(emu, chains, windows, name):
    """-DOPTIK_WIDE_GENERAL_LSI (ik_wide.hpp: Kraft's LSI and Lawson-Hanson's LDP as the general routines, instead of
    the forms written for the box problem's structure) gives the default build's bits, hence the oracle's."""
    sc, ref = SCENARIOS[name], windows[name]
    got = _run(emu, chains, sc, ref, "WPG", 4, general_lsi=True)
    default = _run(emu, chains, sc, ref, "WPG", 4)
    for k in ("x", "f", "key"):
        assert np.array_equal(got[k].view(np.uint64), default[k].view(np.uint64)), k
    assert np.array_equal(got["status"], default["status"]) and np.array_equal(got["evals"], default["evals"])


@pytest.mark.parametrize("form,lanes", FORMS[:3], ids=FORM_IDS[:3])
def test_nonfinite_line_search_and_evaluation_cap(emu, oracle, chains, windows, form, lanes):
    """arm10-nonfinite-speed, all 12 restarts: weights 1e153, f overflows at a trial point of a few restarts, the line
    search halves alpha on its non-finite branch and the merit value never recovers: they return RES_ITER_CAP after
    exactly 100000 evaluations with the best point seen.  WPG (4 and 8 lanes) and WPL; the cooperative form does not
    run this scenario (WPC_RUNS_THE_CAP: 100000 evaluations of 64 threads at a barrier are hours): for WPC these two
    branches stay uncompared -- its w_slsqpb and its driver's cap test are the same text."""
    sc = SCENARIOS["arm10-nonfinite-speed"]
    ref = windows[sc["name"]]
    assert len(ref["status"]) == 12
    _run(emu, chains, sc, ref, form, lanes)
    capped = ref["status"] == oracle.RES_ITER_CAP
    assert 1 <= capped.sum() <= 4
    assert (ref["evals"][capped] == 100000).all() and (ref["evals"][~capped] < 100000).all()
    assert not WPC_RUNS_THE_CAP


RESET_COUNT = ("arm10-far_tols-quality", 72, 84, 78)


@pytest.fixture(scope="module")
def reset_window(oracle, chains):
    name, b, e, _ = RESET_COUNT
    sc = SCENARIOS[name]
    return u.oracle_run(oracle, chains[sc["robot"]][1], sc, b, e)


def test_the_reset_count_is_observable_on_the_oracle(reset_window, tmp_path):
    """Restart 78 of arm10-far_tols-quality makes progress between its Hessian resets, so the count at which SLSQP
    gives up (ireset > 5) decides where it ends: an oracle compiled with `> 4` ends that restart elsewhere."""
    name, b, e, which = RESET_COUNT
    mutant = u.run_mutant_oracle(str(tmp_path), "if (st->ireset > 5) goto L255;", "if (st->ireset > 4) goto L255;",
                                 name, b, e)
    differ = [b + i for i in range(e - b) if (mutant["status"][i], mutant["evals"][i]) !=
              (int(reset_window["status"][i]), int(reset_window["evals"][i]))]
    assert which in differ, f"restarts {b}..{e} no longer tell ireset > 5 from > 4 (only {differ} differ)"


@pytest.mark.parametrize("form,lanes", FORMS, ids=FORM_IDS)
def test_a_fifth_reset_that_follows_progress(emu, chains, reset_window, form, lanes):
    """The window around restart 78 on every form (the cooperative form: restart 78 alone)."""
    name, b, e, which = RESET_COUNT
    if form == "WPC":
        one = {k: (v[which - b:which - b + 1] if isinstance(v, np.ndarray) and v.shape[:1] == (e - b,) else v)
               for k, v in reset_window.items()}
        _run(emu, chains, SCENARIOS[name], one, form, lanes, begin=which)
    else:
        _run(emu, chains, SCENARIOS[name], reset_window, form, lanes, begin=b)


def test_the_comparison_tells_a_wrong_reset_count(emu, chains, reset_window, tmp_path):
    """The emulation built from a copy of ik_wide.hpp in which the reset count reads `> 4` differs from the oracle at
    restart 78: the comparison above bites."""
    from optik_amd import _native as nat
    name, b, e, which = RESET_COUNT
    text, wrong = "if (st.ireset > 5) return 8;", "if (st.ireset > 4) return 8;"
    with open(os.path.join(emu.CSRC, "ik_wide.hpp")) as fh:
        src = fh.read()
    assert src.count(text) == 1
    with open(tmp_path / "ik_wide.hpp", "w") as fh:
        fh.write(src.replace(text, wrong))
    lib = emu.build_wide(force=True, out=str(tmp_path / "libwide_emu_mutant.so"), include_first=str(tmp_path))
    sc = SCENARIOS[name]
    d, _ = chains[sc["robot"]]
    got = emu.wide_solve(d, nat.make_config(**u.config_kw(sc)), np.array(sc["target"]), np.array(sc["x0"]), b, e,
                         form="WPG", lanes=4, lib_path=lib)
    i = which - b
    assert (int(got["status"][i]), int(got["evals"][i])) != (int(reset_window["status"][i]), int(reset_window["evals"][i]))
    same = [b + k for k in range(e - b) if (got["status"][k], got["evals"][k]) ==
            (reset_window["status"][k], reset_window["evals"][k])]
    assert same, "the mutant differs everywhere: it tells nothing about the reset count"
