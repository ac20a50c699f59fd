"""Census of the oracle's solver branches (gcov): what the solver-edge scenario table reaches is a checked fact.

The parity tests draw reachable targets with O(1) weights; a gcov build of oracle/optik_oracle.c shows which branches
of the SLSQP / LSQ / NNLS code those inputs never take, and that the scenario table
(tests/golden/generated/solver_edge_scenarios.json) takes them -- in each joint-count group on its own, since each
group runs on different device code (n <= 7: quad + lane-per-restart, n = 8: quad, n >= 9: the general solver).
The table also bounds the work of what goes to the GPU from the oracle's side: at most GPU_MAX_EVALS evaluations per
restart, nothing at the evaluation cap.  Branches are named by unique source lines (solver_edge_util.ANCHORS)."""
import collections

import pytest

import solver_edge_util as u

RES_FAILURE, RES_ROUNDOFF, RES_FTOL, RES_XTOL, RES_ITER_CAP = -1, -4, 3, 4, -100
# the groups the host emulation takes (tests/test_quad_emulation_solver_edge.py; n >= 9: the general solver,
# tests/test_wide_emulation_solver_edge.py)
EMULATED = ("n<=7", "n=8", "n>=9")


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("oracle_gcov"))
    lib = u.build_coverage_oracle(wd)
    out = {}
    results, lines = u.run_census_child(lib, "baseline", wd)
    out["baseline"] = (results, u.anchor_counts(lines))  # (a missing / ambiguous anchor fails here)
    for g in u.GROUPS:
        if g in EMULATED:
            # the windows the host emulation compares first, counted alone; the other restarts add to them
            first, lines = u.run_census_child(lib, g + ":emu", wd)
            out[g + " emu"] = (first, u.anchor_counts(lines))
            rest, lines = u.run_census_child(lib, g + ":rest", wd, accumulate=True)
            results = {k: {f: first[k][f] + rest[k][f] for f in ("status", "evals")} for k in first}
        else:
            results, lines = u.run_census_child(lib, g, wd)
        out[g] = (results, u.anchor_counts(lines))
    print("\nbranch census (count of the anchored branch; `emu`: the first 16 restarts of each entry alone):")
    print(f"{'':24s}" + "".join(f"{w:>10s}" for w in out))
    for key in u.ANCHORS:
        mark = f"   (not required: {u.NOT_REQUIRED[key]})" if key in u.NOT_REQUIRED else ""
        print(f"{key:24s}" + "".join(f"{out[w][1][key][0]:10d}" for w in out) + mark)
    for w in out:
        hist = collections.Counter(s for r in out[w][0].values() for s in r["status"])
        print(f"{w}: statuses {dict(sorted(hist.items()))}, longest restart "
              f"{max(max(r['evals']) for r in out[w][0].values())} evaluations")
    return out


def test_the_table_has_every_group_mode_and_edge(census):
    scs = u.load_scenarios()
    assert len({s["name"] for s in scs}) == len(scs)
    robots = {s["robot"] for s in scs}
    assert {"panda", "ur10", "ur3e", "panda_hand", "arm8", "arm9", "arm10", "arm16"} <= robots
    assert robots & {"panda1", "panda2", "panda3", "panda4", "panda5"}
    for g in u.GROUPS:
        mine = [s for s in scs if s["group"] == g]
        assert {s["config"]["solution_mode"] for s in mine} == {"speed", "quality"}
        assert any(s["restart_begin"] > 0 for s in mine if s["gpu"])
        assert any(s["ee_offset"] is not None for s in mine if s["gpu"])
        assert all(256 <= s["restart_end"] - s["restart_begin"] <= 2048 for s in mine if s["gpu"])
        assert set(census[g][0]) == {s["name"] for s in mine}  # the census ran exactly the group's entries


@pytest.mark.parametrize("group", u.GROUPS)
def test_each_group_alone_takes_every_required_branch(census, group):
    counts = census[group][1]
    missed = [k for k in u.REQUIRED if counts[k][0] == 0]
    assert not missed, f"group {group} never takes {missed}"


@pytest.mark.parametrize("group", EMULATED)
def test_the_emulated_windows_alone_take_every_required_branch(census, group):
    """tests/test_quad_emulation_solver_edge.py compares the first EMU_RESTARTS restarts of every n <= 8 entry, and
    tests/test_wide_emulation_solver_edge.py those of every n >= 9 entry on the general solver: those windows alone
    take every required branch, also the ones no status names (rnorm <= 0 against the LDP's dual test, NNLS's
    rejected column, the relaxed x test, the repaired t) and the two on the way to the evaluation cap."""
    counts = census[group + " emu"][1]
    missed = [k for k in u.REQUIRED if counts[k][0] == 0]
    assert not missed, f"the emulated windows of group {group} never take {missed}"


@pytest.mark.parametrize("group", u.GROUPS)
def test_gpu_entries_alone_end_in_every_status(census, group):
    """What the -m gpu tests compare: the entries flagged gpu end in every required way but the two that only occur
    on the way to the evaluation cap -- read off the statuses, which name the ending."""
    seen = collections.Counter()
    for s in u.load_scenarios():
        if s["group"] == group and s["gpu"]:
            seen.update(census[group][0][s["name"]]["status"])
    assert all(seen[st] > 0 for st in (RES_FAILURE, RES_ROUNDOFF, RES_FTOL, RES_XTOL)), dict(seen)


@pytest.mark.parametrize("group", u.GROUPS)
def test_status_mix(census, group):
    results = census[group][0]
    hist = collections.Counter(s for r in results.values() for s in r["status"])
    for st in (RES_FAILURE, RES_ROUNDOFF, RES_FTOL, RES_XTOL):
        assert hist[st] > 0, (group, st, dict(hist))
    assert any(max(r["evals"]) == 1 for r in results.values()), "no scenario ends after exactly one evaluation"


def test_gpu_entries_are_bounded_by_the_oracle(census):
    for s in u.load_scenarios():
        r = census[s["group"]][0][s["name"]]
        if s["gpu"]:
            assert max(r["evals"]) <= u.GPU_MAX_EVALS, (s["name"], max(r["evals"]))
            assert RES_ITER_CAP not in r["status"], s["name"]
        else:
            capped = sum(st == RES_ITER_CAP for st in r["status"])
            assert 1 <= capped <= 4, (s["name"], capped)  # the cap is reached, by few restarts


def test_the_reachable_baseline_takes_none_of_them(census):
    """The gap is real: today's parity inputs (a few thousand restarts) take no required branch.  This also checks
    the branch index of every anchor: the index named has count 0 here while the line's other branch runs."""
    results, counts = census["baseline"]
    assert sum(len(r["status"]) for r in results.values()) >= 3000
    taken = {k: counts[k][0] for k in u.REQUIRED if counts[k][0] != 0}
    assert not taken, f"the baseline takes {taken}: drop those anchors, they are not a gap"
    for k in u.ANCHORS:
        other = counts[k][1]
        if other is not None and not u.NOT_REQUIRED.get(k, "").startswith("taken by"):
            assert other > 0, f"anchor {k!r}: the baseline never executes the line, its branch index is unchecked"
