"""-m gpu: the solver-edge scenario table (tests/golden/generated/solver_edge_scenarios.json) on every device solver
that can take it, against the CPU oracle run live, bit for bit: the endings no reachable target takes -- FAILURE and
ROUNDOFF_LIMITED from a failed LSQ sub-problem, five Hessian resets and SLSQP mode 8 with its relaxed tests, the
zero-step XTOL, NNLS rejecting columns, bounds active at the solution (tests/test_oracle_solver_edge_census.py shows
with gcov that these inputs reach those branches, and that no restart launched here needs more than 5000
evaluations or meets the evaluation cap).  n <= 7: the solver a launch of that size gets, the quad solver and the
lane-per-restart form; n = 8: default and quad; n >= 9: the three forms of the general solver; n <= 8 again on the
general solver."""
import numpy as np
import pytest

import solver_edge_util as u
from gpu_util import assert_bit_equal, make_targets

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SCENARIOS = {s["name"]: s for s in u.load_scenarios() if s["gpu"]}


def _solvers(n):
    if n <= 7:
        return ["auto", "quad", "lane64", "general"]
    if n == 8:
        return ["auto", "quad", "general"]
    return ["wide0", "wide1", "wide2"]


def _options(solver):
    return {"auto": {}, "quad": dict(solve_kernel="quad"), "lane64": dict(solve_kernel="lane64"),
            "general": dict(solve_kernel="general", wide_form="lds"),
            "wide0": dict(wide_form=0), "wide1": dict(wide_form=1), "wide2": dict(wide_form=2)}[solver]


@pytest.fixture(scope="module")
def hip_chains(chains):
    from optik_amd import device
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return {name: device.HipChain(**chains[name][0]) for name in {s["robot"] for s in SCENARIOS.values()}}


@pytest.fixture(scope="module")
def refs(oracle, chains):
    """The oracle's per-restart results of every scenario, computed once."""
    return {name: u.oracle_run(oracle, chains[s["robot"]][1], s, n_threads=16) for name, s in SCENARIOS.items()}


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _assert_target_equals(out, t, T, R, ref, what):
    """Target t of a [T x R] launch against ik()'s per-restart dict: every restart and the winner."""
    st = out["status"].cpu().numpy().reshape(T, R)[t]
    assert np.array_equal(st, ref["status"]), (what, np.argwhere(st != ref["status"])[:8].ravel(), st[:8], ref["status"][:8])
    assert np.array_equal(out["evals"].cpu().numpy().reshape(T, R)[t], ref["evals"]), what
    assert_bit_equal(out["f"].cpu().numpy().reshape(T, R)[t], ref["fs"], what + " per-restart f")
    assert_bit_equal(out["x"].cpu().numpy()[:, t * R:(t + 1) * R], ref["xs"].T, what + " per-restart x")
    assert int(out["win_idx"].cpu()[t]) == (ref["winner"] if ref["found"] else -1), what
    if ref["found"]:
        assert_bit_equal(out["win_x"].cpu().numpy()[t], ref["x"], what + " winner x")
        assert_bit_equal(out["win_f"].cpu().numpy()[t], ref["f"], what + " winner f")


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_every_restart_and_the_winner_bit_exact_on_every_solver(hip_chains, refs, name):
    from optik_amd import _native as nat
    sc, ref = SCENARIOS[name], refs[name]
    hc = hip_chains[sc["robot"]]
    b, e = sc["restart_begin"], sc["restart_end"]
    print(f"\n{name}: oracle statuses {dict(zip(*np.unique(ref['status'], return_counts=True)))}, "
          f"longest restart {int(ref['evals'].max())} evaluations")
    assert int(ref["evals"].max()) <= u.GPU_MAX_EVALS and u.RES_ITER_CAP not in ref["status"]
    for solver in _solvers(sc["n"]):
        with nat.options(**_options(solver)):
            out = hc.ik_batch(nat.make_config(**u.config_kw(sc)), _dev([sc["target"]]), _dev([sc["x0"]]), b, e,
                              ee_offset7=sc["ee_offset"])
            torch.cuda.synchronize()
        lds = hc.last_launch()["lds_bytes"]
        if solver == "lane64":
            assert lds > 30000, "the lane-per-restart kernel did not run"
        if solver in ("general", "wide0", "wide2"):
            assert lds > 8192, "the general solver's LDS form did not run"
        if solver == "wide1":
            assert lds <= 8192, "the general solver's HBM form did not run"
        _assert_target_equals(out, 0, 1, e - b, ref, f"{name} on {solver}")


MIXED_WAVES = [("panda", ["panda-corner_lb-quality"], 0), ("ur10", ["ur10-corner_ub-speed", "ur10-far-quality"], 7),
               ("arm8", ["arm8-corner_lb-speed", "arm8-far-speed"], 0), ("arm10", ["arm10-corner_ub-quality"], 0),
               ("arm16", ["arm16-corner_zero-speed", "arm16-far-speed"], 0),
               # under the mixed weights most restarts end in FAILURE after a few evaluations, next to a few of the same
               # wave that run for 1800 - 4300 (the restart ranges are chosen from the oracle for that)
               ("panda", ["panda-mixed_weights-speed"], 500), ("ur3e", ["ur3e-mixed_weights-quality"], 500),
               ("arm8", ["arm8-mixed_weights-speed"], 700), ("arm10", ["arm10-mixed_weights-speed"], 0)]


@pytest.mark.parametrize("robot,names,begin", MIXED_WAVES)
def test_edge_and_reachable_targets_share_a_launch(oracle, chains, hip_chains, robot, names, begin):
    """T > 1: the targets of edge scenarios (under the first one's config) interleaved with reachable ones, 100
    restarts each, so waves hold restarts of both: endings that diverge from the neighbours' must not disturb them.
    Under the mixed weights a wave holds restarts that end in FAILURE at once beside ones that run for thousands of
    evaluations."""
    from optik_amd import _native as nat
    d, ch = chains[robot]
    scs = [SCENARIOS[k] for k in names]
    kw = u.config_kw(scs[0])
    assert all(s["ee_offset"] is None for s in scs)
    tg, x0 = make_targets(oracle, d, ch, np.random.default_rng(23), len(scs) + 1)
    tgs, x0s = [tg[0]], [x0[0]]
    for i, s in enumerate(scs):
        tgs += [np.array(s["target"]), tg[i + 1]]
        x0s += [np.array(s["x0"]), x0[i + 1]]
    T, R = len(tgs), 100
    want = [oracle.ik(ch, oracle.make_config(**kw), tgs[t], x0s[t], begin, begin + R, n_threads=8, early_exit=False,
                      per_restart=True) for t in range(T)]
    assert all(int(w["evals"].max()) <= u.GPU_MAX_EVALS and u.RES_ITER_CAP not in w["status"] for w in want)
    if "mixed_weights" in names[0]:
        assert any(int(w["evals"].max()) >= 1000 for w in want) and all((w["status"] == -1).sum() >= 50 for w in want)
    for solver in _solvers(len(d["lb"])):
        for flags in (0, nat.IK_RESTART_MAJOR):
            with nat.options(**_options(solver)):
                out = hip_chains[robot].ik_batch(nat.make_config(**kw), _dev(tgs), _dev(x0s), begin, begin + R,
                                                 flags=flags)
                torch.cuda.synchronize()
            for t in range(T):
                _assert_target_equals(out, t, T, R, want[t], f"{robot} {solver} flags={flags} target {t}")


@pytest.mark.parametrize("name", ["ur3e-big_weights-speed", "panda-corner_lb-quality", "arm8-corner_ub-quality",
                                  "arm10-big_weights-speed", "arm10-corner_ub-quality"])
def test_ik_solutions_returns_the_oracles_set(hip_chains, refs, name):
    """An all-fail scenario gives the empty set, a mixed one the greedy selection over the oracle's successes."""
    from optik_amd import _native as nat
    from test_gpu_ik_solutions import _np, assert_matches, expected_set
    sc, ref = SCENARIOS[name], refs[name]
    b, e = sc["restart_begin"], sc["restart_end"]
    assert (ref["success"].sum() == 0) == ("big_weights" in name)
    for K, min_dist in ((1, 0.0), (8, 1e-3), (16, 0.5)):
        got = _np(hip_chains[sc["robot"]].ik_solutions(nat.make_config(**u.config_kw(sc)), _dev([sc["target"]]),
                                                        _dev([sc["x0"]]), b, e, K, min_dist,
                                                        ee_offset7=sc["ee_offset"]))
        want = expected_set(ref, np.array(sc["x0"]), sc["config"]["solution_mode"] == "quality", K, min_dist, begin=b)
        assert_matches(got, 0, want, K, sc["n"], f"{name} K={K} min_dist={min_dist}")


@pytest.mark.parametrize("mixed,nothing", [("panda-corner_lb-quality", "ur10-far-quality"),
                                           ("arm8-corner_lb-speed", "arm8-far-speed"),
                                           ("arm10-corner_ub-quality", "arm16-far-speed")])
def test_ik_path_carries_the_seed_past_a_waypoint_with_no_success(oracle, chains, hip_chains, mixed, nothing):
    """Waypoints: a corner target (STOPVAL and FTOL mixed), a target at 4 x the reach (every restart ends on FTOL,
    which is no success with tol_df < 0), the corner target again -- solved from the seed the first one left."""
    import math
    from optik_amd import _native as nat
    from test_gpu_ik_path import _linf, _np, assert_path_matches
    sc = SCENARIOS[mixed]
    d, ch = chains[sc["robot"]]
    kw, mode = u.config_kw(sc), sc["config"]["solution_mode"]
    far = np.array(SCENARIOS[nothing]["target"])
    far = np.concatenate([far[:3] / np.linalg.norm(far[:3]) * 50.0, far[3:]])  # (any robot's far target: out of reach)
    tg = np.array([sc["target"], far, sc["target"]])
    b, e = 0, 256
    c = np.array(sc["x0"])
    n, L = len(c), len(tg)
    want = dict(x=np.full((L, n), np.nan), f=np.full(L, np.nan), idx=np.full(L, -1, dtype=np.int64),
                key=np.full(L, np.inf), step=np.full(L, np.nan))
    for w in range(L):
        r = oracle.ik(ch, oracle.make_config(**kw), tg[w], c, b, e, n_threads=8, early_exit=False, per_restart=True)
        assert int(r["evals"].max()) <= u.GPU_MAX_EVALS and u.RES_ITER_CAP not in r["status"]
        cands = []
        for j in np.nonzero(r["success"])[0]:
            key = math.sqrt(sum((float(p) - float(q)) ** 2 for p, q in zip(r["xs"][j], c))) if mode == "quality" \
                else float(b + int(j))
            cands.append((key, b + int(j), int(j)))
        assert bool(cands) == (w != 1)
        if cands:
            key, i, j = min(cands)
            want["x"][w], want["f"][w], want["idx"][w], want["key"][w] = r["xs"][j], r["fs"][j], i, key
            want["step"][w] = _linf(r["xs"][j], c)
            c = np.array(r["xs"][j])
    want["last"] = c
    got = _np(hip_chains[sc["robot"]].ik_path(nat.make_config(**kw), _dev(tg[:, None, :]), _dev([sc["x0"]]), b, e))
    assert_path_matches(got, 0, want, f"{mixed} path")
