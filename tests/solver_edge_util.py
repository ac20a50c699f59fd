"""The solver-edge scenario table (tests/golden/generated/solver_edge_scenarios.json, tools/gen_solver_edge_scenarios.py)
and the gcov census of oracle/optik_oracle.c that makes "these inputs reach these branches" a checked fact.

Run as a program it is the census's child process: it loads the coverage build of the oracle (or another build
given to it), runs one group of scenarios, the reachable baseline or one window of one scenario, and writes what
every restart returned; the counters flush when it exits."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "generated", "solver_edge_scenarios.json")
ORACLE_SRC = os.path.join(ROOT, "oracle", "optik_oracle.c")

GROUPS = ("n<=7", "n=8", "n>=9")
RES_ITER_CAP = -100
GPU_MAX_EVALS = 5000  # oracle evaluations per restart a scenario launched on the GPU may need at most
BASELINE_ROBOTS = ("ur3e", "panda", "panda_hand", "ur10", "arm8", "arm10")

# Branches of the oracle named by a source line that occurs exactly once.  `which`: "line" = the line's own execution
# count (the line only runs on the ending in question), or the index of the line's branch in gcov -b's order at -O0
# (the census checks the index against the reachable baseline: that branch has count 0 there, the line's other one not).
ANCHORS = {
    "ldp_rnorm_zero": ("if (rnorm <= 0.0) return 4;", 0),
    "ldp_dual_test": ("if (d1 - 1.0 <= 0.0) return 4;", 0),
    "lsi_singular_E": ("if (!(fabs(E(j, j)) >= EPMACH)) return 5;", 0),
    "lsq_failed": ("if (lmode != 1) return lmode; /* modes 3,4,5: LSQ sub-problem failed */", 0),
    "driver_roundoff": ("case 5: case 6: case 7: ret = OK_RES_ROUNDOFF_LIMITED; break;", "line"),
    "driver_failure": ("case 3: case 4: case 9: ret = OK_RES_FAILURE; break;", "line"),
    "five_resets": ("if (st->ireset > 5) goto L255;", 0),
    "mode8_return": ("return 8;", "line"),
    "mode8_relaxed_ftol": ("if (relstop(st.f0, st.f, 0.0, ftol_abs)) ret = OK_RES_FTOL_REACHED;", "line"),
    "mode8_relaxed_xtol": ("else if (stop_x(n, st.x, st.x0, xtol_abs)) ret = OK_RES_XTOL_REACHED;", "line"),
    "stop_x_zero_step": ("if (zero) return 1;", 0),
    "nnls_reject_column": ("A(npp1, j) = asave;", "line"),
    "nnls_dual_check_fails": ("if (d1 - unorm > 0.0) {", 1),
    "ldl_t_repair": ("if (t >= 0.0) t = EPMACH / sigma;", 0),
    "line_search_nonfinite": ("double a = st->alpha * 0.5;", "line"),
    "evaluation_cap": ("if (nevals >= OK_MAX_EVALS_CAP) { ret = OK_RES_ITER_CAP; break; }", 0),
    "nnls_iter_limit": ("if (iter > itmax) { mode = 3; goto done; }", 0),
    "nnls_empty_set": ("if (nsetp <= 0) { mode = 3; goto done; }", 0),
}
# Printed by the census, never asserted on ("Solver endings off the reachable path", says what was tried):
NOT_REQUIRED = {
    "nnls_iter_limit": "unreached by any input found",
    "nnls_empty_set": "unreached by any input found",
    # the reachable baseline takes these (a restart that stalls on a reachable target also resets five times and
    # ends on the relaxed f test), so they are no gap; the far side of mode 8, the relaxed x test, is one
    "five_resets": "taken by the reachable baseline",
    "mode8_return": "taken by the reachable baseline",
    "mode8_relaxed_ftol": "taken by the reachable baseline",
}
REQUIRED = tuple(k for k in ANCHORS if k not in NOT_REQUIRED)
# Reached only on the way to the evaluation cap, so only by entries the GPU never runs.
CAP_ONLY = ("line_search_nonfinite", "evaluation_cap")
EMU_RESTARTS = 16  # of each entry's range, from its begin: what the host emulations (tests/emu) of the solvers run


def emu_window(sc):
    return sc["restart_begin"], min(sc["restart_end"], sc["restart_begin"] + EMU_RESTARTS)


def load_scenarios():
    with open(TABLE) as fh:
        return json.load(fh)["scenarios"]


def config_kw(sc):
    return {k: (tuple(v) if isinstance(v, list) else v) for k, v in sc["config"].items()}


def ee_pose(oracle, sc):
    e = sc["ee_offset"]
    return oracle.Pose.make(e[:3], e[3:]) if e is not None else None


def oracle_run(oracle, ch, sc, begin=None, end=None, n_threads=4):
    """Every restart of the scenario (or of [begin, end)) on the oracle: ik()'s per_restart dict."""
    begin = sc["restart_begin"] if begin is None else begin
    end = sc["restart_end"] if end is None else end
    return oracle.ik(ch, oracle.make_config(**config_kw(sc)), np.array(sc["target"]), np.array(sc["x0"]), begin, end,
                     n_threads=n_threads, early_exit=False, per_restart=True, ee_offset=ee_pose(oracle, sc))


# ---- the coverage build ---------------------------------------------------------------------------------------

def build_coverage_oracle(workdir):
    """gcc -O0 --coverage, compiled to an object and then linked, so that optik_oracle.gcno / .gcda sit in workdir
    under gcov's default names.  Returns the shared object's path."""
    gcc, gcov = shutil.which("gcc"), shutil.which("gcov")
    assert gcc and gcov, "gcc and gcov are needed for the branch census of the oracle"
    obj, lib = os.path.join(workdir, "optik_oracle.o"), os.path.join(workdir, "liboptik_oracle_cov.so")
    flags = ["-O0", "--coverage", "-fprofile-update=atomic", "-fPIC", "-std=c11", "-ffp-contract=off", "-fno-fast-math",
             "-pthread"]
    subprocess.run([gcc, *flags, "-I", os.path.dirname(ORACLE_SRC), "-c", ORACLE_SRC, "-o", obj], check=True, cwd=workdir)
    subprocess.run([gcc, "--coverage", "-shared", "-o", lib, obj, "-lm", "-lpthread"], check=True, cwd=workdir)
    return lib


def run_census_child(lib, what, workdir, accumulate=False):
    """Runs `what` ("baseline", a group name, or "<group>:emu" / "<group>:rest": the group's emulated windows / all
    its other restarts) in a fresh process on the coverage build; returns (per-scenario results, gcov's lines).  The
    .gcda is removed first, so the counts are this run's alone -- unless `accumulate`: then they add to the last run's."""
    gcda = os.path.join(workdir, "optik_oracle.gcda")
    if os.path.exists(gcda) and not accumulate:
        os.remove(gcda)
    out = os.path.join(workdir, "census_" + re.sub(r"\W", "_", what) + ".json")
    subprocess.run([sys.executable, os.path.abspath(__file__), lib, what, out], check=True, cwd=workdir)
    assert os.path.exists(gcda), "the child left no counters"
    subprocess.run([shutil.which("gcov"), "-b", "-c", "-o", workdir, ORACLE_SRC], check=True, cwd=workdir,
                   stdout=subprocess.DEVNULL)
    with open(os.path.join(workdir, "optik_oracle.c.gcov")) as fh:
        lines = parse_gcov(fh.read())
    with open(out) as fh:
        results = json.load(fh)
    return results, lines


def parse_gcov(text):
    """gcov -b -c text -> {source line stripped: [(execution count, [branch counts])]}."""
    out, cur = {}, None
    for row in text.splitlines():
        m = re.match(r"\s*([0-9]+\*?|-|#####|=====):\s*\d+:(.*)$", row)
        if m:
            c = m.group(1).rstrip("*")
            cur = (int(c) if c.isdigit() else 0, [])
            out.setdefault(m.group(2).strip(), []).append(cur)
            continue
        m = re.match(r"branch\s+\d+\s+(?:taken (\d+)|never executed)", row)
        if m and cur is not None:
            cur[1].append(int(m.group(1) or 0))
    return out


def anchor_counts(lines):
    """{anchor key: (count of the anchored branch, count of the line's other branches or None)}; a missing or
    ambiguous anchor is an error."""
    got = {}
    for key, (text, which) in ANCHORS.items():
        hits = lines.get(text, [])
        assert len(hits) == 1, f"anchor {key!r}: {len(hits)} source lines read {text!r}; exactly one must"
        count, branches = hits[0]
        if which == "line":
            got[key] = (count, None)
        else:
            assert len(branches) == 2, f"anchor {key!r}: gcov reports {len(branches)} branches on {text!r}, not 2"
            got[key] = (branches[which], branches[1 - which])
    return got


def run_mutant_oracle(workdir, text, replacement, name, begin, end):
    """Restarts [begin, end) of scenario `name` on an oracle compiled with the one source line `text` replaced:
    {"status": [...], "evals": [...]}.  In a child process: the test's own oracle stays the real one."""
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to build the oracle"
    with open(ORACLE_SRC) as fh:
        src = fh.read()
    assert src.count(text) == 1, f"{src.count(text)} source lines read {text!r}; exactly one must"
    mutated, lib = os.path.join(workdir, "optik_oracle_mutant.c"), os.path.join(workdir, "liboptik_oracle_mutant.so")
    with open(mutated, "w") as fh:
        fh.write(src.replace(text, replacement))
    subprocess.run([gcc, "-O1", "-fPIC", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-I",
                    os.path.dirname(ORACLE_SRC), "-shared", "-o", lib, mutated, "-lm", "-lpthread"], check=True)
    out = os.path.join(workdir, "mutant.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), lib, f"window:{name}:{begin}:{end}", out], check=True,
                   cwd=workdir)
    with open(out) as fh:
        return json.load(fh)[name]


# ---- the child ------------------------------------------------------------------------------------------------

def _child(lib, what, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import ROBOT_SPECS
    from oracle import binding as ob
    from oracle import urdf_chain
    ob._lib_path = lib  # the coverage build, not liboptik_oracle.so

    def chain(name):
        path, base, ee = ROBOT_SPECS[name]
        with open(path) as fh:
            d = urdf_chain.chain_from_urdf(fh.read(), base, ee)
        return d, ob.make_chain(**d)

    results = {}
    if what == "baseline":
        # today's parity inputs: gpu_util.make_targets (FK of a random in-limit configuration, in-limit seed), the
        # default weights, the three tolerances the parity tests use and an FTOL / XTOL configuration
        from gpu_util import make_targets
        rng = np.random.default_rng(2024)
        for name in BASELINE_ROBOTS:
            d, ch = chain(name)
            tg, x0 = make_targets(ob, d, ch, rng, 4)
            for kw in (dict(tol_f=1e-6), dict(tol_f=1e-8), dict(tol_f=1e-12), dict(tol_f=1e-14, tol_df=1e-10, tol_dx=1e-7)):
                for t in range(4):
                    ref = ob.ik(ch, ob.make_config(**kw), tg[t], x0[t], 0, 48, n_threads=4, early_exit=False,
                                per_restart=True)
                    results[f"{name}/{t}/{sorted(kw.items())}"] = dict(status=ref["status"].tolist(),
                                                                      evals=ref["evals"].tolist())
    elif what.startswith("window:"):
        _, name, b, e = what.split(":")
        sc = next(s for s in load_scenarios() if s["name"] == name)
        ref = oracle_run(ob, chain(sc["robot"])[1], sc, int(b), int(e))
        results[name] = dict(status=ref["status"].tolist(), evals=ref["evals"].tolist())
    else:
        group, _, part = what.partition(":")
        for sc in load_scenarios():
            if sc["group"] != group:
                continue
            b, e = sc["restart_begin"], sc["restart_end"]
            if part == "emu":
                b, e = emu_window(sc)
            elif part == "rest":
                b = emu_window(sc)[1]
            results[sc["name"]] = dict(status=[], evals=[])
            if b < e:
                ref = oracle_run(ob, chain(sc["robot"])[1], sc, b, e)
                results[sc["name"]] = dict(status=ref["status"].tolist(), evals=ref["evals"].tolist())
    with open(out, "w") as fh:
        json.dump(results, fh)


if __name__ == "__main__":
    _child(*sys.argv[1:4])
