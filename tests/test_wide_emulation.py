"""The general solver of the 9 .. 16 joint chains (optik_amd/csrc/ik_wide.hpp) on the CPU.

ik_wide.hpp is compiled for the host as it stands (tests/emu/wide_emu.cpp, the wave emulated by one thread per lane)
and every restart -- status, evaluation count, x, f, selection key -- must equal the C oracle's bit for bit, in all
three forms of the solver: WPG (a restart per lane, lane-strided workspace; partial waves of 4 and 8 lanes with more
restarts than lanes, so lanes refill), WPL (a restart per wave, one lane working) and WPC (the 64 lanes of a wave
working on one restart together).  The same contract tests/test_gpu_wide.py checks on the hardware, available without
one.  The functions behind the wide eval_batch / fk_batch / seed_batch kernels are compared as well.

The cooperative form runs 64 host threads through a barrier at every lane read and __syncthreads(): about 0.15 s per
evaluation of a 10-joint chain.  It therefore runs WPC_RESTARTS restarts per case where the one-lane forms run
RESTARTS / WPL_RESTARTS; nothing else is trimmed."""
import math

import numpy as np
import pytest

from test_quad_emulation import _assert_same, _case

RESTARTS = 24       # per case on WPG (4 and 8 lanes: the lanes refill)
WPL_RESTARTS = 12   # per case on WPL
WPC_RESTARTS = 4    # per case on WPC: restart 0 (the caller's seed) and three drawn configurations
FORMS = [("WPG", 4), ("WPG", 8), ("WPL", 4), ("WPC", 64)]
FORM_IDS = ["WPG-4", "WPG-8", "WPL", "WPC"]


@pytest.fixture(scope="module")
def emu():
    from emu import binding
    binding.build_wide()
    return binding


def key_ref(ref, x0, begin, quality):
    """The selection key of lib.rs:402-407 from the oracle's per-restart record: +inf unless the restart succeeded,
    else its index (Speed) or ||x - x0||_2, the sum formed joint by joint (Quality)."""
    out = np.full(len(ref["status"]), np.inf)
    for r in np.flatnonzero(ref["success"]):
        if quality:
            acc = 0.0
            for a, b in zip(ref["xs"][r].tolist(), np.asarray(x0, dtype=np.float64).tolist()):
                d = a - b
                acc += d * d
            out[r] = math.sqrt(acc)
        else:
            out[r] = float(begin + r)
    return out


def assert_same_with_key(got, ref, n, x0, begin, quality):
    _assert_same(got, ref, n)
    assert np.array_equal(got["key"].view(np.uint64), key_ref(ref, x0, begin, quality).view(np.uint64))


def restarts_of(form):
    return {"WPG": RESTARTS, "WPL": WPL_RESTARTS, "WPC": WPC_RESTARTS}[form]


EE_OFFSET = (0.03, -0.05, 0.08, 0.18257418583505536, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214)
# robot, config, restart_begin, range rule, ee offset: the wide chains, two chains of the tuned solvers' range (the
# general solver serves them under solve_kernel = general; panda_hand has the fixed tip joint), both modes, both
# tolerances, an ee offset, the other reading of rand's inclusive range, a range that does not start at 0, and the
# tol_df / tol_dx pairs of tests/test_gpu_wide.py's test_tight_tolerances_and_other_endings
CASES = {
    "arm9-speed": ("arm9", dict(solution_mode="speed", tol_f=1e-6), 0, 0, None),
    "arm10-quality-tight": ("arm10", dict(solution_mode="quality", tol_f=1e-10), 0, 0, None),
    "arm12-speed-tight-ee": ("arm12", dict(solution_mode="speed", tol_f=1e-10), 0, 0, EE_OFFSET),
    "arm16-quality": ("arm16", dict(solution_mode="quality", tol_f=1e-6), 0, 0, None),
    "ur3e-speed-new_inclusive": ("ur3e", dict(solution_mode="speed", tol_f=1e-6), 0, 1, None),
    "panda_hand-quality-tight": ("panda_hand", dict(solution_mode="quality", tol_f=1e-10), 0, 0, None),
    "arm10-speed-from-1000": ("arm10", dict(solution_mode="speed", tol_f=1e-6), 1000, 0, None),
    "arm10-ftol-xtol": ("arm10", dict(solution_mode="quality", tol_f=0.0, tol_df=1e-18, tol_dx=1e-9), 0, 0, None),
    "arm10-zero-step": ("arm10", dict(solution_mode="quality", tol_f=0.0, tol_df=-1.0, tol_dx=-1.0), 0, 0, None),
}


@pytest.fixture(scope="module")
def references(oracle, chains):
    """case -> (chain dict, target, seed, begin, oracle records of RESTARTS restarts): computed once, shared by the forms."""
    out = {}
    for name, (robot, kw, begin, rule, ee) in CASES.items():
        d, ch, tgt, x0 = _case(oracle, chains, robot, 5)
        ee_pose = oracle.Pose.make(ee[:3], ee[3:]) if ee is not None else None
        with oracle.range_rule(rule):
            ref = oracle.ik(ch, oracle.make_config(**kw), tgt, x0, begin, begin + RESTARTS, n_threads=4,
                            early_exit=False, per_restart=True, ee_offset=ee_pose)
        out[name] = (d, tgt, x0, ref)
    return out


def _head(ref, R):
    return {k: (v[:R] if isinstance(v, np.ndarray) and v.shape[:1] == (RESTARTS,) else v) for k, v in ref.items()}


@pytest.mark.parametrize("form,lanes", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("case", list(CASES))
def test_every_restart_bit_equal_to_the_oracle(emu, references, case, form, lanes):
    from optik_amd import _native as nat
    robot, kw, begin, rule, ee = CASES[case]
    d, tgt, x0, ref = references[case]
    R = restarts_of(form)
    got = emu.wide_solve(d, nat.make_config(**kw), tgt, x0, begin, begin + R, form=form, lanes=lanes, range_rule=rule,
                         ee_offset7=ee)
    assert_same_with_key(got, _head(ref, R), len(d["lb"]), x0, begin, kw["solution_mode"] == "quality")


def test_the_cases_end_in_more_than_one_way(references):
    """What the comparisons above ran: successes and failures, the ftol / xtol endings of the tol_f = 0 cases, and a
    drawn configuration next to the caller's seed within the WPC_RESTARTS restarts of the cooperative form."""
    seen = set()
    for name, (_, _, _, ref) in references.items():
        seen.update(ref["status"].tolist())
    assert {2, 3} <= seen and seen & {4, -1, -4}, seen
    assert 2 not in references["arm10-ftol-xtol"][3]["status"] and 2 not in references["arm10-zero-step"][3]["status"]
    assert WPC_RESTARTS >= 2 and RESTARTS > 8


# ---- the functions behind the wide eval_batch / fk_batch / seed_batch kernels ------------------------------------

WIDE = ["arm9", "arm10", "arm12", "arm16"]
WEIGHTS = {"default": ((1, 1, 1), (1, 1, 1)),
           "reference_test": ((0.0, 5.0, 0.25), (0.005, 1.0, 0.99)),  # tests/test_gradient.rs:37-38
           "identity_quirk": ((1, 0, 0), (1, 1, 1))}


def _configurations(d, rng, B=60):
    n = len(d["lb"])
    return np.vstack([rng.uniform(d["lb"], d["ub"], size=(B, n)), d["lb"], d["ub"], np.zeros(n)])


@pytest.mark.parametrize("robot", WIDE + ["panda_hand"])
@pytest.mark.parametrize("weights", list(WEIGHTS))
def test_objective_and_gradient_bit_exact(emu, oracle, chains, robot, weights):
    from optik_amd import _native as nat
    d, ch = chains[robot]
    wl, wa = WEIGHTS[weights]
    rng = np.random.default_rng(7)
    q = _configurations(d, rng)
    quat = rng.normal(size=4)
    quat /= np.linalg.norm(quat)
    tgt = np.concatenate([rng.uniform(-0.5, 0.5, 3), quat])
    ee_off = None
    if weights == "reference_test":
        eq = rng.normal(size=4)
        eq /= np.linalg.norm(eq)
        ee_off = np.concatenate([rng.uniform(-0.1, 0.1, 3), eq])
    got = emu.wide_ops(d, nat.make_config(linear_weight=wl, angular_weight=wa), target7=tgt, q=q, ee_offset7=ee_off)
    ee_pose = oracle.Pose.make(ee_off[:3], ee_off[3:]) if ee_off is not None else None
    for i in range(len(q)):
        f, g = oracle.eval_fg(ch, tgt, q[i], wl, wa, ee_offset=ee_pose)
        assert np.float64(f).view(np.uint64) == got["f"][i].view(np.uint64), (i, f, got["f"][i])
        assert np.array_equal(g.view(np.uint64), got["g"][i].view(np.uint64)), i


@pytest.mark.parametrize("robot", WIDE + ["panda_hand"])
def test_fk_and_jacobian_bit_exact(emu, oracle, chains, robot):
    from optik_amd import _native as nat
    d, ch = chains[robot]
    q = _configurations(d, np.random.default_rng(3))
    got = emu.wide_ops(d, nat.make_config(), q=q)
    for i in range(len(q)):
        _, ee = oracle.fk(ch, q[i])
        assert np.array_equal(np.asarray(ee).view(np.uint64), got["pose"][i].view(np.uint64)), i
        jr = np.ascontiguousarray(oracle.joint_jacobian(ch, q[i]).T).ravel()  # column-major 6 x n
        assert np.array_equal(jr.view(np.uint64), got["jac"][i].view(np.uint64)), i


@pytest.mark.parametrize("robot", WIDE)
@pytest.mark.parametrize("rule", [0, 1])
def test_restart_seeds_bit_exact(emu, oracle, chains, robot, rule):
    """More than eight joints draw from the second ChaCha8 block of the restart's stream (lib.rs:86-91, 358-370); the
    ranges cross the carry of the stream word's low half (2^32) and lie beyond it."""
    from optik_amd import _native as nat
    d, ch = chains[robot]
    for first, count in ((1, 64), (2**32 - 3, 8), (2**40 + 7, 8)):
        got = emu.wide_ops(d, nat.make_config(), seeds=(first, count), range_rule=rule)["seeds"]
        with oracle.range_rule(rule):
            want = np.array([oracle.restart_seed(ch, i) for i in range(first, first + count)])
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), first
