"""-m gpu: up to K distinct solutions per target (optik_hip_ik_solutions, optik_robot_ik_solutions,
HipChain.ik_solutions, Robot.ik_solutions[_batch_arrays]).  The expected set is built from the CPU oracle's
per-restart results with the contract's greedy rule written out in plain Python: candidates = the successful
restarts, ordered by (key, index) -- Quality: sqrt of the squared joint differences to the seed summed left to
right, Speed: the index --, a candidate kept if its largest joint difference to every kept one is > min_dist.
Counts, indices, keys, x and f are compared bit for bit."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROBOT_SPECS, ROBOTS, ROOT
from gpu_util import assert_bit_equal, make_targets

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CHAINS = ["ur3e", "panda", "panda_hand", "ur10", "arm8", "arm10"]
EE7 = np.array([0.01, -0.02, 0.05, 0.0, 0.0, math.sin(0.15), math.cos(0.15)])  # a small tool offset
UNREACHABLE7 = np.array([5.0, 5.0, 5.0, 0.0, 0.0, 0.0, 1.0])


def _linf(a, b):
    d = 0.0
    for u, v in zip(a, b):
        e = abs(float(u) - float(v))
        if e > d:
            d = e
    return d


def expected_set(ref, x0, quality, K, min_dist, begin=0):
    """The contract's greedy rule over the oracle's per-restart results: [(index, key, x, f)] in acceptance order."""
    cands = []
    for r in np.nonzero(ref["success"])[0]:
        i = begin + int(r)
        if quality:
            s = 0.0
            for u, v in zip(ref["xs"][r], x0):
                d = float(u) - float(v)
                s += d * d
            key = math.sqrt(s)
        else:
            key = float(i)
        cands.append((key, i, int(r)))
    cands.sort()
    acc = []
    for key, i, r in cands:
        if all(_linf(ref["xs"][r], ref["xs"][a[2]]) > min_dist for a in acc):
            acc.append((key, i, r))
            if len(acc) == K:
                break
    return [(i, key, ref["xs"][r], ref["fs"][r]) for key, i, r in acc]


def assert_matches(got, t, want, K, n, what):
    """got: dict of numpy arrays (count, x, f, idx, key) of one launch; want: expected_set(...) of target t."""
    m = len(want)
    assert int(got["count"][t]) == m, f"{what}: count {int(got['count'][t])} != {m}"
    assert got["idx"][t, :m].tolist() == [w[0] for w in want], what
    assert (got["idx"][t, m:] == -1).all(), what
    if m:
        assert_bit_equal(got["key"][t, :m], np.array([w[1] for w in want]), what + " key")
        assert_bit_equal(got["x"][t, :m], np.array([w[2] for w in want]), what + " x")
        assert_bit_equal(got["f"][t, :m], np.array([w[3] for w in want]), what + " f")
    assert np.isnan(got["x"][t, m:]).all() and np.isnan(got["f"][t, m:]).all(), what
    assert (got["key"][t, m:] == np.inf).all(), what


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


@pytest.fixture(scope="module")
def hip_chains(chains):
    from optik_amd import device
    return {name: device.HipChain(**chains[name][0]) for name in CHAINS + ["gantry"]}


def _targets(oracle, chains, name, T, seed):
    d, ch = chains[name]
    tg, x0 = make_targets(oracle, d, ch, np.random.default_rng(seed), T)
    tg = np.vstack([tg, UNREACHABLE7])
    x0 = np.vstack([x0, (d["lb"] + d["ub"]) / 2])
    return tg, x0


def _oracle_runs(oracle, ch, mode, tg, x0, begin, end, ee7):
    cfg = oracle.make_config(solution_mode=mode)
    ee = oracle.Pose.make(ee7[:3], ee7[3:]) if ee7 is not None else None
    return [oracle.ik(ch, cfg, tg[t], x0[t], begin, end, n_threads=8, early_exit=False, per_restart=True, ee_offset=ee)
            for t in range(len(tg))]


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("mode", ["quality", "speed"])
@pytest.mark.parametrize("with_ee", [False, True])
def test_solution_sets_equal_the_oracle_bit_for_bit(oracle, chains, hip_chains, name, mode, with_ee):
    from optik_amd import _native as nat
    d, ch = chains[name]
    n = len(d["lb"])
    tg, x0 = _targets(oracle, chains, name, 8, seed=11)
    ee7 = EE7 if with_ee else None
    R = 256
    refs = _oracle_runs(oracle, ch, mode, tg, x0, 0, R, ee7)
    assert sum(int(r["success"].sum()) for r in refs[:-1]) > 0 and refs[-1]["success"].sum() == 0
    hc = hip_chains[name]
    cfg = nat.make_config(solution_mode=mode)
    for K in (1, 4, 16):
        for min_dist in (0.0, 1e-3, 0.5):
            got = _np(hc.ik_solutions(cfg, _dev(tg), _dev(x0), 0, R, K, min_dist, ee_offset7=ee7))
            for t in range(len(tg)):
                want = expected_set(refs[t], x0[t], mode == "quality", K, min_dist)
                assert_matches(got, t, want, K, n, f"{name} {mode} ee={with_ee} K={K} min_dist={min_dist} target {t}")


@pytest.mark.parametrize("mode", ["quality", "speed"])
def test_more_than_one_selection_tile(oracle, chains, hip_chains, mode):
    """R = 5000 crosses the 4096-restart tile: the multi-tile rounds (tile kernel + per-target kernel per round)."""
    from optik_amd import _native as nat
    d, ch = chains["panda"]
    tg, x0 = _targets(oracle, chains, "panda", 2, seed=5)
    R = 5000
    refs = _oracle_runs(oracle, ch, mode, tg, x0, 0, R, None)
    for K, min_dist in ((1, 0.0), (16, 0.0), (16, 0.5), (64, 0.2)):
        got = _np(hip_chains["panda"].ik_solutions(nat.make_config(solution_mode=mode), _dev(tg), _dev(x0), 0, R, K,
                                                   min_dist))
        for t in range(len(tg)):
            assert_matches(got, t, expected_set(refs[t], x0[t], mode == "quality", K, min_dist), K, 7,
                           f"R={R} {mode} K={K} min_dist={min_dist} target {t}")


def _robot(name):
    from optik_amd import Robot
    return Robot.from_urdf_file(*ROBOT_SPECS[name])


def _pose_targets(robot, rng, T, unreachable=True):
    lb, ub = (np.array(v) for v in robot.joint_limits())
    tg = [np.array(robot.fk(rng.uniform(lb, ub))) for _ in range(T)]
    if unreachable:
        far = np.eye(4)
        far[:3, 3] = 5.0
        tg.append(far)
    x0 = rng.uniform(lb, ub, size=(len(tg), len(lb)))
    return np.array(tg), x0


@pytest.mark.parametrize("mode", ["quality", "speed"])
def test_k1_is_the_ik_winner(mode):
    """K = 1 returns ik()'s answer bit for bit: Quality with max_restarts = R, max_time = 0; Speed under
    set_parallelism(1) (the lowest successful index)."""
    from optik_amd import SolverConfig
    robot = _robot("panda")
    if mode == "speed":
        robot.set_parallelism(1)
    tg, x0 = _pose_targets(robot, np.random.default_rng(2), 5)
    R = 512
    cfg = SolverConfig(mode, max_time=0.0, max_restarts=R)
    x, c, idx, count = robot.ik_solutions_batch_arrays(cfg, tg, x0, k=1, min_dist=0.1)
    for t in range(len(tg)):
        win = robot.ik(cfg, tg[t], x0[t], return_index=True)
        sols = robot.ik_solutions(cfg, tg[t], x0[t], k=1, min_dist=0.1, return_index=True)
        if win is None:
            assert count[t] == 0 and idx[t, 0] == -1 and sols == []
            continue
        assert count[t] == 1 and int(idx[t, 0]) == win[2] and sols[0][2] == win[2]
        assert_bit_equal(x[t, 0], win[0], "x")
        assert_bit_equal(c[t, 0], win[1], "c")
        assert_bit_equal(sols[0][0], win[0], "x (single)")
    if mode == "quality":
        bx, bc, found = robot.ik_batch_arrays(cfg, tg, x0)
        assert (found == (count == 1)).all()
        assert_bit_equal(x[found, 0], bx[found], "x vs ik_batch_arrays")
        assert_bit_equal(c[found, 0], bc[found], "c vs ik_batch_arrays")
    assert count[-1] == 0  # the unreachable target


def test_solvers_give_the_same_set(hip_chains, chains, oracle):
    """A launch large enough that auto picks the lane-per-restart form: forced quad and lane64 give the same sets."""
    from optik_amd import _native as nat
    d, ch = chains["panda"]
    tg, x0 = make_targets(oracle, d, ch, np.random.default_rng(9), 64)
    hc = hip_chains["panda"]
    cfg = nat.make_config(solution_mode="quality")
    R = 2048
    outs = {}
    for sk in ("auto", "quad", "lane64"):
        with nat.options(solve_kernel=sk):
            outs[sk] = _np(hc.ik_solutions(cfg, _dev(tg), _dev(x0), 0, R, 8, 0.1))
            if sk == "auto":
                assert hc.last_launch()["lds_bytes"] > 30000, "auto did not pick the lane-per-restart form"
    assert outs["auto"]["count"].sum() > 64
    for sk in ("quad", "lane64"):
        for key in ("count", "idx"):
            assert np.array_equal(outs[sk][key], outs["auto"][key]), (sk, key)
        for key in ("x", "f", "key"):
            assert_bit_equal(outs[sk][key], outs["auto"][key], f"{sk} {key}")


def test_devices_and_chunks_do_not_change_the_result():
    from optik_amd import SolverConfig
    rng = np.random.default_rng(4)
    one, two = _robot("panda"), _robot("panda")
    two.set_devices([0, 0])
    tg, x0 = _pose_targets(one, rng, 6)  # T = 7: an odd count over two devices
    cfg = SolverConfig("quality", max_time=0.0, max_restarts=300)
    a = one.ik_solutions_batch_arrays(cfg, tg, x0, k=6, min_dist=0.2)
    b = two.ik_solutions_batch_arrays(cfg, tg, x0, k=6, min_dist=0.2)
    assert two.last_parts() == 2
    for u, v, what in zip(a, b, ("x", "c", "idx", "count")):
        assert_bit_equal(u.astype(np.float64) if what in ("idx", "count") else u,
                         v.astype(np.float64) if what in ("idx", "count") else v, what + " (two devices)")
    # 1.5 M restarts per target: launches of two targets (4 M items at most), so three targets take two launches
    cfg = SolverConfig("speed", max_time=0.0, max_restarts=1_500_000)
    tg3, x03 = tg[:3], x0[:3]
    many = one.ik_solutions_batch_arrays(cfg, tg3, x03, k=5, min_dist=0.3)
    for t in range(3):
        single = one.ik_solutions_batch_arrays(cfg, tg3[t:t + 1], x03[t:t + 1], k=5, min_dist=0.3)
        assert many[3][t] == single[3][0] and many[3][t] == 5
        assert np.array_equal(many[2][t], single[2][0])
        assert_bit_equal(many[0][t], single[0][0], "x (chunked)")
        assert_bit_equal(many[1][t], single[1][0], "c (chunked)")


def test_device_form_on_a_side_stream_with_an_offset_range(oracle, chains, hip_chains):
    from optik_amd import _native as nat
    d, ch = chains["ur10"]
    tg, x0 = _targets(oracle, chains, "ur10", 3, seed=21)
    begin, end = 100, 400
    refs = _oracle_runs(oracle, ch, "quality", tg, x0, begin, end, EE7)
    hc = hip_chains["ur10"]
    s = torch.cuda.Stream()
    tgd, x0d = _dev(tg), _dev(x0)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        out = hc.ik_solutions(nat.make_config(solution_mode="quality"), tgd, x0d, begin, end, 6, 0.05, ee_offset7=EE7)
    s.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for t in range(len(tg)):
        assert_matches(got, t, expected_set(refs[t], x0[t], True, 6, 0.05, begin=begin), 6, 6, f"target {t}")


def test_an_ik_batch_after_ik_solutions_is_unchanged(oracle, chains):
    """The solutions launch leaves the chain's work-item counter (and first-success bookkeeping) as ik_batch expects:
    ik_batch after it, on the same chain and stream, gives what ik_batch gives alone."""
    from optik_amd import _native as nat
    from optik_amd import device
    d, ch = chains["panda"]
    tg, x0 = make_targets(oracle, d, ch, np.random.default_rng(8), 6)
    tgd, x0d = _dev(tg), _dev(x0)
    speed, quality = nat.make_config(solution_mode="speed"), nat.make_config(solution_mode="quality")
    early = nat.IK_EARLY_EXIT | nat.IK_RESTART_MAJOR

    def batches(hc, interleave):
        res = []
        for cfg, flags in ((speed, early), (quality, 0), (speed, early)):
            if interleave:
                hc.ik_solutions(cfg, tgd, x0d, 0, 300, 4, 0.1)
            out = hc.ik_batch(cfg, tgd, x0d, 0, 300, flags=flags, per_restart=(flags == 0))
            res.append(_np(out))
        return res

    alone = batches(device.HipChain(**d), False)
    mixed = batches(device.HipChain(**d), True)
    for a, b in zip(alone, mixed):
        assert a.keys() == b.keys()
        for key in a:
            assert_bit_equal(b[key].astype(np.float64) if b[key].dtype != np.float64 else b[key],
                             a[key].astype(np.float64) if a[key].dtype != np.float64 else a[key], key)


def test_refusals(hip_chains, chains, oracle):
    import ctypes as C

    from optik_amd import SolverConfig
    from optik_amd import _native as nat
    cfg = nat.make_config(solution_mode="quality")
    g = hip_chains["gantry"]
    gd = chains["gantry"][0]
    with pytest.raises(nat.OptikHipError, match="prismatic"):
        g.ik_solutions(cfg, _dev(np.array([[0, 0, 0.5, 0, 0, 0, 1.0]])), _dev([(gd["lb"] + gd["ub"]) / 2]), 0, 16, 4, 0.1)
    gantry = _robot("gantry")
    with pytest.raises(RuntimeError, match="prismatic"):
        gantry.ik_solutions(SolverConfig(max_time=0.0, max_restarts=16), np.eye(4), (gd["lb"] + gd["ub"]) / 2)
    hc = hip_chains["panda"]
    d, ch = chains["panda"]
    tg, x0 = make_targets(oracle, d, ch, np.random.default_rng(1), 2)
    tgd, x0d = _dev(tg), _dev(x0)
    for k, md in ((0, 0.1), (257, 0.1), (4, -1.0), (4, float("nan"))):
        with pytest.raises(ValueError):
            hc.ik_solutions(cfg, tgd, x0d, 0, 64, k, md)
    with pytest.raises(ValueError):
        hc.ik_solutions(cfg, tgd, x0d[:1], 0, 64, 4, 0.1)
    # the C ABI itself refuses them too
    o = nat.IkSolutionsOutputs()
    for k, md in ((0, 0.1), (257, 0.1), (4, -1.0), (4, float("nan"))):
        rc = nat.lib().optik_hip_ik_solutions(hc._h, C.byref(cfg), C.c_void_p(tgd.data_ptr()), C.c_void_p(x0d.data_ptr()),
                                              2, None, 0, 64, 0.0, k, md, C.byref(o), None)
        assert rc == -1, (k, md)
    robot = _robot("panda")
    rcfg = SolverConfig("quality", max_time=0.0, max_restarts=64)
    with pytest.raises(ValueError):
        robot.ik_solutions_batch_arrays(rcfg, np.tile(np.eye(4), (2, 1, 1)), np.zeros((3, 7)))


def test_example_prints_several_solutions():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ik_solutions.py"),
                          os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"],
                         env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("solution ")]
    assert len(lines) >= 2, res.stdout
