"""-m gpu: the manipulability and condition solution modes (3 and 4) of optik_hip_ik_batch / _ik_solutions / _ik_path,
Robot.ik / ik_batch_arrays / ik_solutions / ik_path, and optik_hip_manip_batch (HipChain.manip_batch,
Robot.manipulability_batch_arrays).  The expected result is the contract written out over the CPU oracle: the
per-restart results of oracle.ik(early_exit=False, per_restart=True) (they do not depend on the mode when nothing
exits early), each success's Jacobian from oracle.joint_jacobian, scored by the g++-built manip_measure.hpp; the key
is -w (manipulability) or -c (condition), and the winner the (key, index) minimum.  x, f, index and key are
compared bit for bit."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROBOT_SPECS, ROBOTS, ROOT
from gpu_util import assert_bit_equal, make_targets
from manip_util import build_measure

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CHAINS = ["ur3e", "panda", "panda_hand", "arm8", "panda3", "arm10"]
MODES = ["manipulability", "condition"]
EE7 = np.array([0.01, -0.02, 0.05, 0.0, 0.0, math.sin(0.15), math.cos(0.15)])  # a small tool offset
UNREACHABLE7 = np.array([5.0, 5.0, 5.0, 0.0, 0.0, 0.0, 1.0])
INF = float("inf")
THREADS = 16


@pytest.fixture(scope="module")
def measure(tmp_path_factory):
    return build_measure(str(tmp_path_factory.mktemp("manip_measure")))


@pytest.fixture(scope="module")
def hip_chains(chains):
    from optik_amd import device
    return {name: device.HipChain(**chains[name][0]) for name in CHAINS + ["gantry"]}


def _linf(a, b):
    d = 0.0
    for u, v in zip(a, b):
        e = abs(float(u) - float(v))
        if e > d:
            d = e
    return d


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _ee(oracle, ee7):
    return oracle.Pose.make(ee7[:3], ee7[3:]) if ee7 is not None else None


def candidates(oracle, measure, ch, mode, tg, x0, begin, end, ee7):
    """The contract's candidates of one target: [(key, index, x, f)] sorted by (key, index)."""
    cfg = oracle.make_config(solution_mode="quality")
    ee = _ee(oracle, ee7)
    r = oracle.ik(ch, cfg, tg, x0, begin, end, n_threads=THREADS, early_exit=False, per_restart=True, ee_offset=ee)
    succ = np.nonzero(r["success"])[0]
    w, c = measure([oracle.joint_jacobian(ch, r["xs"][j], ee) for j in succ])
    keys = -(c if mode == "condition" else w)
    cands = [(float(keys[k]), begin + int(j), r["xs"][j], r["fs"][j]) for k, j in enumerate(succ)]
    cands.sort(key=lambda t: (t[0], t[1]))
    return cands


def make_case(oracle, chains, name, T, seed, unreachable=True, ee7=None):
    """T reachable targets (FK with the tool offset ee7) and in-limit seeds; the middle one unreachable."""
    d, ch = chains[name]
    tg, x0 = make_targets(oracle, d, ch, np.random.default_rng(seed), T)
    if ee7 is not None:
        rng = np.random.default_rng(seed + 1)
        tg = np.array([oracle.fk(ch, rng.uniform(d["lb"], d["ub"]), ee_offset=_ee(oracle, ee7))[1] for _ in range(T)])
    if unreachable:
        tg[T // 2] = UNREACHABLE7
    return tg, x0


def check_batch(oracle, measure, chains, hc, name, mode, tg, x0, begin, end, ee7, what, got=None):
    from optik_amd import _native as nat
    d, ch = chains[name]
    if got is None:
        got = _np(hc.ik_batch(nat.make_config(solution_mode=mode), _dev(tg), _dev(x0), begin, end, ee_offset7=ee7,
                              per_restart=False))
    found = 0
    for t in range(len(tg)):
        cands = candidates(oracle, measure, ch, mode, tg[t], x0[t], begin, end, ee7)
        if not cands:
            assert got["win_idx"][t] == -1, f"{what} target {t}: a winner where the contract has none"
            continue
        key, i, x, f = cands[0]
        found += 1
        assert int(got["win_idx"][t]) == i, f"{what} target {t} idx"
        assert_bit_equal(got["win_key"][t], key, f"{what} target {t} key")
        assert_bit_equal(got["win_x"][t], x, f"{what} target {t} x")
        assert_bit_equal(got["win_f"][t], f, f"{what} target {t} f")
    return got, found


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("with_ee", [False, True])
def test_ik_batch_equals_the_contract_bit_for_bit(oracle, measure, chains, hip_chains, name, mode, with_ee):
    ee7 = EE7 if with_ee else None
    tg, x0 = make_case(oracle, chains, name, 5, seed=31, ee7=ee7)
    got, found = check_batch(oracle, measure, chains, hip_chains[name], name, mode, tg, x0, 0, 64, ee7,
                             f"{name} {mode} ee={with_ee}")
    assert found >= 2
    assert got["win_idx"][2] == -1  # the unreachable target
    assert (got["win_key"][got["win_idx"] >= 0] <= 0.0).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T, begin, end", [(3, 0, 1), (3, 0, 64), (1, 0, 4096), (4, 100, 164), (300, 0, 16)])
def test_restart_ranges_and_target_counts(oracle, measure, chains, hip_chains, mode, T, begin, end):
    tg, x0 = make_case(oracle, chains, "panda", T, seed=T + end, unreachable=T > 1)
    check_batch(oracle, measure, chains, hip_chains["panda"], "panda", mode, tg, x0, begin, end, None,
                f"T={T} [{begin}, {end}) {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_robot_ik_and_batch_arrays_agree(chains, hip_chains, mode):
    """Robot.ik and Robot.ik_batch_arrays (max_time = 0, max_restarts = R) pick the same restart with the same bits."""
    from optik_amd import Robot, SolverConfig
    robot = Robot.from_urdf_file(*ROBOT_SPECS["ur3e"])
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(17)
    T, R = 6, 128
    poses = np.array([robot.fk(rng.uniform(lb, ub)) for _ in range(T)])
    poses[1] = np.eye(4)
    poses[1, :3, 3] = 5.0
    x0 = rng.uniform(lb, ub, size=(T, 6))
    cfg = SolverConfig(mode, max_time=0.0, max_restarts=R)
    x, f, found = robot.ik_batch_arrays(cfg, poses, x0)
    assert found.sum() >= T - 2 and not found[1]
    w, c = robot.manipulability_batch_arrays(x[found])
    assert (w > 0).all() and (c > 0).all()
    for t in range(T):
        single = robot.ik(cfg, poses[t], x0[t], return_index=True)
        if not found[t]:
            assert single is None
            continue
        assert_bit_equal(single[0], x[t], f"target {t} x")
        assert_bit_equal(single[1], f[t], f"target {t} f")


def expected_set(cands, K, min_dist):
    acc = []
    for key, i, x, f in cands:
        if all(_linf(x, a[2]) > min_dist for a in acc):
            acc.append((key, i, x, f))
            if len(acc) == K:
                break
    return acc


@pytest.mark.parametrize("name", ["panda", "arm10"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("min_dist", [0.2, 0.0])
def test_ik_solutions_take_the_successes_in_key_order(oracle, measure, chains, hip_chains, name, mode, min_dist):
    from optik_amd import _native as nat
    d, ch = chains[name]
    K, R = 8, 64
    tg, x0 = make_case(oracle, chains, name, 4, seed=5, ee7=EE7)
    got = _np(hip_chains[name].ik_solutions(nat.make_config(solution_mode=mode), _dev(tg), _dev(x0), 0, R, K,
                                            min_dist, ee_offset7=EE7))
    total = 0
    for t in range(len(tg)):
        want = expected_set(candidates(oracle, measure, ch, mode, tg[t], x0[t], 0, R, EE7), K, min_dist)
        assert int(got["count"][t]) == len(want), f"target {t} count"
        total += len(want)
        for s, (key, i, x, f) in enumerate(want):
            assert int(got["idx"][t, s]) == i, f"target {t} slot {s} idx"
            assert_bit_equal(got["key"][t, s], key, f"target {t} slot {s} key")
            assert_bit_equal(got["x"][t, s], x, f"target {t} slot {s} x")
            assert_bit_equal(got["f"][t, s], f, f"target {t} slot {s} f")
    assert total >= 4


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("max_step", [INF, 0.2])
def test_ik_path_accepts_the_best_success_within_max_step(oracle, measure, chains, hip_chains, mode, max_step):
    from optik_amd import _native as nat
    d, ch = chains["panda"]
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    rng = np.random.default_rng(9)
    P, L, R = 4, 4, 64
    tg = np.empty((L, P, 7))
    x0 = np.empty((P, 7))
    for p in range(P):
        qa = rng.uniform(lb, ub)
        qb = np.clip(qa + rng.uniform(-0.5, 0.5, size=7), lb, ub)
        for w, s in enumerate(np.linspace(0.0, 1.0, L)):
            tg[w, p] = oracle.fk(ch, (1.0 - s) * qa + s * qb)[1]
        tg[2, p] = UNREACHABLE7
        x0[p] = qa
    got = _np(hip_chains["panda"].ik_path(nat.make_config(solution_mode=mode), _dev(tg), _dev(x0), 0, R, max_step))
    accepted = 0
    for p in range(P):
        c = x0[p].copy()
        for w in range(L):
            cands = [cd for cd in candidates(oracle, measure, ch, mode, tg[w, p], c, 0, R, None)
                     if _linf(cd[2], c) <= max_step]
            if not cands:
                assert got["idx"][w, p] == -1, (p, w)
                continue
            key, i, x, f = cands[0]
            accepted += 1
            assert int(got["idx"][w, p]) == i, (p, w)
            assert_bit_equal(got["key"][w, p], key, f"path {p} waypoint {w} key")
            assert_bit_equal(got["x"][w, p], x, f"path {p} waypoint {w} x")
            assert_bit_equal(got["f"][w, p], f, f"path {p} waypoint {w} f")
            c = np.array(x, dtype=np.float64)
        assert_bit_equal(got["last"][p], c, f"path {p} last")
    assert accepted >= P


def test_solvers_devices_and_streams_give_the_same_bits(oracle, chains, hip_chains):
    from optik_amd import Robot, SolverConfig
    from optik_amd import _native as nat
    d, ch = chains["panda"]
    hc = hip_chains["panda"]
    tg, x0 = make_case(oracle, chains, "panda", 256, seed=44)
    for mode in MODES:
        cfg = nat.make_config(solution_mode=mode)
        outs = {}
        for sk in ("auto", "quad", "lane64", "general"):
            with nat.options(solve_kernel=sk):
                outs[sk] = _np(hc.ik_batch(cfg, _dev(tg), _dev(x0), 0, 256, per_restart=False))
        assert (outs["auto"]["win_idx"] >= 0).sum() > 200
        for sk in ("quad", "lane64", "general"):
            assert np.array_equal(outs[sk]["win_idx"], outs["auto"]["win_idx"]), (mode, sk)
            for k in ("win_x", "win_f", "win_key"):
                assert_bit_equal(outs[sk][k], outs["auto"][k], f"{mode} {sk} {k}")
        # a side stream and an offset range
        s = torch.cuda.Stream()
        tgd, x0d = _dev(tg[:16]), _dev(x0[:16])
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            side = hc.ik_batch(cfg, tgd, x0d, 40, 104, per_restart=False)
        s.synchronize()
        side = {k: v.cpu().numpy() for k, v in side.items()}
        main = _np(hc.ik_batch(cfg, tgd, x0d, 40, 104, per_restart=False))
        for k in ("win_idx", "win_x", "win_f", "win_key"):
            assert_bit_equal(side[k].astype(np.float64), main[k].astype(np.float64), f"{mode} side stream {k}")
    # two devices: the robot splits the targets (and a single call's rounds) over them
    one, two = Robot.from_urdf_file(*ROBOT_SPECS["panda"]), Robot.from_urdf_file(*ROBOT_SPECS["panda"])
    two.set_devices([0, 0])
    lb, ub = (np.array(v) for v in one.joint_limits())
    rng = np.random.default_rng(2)
    poses = np.array([one.fk(rng.uniform(lb, ub)) for _ in range(64)])
    seeds = rng.uniform(lb, ub, size=(64, 7))
    for mode in MODES:
        cfg = SolverConfig(mode, max_time=0.0, max_restarts=300)
        a, b = one.ik_batch_arrays(cfg, poses, seeds), two.ik_batch_arrays(cfg, poses, seeds)
        assert np.array_equal(a[2], b[2])
        assert_bit_equal(b[0], a[0], f"{mode} two devices x")
        assert_bit_equal(b[1], a[1], f"{mode} two devices f")
        big = SolverConfig(mode, max_time=0.0, max_restarts=40000)  # all at once, cut over the devices
        sa, sb = one.ik(big, poses[0], seeds[0], return_index=True), two.ik(big, poses[0], seeds[0], return_index=True)
        assert sa is not None and sa[2] == sb[2]
        assert_bit_equal(sb[0], sa[0], f"{mode} single call on two devices")


@pytest.mark.parametrize("name", CHAINS)
def test_manip_batch_equals_the_header_on_oracle_jacobians(oracle, measure, chains, hip_chains, name):
    d, ch = chains[name]
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    rng = np.random.default_rng(100)
    B = 10000
    q = rng.uniform(lb, ub, size=(B, len(lb)))
    q[0] = 0.0
    plain = None
    for ee7 in (None, EE7):
        ee = _ee(oracle, ee7)
        w_want, c_want = measure([oracle.joint_jacobian(ch, qb, ee) for qb in q])
        if ee7 is None:
            plain = (w_want, c_want)
        w, c = (t.cpu().numpy() for t in hip_chains[name].manip_batch(_dev(q.T), ee_offset7=ee7))
        assert_bit_equal(w, w_want, f"{name} w ee={ee7 is not None}")
        assert_bit_equal(c, c_want, f"{name} c ee={ee7 is not None}")
        if name in ("panda", "panda3"):
            assert w[0] == 0.0 and c[0] == 0.0  # q = 0: an exactly singular Jacobian
        assert (w[1:] > 0).all() and (c[1:] > 0).all() and (c <= 1.0).all()
    # the robot's host-buffer form: the same numbers
    if name in ("panda", "ur3e", "arm10"):
        from optik_amd import Robot
        robot = Robot.from_urdf_file(*ROBOT_SPECS[name])
        rw, rc = robot.manipulability_batch_arrays(q[:300])
        assert_bit_equal(rw, plain[0][:300], f"{name} robot w")
        assert_bit_equal(rc, plain[1][:300], f"{name} robot c")
        assert robot.manipulability(q[5]) == (float(plain[0][5]), float(plain[1][5]))


def test_the_manipulability_winner_is_at_least_as_manipulable(oracle, chains):
    """Panda, 256 targets, R = 256: the manipulability winner's w is >= that of the Quality and Speed winners on
    every target that has a solution, and its residual passes the success test (f <= tol_f)."""
    from optik_amd import Robot, SolverConfig
    robot = Robot.from_urdf_file(*ROBOT_SPECS["panda"])
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(256)
    T, R = 256, 256
    poses = np.array([robot.fk(rng.uniform(lb, ub)) for _ in range(T)])
    seeds = rng.uniform(lb, ub, size=(T, 7))
    res = {m: robot.ik_batch_arrays(SolverConfig(m, max_time=0.0, max_restarts=R), poses, seeds)
           for m in ("manipulability", "quality", "speed", "condition")}
    xm, fm, found = res["manipulability"]
    assert found.sum() > 200
    assert (fm[found] <= 1e-6).all()
    wm, _ = robot.manipulability_batch_arrays(xm[found])
    for other in ("quality", "speed"):
        xo, _, fo = res[other]
        assert np.array_equal(fo, found), other
        wo, _ = robot.manipulability_batch_arrays(xo[found])
        assert (wm >= wo).all(), other
    xc, fc, foundc = res["condition"]
    assert np.array_equal(foundc, found) and (fc[found] <= 1e-6).all()
    _, cc = robot.manipulability_batch_arrays(xc[found])
    _, cm = robot.manipulability_batch_arrays(xm[found])
    assert (cc >= cm).all()


def test_new_modes_leave_speed_and_quality_unchanged(oracle, chains):
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
                for m in MODES:
                    hc.ik_batch(nat.make_config(solution_mode=m), tgd, x0d, 0, 300, per_restart=False)
                    hc.ik_solutions(nat.make_config(solution_mode=m), tgd, x0d, 0, 300, 4, 0.1)
            res.append(_np(hc.ik_batch(cfg, tgd, x0d, 0, 300, flags=flags, per_restart=(flags == 0))))
        return res

    alone = batches(device.HipChain(**d), False)
    mixed = batches(device.HipChain(**d), True)
    for a, b in zip(alone, mixed):
        assert a.keys() == b.keys()
        for key in a:
            assert_bit_equal(b[key].astype(np.float64), a[key].astype(np.float64), key)


def test_refusals(hip_chains, chains):
    from optik_amd import Robot, SolverConfig
    from optik_amd import _native as nat
    g = hip_chains["gantry"]
    gd = chains["gantry"][0]
    for m in MODES:
        with pytest.raises(nat.OptikHipError, match="prismatic"):
            g.ik_batch(nat.make_config(solution_mode=m), _dev(np.array([[0, 0, 0.5, 0, 0, 0, 1.0]])),
                       _dev([(gd["lb"] + gd["ub"]) / 2]), 0, 16)
    with pytest.raises(nat.OptikHipError, match="prismatic"):
        g.manip_batch(_dev(np.zeros((len(gd["lb"]), 4))))
    gantry = Robot.from_urdf_file(*ROBOT_SPECS["gantry"])
    with pytest.raises(RuntimeError, match="prismatic"):
        gantry.manipulability_batch_arrays(np.zeros((2, gantry.num_positions())))
    with pytest.raises(ValueError):
        hip_chains["panda"].manip_batch(_dev(np.zeros((6, 4))))


def test_example_solves_in_all_four_modes():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ik_modes.py"),
                          os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"],
                         env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.split(" ")[0] in ("quality", "speed", "manipulability",
                                                                          "condition")]
    assert len(lines) == 4, res.stdout
