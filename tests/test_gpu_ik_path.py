"""-m gpu: warm-started IK along waypoint sequences (optik_hip_ik_path, optik_robot_ik_path, HipChain.ik_path,
Robot.ik_path / ik_paths_arrays).  The expected result is the contract written out in plain Python over the CPU
oracle: per path c = x0; each waypoint is solved from c -- Speed with max_step = inf: the oracle's deterministic
early-exit winner; otherwise the oracle's per-restart results, the successes within max_step of c (L-infinity),
their (key, index) minimum with Quality's key the sqrt of the squared differences to c summed left to right --, and
c becomes the accepted solution if there is one.  x, f, idx, key and step are compared bit for bit."""
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
INF = float("inf")
THREADS = 16


def _linf(a, b):
    d = 0.0
    for u, v in zip(a, b):
        e = abs(float(u) - float(v))
        if e > d:
            d = e
    return d


def expected_path(oracle, ch, mode, tg, x0, begin, end, max_step, ee7):
    """The contract for one path: tg [L, 7], x0 [n] -> dict of x [L, n], f, idx, key, step [L], last [n], and the
    number of successes the step filter rejected."""
    cfg = oracle.make_config(solution_mode=mode)
    ee = oracle.Pose.make(ee7[:3], ee7[3:]) if ee7 is not None else None
    n = len(x0)
    c = np.array(x0, dtype=np.float64)
    L = len(tg)
    out = dict(x=np.full((L, n), np.nan), f=np.full(L, np.nan), idx=np.full(L, -1, dtype=np.int64),
               key=np.full(L, INF), step=np.full(L, np.nan), rejected=0)
    for w in range(L):
        if mode == "speed" and max_step == INF:
            r = oracle.ik(ch, cfg, tg[w], c, begin, end, n_threads=THREADS, early_exit=True, ee_offset=ee)
            win = (float(r["winner"]), int(r["winner"]), r["x"], r["f"]) if r["found"] else None
        else:
            r = oracle.ik(ch, cfg, tg[w], c, begin, end, n_threads=THREADS, early_exit=False, per_restart=True,
                          ee_offset=ee)
            cands = []
            for j in np.nonzero(r["success"])[0]:
                if not _linf(r["xs"][j], c) <= max_step:
                    out["rejected"] += 1
                    continue
                i = begin + int(j)
                if mode == "quality":
                    s = 0.0
                    for u, v in zip(r["xs"][j], c):
                        d = float(u) - float(v)
                        s += d * d
                    key = math.sqrt(s)
                else:
                    key = float(i)
                cands.append((key, i, int(j)))
            win = None
            if cands:
                key, i, j = min(cands)
                win = (key, i, r["xs"][j], r["fs"][j])
        if win is None:
            continue
        key, i, x, f = win
        out["x"][w], out["f"][w], out["idx"][w], out["key"][w] = x, f, i, key
        out["step"][w] = _linf(x, c)
        c = np.array(x, dtype=np.float64)
    out["last"] = c
    return out


def assert_path_matches(got, p, want, what):
    """got: numpy dict of one device call ([L, P] layout); want: expected_path(...) of path p."""
    assert got["idx"][:, p].tolist() == want["idx"].tolist(), what + " idx"
    for k in ("x", "f", "key", "step"):
        assert_bit_equal(got[k][:, p], want[k], f"{what} {k}")
    assert_bit_equal(got["last"][p], want["last"], what + " last")


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


@pytest.fixture(scope="module")
def hip_chains(chains):
    from optik_amd import device
    return {name: device.HipChain(**chains[name][0]) for name in CHAINS + ["gantry"]}


def make_paths(oracle, chains, name, P, L, seed, unreachable=True, spread=0.6, ee7=None):
    """P paths of L waypoints: FK (with the tool offset ee7) of joint configurations interpolated between a random
    start and a nearby end; the middle waypoint of every path unreachable (unless told otherwise).
    -> targets [L, P, 7], x0 [P, n]."""
    d, ch = chains[name]
    ee = oracle.Pose.make(ee7[:3], ee7[3:]) if ee7 is not None else None
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    rng = np.random.default_rng(seed)
    tg = np.empty((L, P, 7))
    x0 = np.empty((P, len(lb)))
    for p in range(P):
        qa = rng.uniform(lb, ub)
        qb = np.clip(qa + rng.uniform(-spread, spread, size=qa.shape), lb, ub)
        for w, s in enumerate(np.linspace(0.0, 1.0, L)):
            tg[w, p] = oracle.fk(ch, (1.0 - s) * qa + s * qb, ee_offset=ee)[1]
        if unreachable and L >= 3:
            tg[L // 2, p] = UNREACHABLE7
        x0[p] = np.clip(qa + rng.uniform(-0.05, 0.05, size=qa.shape), lb, ub)
    return tg, x0


def _check_against_oracle(oracle, chains, hc, name, mode, tg, x0, begin, end, max_step, ee7, what, got=None):
    from optik_amd import _native as nat
    d, ch = chains[name]
    if got is None:
        got = _np(hc.ik_path(nat.make_config(solution_mode=mode), _dev(tg), _dev(x0), begin, end, max_step,
                             ee_offset7=ee7))
    rejected = found = 0
    for p in range(tg.shape[1]):
        want = expected_path(oracle, ch, mode, tg[:, p], x0[p], begin, end, max_step, ee7)
        assert_path_matches(got, p, want, f"{what} path {p}")
        rejected += want["rejected"]
        found += int((want["idx"] >= 0).sum())
    return got, found, rejected


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("mode", ["quality", "speed"])
@pytest.mark.parametrize("max_step", [INF, 0.2])
@pytest.mark.parametrize("with_ee", [False, True])
def test_paths_equal_the_oracle_bit_for_bit(oracle, chains, hip_chains, name, mode, max_step, with_ee):
    P, L, R = 7, 5, 64
    ee7 = EE7 if with_ee else None
    tg, x0 = make_paths(oracle, chains, name, P, L, seed=3, ee7=ee7)
    got, found, rejected = _check_against_oracle(oracle, chains, hip_chains[name], name, mode, tg, x0, 0, R,
                                                 max_step, ee7, f"{name} {mode} max_step={max_step} ee={with_ee}")
    assert found > 0
    assert (got["idx"][L // 2] == -1).all()  # the unreachable waypoint: carried over
    if max_step != INF and name in ("ur3e", "panda", "ur10"):
        assert rejected > 0, "max_step rejected no success: the filter was not exercised"


@pytest.mark.parametrize("mode", ["quality", "speed"])
@pytest.mark.parametrize("P, L, R", [(7, 6, 1), (1, 3, 4096), (300, 3, 16)])
def test_restart_counts_and_path_counts(oracle, chains, hip_chains, mode, P, L, R):
    tg, x0 = make_paths(oracle, chains, "panda", P, L, seed=P + R)
    for max_step in (INF, 0.2) if P < 100 else (INF,):
        _check_against_oracle(oracle, chains, hip_chains["panda"], "panda", mode, tg, x0, 0, R, max_step, None,
                              f"P={P} L={L} R={R} {mode} max_step={max_step}")


def test_speed_path_is_a_host_loop_of_ik_batch_and_of_ik(oracle, chains, hip_chains):
    """Speed, max_step = inf: each waypoint equals HipChain.ik_batch (EARLY_EXIT) seeded from the previous result,
    and Robot.ik with set_parallelism(1), max_time = 0, max_restarts = R."""
    from optik_amd import Robot, SolverConfig
    from optik_amd import _native as nat
    robot = Robot.from_urdf_file(*ROBOT_SPECS["panda"])
    robot.set_parallelism(1)
    lb, ub = (np.array(v) for v in robot.joint_limits())
    rng = np.random.default_rng(12)
    P, L, R = 4, 8, 64
    poses = np.empty((P, L, 4, 4))
    x0 = np.empty((P, 7))
    for p in range(P):
        qa = rng.uniform(lb, ub)
        qb = np.clip(qa + rng.uniform(-0.6, 0.6, size=7), lb, ub)
        for w, s in enumerate(np.linspace(0.0, 1.0, L)):
            poses[p, w] = np.array(robot.fk((1.0 - s) * qa + s * qb))
        poses[p, 3] = np.eye(4)
        poses[p, 3, :3, 3] = 5.0  # unreachable
        x0[p] = qa
    cfg = SolverConfig("speed", max_time=0.0, max_restarts=R)
    x, f, idx, step, found = robot.ik_paths_arrays(cfg, poses, x0)
    assert found.sum() > P * (L - 2) // 2 and not found[:, 3].any()
    for p in range(P):
        c = x0[p]
        single = robot.ik_path(cfg, poses[p], x0[p])
        for w in range(L):
            win = robot.ik(cfg, poses[p, w], c, return_index=True)
            if win is None:
                assert not found[p, w] and idx[p, w] == -1 and single[w] is None
                assert np.isnan(x[p, w]).all() and np.isnan(step[p, w])
                continue
            assert found[p, w] and int(idx[p, w]) == win[2], (p, w)
            assert_bit_equal(x[p, w], win[0], f"path {p} waypoint {w} x")
            assert_bit_equal(f[p, w], win[1], f"path {p} waypoint {w} c")
            assert_bit_equal(single[w][0], win[0], f"path {p} waypoint {w} x (ik_path)")
            assert_bit_equal(step[p, w], _linf(win[0], c), "step")
            c = np.array(win[0])
    # the device form against a host loop of ik_batch on the same chain
    d, ch = chains["panda"]
    hc = hip_chains["panda"]
    tg7, x07 = make_paths(oracle, chains, "panda", 5, 6, seed=40)
    ncfg = nat.make_config(solution_mode="speed")
    got = _np(hc.ik_path(ncfg, _dev(tg7), _dev(x07), 0, R, flags=nat.IK_RESTART_MAJOR))
    c = _dev(x07)
    for w in range(tg7.shape[0]):
        out = _np(hc.ik_batch(ncfg, _dev(tg7[w]), c, 0, R, flags=nat.IK_EARLY_EXIT | nat.IK_RESTART_MAJOR,
                              per_restart=False))
        assert np.array_equal(got["idx"][w], out["win_idx"]), w
        ok = out["win_idx"] >= 0
        for k in ("x", "f"):
            assert_bit_equal(got[k][w], out["win_" + k], f"waypoint {w} {k}")
        assert_bit_equal(got["key"][w][ok], out["win_key"][ok], f"waypoint {w} key")
        assert (got["key"][w][~ok] == INF).all()
        nxt = c.cpu().numpy().copy()
        nxt[ok] = out["win_x"][ok]
        c = _dev(nxt)
    assert_bit_equal(got["last"], c.cpu().numpy(), "last")


def test_solvers_devices_chunks_streams_and_offsets_give_the_same_bits(oracle, chains, hip_chains):
    from optik_amd import Robot, SolverConfig
    from optik_amd import _native as nat
    hc = hip_chains["panda"]
    # a launch large enough that auto picks the lane-per-restart form; every restart runs (Quality)
    tg, x0 = make_paths(oracle, chains, "panda", 256, 2, seed=8, unreachable=False)
    cfg = nat.make_config(solution_mode="quality")
    outs = {}
    for sk in ("auto", "quad", "lane64", "general"):
        with nat.options(solve_kernel=sk):
            outs[sk] = _np(hc.ik_path(cfg, _dev(tg), _dev(x0), 0, 512, 0.5))
            if sk == "auto":
                assert hc.last_launch()["lds_bytes"] > 30000, "auto did not pick the lane-per-restart form"
    assert (outs["auto"]["idx"] >= 0).sum() > 256
    for sk in ("quad", "lane64", "general"):
        assert np.array_equal(outs[sk]["idx"], outs["auto"]["idx"]), sk
        for k in ("x", "f", "key", "step", "last"):
            assert_bit_equal(outs[sk][k], outs["auto"][k], f"{sk} {k}")

    # two devices, and chunks: at R = 4096 a chunk holds 1024 paths, so 1030 paths take two
    one, two = Robot.from_urdf_file(*ROBOT_SPECS["panda"]), Robot.from_urdf_file(*ROBOT_SPECS["panda"])
    two.set_devices([0, 0])
    lb, ub = (np.array(v) for v in one.joint_limits())
    rng = np.random.default_rng(5)
    P, L = 1030, 2
    qa = rng.uniform(lb, ub, size=(P, 7))
    qb = np.clip(qa + rng.uniform(-0.3, 0.3, size=(P, 7)), lb, ub)
    poses = np.array([[one.fk(q) for q in (qa[p], qb[p])] for p in range(P)])
    rcfg = SolverConfig("speed", max_time=0.0, max_restarts=4096)
    a = one.ik_paths_arrays(rcfg, poses, qa)
    b = two.ik_paths_arrays(rcfg, poses, qa)
    assert two.last_parts() == 2
    picks = [0, 1, 514, 515, 1022, 1023, 1024, 1029]
    sub = one.ik_paths_arrays(rcfg, poses[picks], qa[picks])
    for u, v, s, what in zip(a, b, sub, ("x", "c", "idx", "step", "found")):
        assert_bit_equal(v.astype(np.float64), u.astype(np.float64), what + " (two devices)")
        assert_bit_equal(s.astype(np.float64), u[picks].astype(np.float64), what + " (chunked)")
    assert a[4].sum() > P

    # a side stream and an offset restart range, against the oracle
    tg, x0 = make_paths(oracle, chains, "ur10", 3, 5, seed=21, ee7=EE7)
    s = torch.cuda.Stream()
    tgd, x0d = _dev(tg), _dev(x0)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        out = hip_chains["ur10"].ik_path(nat.make_config(solution_mode="quality"), tgd, x0d, 100, 400, 1.0,
                                         ee_offset7=EE7)
    s.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    _check_against_oracle(oracle, chains, None, "ur10", "quality", tg, x0, 100, 400, 1.0, EE7, "side stream",
                          got=got)


def test_ik_batch_and_ik_solutions_after_ik_path_are_unchanged(oracle, chains):
    """ik_path puts the chain's work-item counter and first-success words back: ik_batch and ik_solutions after it,
    on the same chain and stream, give what they give on a fresh chain."""
    from optik_amd import _native as nat
    from optik_amd import device
    d, ch = chains["panda"]
    tg, x0 = make_targets(oracle, d, ch, np.random.default_rng(8), 6)
    tgd, x0d = _dev(tg), _dev(x0)
    ptg, px0 = make_paths(oracle, chains, "panda", 9, 3, seed=9)
    ptgd, px0d = _dev(ptg), _dev(px0)
    speed, quality = nat.make_config(solution_mode="speed"), nat.make_config(solution_mode="quality")
    early = nat.IK_EARLY_EXIT | nat.IK_RESTART_MAJOR

    def calls(hc, interleave):
        res = []
        for cfg, flags in ((speed, early), (quality, 0), (speed, early), (speed, 0)):
            if interleave:
                hc.ik_path(speed, ptgd, px0d, 0, 64)  # (early exit over 9 first-success words)
                hc.ik_path(cfg, ptgd, px0d, 0, 32, 0.3)
            res.append(_np(hc.ik_batch(cfg, tgd, x0d, 0, 300, flags=flags, per_restart=(flags == 0))))
            if interleave:
                hc.ik_path(speed, ptgd, px0d, 0, 64)
            res.append(_np(hc.ik_solutions(cfg, tgd, x0d, 0, 300, 4, 0.1)))
        return res

    alone = calls(device.HipChain(**d), False)
    mixed = calls(device.HipChain(**d), True)
    for a, b in zip(alone, mixed):
        assert a.keys() == b.keys()
        for key in a:
            assert_bit_equal(b[key].astype(np.float64), a[key].astype(np.float64), key)


def test_refusals(hip_chains, chains, oracle):
    import ctypes as C

    from optik_amd import Robot, SolverConfig
    from optik_amd import _native as nat
    cfg = nat.make_config(solution_mode="speed")
    gd = chains["gantry"][0]
    g_tg = _dev(np.array([[[0, 0, 0.5, 0, 0, 0, 1.0]]]))
    with pytest.raises(nat.OptikHipError, match="prismatic"):
        hip_chains["gantry"].ik_path(cfg, g_tg, _dev([(gd["lb"] + gd["ub"]) / 2]), 0, 16)
    gantry = Robot.from_urdf_file(*ROBOT_SPECS["gantry"])
    with pytest.raises(RuntimeError, match="prismatic"):
        gantry.ik_path(SolverConfig(max_time=0.0, max_restarts=16), np.eye(4)[None], (gd["lb"] + gd["ub"]) / 2)
    hc = hip_chains["panda"]
    tg, x0 = make_paths(oracle, chains, "panda", 2, 3, seed=1)
    tgd, x0d = _dev(tg), _dev(x0)
    with pytest.raises(ValueError, match="4096"):
        hc.ik_path(cfg, tgd, x0d, 0, 4097)
    with pytest.raises(ValueError, match="flags"):
        hc.ik_path(cfg, tgd, x0d, 0, 64, flags=nat.IK_EARLY_EXIT | nat.IK_FIND_ANY)
    for ms in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="max_step"):
            hc.ik_path(cfg, tgd, x0d, 0, 64, ms)
    with pytest.raises(ValueError):
        hc.ik_path(cfg, tgd, x0d[:1], 0, 64)
    # the C ABI itself: EUNSUPPORTED for the gantry, EINVAL for FIND_ANY, R > 4096, a bad max_step, P or L of 0
    L = nat.lib()
    o = nat.IkPathOutputs()

    def raw(h, t, x, P, W, e=64, flags=0, ms=INF):
        return L.optik_hip_ik_path(h, C.byref(cfg), C.c_void_p(t.data_ptr()), C.c_void_p(x.data_ptr()), P, W, None,
                                   0, e, flags, 0.0, ms, C.byref(o), None)

    g_x0 = _dev([(gd["lb"] + gd["ub"]) / 2])
    assert raw(hip_chains["gantry"]._h, g_tg, g_x0, 1, 1) == -2  # OPTIK_HIP_EUNSUPPORTED
    for kw in ({"flags": nat.IK_FIND_ANY}, {"flags": nat.IK_EARLY_EXIT | nat.IK_FIND_ANY},
               {"flags": nat.IK_EARLY_EXIT}, {"e": 4097}, {"ms": -1.0}, {"ms": float("nan")}, {"P": 0}, {"W": 0}):
        args = dict(P=2, W=3)
        args.update(kw)
        assert raw(hc._h, tgd, x0d, **args) == -1, kw
    # the robot layer refuses before any device call
    robot = Robot.from_urdf_file(*ROBOT_SPECS["panda"])
    with pytest.raises(ValueError, match="max_restarts"):
        robot.ik_path(SolverConfig("speed", max_time=0.0, max_restarts=4097), np.tile(np.eye(4), (2, 1, 1)),
                      np.zeros(7))


def test_example_prints_the_path():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ik_path.py"),
                          os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"],
                         env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("max_step = ")]
    assert len(lines) == 2, res.stdout
    assert "waypoints solved" in lines[0] and "largest joint step" in lines[1], res.stdout
