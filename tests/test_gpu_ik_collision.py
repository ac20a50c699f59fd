"""-m gpu: the collision filter (include/optik_hip.h; csrc/ik_collision.hip, csrc/collision_measure.hpp).

The expected result of a filtered launch is the contract written out over the CPU oracle: the per-restart status and
x of oracle.ik(early_exit=False, per_restart=True), the free flag of every success from collision_batch on its x, and
the winner the (key, index) minimum over the free successes (Speed: the index; Quality: the distance to the seed;
Manipulability: -w from manip_batch).  x, f, index and key are compared bit for bit.  collision_batch itself is
compared bit for bit with the g++-built header applied to link_frames_batch's frames."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from collision_util import build_measure
from conftest import ROBOT_SPECS, ROBOTS, ROOT
from gpu_util import assert_bit_equal, make_targets

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CHAINS = ["panda", "ur10", "arm10"]
EE7 = np.array([0.01, -0.02, 0.05, 0.0, 0.0, math.sin(0.15), math.cos(0.15)])
UNREACHABLE7 = np.array([5.0, 5.0, 5.0, 0.0, 0.0, 0.0, 1.0])
THREADS = 16
MARGIN = 0.01


@pytest.fixture(scope="module")
def measure(tmp_path_factory):
    return build_measure(str(tmp_path_factory.mktemp("collision_measure")))


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _ee(oracle, ee7):
    return oracle.Pose.make(ee7[:3], ee7[3:]) if ee7 is not None else None


def _robot(name):
    from optik_amd import Robot
    return Robot.from_urdf_file(*ROBOT_SPECS[name])


def model_of(name, radius=0.04, per_link=4):
    from optik_amd.collision import auto_pairs, spheres_along_chain
    frames, centers, radii = spheres_along_chain(_robot(name), radius, per_link)
    return dict(frames=frames, centers=centers, radii=radii, self_pairs=auto_pairs(frames), margin=MARGIN)


def world_of(seed, reach=0.8, n_spheres=12, n_boxes=6):
    rng = np.random.default_rng(seed)
    sph = np.concatenate([rng.uniform(-reach, reach, (n_spheres, 3)), rng.uniform(0.04, 0.12, (n_spheres, 1))], 1)
    q = rng.normal(size=(n_boxes, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    box = np.concatenate([rng.uniform(-reach, reach, (n_boxes, 3)), q, rng.uniform(0.03, 0.15, (n_boxes, 3))], 1)
    return sph, box


@pytest.fixture(scope="module")
def filtered(chains):
    """name -> HipChain with a model (spheres along the links, "auto" pairs) and a world of spheres and boxes."""
    from optik_amd import device
    out = {}
    for i, name in enumerate(CHAINS):
        hc = device.HipChain(**chains[name][0])
        hc.set_collision_model(**model_of(name))
        sph, box = world_of(10 + i)
        hc.set_world(sph, box)
        out[name] = hc
    return out


@pytest.fixture(scope="module")
def plain(chains):
    from optik_amd import device
    return {name: device.HipChain(**chains[name][0]) for name in CHAINS + ["gantry"]}


def _np_frames(d, q, ee7):
    """The n + 2 frames as 4x4 matrices, from the chain tables (float64 numpy; a different operation order)."""
    def mat(p):
        i, j, k, w = p[3:]
        m = np.eye(4)
        m[:3, :3] = [[1 - 2 * (j * j + k * k), 2 * (i * j - k * w), 2 * (i * k + j * w)],
                     [2 * (i * j + k * w), 1 - 2 * (i * i + k * k), 2 * (j * k - i * w)],
                     [2 * (i * k - j * w), 2 * (j * k + i * w), 1 - 2 * (i * i + j * j)]]
        m[:3, 3] = p[:3]
        return m
    origins, axes = np.asarray(d["origins"]).reshape(-1, 7), np.asarray(d["axes"]).reshape(-1, 3)
    n = len(q)
    out = [np.eye(4)]
    cur = np.eye(4)
    for j in range(n):
        s, c = math.sin(q[j] / 2), math.cos(q[j] / 2)
        cur = cur @ mat(origins[j]) @ mat(np.concatenate([[0, 0, 0], axes[j] * s, [c]]))
        out.append(cur)
    if len(origins) > n:
        cur = cur @ mat(origins[n])
    if ee7 is not None:
        cur = cur @ mat(ee7)
    out.append(cur)
    return np.array(out)


def _mats(frames7):
    from test_collision_host import _rot
    m = np.zeros(frames7.shape[:-1] + (4, 4))
    for idx in np.ndindex(frames7.shape[:-1]):
        m[idx][:3, :3] = _rot(frames7[idx][3:])
        m[idx][:3, 3] = frames7[idx][:3]
        m[idx][3, 3] = 1.0
    return m


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("with_ee", [False, True])
def test_link_frames_match_fk_batch_and_numpy(chains, plain, name, with_ee):
    d = chains[name][0]
    ee7 = EE7 if with_ee else None
    rng = np.random.default_rng(1)
    B = 2000
    q = rng.uniform(d["lb"], d["ub"], size=(B, len(d["lb"])))
    hc = plain[name]
    fr = hc.link_frames_batch(_dev(q.T), ee_offset7=ee7).cpu().numpy()
    n = len(d["lb"])
    assert fr.shape == (B, n + 2, 7)
    pose = hc.fk_batch(_dev(q.T), ee_offset7=ee7).cpu().numpy().T
    assert_bit_equal(fr[:, n + 1], pose, f"{name} frame n + 1 vs fk_batch")
    assert (fr[:, 0] == [0, 0, 0, 0, 0, 0, 1]).all()
    got = _mats(fr[:50])
    for b in range(50):
        want = _np_frames(d, q[b], ee7)
        assert np.abs(got[b] - want).max() <= 1e-12, (name, b)


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("with_ee", [False, True])
def test_collision_batch_equals_the_header(chains, filtered, measure, name, with_ee):
    d = chains[name][0]
    ee7 = EE7 if with_ee else None
    rng = np.random.default_rng(2)
    B = 3000
    q = rng.uniform(d["lb"], d["ub"], size=(B, len(d["lb"])))
    q[0, 0] = math.nan
    hc = filtered[name]
    fr = hc.link_frames_batch(_dev(q.T), ee_offset7=ee7).cpu().numpy()
    clr, free = (t.cpu().numpy() for t in hc.collision_batch(_dev(q.T), ee_offset7=ee7))
    m = model_of(name)
    sph, box = world_of(10 + CHAINS.index(name))
    want = measure.clearance(fr, m["frames"], m["centers"], m["radii"], m["self_pairs"], sph, box)
    assert_bit_equal(clr, want, f"{name} clearance")
    assert math.isnan(clr[0]) and not free[0]
    assert np.array_equal(free, clr >= MARGIN)
    assert 0.05 < free.mean() < 0.98, free.mean()  # (the world is in the way of some configurations, not all)


def _keys(mode, succ_x, idx, x0, hc, ee7):
    if mode == "speed":
        return idx.astype(np.float64)
    if mode == "quality":
        out = []
        for x in succ_x:
            s = 0.0
            for u, v in zip(x, x0):
                dd = float(u) - float(v)
                s += dd * dd
            out.append(math.sqrt(s))
        return np.array(out)
    w, _ = hc.manip_batch(_dev(np.asarray(succ_x).T), ee_offset7=ee7)
    return -w.cpu().numpy()


def candidates(oracle, hc, ch, mode, tg, x0, begin, end, ee7, free_only=True):
    """[(key, index, x, f)] of the free successes, sorted by (key, index)."""
    r = oracle.ik(ch, oracle.make_config(solution_mode="quality"), tg, x0, begin, end, n_threads=THREADS,
                  early_exit=False, per_restart=True, ee_offset=_ee(oracle, ee7))
    succ = np.nonzero(r["success"])[0]
    if len(succ) == 0:
        return []
    xs = r["xs"][succ]
    _, free = (t.cpu().numpy() for t in hc.collision_batch(_dev(xs.T), ee_offset7=ee7))
    keys = _keys(mode, xs, begin + succ, x0, hc, ee7)
    cands = [(float(keys[k]), begin + int(j), r["xs"][j], r["fs"][j]) for k, j in enumerate(succ)
             if free[k] or not free_only]
    cands.sort(key=lambda t: (t[0], t[1]))
    return cands


def check_batch(oracle, chains, hc, name, mode, tg, x0, begin, end, ee7, what, flags=0):
    from optik_amd import _native as nat
    d, ch = chains[name]
    got = _np(hc.ik_batch(nat.make_config(solution_mode=mode), _dev(tg), _dev(x0), begin, end, flags=flags,
                          ee_offset7=ee7, per_restart=False))
    found = 0
    for t in range(len(tg)):
        cands = candidates(oracle, hc, ch, mode, tg[t], x0[t], begin, end, ee7)
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


def make_case(oracle, chains, name, T, seed, ee7=None):
    d, ch = chains[name]
    tg, x0 = make_targets(oracle, d, ch, np.random.default_rng(seed), T)
    if ee7 is not None:
        rng = np.random.default_rng(seed + 1)
        tg = np.array([oracle.fk(ch, rng.uniform(d["lb"], d["ub"]), ee_offset=_ee(oracle, ee7))[1] for _ in range(T)])
    if T > 2:
        tg[T // 2] = UNREACHABLE7
    return tg, x0


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("mode", ["speed", "quality", "manipulability"])
@pytest.mark.parametrize("with_ee", [False, True])
def test_ik_batch_equals_the_contract(oracle, chains, filtered, name, mode, with_ee):
    from optik_amd import _native as nat
    ee7 = EE7 if with_ee else None
    tg, x0 = make_case(oracle, chains, name, 5, seed=31, ee7=ee7)
    # (Speed with the early-exit flags: they have no effect under the filter)
    flags = nat.IK_EARLY_EXIT | nat.IK_FIND_ANY | nat.IK_RESTART_MAJOR if mode == "speed" else 0
    got, found = check_batch(oracle, chains, filtered[name], name, mode, tg, x0, 0, 64, ee7,
                             f"{name} {mode} ee={with_ee}", flags=flags)
    assert found >= 2 and got["win_idx"][2] == -1


@pytest.mark.parametrize("mode", ["speed", "quality", "manipulability"])
@pytest.mark.parametrize("T, begin, end", [(3, 0, 1), (1, 0, 4096), (4, 100, 164), (300, 0, 16)])
def test_restart_ranges_and_target_counts(oracle, chains, filtered, mode, T, begin, end):
    tg, x0 = make_case(oracle, chains, "panda", T, seed=T + end)
    check_batch(oracle, chains, filtered["panda"], "panda", mode, tg, x0, begin, end, None,
                f"T={T} [{begin}, {end}) {mode}")


def test_a_model_that_cannot_collide_changes_nothing(oracle, chains):
    from optik_amd import _native as nat
    from optik_amd import device
    d, _ = chains["panda"]
    a, b = device.HipChain(**d), device.HipChain(**d)
    m = model_of("panda")
    b.set_collision_model(m["frames"], m["centers"], m["radii"], self_pairs=None, margin=0.0)
    tg, x0 = make_case(oracle, chains, "panda", 64, seed=4)
    for mode in ("quality", "manipulability"):
        cfg = nat.make_config(solution_mode=mode)
        ra = _np(a.ik_batch(cfg, _dev(tg), _dev(x0), 0, 200, per_restart=False))
        rb = _np(b.ik_batch(cfg, _dev(tg), _dev(x0), 0, 200, per_restart=False))
        for k in ra:
            assert_bit_equal(rb[k].astype(np.float64), ra[k].astype(np.float64), f"{mode} {k}")
    # Speed: the lowest-index success -- today's deterministic early-exit winner
    cfg = nat.make_config(solution_mode="speed")
    ra = _np(a.ik_batch(cfg, _dev(tg), _dev(x0), 0, 200, flags=nat.IK_EARLY_EXIT | nat.IK_RESTART_MAJOR,
                        per_restart=False))
    rb = _np(b.ik_batch(cfg, _dev(tg), _dev(x0), 0, 200, flags=nat.IK_EARLY_EXIT | nat.IK_FIND_ANY,
                        per_restart=False))
    assert (ra["win_idx"] >= 0).sum() > 50
    for k in ra:
        assert_bit_equal(rb[k].astype(np.float64), ra[k].astype(np.float64), f"speed {k}")


def test_an_obstacle_on_the_winner_moves_the_answer(oracle, chains):
    from optik_amd import _native as nat
    from optik_amd import device
    d, _ = chains["panda"]
    hc = device.HipChain(**d)
    m = model_of("panda")
    hc.set_collision_model(**m)
    tg, x0 = make_case(oracle, chains, "panda", 1, seed=77)
    cfg = nat.make_config(solution_mode="quality")
    before = _np(hc.ik_batch(cfg, _dev(tg), _dev(x0), 0, 512, per_restart=False))
    assert before["win_idx"][0] >= 0
    xw = before["win_x"][0]
    elbow = hc.link_frames_batch(_dev(xw[:, None]))[0, 4, :3].cpu().numpy()
    hc.set_world(spheres=[np.concatenate([elbow, [0.05]])])
    clr, _ = hc.collision_batch(_dev(xw[:, None]))
    assert clr.item() < MARGIN
    after = _np(hc.ik_batch(cfg, _dev(tg), _dev(x0), 0, 512, per_restart=False))
    assert after["win_idx"][0] >= 0 and after["win_idx"][0] != before["win_idx"][0]
    clr2, free2 = hc.collision_batch(_dev(after["win_x"][0][:, None]))
    assert clr2.item() >= MARGIN and bool(free2.item())
    assert after["win_f"][0] <= 1e-6


def test_ik_solutions_equal_the_contract(oracle, chains, filtered):
    from optik_amd import _native as nat
    d, ch = chains["panda"]
    hc = filtered["panda"]
    K, R, min_dist = 8, 128, 0.1
    tg, x0 = make_case(oracle, chains, "panda", 4, seed=5, ee7=EE7)
    for mode in ("quality", "speed"):
        got = _np(hc.ik_solutions(nat.make_config(solution_mode=mode), _dev(tg), _dev(x0), 0, R, K, min_dist,
                                  ee_offset7=EE7))
        total = 0
        for t in range(len(tg)):
            acc = []
            for key, i, x, f in candidates(oracle, hc, ch, mode, tg[t], x0[t], 0, R, EE7):
                if all(np.max(np.abs(np.asarray(x) - a[2])) > min_dist for a in acc):
                    acc.append((key, i, x, f))
                    if len(acc) == K:
                        break
            c = int(got["count"][t])
            assert c == len(acc), (mode, t)
            total += c
            for s, (key, i, x, f) in enumerate(acc):
                assert int(got["idx"][t, s]) == i
                assert_bit_equal(got["key"][t, s], key, f"{mode} {t} {s} key")
                assert_bit_equal(got["x"][t, s], x, f"{mode} {t} {s} x")
                assert_bit_equal(got["f"][t, s], f, f"{mode} {t} {s} f")
            if c:
                assert np.isfinite(got["key"][t, :c]).all()
                _, free = hc.collision_batch(_dev(got["x"][t, :c].T), ee_offset7=EE7)
                assert bool(free.all())
        assert total >= 4


@pytest.mark.parametrize("max_step", [math.inf, 0.3])
def test_ik_path_through_an_obstacle(oracle, chains, max_step):
    from optik_amd import _native as nat
    from optik_amd import device
    d, ch = chains["panda"]
    hc = device.HipChain(**d)
    hc.set_collision_model(**model_of("panda"))
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    rng = np.random.default_rng(9)
    P, L, R = 3, 5, 64
    tg = np.empty((L, P, 7))
    x0 = np.empty((P, 7))
    mids = []
    for p in range(P):
        qa = rng.uniform(lb, ub)
        qb = np.clip(qa + rng.uniform(-0.5, 0.5, size=7), lb, ub)
        for w, s in enumerate(np.linspace(0.0, 1.0, L)):
            tg[w, p] = oracle.fk(ch, (1.0 - s) * qa + s * qb)[1]
        x0[p] = qa
        mids.append(hc.link_frames_batch(_dev(((qa + qb) / 2)[:, None]))[0, 4, :3].cpu().numpy())
    # an obstacle on each path's straight-line elbow half way
    hc.set_world(spheres=[np.concatenate([m, [0.06]]) for m in mids])
    for mode in ("speed", "quality"):
        got = _np(hc.ik_path(nat.make_config(solution_mode=mode), _dev(tg), _dev(x0), 0, R, max_step))
        for p in range(P):
            c = x0[p].copy()
            for w in range(L):
                cands = [cd for cd in candidates(oracle, hc, ch, mode, tg[w, p], c, 0, R, None)
                         if np.max(np.abs(np.asarray(cd[2]) - c)) <= max_step]
                if not cands:
                    assert got["idx"][w, p] == -1, (mode, p, w)
                    continue
                key, i, x, f = cands[0]
                assert int(got["idx"][w, p]) == i, (mode, p, w)
                assert_bit_equal(got["key"][w, p], key, f"path {p} waypoint {w} key")
                assert_bit_equal(got["x"][w, p], x, f"path {p} waypoint {w} x")
                assert_bit_equal(got["f"][w, p], f, f"path {p} waypoint {w} f")
                assert np.max(np.abs(got["x"][w, p] - c)) <= max_step
                _, free = hc.collision_batch(_dev(got["x"][w, p][:, None]))
                assert bool(free.item())
                c = np.array(x, dtype=np.float64)


def test_robot_surface_agrees(oracle, chains):
    from optik_amd import SolverConfig
    from optik_amd import _native as nat
    from optik_amd import device
    name = "panda"
    d, ch = chains[name]
    m = model_of(name)
    sph, box = world_of(10)
    robots = []
    for devices in (None, [0, 0]):
        r = _robot(name)
        if devices:
            r.set_devices(devices)
        r.set_collision_model(**m)
        r.set_world(sph, box)
        robots.append(r)
    hc = device.HipChain(**d)
    hc.set_collision_model(**m)
    hc.set_world(sph, box)
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    rng = np.random.default_rng(17)
    T, R = 6, 256
    qs = rng.uniform(lb, ub, size=(T, 7))
    poses = np.array([robots[0].fk(q) for q in qs])
    x0 = rng.uniform(lb, ub, size=(T, 7))
    # the robot's clearance and frames are the chain's
    clr_r, free_r = robots[0].collision_clearance_batch_arrays(qs)
    clr_h, free_h = (t.cpu().numpy() for t in hc.collision_batch(_dev(qs.T)))
    assert_bit_equal(clr_r, clr_h, "robot clearance")
    assert np.array_equal(free_r, free_h)
    fr = robots[0].link_frames_batch_arrays(qs)
    assert fr.shape == (T, 9, 4, 4)
    assert_bit_equal(fr[:, 8], np.array([robots[0].fk(q) for q in qs]), "robot frame n + 1 vs fk")
    assert robots[0].collision_clearance(qs[0]) == clr_r[0]
    for mode in ("speed", "quality", "manipulability"):
        cfg = SolverConfig(mode, max_time=0.0, max_restarts=R)
        xs, fs, found = robots[0].ik_batch_arrays(cfg, poses, x0)
        assert found.sum() >= 2
        _, ok = robots[0].collision_clearance_batch_arrays(xs[found])
        assert ok.all(), mode
        for r in robots:
            for par in (0, 1):
                r.set_parallelism(par)
                x2, f2, found2 = r.ik_batch_arrays(cfg, poses, x0)
                assert np.array_equal(found2, found)
                assert_bit_equal(x2, xs, f"{mode} batch par={par}")
                for t in range(T):
                    single = r.ik(cfg, poses[t], x0[t])
                    assert (single is None) == (not found[t])
                    if single is not None:
                        assert_bit_equal(single[0], xs[t], f"{mode} ik target {t} par={par}")
            r.set_parallelism(0)
        # the chain's own winners from the oracle's targets: free as well
        tg7 = np.array([oracle.fk(ch, q)[1] for q in qs])
        got = _np(hc.ik_batch(nat.make_config(solution_mode=mode), _dev(tg7), _dev(x0), 0, R, per_restart=False))
        won = got["win_idx"] >= 0
        assert won.sum() >= 2
        _, ok = hc.collision_batch(_dev(got["win_x"][won].T))
        assert bool(ok.all())
        sols = robots[1].ik_solutions(cfg, poses[0], x0[0], k=6, min_dist=0.1)
        if sols:
            _, ok = robots[1].collision_clearance_batch_arrays(np.array([s[0] for s in sols]))
            assert ok.all()
    path = robots[0].ik_path(SolverConfig("speed", max_time=0.0, max_restarts=64), poses[:3], x0[0], max_step=math.inf)
    xs_ok = [p[0] for p in path if p is not None]
    if xs_ok:
        _, ok = robots[0].collision_clearance_batch_arrays(np.array(xs_ok))
        assert ok.all()


def test_clearing_the_model_restores_todays_bits(oracle, chains):
    from optik_amd import _native as nat
    from optik_amd import device
    d, _ = chains["panda"]
    a, b = device.HipChain(**d), device.HipChain(**d)
    b.set_collision_model(**model_of("panda"))
    b.set_world(*world_of(3))
    tg, x0 = make_case(oracle, chains, "panda", 32, seed=8)
    tgd, x0d = _dev(tg), _dev(x0)
    b.ik_batch(nat.make_config(solution_mode="speed"), tgd, x0d, 0, 128)
    b.clear_collision_model()
    early = nat.IK_EARLY_EXIT | nat.IK_RESTART_MAJOR
    for mode, flags in (("speed", early), ("quality", 0), ("manipulability", 0)):
        cfg = nat.make_config(solution_mode=mode)
        # (per-restart outputs only without early exit: where a restart is abandoned depends on timing)
        ra = _np(a.ik_batch(cfg, tgd, x0d, 0, 300, flags=flags, per_restart=(flags == 0)))
        rb = _np(b.ik_batch(cfg, tgd, x0d, 0, 300, flags=flags, per_restart=(flags == 0)))
        for k in ra:
            assert_bit_equal(rb[k].astype(np.float64), ra[k].astype(np.float64), f"{mode} {k}")
    # Speed's early exit is back: restarts past each target's first success are abandoned (status untouched)
    ha = a.ik_host(nat.make_config(solution_mode="speed"), tg[:1], x0[:1], 0, 4096,
                   flags=nat.IK_EARLY_EXIT | nat.IK_FIND_ANY)
    hb = b.ik_host(nat.make_config(solution_mode="speed"), tg[:1], x0[:1], 0, 4096,
                   flags=nat.IK_EARLY_EXIT | nat.IK_FIND_ANY)
    assert ha["win_idx"][0] >= 0 and hb["win_idx"][0] >= 0


def test_refusals_on_device_paths(chains, plain):
    from optik_amd import _native as nat
    g = plain["gantry"]
    n = len(chains["gantry"][0]["lb"])
    with pytest.raises(nat.OptikHipError, match="prismatic"):
        g.set_collision_model([1], [[0, 0, 0]], [0.1])
    with pytest.raises(nat.OptikHipError, match="prismatic"):
        g.link_frames_batch(_dev(np.zeros((n, 4))))
    with pytest.raises(nat.OptikHipError, match="prismatic"):
        g.collision_batch(_dev(np.zeros((n, 4))))
    g.set_collision_model([], np.zeros((0, 3)), [])  # (S = 0 clears: accepted on any chain)
    hc = plain["panda"]
    for kw in (dict(frames=[9], centers=[[0, 0, 0]], radii=[0.1]),
               dict(frames=[1], centers=[[0, 0, 0]], radii=[-1.0]),
               dict(frames=[1, 4], centers=[[0, 0, 0]] * 2, radii=[0.1, 0.1], self_pairs=[[0, 0]]),
               dict(frames=[1], centers=[[0, 0, 0]], radii=[0.1], margin=-1.0)):
        with pytest.raises(nat.OptikHipError):
            hc.set_collision_model(**kw)
    with pytest.raises(nat.OptikHipError, match="unit quaternion"):
        hc.set_world(boxes=[[0, 0, 0, 0, 0, 0, 2.0, 0.1, 0.1, 0.1]])
    with pytest.raises(ValueError):
        hc.collision_batch(_dev(np.zeros((6, 4))))
    from optik_amd import Robot
    gantry = Robot.from_urdf_file(*ROBOT_SPECS["gantry"])
    with pytest.raises(RuntimeError, match="prismatic"):
        gantry.collision_clearance_batch_arrays(np.zeros((2, gantry.num_positions())))


def test_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ik_collision.py"),
                          os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"],
                         env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    assert "all free: True" in res.stdout, res.stdout
