"""-m gpu: the motion check (include/optik_hip.h; csrc/ik_motion.hip, csrc/motion_measure.hpp).

collision_motion_batch is compared bit for bit with its own definition by composition: every segment's samples are
generated on the host with numpy in the documented order, sent through collision_batch, and reduced per segment on the
host (minimum, all, lowest non-free k, count).

ik_path with the check on is compared bit for bit with the contract written out over the CPU oracle's per-restart
results: the collision filter (collision_batch on each success), then the motion filter from the carried seed -- the
samples from numpy, their frames from link_frames_batch, the reduction by the g++-built header (motion_util) -- then
max_step, the (key, index) minimum, and the carry."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROBOT_SPECS, ROBOTS, ROOT
from gpu_util import assert_bit_equal
from motion_util import build_motion, np_reduce, np_samples

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EE7 = np.array([0.01, -0.02, 0.05, 0.0, 0.0, math.sin(0.15), math.cos(0.15)])
THREADS = 16
MARGIN = 0.01


@pytest.fixture(scope="module")
def motion(tmp_path_factory):
    return build_motion(str(tmp_path_factory.mktemp("motion_measure")))


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _robot(name):
    from optik_amd import Robot
    return Robot.from_urdf_file(*ROBOT_SPECS[name])


def model_of(name, pairs=True, margin=MARGIN):
    from optik_amd.collision import auto_pairs, spheres_along_chain
    if name == "panda1":  # (one joint: no segment long enough for spheres_along_chain) a sphere off the joint's axis
        return dict(frames=np.array([1], dtype=np.int32), centers=np.array([[0.3, 0.0, 0.1]]), radii=np.array([0.05]),
                    self_pairs=None, margin=margin)
    frames, centers, radii = spheres_along_chain(_robot(name), 0.04, 4)
    return dict(frames=frames, centers=centers, radii=radii, self_pairs=auto_pairs(frames) if pairs else None,
                margin=margin)


def path_model(name):
    from optik_amd.collision import auto_pairs, spheres_along_chain
    frames, centers, radii = spheres_along_chain(_robot(name), 0.025, 4)
    return dict(frames=frames, centers=centers, radii=radii, self_pairs=auto_pairs(frames), margin=MARGIN)


def world_of(seed, reach=0.8, n_spheres=12, n_boxes=6):
    rng = np.random.default_rng(seed)
    sph = np.concatenate([rng.uniform(-reach, reach, (n_spheres, 3)), rng.uniform(0.04, 0.12, (n_spheres, 1))], 1)
    q = rng.normal(size=(n_boxes, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    box = np.concatenate([rng.uniform(-reach, reach, (n_boxes, 3)), q, rng.uniform(0.03, 0.15, (n_boxes, 3))], 1)
    return sph, box


def compose(hc, qa, qb, h, ee7=None):
    """The definition, by composition: (clearance, free, first, steps) of every segment from collision_batch on the
    numpy samples."""
    B = len(qa)
    Ks, parts = [], []
    for b in range(B):
        _, K, s = np_samples(qa[b], qb[b], h)
        Ks.append(K)
        if K >= 1:
            parts.append(s)
    allq = np.concatenate(parts) if parts else np.zeros((0, qa.shape[1]))
    if len(allq):
        c, _ = hc.collision_batch(_dev(allq.T), ee_offset7=ee7)
        c = c.cpu().numpy()
    else:
        c = np.zeros(0)
    margin = hc._test_margin
    out, o = [], 0
    for K in Ks:
        if K < 1:
            out.append(np_reduce(K, None, margin))
            continue
        out.append(np_reduce(K, c[o:o + K + 1], margin))
        o += K + 1
    clr = np.array([r[0] for r in out])
    return clr, np.array([r[1] for r in out]), np.array([r[2] for r in out]), np.array([r[3] for r in out])


def make_segments(d, B, seed):
    """Segment lengths mixed within one call: d = 0, a few hundredths of a radian, about a radian, and (with h = 0.001)
    thousands of steps; two segments over the limit and one with a NaN."""
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    n = len(lb)
    rng = np.random.default_rng(seed)
    qa = rng.uniform(lb, ub, (B, n))
    scale = rng.choice([0.0, 0.004, 0.03, 0.3, 1.5], size=(B, 1), p=[0.05, 0.15, 0.2, 0.35, 0.25])
    qb = np.clip(qa + rng.uniform(-1.0, 1.0, (B, n)) * scale, lb, ub)
    return qa, qb


def sphere_point(hc, model, q, ee7=None):
    """Where the model's last sphere is at configuration q (from link_frames_batch)."""
    f7 = hc.link_frames_batch(_dev(np.asarray(q)[:, None]), ee_offset7=ee7)[0, int(model["frames"][-1])].cpu().numpy()
    i, j, k, w = f7[3:]
    Rm = np.array([[1 - 2 * (j * j + k * k), 2 * (i * j - k * w), 2 * (i * k + j * w)],
                   [2 * (i * j + k * w), 1 - 2 * (i * i + k * k), 2 * (j * k - i * w)],
                   [2 * (i * k - j * w), 2 * (j * k + i * w), 1 - 2 * (i * i + j * j)]])
    return f7[:3] + Rm @ np.asarray(model["centers"][-1])


def chain_with(chains, name, world=True, pairs=True, margin=MARGIN, seed=21):
    from optik_amd import device
    hc = device.HipChain(**chains[name][0])
    hc.set_collision_model(**model_of(name, pairs, margin))
    if world:
        hc.set_world(*world_of(seed))
    hc._test_margin = margin
    return hc


# The scene: spheres of 4 cm along the links (panda1: one sphere off the axis), a margin of 1 cm, 12 spheres and 6
# boxes of 3 .. 15 cm inside the reach -- the world of the collision filter's tests, where a tenth to a half of the
# random configurations are in collision.  Segments of a few hundredths of a radian mostly stay on one side of every
# obstacle (free), those of a radian mostly do not; h = 0.001 makes the long ones thousands of steps.  The assertions
# on the mix below are taken from the composed expectation.
@pytest.mark.parametrize("name, B, h", [("panda", 700, 0.001), ("ur10", 300, 0.004), ("arm10", 300, 0.004),
                                        ("arm16", 130, 0.01), ("panda1", 300, 0.002)])
def test_motion_batch_equals_the_composition(chains, name, B, h):
    d = chains[name][0]
    hc = chain_with(chains, name)
    qa, qb = make_segments(d, B, seed=len(name) + B)
    if name == "panda":
        # How the scene was picked: in this world the free space is so well connected that only about one random
        # segment in 60 is blocked between two free ends.  So the segments are drawn from a pool of 20000: the composed
        # expectation at a coarser resolution names the pool's segments of that kind, a hundred of them are taken,
        # and the other 600 are the pool's first ones of any other kind.
        pa, pb = make_segments(d, 20000, seed=77)
        pool = compose(hc, pa, pb, 0.01, EE7)
        ends, _ = hc.collision_batch(_dev(np.concatenate([pa, pb]).T), ee_offset7=EE7)
        ends = ends.cpu().numpy() >= MARGIN
        kind = ends[:20000] & ends[20000:] & ~pool[1] & (pool[3] > 0)
        some = np.nonzero(kind)[0][:100]
        pick = np.sort(np.concatenate([some, np.nonzero(~kind)[0][:B - len(some)]]))
        qa, qb = pa[pick].copy(), pb[pick].copy()
        assert len(qa) == B
    qb[3] = qa[3]                                  # d = 0
    if name == "panda":
        qa[5] = d["lb"]; qb[5] = d["ub"]           # over the limit at h = 0.001
        qb[6, 2] = math.nan
        ee7 = EE7
    else:
        ee7 = None
    want = compose(hc, qa, qb, h, ee7)
    got = hc.collision_motion_batch(_dev(qa.T), _dev(qb.T), h, ee_offset=ee7)
    got = [t.cpu().numpy() for t in got]
    cls = hc.collision_motion_batch(_dev(qa.T), _dev(qb.T), h, ee_offset=ee7, clearance=False)
    assert cls[0] is None
    cls = [t.cpu().numpy() for t in cls[1:]]
    print(f"{name}: B {B} samples {int((want[3][want[3] > 0] + 1).sum())} free {want[1].mean():.3f} "
          f"max K {want[3].max()} first max {want[2].max()}")
    assert_bit_equal(got[0], want[0], f"{name} clearance")
    for k, what in ((1, "free"), (2, "first"), (3, "steps")):
        assert np.array_equal(got[k], want[k]), (name, what, np.nonzero(got[k] != want[k])[0][:10])
        assert np.array_equal(cls[k - 1], want[k]), (name, "classify-only " + what)
    assert B % 256 != 0 and want[3][3] == 1
    if name == "panda":
        assert want[3][5] == -1 and want[3][6] == -1 and math.isnan(got[0][5]) and not got[1][5] and got[2][6] == -1
        assert want[3].max() > 1000
        # not vacuous (from the composition): free ones, blocked ones whose endpoints are both free, a deep first
        ends, _ = hc.collision_batch(_dev(np.concatenate([qa, qb]).T), ee_offset7=ee7)
        ends = ends.cpu().numpy() >= MARGIN
        both = ends[:B] & ends[B:]
        assert want[1].mean() >= 0.1, want[1].mean()
        assert (both & ~want[1] & (want[3] > 0)).mean() >= 0.1, (both & ~want[1]).mean()
        assert (want[2] > 64).any()


@pytest.mark.parametrize("world, pairs, margin", [(False, True, MARGIN), (True, False, 0.0), (False, False, 0.0)])
def test_motion_batch_without_world_or_pairs(chains, world, pairs, margin):
    d = chains["panda"][0]
    hc = chain_with(chains, "panda", world, pairs, margin)
    qa, qb = make_segments(d, 257, seed=3)
    want = compose(hc, qa, qb, 0.01)
    got = [t.cpu().numpy() for t in hc.collision_motion_batch(_dev(qa.T), _dev(qb.T), 0.01)]
    assert_bit_equal(got[0], want[0], "clearance")
    for k in (1, 2, 3):
        assert np.array_equal(got[k], want[k]), k
    if not world and not pairs:
        assert (got[0] == math.inf).all() and got[1].all()


def test_runs_of_segments_without_samples(chains):
    """300 segments in a row that are not sampled (a NaN joint), between sampled ones: the chunks that straddle the run
    span more segments than the kernel's LDS window holds and take its other path -- the search in global memory and the
    global minima -- in the clearance form and in the classify-only form."""
    d = chains["panda"][0]
    hc = chain_with(chains, "panda")
    qa, qb = make_segments(d, 700, seed=9)
    qb[100:400, 1] = math.nan
    qb[450:600:2, 0] = math.inf       # and an alternating stretch
    want = compose(hc, qa, qb, 0.01)
    assert (want[3][100:400] == -1).all() and (want[3][:100] > 0).all() and 0.05 < want[1].mean() < 0.95
    got = [t.cpu().numpy() for t in hc.collision_motion_batch(_dev(qa.T), _dev(qb.T), 0.01)]
    assert_bit_equal(got[0], want[0], "clearance")
    for k in (1, 2, 3):
        assert np.array_equal(got[k], want[k]), k
    cls = [t.cpu().numpy() for t in hc.collision_motion_batch(_dev(qa.T), _dev(qb.T), 0.01, clearance=False)[1:]]
    for k in (1, 2, 3):
        assert np.array_equal(cls[k - 1], want[k]), k


def test_motion_batch_without_a_model(chains):
    from optik_amd import device
    d = chains["panda"][0]
    hc = device.HipChain(**d)
    qa, qb = make_segments(d, 100, seed=4)
    qb[7, 0] = math.inf
    clr, free, first, steps = (t.cpu().numpy() for t in hc.collision_motion_batch(_dev(qa.T), _dev(qb.T), 0.01))
    ok = np.arange(100) != 7
    assert (clr[ok] == math.inf).all() and free[ok].all() and (first == -1).all()
    assert math.isnan(clr[7]) and not free[7] and steps[7] == -1
    assert np.array_equal(steps[ok], [np_samples(a, b, 0.01)[1] for a, b in zip(qa[ok], qb[ok])])


# ---- ik_path ---------------------------------------------------------------------------------------------------
def _keys(mode, xs, idx, x0, hc, ee7):
    if mode == "speed":
        return idx.astype(np.float64)
    if mode == "quality":
        out = []
        for x in xs:
            s = 0.0
            for u, v in zip(x, x0):
                dd = float(u) - float(v)
                s += dd * dd
            out.append(math.sqrt(s))
        return np.array(out)
    w, _ = hc.manip_batch(_dev(np.asarray(xs).T), ee_offset7=ee7)
    return -w.cpu().numpy()


def contract_path(oracle, ch, hc, motion, model, world, mode, tg, x0, R, max_step, h, ee7, check):
    """The waypoints of every path as the contract gives them: [(idx, key, x, f, step) or None][L][P] (step: the
    L-infinity distance of x to the seed the waypoint was solved from), and the last seeds."""
    L, P = tg.shape[:2]
    ee = oracle.Pose.make(ee7[:3], ee7[3:]) if ee7 is not None else None
    seeds = x0.copy()
    out = []
    cfgq = oracle.make_config(solution_mode="quality")
    for w in range(L):
        cands = []  # (p, key, index, x, f)
        for p in range(P):
            r = oracle.ik(ch, cfgq, tg[w, p], seeds[p], 0, R, n_threads=THREADS, early_exit=False, per_restart=True,
                          ee_offset=ee)
            succ = np.nonzero(r["success"])[0]
            if len(succ) == 0:
                continue
            keys = _keys(mode, r["xs"][succ], succ, seeds[p], hc, ee7)
            cands += [(p, float(keys[k]), int(j), r["xs"][j], r["fs"][j]) for k, j in enumerate(succ)]
        keep = np.zeros(len(cands), dtype=bool)
        if cands:
            xs = np.array([c[3] for c in cands])
            _, free = hc.collision_batch(_dev(xs.T), ee_offset7=ee7)
            keep = free.cpu().numpy().copy()
            within = np.array([np.max(np.abs(c[3] - seeds[c[0]])) <= max_step for c in cands])
            if check:
                todo = np.nonzero(keep & within)[0]
                Ks, frs = [], []
                for i in todo:
                    _, K, s = np_samples(seeds[cands[i][0]], cands[i][3], h)
                    Ks.append(K)
                    frs.append(hc.link_frames_batch(_dev(s.T), ee_offset7=ee7).cpu().numpy() if K >= 1 else None)
                if len(todo):
                    _, mfree, _, _ = motion.reduce(Ks, frs, model["margin"], model["frames"], model["centers"],
                                                   model["radii"], model["self_pairs"], world[0], world[1])
                    keep[todo] &= mfree
            keep &= within
        row = [None] * P
        for i in np.nonzero(keep)[0]:
            p, key, j, x, f = cands[i]
            if row[p] is None or (key, j) < (row[p][1], row[p][0]):
                row[p] = (j, key, x, f)
        for p in range(P):
            if row[p] is not None:
                row[p] = row[p] + (float(np.max(np.abs(np.asarray(row[p][2]) - seeds[p]))),)
                seeds[p] = row[p][2]
        out.append(row)
    return out, seeds


def wall_scene(oracle, chains, hc_base, name, model, P, L, seed, spread):
    """P paths of L waypoints (FK of a joint-space line, out and back), every waypoint's own configuration free in the
    base world of hc_base, and for every path whose outermost model sphere travels more than 9 cm between waypoints
    L/4 and L/4 + 1 a wall of 8 mm across that move: thinner than the travel, and far enough from both waypoints."""
    d, ch = chains[name]
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    n = len(lb)
    rng = np.random.default_rng(seed)
    tg, x0, walls = np.empty((L, P, 7)), np.empty((P, n)), []
    half = L // 2
    # (out and back: the waypoints beyond the wall are followed by waypoints on the seed's side again, so a path that
    # loses the crossing has something to go on with from its old seed)
    ss = [w / half if w <= half else (L - w) / half for w in range(L)]
    for p in range(P):
        for _ in range(200):
            qa = rng.uniform(lb, ub)
            qb = np.clip(qa + rng.uniform(-spread, spread, n), lb, ub)
            qs = np.array([(1.0 - s) * qa + s * qb for s in ss])
            if bool(hc_base.collision_batch(_dev(qs.T))[1].all()):
                break
        for w in range(L):
            tg[w, p] = oracle.fk(ch, qs[w])[1]
        x0[p] = qa
        a, b = sphere_point(hc_base, model, qs[L // 4]), sphere_point(hc_base, model, qs[L // 4 + 1])
        u = b - a
        travel = np.linalg.norm(u)
        if travel < 0.09:
            continue
        u /= travel
        # the quaternion turning x onto u
        q = np.concatenate([np.cross([1.0, 0, 0], u), [1.0 + u[0]]])
        if np.linalg.norm(q) < 1e-9:
            q = np.array([0.0, 0, 1, 0])
        q /= np.linalg.norm(q)
        walls.append(np.concatenate([(a + b) / 2, q, [0.004, 0.1, 0.1]]))
    return tg, x0, np.array(walls)


def _compare(got, want, seeds, what):
    L, P = got["idx"].shape
    for w in range(L):
        for p in range(P):
            r = want[w][p]
            if r is None:
                assert got["idx"][w, p] == -1, (what, w, p)
                assert math.isinf(got["key"][w, p]) and math.isnan(got["step"][w, p]) and np.isnan(got["x"][w, p]).all()
                continue
            assert int(got["idx"][w, p]) == r[0], (what, w, p)
            assert_bit_equal(got["key"][w, p], r[1], f"{what} key {w} {p}")
            assert_bit_equal(got["x"][w, p], r[2], f"{what} x {w} {p}")
            assert_bit_equal(got["f"][w, p], r[3], f"{what} f {w} {p}")
            assert_bit_equal(got["step"][w, p], r[4], f"{what} step {w} {p}")
    assert_bit_equal(got["last"], seeds, f"{what} last")


@pytest.mark.parametrize("name, mode, max_step", [("panda", "speed", math.inf), ("panda", "quality", 0.6),
                                                  ("panda", "manipulability", 0.6), ("arm10", "quality", math.inf)])
def test_ik_path_equals_the_contract(oracle, chains, motion, name, mode, max_step):
    from optik_amd import _native as nat
    from optik_amd import device
    d, ch = chains[name]
    P, L, R, h = 64, 8, 24, 0.05
    plain = device.HipChain(**d)
    # (spheres of 2.5 cm: a wall of 8 mm between two waypoints 9 cm apart leaves both of them free)
    model = path_model(name)
    sph, box = world_of(33, n_spheres=6, n_boxes=2)
    hc = device.HipChain(**d)
    hc.set_collision_model(**model)
    hc.set_world(sph, box)
    tg, x0, walls = wall_scene(oracle, chains, hc, name, model, P, L, seed=40, spread=1.2)
    assert len(walls) >= P // 8
    world = (sph, np.concatenate([box, walls]))
    hc.set_world(*world)
    cfg = nat.make_config(solution_mode=mode)
    args = (oracle, ch, hc, motion, model, world, mode, tg, x0, R, max_step, h, None)
    off, off_seeds = contract_path(*args, check=False)
    on, on_seeds = contract_path(*args, check=True)
    # the scene does something (from the contract side): an accepted solution that the check changes, and a path that
    # loses a waypoint to the check and goes on from its old seed
    differ = sum(1 for w in range(L) for p in range(P)
                 if (off[w][p] is None) != (on[w][p] is None) or (on[w][p] and off[w][p][0] != on[w][p][0]))
    lost = [(w, p) for w in range(L) for p in range(P) if on[w][p] is None and off[w][p] is not None]
    goes_on = [(w, p) for w, p in lost if any(on[v][p] is not None for v in range(w + 1, L))]
    print(f"{name} {mode} {max_step}: differ {differ} lost {len(lost)} go on {len(goes_on)} "
          f"found on {sum(r is not None for row in on for r in row)} off {sum(r is not None for row in off for r in row)}")
    assert differ >= 1 and len(goes_on) >= 1
    got_off = _np(hc.ik_path(cfg, _dev(tg), _dev(x0), 0, R, max_step))
    _compare(got_off, off, off_seeds, f"{name} {mode} off")
    hc.set_motion_resolution(h)
    got_on = _np(hc.ik_path(cfg, _dev(tg), _dev(x0), 0, R, max_step))
    _compare(got_on, on, on_seeds, f"{name} {mode} on")
    if name == "panda" and mode == "quality":
        for sk in ("quad", "lane64"):
            with nat.options(solve_kernel=sk):
                again = _np(hc.ik_path(cfg, _dev(tg), _dev(x0), 0, R, max_step))
            for k in got_on:
                assert_bit_equal(again[k].astype(np.float64), got_on[k].astype(np.float64), f"{sk} {k}")
    # off again: the parent's bits; and h > 0 without a model as well
    hc.set_motion_resolution(0)
    again = _np(hc.ik_path(cfg, _dev(tg), _dev(x0), 0, R, max_step))
    for k in got_off:
        assert_bit_equal(again[k].astype(np.float64), got_off[k].astype(np.float64), f"h = 0 {k}")
    plain_off = _np(plain.ik_path(cfg, _dev(tg), _dev(x0), 0, R, max_step))
    plain.set_motion_resolution(h)
    plain_on = _np(plain.ik_path(cfg, _dev(tg), _dev(x0), 0, R, max_step))
    for k in plain_off:
        assert_bit_equal(plain_on[k].astype(np.float64), plain_off[k].astype(np.float64), f"no model {k}")


def test_ik_batch_and_ik_solutions_ignore_the_setting(oracle, chains):
    from optik_amd import _native as nat
    hc = chain_with(chains, "panda")
    d, ch = chains["panda"]
    rng = np.random.default_rng(2)
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    tg = np.array([oracle.fk(ch, rng.uniform(lb, ub))[1] for _ in range(8)])
    x0 = rng.uniform(lb, ub, (8, 7))
    cfg = nat.make_config(solution_mode="quality")
    a = _np(hc.ik_batch(cfg, _dev(tg), _dev(x0), 0, 64, per_restart=False))
    sa = _np(hc.ik_solutions(cfg, _dev(tg), _dev(x0), 0, 64, 4, 0.1))
    ha = hc.ik_host(cfg, tg, x0, 0, 64)
    hc.set_motion_resolution(0.02)
    b = _np(hc.ik_batch(cfg, _dev(tg), _dev(x0), 0, 64, per_restart=False))
    sb = _np(hc.ik_solutions(cfg, _dev(tg), _dev(x0), 0, 64, 4, 0.1))
    hb = hc.ik_host(cfg, tg, x0, 0, 64)
    for x, y in ((a, b), (sa, sb), (ha, hb)):
        for k in x:
            assert_bit_equal(np.asarray(y[k], dtype=np.float64), np.asarray(x[k], dtype=np.float64), k)


def test_refusals(chains):
    import ctypes as C
    from optik_amd import _native as nat
    from optik_amd import device
    L = nat.lib()
    hc = chain_with(chains, "panda")
    q = _dev(np.zeros((7, 4)))
    out = torch.empty(4, dtype=torch.float64, device="cuda")
    for h in (math.nan, 0.0, -0.5, math.inf):
        with pytest.raises(ValueError, match="resolution"):
            hc.collision_motion_batch(q, q, h)
        rc = L.optik_hip_collision_motion_batch(hc._h, None, C.c_void_p(q.data_ptr()), C.c_void_p(q.data_ptr()), 4, h,
                                                C.c_void_p(out.data_ptr()), None, None, None, None)
        assert rc == -1 and b"resolution" in L.optik_hip_last_error()
    for h in (math.nan, -0.5, math.inf):
        with pytest.raises(ValueError, match="resolution"):
            hc.set_motion_resolution(h)
        assert L.optik_hip_chain_set_motion_resolution(hc._h, h) == -1
    with pytest.raises(ValueError):
        hc.collision_motion_batch(q, _dev(np.zeros((7, 5))), 0.1)
    with pytest.raises(ValueError):
        hc.collision_motion_batch(_dev(np.zeros((6, 4))), _dev(np.zeros((6, 4))), 0.1)
    # B = 0: a no-op
    e = _dev(np.zeros((7, 0)))
    clr, free, first, steps = hc.collision_motion_batch(e, e, 0.1)
    assert clr.shape == (0,) and steps.shape == (0,)
    assert L.optik_hip_collision_motion_batch(hc._h, None, None, None, 0, 0.1, None, None, None, None, None) == 0
    # prismatic chains
    g = device.HipChain(**chains["gantry"][0])
    ng = len(chains["gantry"][0]["lb"])
    with pytest.raises(nat.OptikHipError, match="prismatic"):
        g.collision_motion_batch(_dev(np.zeros((ng, 2))), _dev(np.zeros((ng, 2))), 0.1)
    rc = L.optik_hip_collision_motion_batch(g._h, None, None, None, 0, 0.1, None, None, None, None, None)
    assert rc == -2
    # the robot layer
    r = _robot("panda")
    z = np.zeros((2, 7))
    with pytest.raises(ValueError, match="resolution"):
        r.collision_motion_batch_arrays(z, z, 0.0)
    assert r._L.optik_robot_collision_motion_batch(r._h, 2, z.ctypes.data_as(C.POINTER(C.c_double)),
                                                   z.ctypes.data_as(C.POINTER(C.c_double)), math.nan, None, None,
                                                   None, None, None) == -1
    assert r._L.optik_robot_set_motion_resolution(r._h, -1.0) == -1
    clr, free, first, steps = r.collision_motion_batch_arrays(np.zeros((0, 7)), np.zeros((0, 7)), 0.1)
    assert len(clr) == 0
    gr = _robot("gantry")
    with pytest.raises(RuntimeError, match="prismatic"):
        gr.collision_motion_batch_arrays(np.zeros((2, ng)), np.zeros((2, ng)), 0.1)


def test_robot_surface_and_set_devices(oracle, chains):
    """The robot's motion batch is the chain's, and the resolution follows the robot onto chains created later by
    set_devices (two logical chains on one GPU)."""
    from optik_amd import SolverConfig
    name = "panda"
    d, ch = chains[name]
    hc = chain_with(chains, name)
    model, world = model_of(name), world_of(21)
    qa, qb = make_segments(d, 300, seed=6)
    want = [t.cpu().numpy() for t in hc.collision_motion_batch(_dev(qa.T), _dev(qb.T), 0.01)]
    robots = []
    for devices in (None, [0, 0]):
        r = _robot(name)
        r.set_collision_model(**model)
        r.set_world(*world)
        r.set_motion_resolution(0.05)   # (before any device chain exists)
        if devices:
            r.set_devices(devices)
        robots.append(r)
    got = robots[0].collision_motion_batch_arrays(qa, qb, 0.01)
    assert_bit_equal(got[0], want[0], "robot clearance")
    for k in (1, 2, 3):
        assert np.array_equal(got[k], want[k])
    one = robots[0].collision_motion(qa[0], qb[0], 0.01)
    assert one[1] == bool(want[1][0]) and one[2] == want[2][0] and one[3] == want[3][0]
    # paths: the two robots agree, every accepted move is free at the resolution, and the check changes something
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    rng = np.random.default_rng(12)
    P, L = 12, 4
    x0 = rng.uniform(lb, ub, (P, 7))
    poses = np.array([[robots[0].fk(np.clip(x0[p] + 0.1 * (w + 1), lb, ub)) for w in range(L)] for p in range(P)])
    cfg = SolverConfig("speed", max_time=0.0, max_restarts=32)
    res = [r.ik_paths_arrays(cfg, poses, x0, math.inf) for r in robots]
    for a, b in zip(res[0], res[1]):
        assert_bit_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), "set_devices")
    x, f, _, _, found = res[0]
    assert found.any()
    moves_a, moves_b = [], []
    for p in range(P):
        c = x0[p]
        for w in range(L):
            if found[p, w]:
                moves_a.append(c); moves_b.append(x[p, w])
                c = x[p, w]
    _, free, _, _ = robots[0].collision_motion_batch_arrays(np.array(moves_a), np.array(moves_b), 0.05)
    assert free.all()
    robots[0].set_motion_resolution(0)
    x_off = robots[0].ik_paths_arrays(cfg, poses, x0, math.inf)[0]
    assert not np.array_equal(np.nan_to_num(x_off), np.nan_to_num(x))


def test_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ik_motion.py"),
                          os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"],
                         env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    assert "every checked move free: True" in res.stdout, res.stdout
