"""-m gpu: the certified motion check (include/optik_hip.h; csrc/ik_advance.hip, csrc/advance_measure.hpp).

Parity: optik_hip_collision_motion_certify_batch against the g++ build of the header driven step by step from here
(advance_util): at step k the current configurations of all segments still walking go through link_frames_batch in
one call, the header turns the frames into (c, A) and advances.  Status, steps, t_stop and clearance bit for bit.

Soundness, independent of the header: against the sampled check at 2 000 .. 4 096 steps per segment.

A thin plate between two samples of the sampled check; the launch shape under a capped grid; the layers."""
import ctypes as C
import math

import numpy as np
import pytest

from advance_util import BLOCKED, FREE, LIMIT, NOT_A_NUMBER, Scene, build_advance
from conftest import ROBOT_SPECS
from gpu_util import assert_bit_equal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EE7 = np.array([0.01, -0.02, 0.05, 0.0, 0.0, math.sin(0.15), math.cos(0.15)])
MARGIN, TOL, MAX_STEPS = 0.01, 0.01, 256
GRID_ORIGIN, GRID_VOXEL, GRID_SHAPE = [0.0, -0.4, 0.0], 0.1, (9, 9, 9)  # a part of the workspace only
MAX_PAIRS = 4096  # OPTIK_HIP_MAX_COLLISION_PAIRS
F64_SENTINEL, BYTE_SENTINEL = 0x7FF8000000005E17, 0x7F
# per chain: (seed of the segments, the largest joint step): chosen on the host (the header over a numpy FK) so that the
# 67 segments hold at least 8 free and at least 8 blocked ones in both worlds -- asserted below on the device's results
SEGMENTS = {"panda": (1, 0.5), "ur10": (0, 0.5), "arm10": (1, 0.25)}


@pytest.fixture(scope="module")
def adv(tmp_path_factory):
    return build_advance(str(tmp_path_factory.mktemp("advance_measure")))


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _robot(name):
    from optik_amd import Robot
    return Robot.from_urdf_file(*ROBOT_SPECS[name])


def model_of(name):
    """spheres_along_chain(robot, 0.05, 12) with "auto" pairs (arm10 has 5 184 of them: the first 4 096, the most a
    model may hold)."""
    from optik_amd.collision import auto_pairs, spheres_along_chain
    frames, centers, radii = spheres_along_chain(_robot(name), 0.05, 12)
    pairs = np.asarray(auto_pairs(frames), dtype=np.int32).reshape(-1, 2)[:MAX_PAIRS]
    return dict(frames=frames, centers=centers, radii=radii, self_pairs=pairs, margin=MARGIN)


def world_of(seed=21, reach=0.8):
    rng = np.random.default_rng(seed)
    sph = np.concatenate([rng.uniform(-reach, reach, (5, 3)), rng.uniform(0.04, 0.12, (5, 1))], 1)
    q = rng.normal(size=(3, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    box = np.concatenate([rng.uniform(-reach, reach, (3, 3)), q, rng.uniform(0.03, 0.15, (3, 3))], 1)
    return sph, box


def segments_of(d, B, seed, step):
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    rng = np.random.default_rng(seed)
    qa = rng.uniform(lb, ub, (B, len(lb)))
    qb = np.clip(qa + rng.uniform(-step, step, qa.shape) * rng.choice([0.1, 0.4, 1.0], (B, 1)), lb, ub)
    return qa, qb


def setup(chains, name, grid):
    """(HipChain with the model, the world and maybe the grid installed; the same as a Scene for the header)."""
    from optik_amd import device
    d = chains[name][0]
    hc = device.HipChain(**d)
    model = model_of(name)
    hc.set_collision_model(**model)
    sph, box = world_of()
    hc.set_world(sph, box)
    g = None
    if grid:
        values = hc.bake_world_grid(GRID_ORIGIN, GRID_VOXEL, GRID_SHAPE).cpu().numpy()
        hc.set_world_grid(GRID_ORIGIN, GRID_VOXEL, values)
        g = (GRID_ORIGIN, GRID_VOXEL, values)
    scene = Scene(frames=model["frames"], centers=model["centers"], radii=model["radii"], pairs=model["self_pairs"],
                  margin=MARGIN, spheres=sph, boxes=box, grid=g)
    return hc, scene


def frames_of(hc, ee7):
    return lambda q: hc.link_frames_batch(_dev(q.T), ee_offset7=ee7).cpu().numpy()


@pytest.mark.parametrize("grid", [False, True], ids=["primitives", "grid"])
@pytest.mark.parametrize("name", ["panda", "ur10", "arm10"])
def test_parity_with_the_header_bit_for_bit(chains, adv, name, grid):
    d = chains[name][0]
    n = len(d["lb"])
    hc, scene = setup(chains, name, grid)
    seed, step = SEGMENTS[name]
    qa, qb = segments_of(d, 67, seed, step)  # 67: a partly filled block of 4 waves
    nan_seg = qa[3].copy()
    nan_seg[n // 2] = math.nan
    qa = np.concatenate([qa, nan_seg[None], qa[5:6]])
    qb = np.concatenate([qb, qb[3:4], qa[5:6]])  # the last: qa == qb
    G = math.sqrt(3.0)
    reach = adv.reach(d, n, EE7)
    want = adv.walk(n, qa, qb, scene, reach, TOL, G, MAX_STEPS, frames_of(hc, EE7))
    got = _np(hc.collision_motion_certify(_dev(qa.T), _dev(qb.T), TOL, max_steps=MAX_STEPS, ee_offset=EE7))
    print(name, grid, "status counts", np.bincount(got["status"], minlength=4), "steps", got["steps"][:67].min(),
          int(np.median(got["steps"][:67])), got["steps"][:67].max())
    assert np.array_equal(got["status"], want["status"]), np.nonzero(got["status"] != want["status"])
    assert np.array_equal(got["steps"], want["steps"]), np.nonzero(got["steps"] != want["steps"])
    assert_bit_equal(got["t_stop"], want["t_stop"], "t_stop")
    assert_bit_equal(got["clearance"], want["clearance"], "clearance")
    assert (got["status"][:67] == FREE).sum() >= 8 and (got["status"][:67] == BLOCKED).sum() >= 8
    assert got["status"][67] == NOT_A_NUMBER and got["steps"][67] == 0 and math.isnan(got["t_stop"][67])
    assert math.isnan(got["clearance"][67])
    assert got["steps"][68] == (2 if got["status"][68] == FREE else 1) and got["status"][68] in (FREE, BLOCKED)
    # the clearance is collision_batch's at the evaluated samples: check the last one of every walked segment
    walked = np.nonzero(got["steps"] > 0)[0]
    last = adv.samples(qa[walked], qb[walked], got["t_stop"][walked])
    c_last = hc.collision_batch(_dev(last.T), ee_offset7=EE7)[0].cpu().numpy()
    blocked = got["status"][walked] == BLOCKED
    assert (c_last[blocked] < MARGIN).all() and (c_last[~blocked] >= MARGIN).all()
    assert (got["clearance"][walked] <= c_last).all()
    assert_bit_equal(got["clearance"][walked][blocked], c_last[blocked], "a blocked walk's minimum is its last sample")
    if grid:
        # the outside rule ran: some sphere centre of some evaluated sample lies outside the grid, some inside
        fr = frames_of(hc, EE7)(last)
        p = fr[:, scene.frame, :3]  # (frame origins are enough to tell)
        lo, hi = np.array(GRID_ORIGIN), np.array(GRID_ORIGIN) + GRID_VOXEL * (np.array(GRID_SHAPE) - 1)
        inside = ((p >= lo) & (p <= hi)).all(axis=2)
        assert inside.any() and (~inside).any()


def test_without_a_model_and_at_the_step_limit(chains, adv):
    from optik_amd import device
    d = chains["panda"][0]
    hc = device.HipChain(**d)
    qa, qb = segments_of(d, 9, 2, 1.0)
    got = _np(hc.collision_motion_certify(_dev(qa.T), _dev(qb.T), 0.01, max_steps=2))
    assert (got["status"] == FREE).all() and (got["steps"] == 2).all() and (got["t_stop"] == 1.0).all()
    assert (got["clearance"] == math.inf).all()
    # a budget that is too small: LIMIT, with the header's bits
    hc, scene = setup(chains, "panda", False)
    want = adv.walk(7, qa, qb, scene, adv.reach(d, 7), 1e-3, math.sqrt(3.0), 3, frames_of(hc, None))
    got = _np(hc.collision_motion_certify(_dev(qa.T), _dev(qb.T), 1e-3, max_steps=3))
    assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["steps"], want["steps"])
    assert_bit_equal(got["t_stop"], want["t_stop"], "t_stop")
    assert (got["status"] == LIMIT).any() and (got["steps"][got["status"] == LIMIT] == 3).all()


@pytest.mark.parametrize("grid", [False, True], ids=["primitives", "grid"])
def test_soundness_against_dense_sampling(grid):
    """Independent of the header: the sampled check at 2 000 .. 4 096 steps per segment gives a dense minimum."""
    r = _robot("panda")
    model = model_of("panda")
    r.set_collision_model(**model)
    sph, box = world_of()
    r.set_world(sph, box)
    if grid:
        r.set_world_grid(GRID_ORIGIN, GRID_VOXEL, r.bake_world_grid(GRID_ORIGIN, GRID_VOXEL, GRID_SHAPE))
    lb, ub = (np.asarray(v) for v in r.joint_limits())
    rng = np.random.default_rng(8)
    B = 256
    qa, qb = rng.uniform(lb, ub, (B, 7)), rng.uniform(lb, ub, (B, 7))
    d0 = np.abs(qb - qa).max(axis=1)
    target = rng.uniform(0.55, 0.95, B)
    qb = qa + (qb - qa) * np.minimum(1.0, target / d0)[:, None]
    h = 1.0 / 4000.0
    dense, _, _, steps = r.collision_motion_batch_arrays(qa, qb, h)
    assert steps.min() >= 2000 and steps.max() <= 4096
    got = r.collision_motion_certify_batch_arrays(qa, qb, TOL)
    st = got["status"]
    print("grid" if grid else "primitives", "status counts", np.bincount(st, minlength=4), "steps median / max",
          int(np.median(got["steps"])), got["steps"].max())
    assert (dense[st == FREE] >= MARGIN - TOL).all()
    assert not (st[dense >= MARGIN] == BLOCKED).any()
    assert (st[dense < MARGIN - TOL] != FREE).all()
    assert (st == FREE).sum() >= 8 and (st == BLOCKED).sum() >= 8 and not (st == NOT_A_NUMBER).any()
    blocked = np.nonzero(st == BLOCKED)[0]
    t = got["t_stop"][blocked][:, None]
    q_stop = np.where(t == 0.0, qa[blocked], np.where(t == 1.0, qb[blocked], qa[blocked] + t * (qb[blocked] - qa[blocked])))
    c_stop, free_stop = r.collision_clearance_batch_arrays(q_stop)
    assert not free_stop.any()
    assert_bit_equal(got["clearance"][blocked], c_stop, "a blocked walk's clearance is that of q(t_stop)")
    # a free walk's minimum over its few samples cannot lie below the dense one by more than the walk allows
    assert (got["clearance"][st == FREE] >= MARGIN).all()
    r.clear_collision_model()
    r.set_world()
    r.clear_world_grid()


def test_thin_plate_between_two_samples():
    """One sphere of 5 mm on the end-effector frame, a 2 mm plate, joint 1 swept by 1 rad across it."""
    r = _robot("panda")
    r.set_collision_model(frames=[8], centers=[[0.0, 0.0, 0.0]], radii=[0.005], self_pairs=None, margin=0.0)
    qa = np.array([-0.5, 0.5, 0.0, -1.5, 0.0, 1.5, 0.0])
    qb = qa.copy()
    qb[0] = 0.5
    h = 0.1  # K = 10: samples at q1 = -0.5, -0.4 .. 0.5; the plate at q1 = 0.05, between two of them

    def ee(q1):
        q = qa.copy()
        q[0] = q1
        return np.array(r.fk(q))[:3, 3]
    p = ee(0.05)
    u = ee(0.051) - ee(0.049)
    u /= np.linalg.norm(u)
    quat = np.concatenate([np.cross([1.0, 0.0, 0.0], u), [1.0 + u[0]]])
    quat /= np.linalg.norm(quat)
    r.set_world(boxes=[np.concatenate([p, quat, [0.001, 0.2, 0.2]])])
    clr, free, first, steps = r.collision_motion(qa, qb, h)
    assert free and first == -1 and steps == 10 and clr > 0.005, (clr, free, first, steps)
    status, n, t_stop, c = r.collision_motion_certify(qa, qb, 1e-3)
    assert status == BLOCKED and c < 0.0, (status, n, t_stop, c)
    # the interval where dense sampling is below the margin
    K = 4000
    t = np.arange(K + 1) / K
    dense, _ = r.collision_clearance_batch_arrays(qa[None] + t[:, None] * (qb - qa)[None])
    below = np.nonzero(dense < 0.0)[0]
    assert len(below) > 20 and (np.diff(below) == 1).all()
    print("plate: blocked for t in [%.5f, %.5f], certified t_stop %.5f after %d samples" % (t[below[0]], t[below[-1]],
                                                                                         t_stop, n))
    assert t[below[0] - 1] <= t_stop <= t[below[-1] + 1]
    assert 0.04 < -0.5 + t_stop < 0.06
    r.clear_collision_model()
    r.set_world()


def _out(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    if dtype == torch.float64:
        t.view(torch.int64).fill_(F64_SENTINEL)
    else:
        t.view(torch.uint8).fill_(BYTE_SENTINEL)
    return t


def _raw(hc, qa, qb, tol, G, max_steps, ee7, which=("status", "steps", "t_stop", "clearance")):
    """The C entry point into sentinel-filled outputs; outputs not in `which` are passed as NULL."""
    from optik_amd import _native as nat
    B = qa.shape[1]
    out = dict(status=_out(B, torch.int32), steps=_out(B, torch.int32), t_stop=_out(B, torch.float64),
               clearance=_out(B, torch.float64))
    ptr = {k: (C.c_void_p(v.data_ptr()) if k in which else None) for k, v in out.items()}
    ee = np.ascontiguousarray(ee7) if ee7 is not None else None
    rc = nat.lib().optik_hip_collision_motion_certify_batch(
        hc._h, ee.ctypes.data_as(C.POINTER(C.c_double)) if ee is not None else None, C.c_void_p(qa.data_ptr()),
        C.c_void_p(qb.data_ptr()), B, tol, G, max_steps, ptr["status"], ptr["steps"], ptr["t_stop"], ptr["clearance"],
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def _is_sentinel(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) == F64_SENTINEL if a.dtype == np.float64 else a.view(np.uint32) == 0x7F7F7F7F


@pytest.mark.parametrize("name", ["panda", "arm10"])
def test_launch_shape_under_a_capped_grid(chains, name):
    from optik_amd import _native as nat
    d = chains[name][0]
    hc, _ = setup(chains, name, True)
    qa, qb = segments_of(d, 805, 13, 0.3)
    qa[17, 0] = math.inf
    dqa, dqb = _dev(qa.T), _dev(qb.T)
    G = math.sqrt(3.0)
    rc, ref = _raw(hc, dqa, dqb, TOL, G, 64, EE7)
    assert rc == 0 and not any(_is_sentinel(v).any() for v in ref.values())
    assert len(set(ref["status"].tolist())) >= 3 and ref["status"][17] == NOT_A_NUMBER
    for cap in (1, 3):
        with nat.options(grid_cap=cap):
            rc, got = _raw(hc, dqa, dqb, TOL, G, 64, EE7)
            assert rc == 0
            for k in ref:
                assert not _is_sentinel(got[k]).any(), (cap, k)
                assert np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)), (cap, k)
            # NULL outputs are left alone, the others are what they were
            rc, part = _raw(hc, dqa, dqb, TOL, G, 64, EE7, which=("status", "t_stop"))
            assert rc == 0 and _is_sentinel(part["steps"]).all() and _is_sentinel(part["clearance"]).all()
            assert np.array_equal(part["status"], ref["status"])
            assert np.array_equal(part["t_stop"].view(np.uint64), ref["t_stop"].view(np.uint64))


def test_layers_agree(chains):
    from optik_amd import _native as nat
    r = _robot("panda")
    model = model_of("panda")
    sph, box = world_of()
    r.set_collision_model(**model)
    r.set_world(sph, box)
    hc, _ = setup(chains, "panda", False)
    d = chains["panda"][0]
    qa, qb = segments_of(d, 40, 31, 0.5)
    dev = _np(hc.collision_motion_certify(_dev(qa.T), _dev(qb.T), TOL, max_steps=512))
    rob = r.collision_motion_certify_batch_arrays(qa, qb, TOL, max_steps=512)
    # the C ABI's row-major form, straight
    st, steps = np.zeros(40, dtype=np.int32), np.zeros(40, dtype=np.int32)
    ts, clr = np.zeros(40), np.zeros(40)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    a, b = np.ascontiguousarray(qa), np.ascontiguousarray(qb)
    assert r._L.optik_robot_collision_motion_certify_batch(r._h, 40, a.ctypes.data_as(dp), b.ctypes.data_as(dp), TOL,
                                                           math.sqrt(3.0), 512, None, st.ctypes.data_as(ip),
                                                           steps.ctypes.data_as(ip), ts.ctypes.data_as(dp),
                                                           clr.ctypes.data_as(dp)) == 0
    cabi = dict(status=st, steps=steps, t_stop=ts, clearance=clr)
    for k in dev:
        assert np.array_equal(dev[k].view(np.uint8), rob[k].view(np.uint8)), k
        assert np.array_equal(dev[k].view(np.uint8), cabi[k].view(np.uint8)), k
    one = r.collision_motion_certify(qa[3], qb[3], TOL, max_steps=512)
    assert one == (int(dev["status"][3]), int(dev["steps"][3]), float(dev["t_stop"][3]), float(dev["clearance"][3]))
    # certify_paths: 8 paths of 5 segments from the same 40 segments' starts; lens vary
    paths = np.zeros((8, 6, 7))
    for p in range(8):
        paths[p, 0] = qa[5 * p]
        for s in range(5):
            paths[p, s + 1] = paths[p, s] + (qb[5 * p + s] - qa[5 * p + s]) * 0.3
    lens = np.array([6, 6, 5, 4, 3, 2, 1, 6], dtype=np.int32)
    cert = r.certify_paths(paths, lens, tol=TOL)
    rank = {FREE: 0, LIMIT: 1, BLOCKED: 2, NOT_A_NUMBER: 3}
    for p in range(8):
        L = int(lens[p])
        if L < 2:
            assert cert["status"][p] == FREE and cert["segment"][p] == -1 and cert["clearance"][p] == math.inf
            continue
        seg = r.collision_motion_certify_batch_arrays(paths[p, :L - 1], paths[p, 1:L], TOL)
        worst = max(seg["status"], key=lambda s: rank[int(s)])
        assert cert["status"][p] == worst
        assert cert["segment"][p] == (-1 if worst == FREE else list(seg["status"]).index(worst))
        assert cert["clearance"][p] == seg["clearance"].min()
    assert len(set(cert["status"].tolist())) >= 2
    # refusals come back before any launch
    for kw in (dict(tol=0.0), dict(tol=math.nan), dict(tol=0.01, grid_lipschitz=0.0), dict(tol=0.01, max_steps=1),
               dict(tol=0.01, max_steps=65537)):
        with pytest.raises(ValueError):
            hc.collision_motion_certify(_dev(qa.T), _dev(qb.T), **kw)
    z = C.c_void_p(_dev(qa.T).data_ptr())
    for tol, G, ms, B in ((0.0, 1.0, 16, 4), (math.inf, 1.0, 16, 4), (0.01, math.nan, 16, 4), (0.01, 1.0, 1, 4),
                          (0.01, 1.0, 65537, 4), (0.01, 1.0, 16, -1), (0.01, 1.0, 16, (1 << 30) + 1)):
        assert nat.lib().optik_hip_collision_motion_certify_batch(hc._h, None, z, z, B, tol, G, ms, z, z, z, z,
                                                                  None) == -1  # OPTIK_HIP_EINVAL
    assert nat.lib().optik_hip_collision_motion_certify_batch(hc._h, None, z, z, 0, 0.01, 1.0, 16, z, z, z, z, None) == 0
    r.clear_collision_model()
    r.set_world()


def test_certify_paths_on_a_planned_route():
    """The wall of examples/plan_path.py: the route plan_paths finds around it, certified."""
    import importlib.util
    import os

    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("plan_path_example", os.path.join(ROOT, "examples", "plan_path.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    r = _robot("panda")
    start, goal, mid, (frames, centers, radii) = ex.scene(r)
    r.set_collision_model(frames, centers, radii, self_pairs=None)

    def point(q):
        link = np.array(r.link_frames_batch_arrays(q[None]))[0, frames[-1]]
        return (link @ np.append(centers[-1], 1.0))[:3]
    a, b = point(start), point(goal)
    u = (b - a) / np.linalg.norm(b - a)
    quat = np.concatenate([np.cross([1.0, 0.0, 0.0], u), [1.0 + u[0]]])
    quat /= np.linalg.norm(quat)
    r.set_world(boxes=[np.concatenate([point(mid), quat, [0.01, 0.15, 0.15]])])
    r.build_roadmap(resolution=ex.RESOLUTION)
    plan = r.plan_paths(start[None], goal[None])
    assert plan["status"][0] == 0 and plan["len"][0] >= 3
    cert = r.certify_paths(plan["paths"], plan["len"], tol=0.005)
    for p in range(1):
        L = int(plan["len"][p])
        seg = r.collision_motion_certify_batch_arrays(plan["paths"][p, :L - 1], plan["paths"][p, 1:L], 0.005)
        order = [NOT_A_NUMBER, BLOCKED, LIMIT, FREE]
        worst = min(seg["status"], key=lambda s: order.index(int(s)))
        assert cert["status"][p] == worst
        assert cert["segment"][p] == (-1 if worst == FREE else list(seg["status"]).index(worst))
        assert cert["clearance"][p] == seg["clearance"].min()
    # the straight move through the wall is blocked, and the direct certificate says where
    status, _, t_stop, _ = r.collision_motion_certify(start, goal, 0.005)
    assert status == BLOCKED and 0.3 < t_stop < 0.7
    # every segment of the planned route passed the sampled check; what the certificate adds is a statement: none of
    # them may be certified free with a clearance below margin - tol
    assert cert["status"][0] in (FREE, BLOCKED, LIMIT)
    if cert["status"][0] == FREE:
        assert cert["clearance"][0] >= 0.0
    r.clear_collision_model()
    r.set_world()
