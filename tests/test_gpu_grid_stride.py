"""-m gpu: the second and later trips of the grid-stride loops, under a capped grid.

The row kernels size their grid with grid_for (csrc/ik_host.hpp): as many blocks as the rows need, at most 8 per CU.
One trip of a full device covers half a million rows, so no other test takes a loop past its first trip.  The option
grid_cap (csrc/ik_grid.hpp) puts 1 or 3 blocks in the device's place: 805 = 3 * 256 + 37 rows are then four trips of
one block, the last with 37 live lanes, or a ragged second trip of one block out of three.

Every case runs the same inputs capped and uncapped and asserts that
  (a) the capped outputs equal the operator's CPU reference bit for bit -- the C oracle for forward kinematics,
      Jacobian, objective and seeds, the g++ builds of the shared headers (tests/*_util.py) for everything else, all
      of them fed with the oracle's frames and Jacobians, never with the device's;
  (b) the capped outputs equal the uncapped outputs bit for bit.
Every output buffer is allocated here and filled with a sentinel right before the call -- a NaN with a payload of its
own for float64 and float32, 0x7f bytes for integers and flags --, and no sentinel may remain: a kernel that skips rows
under the cap cannot pass on what the caching allocator left in the block."""
import ctypes as C
import math

import numpy as np
import pytest

from avoid_util import Scene, build_avoid, make_test_world
from collision_util import build_measure as build_collision_measure
from collision_util import small_scene
from conftest import ROBOT_SPECS
from gpu_util import _out, _sentinels_left, assert_bit_equal
from grid_util import build_grid_measure
from manip_util import build_measure as build_manip_measure
from motion_util import build_motion
from occupancy_util import build_occupancy_measure
from path_optimize_util import BLOCKED_SPHERE, Params, build_path_optimize, line_path
import time_util as tu

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CAPS = [1, 3]
B = 805            # 3 * 256 + 37
SIZES = [(B, CAPS), (37, [1])]  # (rows, caps): 37 rows under cap 1 are a single partial trip
EE7 = np.array([0.01, -0.02, 0.05, 0.0, 0.0, math.sin(0.15), math.cos(0.15)])
ROW_CHAINS = ["panda", "ur10", "panda1", "arm8", "arm10"]
F64, F32, I32, I64, U8 = torch.float64, torch.float32, torch.int32, torch.int64, torch.uint8


# ---- launches with sentinels ------------------------------------------------------------------------------------------
def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _launch(cap, spec, call, what):
    """One call under grid_cap = cap (0: the device's own) into sentinel-filled outputs {name: (shape, dtype)};
    call(outs) returns the C ABI's code.  The outputs as host arrays, none of them with a sentinel left."""
    from optik_amd import _native as nat
    outs = {k: _out(shape, dt) for k, (shape, dt) in spec.items()}
    with nat.options(grid_cap=cap):
        assert nat.get_option("grid_cap") == cap
        nat.check(call(outs))
        torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in outs.items()}
    for k, a in res.items():
        assert _sentinels_left(a) == 0, f"{what}, cap {cap}: {_sentinels_left(a)} of {a.size} values of {k} not written"
    return res


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype == np.float64:
        assert_bit_equal(got, want, what)
    elif got.dtype == np.float32:
        assert want.dtype == np.float32, what
        same = (got.view(np.uint32) == want.view(np.uint32)) | ((got == 0) & (want == 0)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), f"{what}: {(~same).sum()} of {got.size} values differ, first at {np.argwhere(~same)[0]}"
    else:
        assert np.array_equal(got.astype(np.int64), np.asarray(want).astype(np.int64)), \
            f"{what}: first difference at {np.argwhere(got.astype(np.int64) != np.asarray(want).astype(np.int64))[:3]}"


def _check(spec, call, want, what, caps=CAPS):
    """(a) and (b) of the module docstring for every cap; returns the uncapped outputs."""
    base = _launch(0, spec, call, what)
    for cap in caps:
        got = _launch(cap, spec, call, what)
        for k, w in want.items():
            _same(got[k], w, f"{what}, cap {cap}: {k} vs the CPU reference")
        for k in got:
            assert got[k].tobytes() == base[k].tobytes(), f"{what}, cap {cap}: {k} differs from the uncapped launch"
    return base


# ---- chains, scenes and the CPU side ------------------------------------------------------------------------------------
def _robot(name):
    from optik_amd import Robot
    return Robot.from_urdf_file(*ROBOT_SPECS[name])


def _model(name):
    if name == "panda1":  # (one joint: no link long enough for spheres_along_chain) a sphere off the joint's axis
        return dict(frames=np.array([1], dtype=np.int32), centers=np.array([[0.3, 0.0, 0.1]]), radii=np.array([0.05]),
                    self_pairs=None, margin=0.01), np.array([[0.45, 0.10, 0.40, 0.12], [-0.20, -0.35, 0.65, 0.10]])
    return small_scene(_robot(name))


_SCENES = {}


def _scene(name, grid):
    """collision_util.small_scene, the two boxes of avoid_util.make_test_world and (grid) its small world grid: the
    model, the world and the HipChain that holds them."""
    key = (name, grid)
    if key not in _SCENES:
        from oracle import urdf_chain
        from optik_amd import device
        from optik_amd.collision import model_arrays
        path, base, ee = ROBOT_SPECS[name]
        with open(path) as fh:
            d = urdf_chain.chain_from_urdf(fh.read(), base, ee)
        model, spheres = _model(name)
        _, boxes, g = make_test_world()
        hc = device.HipChain(**d)
        hc.set_collision_model(**model)
        hc.set_world(spheres=spheres, boxes=boxes)
        if grid:
            hc.set_world_grid(*g)
        pairs = model_arrays(model["frames"], model["centers"], model["radii"], model["self_pairs"], model["margin"])[3]
        _SCENES[key] = dict(hc=hc, d=d, model=model, pairs=np.asarray(pairs).reshape(-1, 2), spheres=spheres,
                            boxes=boxes, grid=g if grid else None)
    return _SCENES[key]


def _avoid_scene(sc, influence=0.25, safety=0.03, gain=1.0):
    n = sc["hc"].n
    m = sc["model"]
    return Scene(np.asarray(sc["d"]["axes"]).reshape(-1, 3)[:n], m["frames"], m["centers"], m["radii"], sc["pairs"],
                 sc["spheres"], sc["boxes"], sc["grid"], influence, safety, gain)


def _rows(d, seed=805, count=B):
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    return np.random.default_rng(seed).uniform(np.maximum(lb, -2.8), np.minimum(ub, 2.8), size=(count, len(lb)))


def _oracle_frames(oracle, ch, q, ee=None):
    """The n + 2 frames [n + 2, 7] of a revolute chain from the C oracle: the base, the frame after each joint, the
    end effector."""
    jt, pose = oracle.fk(ch, q, ee_offset=ee)
    return np.concatenate([[[0.0, 0, 0, 0, 0, 0, 1.0]], jt[:len(q)], [pose]])


_CPU = {}


@pytest.fixture(scope="module")
def cpu(oracle, chains):
    """name -> the oracle's rows of the chain's 805 configurations, computed once: q [B, n], frames [B, n + 2, 7], jac
    [B, 6n] (column-major 6 x n), and with the tool offset EE7 pose_ee [B, 7], jac_ee [B, 6n]."""
    ee = oracle.Pose.make(EE7[:3], EE7[3:])

    def get(name):
        if name not in _CPU:
            d, ch = chains[name]
            q = _rows(d)
            _CPU[name] = dict(q=q, frames=np.array([_oracle_frames(oracle, ch, x) for x in q]),
                              jac=np.array([oracle.joint_jacobian(ch, x).T.ravel() for x in q]),
                              pose_ee=np.array([oracle.fk(ch, x, ee_offset=ee)[1] for x in q]),
                              jac_ee=np.array([oracle.joint_jacobian(ch, x, ee).T.ravel() for x in q]))
        return _CPU[name]
    return get


@pytest.fixture(scope="module")
def avoid(tmp_path_factory):
    return build_avoid(str(tmp_path_factory.mktemp("stride_avoid")))


@pytest.fixture(scope="module")
def clearance_measure(tmp_path_factory):
    return build_collision_measure(str(tmp_path_factory.mktemp("stride_collision")))


def _lib():
    from optik_amd import _native as nat
    return nat.lib()


# ---- the row kernels of ik_batch_ops.hip ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROW_CHAINS)
def test_fk_and_jacobian_rows(cpu, name):
    """fk_batch_kernel with the Jacobian and a tool offset (9 .. 16 joints: wide_batch_launch mode 1)."""
    sc, ref = _scene(name, False), cpu(name)
    hc, n = sc["hc"], sc["hc"].n
    for rows, caps in SIZES:
        q = _dev(ref["q"][:rows].T)
        _check(dict(pose=((7, rows), F64), jac=((6 * n, rows), F64)),
               lambda o: _lib().optik_hip_fk_batch(hc._h, _dp(EE7), _p(q), rows, _p(o["pose"]), _p(o["jac"]), _stream()),
               dict(pose=ref["pose_ee"][:rows].T, jac=ref["jac_ee"][:rows].T), f"{name} fk_batch B={rows}", caps)


def test_fk_rows_of_a_prismatic_chain(oracle, chains):
    """fk_general_kernel."""
    from optik_amd import device
    d, ch = chains["gantry"]
    hc = device.HipChain(**d)
    x = np.random.default_rng(31).uniform(d["lb"], d["ub"], size=(B, len(d["lb"])))
    ee = oracle.Pose.make(EE7[:3], EE7[3:])
    q = _dev(x.T)
    for off, pose_off in ((None, None), (EE7, ee)):
        want = np.array([oracle.fk(ch, r, ee_offset=pose_off)[1] for r in x]).T
        _check(dict(pose=((7, B), F64)),
               lambda o: _lib().optik_hip_fk_batch(hc._h, _dp(off), _p(q), B, _p(o["pose"]), None, _stream()),
               dict(pose=want), f"gantry fk_batch ee={off is not None}")


@pytest.mark.parametrize("name", ROW_CHAINS)
def test_objective_and_gradient_rows(oracle, chains, cpu, name):
    """eval_batch_kernel with the gradient (9 .. 16 joints: wide_batch_launch mode 0)."""
    from optik_amd import _native as nat
    d, ch = chains[name]
    hc, n = _scene(name, False)["hc"], len(d["lb"])
    x = cpu(name)["q"]
    wl, wa = (0.0, 5.0, 0.25), (0.005, 1.0, 0.99)
    rng = np.random.default_rng(7)
    quat = rng.normal(size=4)
    tgt = np.concatenate([rng.uniform(-0.5, 0.5, 3), quat / np.linalg.norm(quat)])
    cfg = nat.make_config(linear_weight=wl, angular_weight=wa)
    fr, gr = np.empty(B), np.empty((n, B))
    for i in range(B):
        fr[i], gr[:, i] = oracle.eval_fg(ch, tgt, x[i], wl, wa)
    for rows, caps in SIZES:
        q = _dev(x[:rows].T)
        _check(dict(f=((rows,), F64), g=((n, rows), F64)),
               lambda o: _lib().optik_hip_eval_batch(hc._h, C.byref(cfg), _dp(tgt), None, _p(q), rows, _p(o["f"]),
                                                     _p(o["g"]), _stream()),
               dict(f=fr[:rows], g=gr[:, :rows]), f"{name} eval_batch B={rows}", caps)


@pytest.mark.parametrize("name", ["panda", "arm10"])
def test_seed_rows_across_two_to_the_thirty_two(oracle, chains, name):
    """seed_batch_kernel (9 .. 16 joints: wide_batch_launch mode 2): the 64-bit stream index crosses 2^32 on the first
    trip and every later trip starts beyond it."""
    d, ch = chains[name]
    hc, n = _scene(name, False)["hc"], len(d["lb"])
    first = 2 ** 32 - 3
    want = np.array([oracle.restart_seed(ch, i) for i in range(first, first + B)]).T
    for rows, caps in SIZES:
        _check(dict(q=((n, rows), F64)),
               lambda o: _lib().optik_hip_seed_batch(hc._h, first, rows, _p(o["q"]), _stream()),
               dict(q=want[:, :rows]), f"{name} seed_batch count={rows}", caps)


def _twists(n, seed):
    rng = np.random.default_rng(seed)
    V = rng.normal(size=(B, 6)) * rng.choice([0.0, 1e-3, 0.05, 1.0, 10.0], p=[0.1, 0.2, 0.2, 0.4, 0.1], size=B)[:, None]
    vm = rng.uniform(0.2, 2.0, size=(B, n))
    vm[3::10, rng.integers(n)] = 0.0
    vm[5::50, rng.integers(n)] = -0.5
    return V, vm


def test_diff_ik_rows(avoid, cpu):
    """diff_ik_batch_kernel, with one twist and limit vector for every row (ld = 0) and with one per row: the LP of
    diff_ik_lp.hpp (g++) on the oracle's Jacobian and end-effector rotation."""
    sc, ref = _scene("panda", True), cpu("panda")
    hc, n = sc["hc"], 7
    V, vm = _twists(n, 1000)
    for shared in (True, False):
        Vr = np.tile(V[0], (B, 1)) if shared else V
        vmr = np.tile(vm[1], (B, 1)) if shared else vm
        lp = avoid.lp([(n, ref["frames"][b, n + 1, 3:], ref["jac"][b].reshape(n, 6).T, Vr[b], vmr[b], np.zeros((0, n)), [])
                       for b in range(B)], damped=False)
        status = (lp[:, 0] != 0).astype(np.int32)
        alpha = np.where(status == 0, lp[:, 1], 0.0)
        v = np.where((status == 0)[:, None], lp[:, 2:2 + n], 0.0)
        assert 0 < status.sum() < B or shared
        Vd, vmd = (_dev(V[0]), _dev(vm[1])) if shared else (_dev(V.T), _dev(vm.T))
        for rows, caps in SIZES:
            q = _dev(ref["q"][:rows].T)
            # (the per-row form with the leading dimension of the whole batch: rows <= B of it are read)
            ld = 0 if shared else B
            _check(dict(alpha=((rows,), F64), v=((n, rows), F64), status=((rows,), I32)),
                   lambda o: _lib().optik_hip_diff_ik_batch(hc._h, None, _p(q), _p(Vd), ld, _p(vmd), ld, rows,
                                                            _p(o["alpha"]), _p(o["v"]), _p(o["status"]), _stream()),
                   dict(alpha=alpha[:rows], v=v[:rows].T, status=status[:rows]),
                   f"panda diff_ik_batch shared={shared} B={rows}", caps)


# ---- ik_manip.hip -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["panda", "arm10"])
def test_manipulability_rows(tmp_path_factory, cpu, name):
    """manip_batch_kernel and its wide form: manip_measure.hpp (g++) on the oracle's Jacobians."""
    measure = build_manip_measure(str(tmp_path_factory.mktemp("stride_manip")))
    sc, ref = _scene(name, False), cpu(name)
    hc, n = sc["hc"], sc["hc"].n
    w, c = measure([j.reshape(n, 6).T for j in ref["jac_ee"]])
    for rows, caps in SIZES:
        q = _dev(ref["q"][:rows].T)
        _check(dict(w=((rows,), F64), c=((rows,), F64)),
               lambda o: _lib().optik_hip_manip_batch(hc._h, _dp(EE7), _p(q), rows, _p(o["w"]), _p(o["c"]), _stream()),
               dict(w=w[:rows], c=c[:rows]), f"{name} manip_batch B={rows}", caps)


# ---- ik_collision.hip ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROW_CHAINS)
def test_link_frame_rows(cpu, name):
    """link_frames_batch_kernel and its wide form against the oracle's joint transforms."""
    sc, ref = _scene(name, False), cpu(name)
    hc, n = sc["hc"], sc["hc"].n
    for rows, caps in SIZES:
        q = _dev(ref["q"][:rows].T)
        _check(dict(frames=((rows, n + 2, 7), F64)),
               lambda o: _lib().optik_hip_link_frames_batch(hc._h, None, _p(q), rows, _p(o["frames"]), _stream()),
               dict(frames=ref["frames"][:rows]), f"{name} link_frames_batch B={rows}", caps)


@pytest.mark.parametrize("name", ROW_CHAINS)
def test_clearance_rows(clearance_measure, cpu, name):
    """collision_batch_kernel and its wide form against spheres and boxes: collision_measure.hpp (g++) on the oracle's
    frames."""
    sc, ref = _scene(name, False), cpu(name)
    hc, m = sc["hc"], sc["model"]
    clr = clearance_measure.clearance(ref["frames"], m["frames"], m["centers"], m["radii"], sc["pairs"], sc["spheres"],
                                      sc["boxes"])
    free = (clr >= m["margin"]).astype(np.uint8)
    assert 0 < free.sum() < B, free.mean()  # (the scene bites, and not everywhere)
    for rows, caps in SIZES:
        q = _dev(ref["q"][:rows].T)
        _check(dict(clearance=((rows,), F64), free=((rows,), U8)),
               lambda o: _lib().optik_hip_collision_batch(hc._h, None, _p(q), rows, _p(o["clearance"]), _p(o["free"]),
                                                          _stream()),
               dict(clearance=clr[:rows], free=free[:rows]), f"{name} collision_batch B={rows}", caps)


def test_clearance_and_witness_rows_with_all_three_obstacle_kinds(avoid, cpu):
    """collision_batch_kernel and collision_witness_kernel against spheres, boxes and the grid: the witness rows of
    collision_gradient.hpp (g++) on the oracle's frames; the clearance is their minimum."""
    sc, ref = _scene("panda", True), cpu("panda")
    hc, n, m = sc["hc"], 7, sc["model"]
    dist, wit, grad = avoid.witness(_avoid_scene(sc), ref["frames"])
    assert set(np.unique(wit[:, :, 1])) >= {0, 1, 2, 3}  # sphere, box, grid and self-pair witnesses
    clr = dist.min(axis=1)
    free = (clr >= m["margin"]).astype(np.uint8)
    for rows, caps in SIZES:
        q = _dev(ref["q"][:rows].T)
        _check(dict(clearance=((rows,), F64), free=((rows,), U8)),
               lambda o: _lib().optik_hip_collision_batch(hc._h, None, _p(q), rows, _p(o["clearance"]), _p(o["free"]),
                                                          _stream()),
               dict(clearance=clr[:rows], free=free[:rows]), f"panda collision_batch with a grid B={rows}", caps)
        _check(dict(dist=((n + 2, rows), F64), grad=((n + 2, n, rows), F64), wit=((n + 2, 3, rows), I32)),
               lambda o: _lib().optik_hip_collision_witness_batch(hc._h, None, _p(q), rows, _p(o["dist"]), _p(o["grad"]),
                                                                  _p(o["wit"]), _stream()),
               dict(dist=dist[:rows].T, grad=grad[:rows].transpose(1, 2, 0), wit=wit[:rows].transpose(1, 2, 0)),
               f"panda collision_witness_batch B={rows}", caps)


# ---- ik_avoid.hip -------------------------------------------------------------------------------------------------------
def test_avoiding_diff_ik_rows(avoid, cpu):
    """diff_ik_avoid_kernel: witness rows, damper rows and the damped LP (g++) on the oracle's frames and Jacobians."""
    sc, ref = _scene("panda", True), cpu("panda")
    hc, n = sc["hc"], 7
    influence, safety, gain = 0.25, 0.03, 1.0
    V, vm = _twists(n, 70)
    want = avoid.avoid(_avoid_scene(sc, influence, safety, gain), ref["frames"], ref["jac"], V, vm)
    assert (want["m"] > 0).sum() >= B // 10 and 0 < (want["status"] == 0).sum() < B
    Vd, vmd = _dev(V.T), _dev(vm.T)
    for rows, caps in SIZES:
        q = _dev(ref["q"][:rows].T)
        _check(dict(alpha=((rows,), F64), v=((n, rows), F64), status=((rows,), I32)),
               lambda o: _lib().optik_hip_diff_ik_avoid_batch(hc._h, None, _p(q), _p(Vd), B, _p(vmd), B, rows, influence,
                                                              safety, gain, _p(o["alpha"]), _p(o["v"]), _p(o["status"]),
                                                              _stream()),
               dict(alpha=want["alpha"][:rows], v=want["v"][:rows].T, status=(want["status"] != 0).astype(np.int32)[:rows]),
               f"panda diff_ik_avoid_batch B={rows}", caps)


# ---- ik_path_optimize.hip -------------------------------------------------------------------------------------------------
PO_L, PO_P = 16, 11
PO_PRM = Params(0.05, 1.0, 1.0, 0.2, 0.05)


def _po_scene(name):
    """The row scene with the grid and, in front of it, the sphere of the optimiser's blocked scene; as there, the
    model has no self pairs (neighbouring links are always within the influence distance of each other, and no path
    would be in free space)."""
    key = (name, "pathopt")
    if key not in _SCENES:
        from optik_amd import device
        base = _scene(name, False)
        _, boxes, g = make_test_world()
        spheres = np.concatenate([[BLOCKED_SPHERE], base["spheres"]])
        hc = device.HipChain(**base["d"])
        model = dict(base["model"], self_pairs=None, margin=0.0)
        hc.set_collision_model(**model)
        hc.set_world(spheres=spheres, boxes=boxes)
        hc.set_world_grid(*g)
        _SCENES[key] = dict(base, hc=hc, model=model, pairs=np.zeros((0, 2)), spheres=spheres, boxes=boxes, grid=g)
    return _SCENES[key]


def _po_paths(oracle, ch, po, sc):
    """11 paths whose neighbours in a wave's sequence (p, p + 4, p + 8) differ strongly: even ones through obstacles
    (F_obs > 0 on the host reference), odd ones in free space (F_obs = 0), path 4 with a NaN waypoint."""
    d = sc["d"]
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    n = len(lb)
    lo, hi = np.maximum(lb, -2.8), np.minimum(ub, 2.8)
    rng = np.random.default_rng(16)
    a = rng.uniform(lo, hi, size=(120, n))
    far = np.clip(a + rng.uniform(-1.5, 1.5, size=a.shape), lo, hi)
    near = np.clip(a + rng.uniform(-0.15, 0.15, size=a.shape), lo, hi)
    cand = np.array([line_path(x, y, PO_L) for x, y in zip(np.concatenate([a, a]), np.concatenate([far, near]))])
    cand[:, 1:-1] = np.clip(cand[:, 1:-1] + rng.normal(size=cand[:, 1:-1].shape) * 0.02, lo, hi)
    frames = np.array([[_oracle_frames(oracle, ch, x) for x in path] for path in cand])
    fobs = po.step(_avoid_scene(sc, PO_PRM.influence, PO_PRM.safety), PO_PRM, lb, ub, cand, frames)["cost"][:, 2]
    blocked, clear = np.flatnonzero(fobs > 1e-3), np.flatnonzero(fobs == 0.0)
    assert len(blocked) >= 6 and len(clear) >= 5, (len(blocked), len(clear))
    paths = np.empty((PO_P, PO_L, n))
    paths[0::2], paths[1::2] = cand[blocked[:6]], cand[clear[:5]]
    paths[4, 7, n // 2] = math.nan
    return paths


@pytest.mark.parametrize("name", ["panda", "arm8"])
def test_path_optimize_waves_take_three_paths_each(tmp_path_factory, oracle, chains, name):
    """path_optimize_kernel, 11 paths of 16 waypoints, the default 100 updates: under cap 1 each of the block's four
    waves takes paths p, p + 4, p + 8 through the same LDS slices (the last trip with one idle wave).  All five outputs
    against path_optimize.hpp (g++) iterated on the oracle's frames."""
    from optik_amd import _native as nat
    po = build_path_optimize(str(tmp_path_factory.mktemp("stride_pathopt")))
    sc = _po_scene(name)
    hc, n, ch = sc["hc"], sc["hc"].n, chains[name][1]
    lb, ub = np.asarray(sc["d"]["lb"]), np.asarray(sc["d"]["ub"])
    scene = _avoid_scene(sc, PO_PRM.influence, PO_PRM.safety)
    paths = _po_paths(oracle, ch, po, sc)
    iters = nat.PATH_OPTIMIZE_ITERS
    q, first, last = paths.copy(), None, None
    for it in range(iters + 1):
        frames = np.array([[_oracle_frames(oracle, ch, x) for x in path] for path in q])
        last = po.step(scene, PO_PRM, lb, ub, q, frames)
        first = last if it == 0 else first
        if it < iters:
            q = last["q"]
    status = np.isnan(last["cost"][:, 0]).astype(np.int32)
    assert status.tolist() == [0, 0, 0, 0, 1] + [0] * 6
    ok = status == 0
    assert (last["cost"][ok, 2] <= first["cost"][ok, 2]).all() and not np.array_equal(q[ok], paths[ok])
    q_in = _dev(paths.transpose(1, 0, 2))
    p = PO_PRM
    _check(dict(q=((PO_L, PO_P, n), F64), cost_first=((PO_P, 3), F64), cost_last=((PO_P, 3), F64),
                clearance=((PO_P,), F64), status=((PO_P,), I32)),
           lambda o: _lib().optik_hip_path_optimize(hc._h, None, _p(q_in), PO_L, PO_P, iters, p.step, p.w_smooth, p.w_obs,
                                                    p.influence, p.safety, _p(o["q"]), _p(o["cost_first"]),
                                                    _p(o["cost_last"]), _p(o["clearance"]), _p(o["status"]), _stream()),
           dict(q=q.transpose(1, 0, 2), cost_first=first["cost"], cost_last=last["cost"], clearance=last["clearance"],
                status=status), f"{name} path_optimize", [1])


# ---- ik_motion.hip ------------------------------------------------------------------------------------------------------
MOTION_H, MOTION_B = 0.05, 300


def _segments(d):
    """300 segments of 3 .. 40 samples at h = 0.05, some with equal end points, some that are not sampled (a NaN)."""
    lb, ub = np.asarray(d["lb"]), np.asarray(d["ub"])
    n = len(lb)
    rng = np.random.default_rng(300 + n)
    lo, hi = np.maximum(lb, -2.0), np.minimum(ub, 2.0)
    qa = rng.uniform(lo + 0.1, hi - 0.1, size=(MOTION_B, n))
    # (the largest joint difference is drawn, the others stay below it)
    dmax = rng.uniform(0.06, 1.94, size=MOTION_B)
    step = rng.uniform(-1.0, 1.0, size=(MOTION_B, n))
    step /= np.abs(step).max(axis=1, keepdims=True)
    qb = qa + step * dmax[:, None]
    qb[11::37] = qa[11::37]
    qb[5::53, n - 1] = math.nan
    return qa, qb


@pytest.mark.parametrize("name", ["panda", "arm10"])
def test_motion_chunks_within_one_block(tmp_path_factory, oracle, chains, clearance_measure, name):
    """motion_kernel and wide_motion_kernel, with clearance and classify-only: under cap 1 one block walks every chunk
    of 256 samples and its LDS window is handed from chunk to chunk across segment borders; under cap 3 three blocks
    walk a third each.  motion_measure.hpp (g++): its samples, their frames from the oracle, its reduction."""
    motion = build_motion(str(tmp_path_factory.mktemp("stride_motion")))
    sc = _scene(name, False)
    hc, m, ch = sc["hc"], sc["model"], chains[name][1]
    qa, qb = _segments(sc["d"])
    smp = motion.samples(qa, qb, MOTION_H)
    Ks = [K for _, K, _ in smp]
    sampled = np.array([K for K in Ks if K >= 1])
    assert set(Ks) - {-1, 1} <= set(range(2, 40)) and Ks.count(-1) >= 3 and Ks.count(1) >= 3
    assert (sampled + 1).sum() > 8 * 256  # (more than eight chunks: under cap 3 every block walks several)
    frames = [np.array([_oracle_frames(oracle, ch, x) for x in s]) if K >= 1 else None for _, K, s in smp]
    clr, free, first, steps = motion.reduce(Ks, frames, m["margin"], m["frames"], m["centers"], m["radii"], sc["pairs"],
                                            sc["spheres"], sc["boxes"])
    assert 0.05 < free.mean() < 0.95, free.mean()
    a, b = _dev(qa.T), _dev(qb.T)
    ints = dict(free=((MOTION_B,), U8), first=((MOTION_B,), I32), steps=((MOTION_B,), I32))
    want = dict(free=free.astype(np.uint8), first=first, steps=steps)
    _check(dict(ints, clearance=((MOTION_B,), F64)),
           lambda o: _lib().optik_hip_collision_motion_batch(hc._h, None, _p(a), _p(b), MOTION_B, MOTION_H,
                                                             _p(o["clearance"]), _p(o["free"]), _p(o["first"]),
                                                             _p(o["steps"]), _stream()),
           dict(want, clearance=clr), f"{name} collision_motion_batch")
    _check(ints,
           lambda o: _lib().optik_hip_collision_motion_batch(hc._h, None, _p(a), _p(b), MOTION_B, MOTION_H, None,
                                                             _p(o["free"]), _p(o["first"]), _p(o["steps"]), _stream()),
           want, f"{name} collision_motion_batch, classify only")


def test_ik_path_motion_keys_under_one_block(oracle, chains, tmp_path_factory):
    """motion_key_launch (and the collision key pass in front of it): ik_path with the motion check and max_step on
    the wall scene of tests/test_gpu_collision_motion.py, against that file's contract over the CPU oracle."""
    from optik_amd import _native as nat
    from optik_amd import device
    from test_gpu_collision_motion import contract_path, path_model, wall_scene, world_of
    motion = build_motion(str(tmp_path_factory.mktemp("stride_motion_key")))
    name, mode, max_step = "panda", "quality", 0.6
    d, ch = chains[name]
    P, L, R, h = 16, 8, 24, 0.05
    model = path_model(name)
    sph, box = world_of(33, n_spheres=6, n_boxes=2)
    hc = device.HipChain(**d)
    hc.set_collision_model(**model)
    hc.set_world(sph, box)
    tg, x0, walls = wall_scene(oracle, chains, hc, name, model, P, L, seed=40, spread=1.2)
    assert len(walls) >= 1
    world = (sph, np.concatenate([box, walls]))
    hc.set_world(*world)
    hc.set_motion_resolution(h)
    want, seeds = contract_path(oracle, ch, hc, motion, model, world, mode, tg, x0, R, max_step, h, None, check=True)
    found = np.array([[r is not None for r in row] for row in want])
    assert found.sum() >= P
    cfg = nat.make_config(solution_mode=mode)
    tgd, x0d = _dev(tg), _dev(x0)

    def call(o):
        outs = nat.IkPathOutputs()
        outs.d_x, outs.d_f, outs.d_idx = _p(o["x"]), _p(o["f"]), _p(o["idx"])
        outs.d_key, outs.d_step, outs.d_last = _p(o["key"]), _p(o["step"]), _p(o["last"])
        return _lib().optik_hip_ik_path(hc._h, C.byref(cfg), _p(tgd), _p(x0d), P, L, None, 0, R, 0, 0.0, max_step,
                                        C.byref(outs), _stream())

    idx = np.array([[r[0] if r is not None else -1 for r in row] for row in want])
    ref = dict(idx=idx, last=seeds)
    for k, col in (("key", 1), ("x", 2), ("f", 3), ("step", 4)):
        none = {"key": math.inf, "x": np.full(7, math.nan), "f": math.nan, "step": math.nan}[k]
        ref[k] = np.array([[r[col] if r is not None else none for r in row] for row in want], dtype=np.float64)
    spec = dict(x=((L, P, 7), F64), f=((L, P), F64), idx=((L, P), I64), key=((L, P), F64), step=((L, P), F64),
                last=((P, 7), F64))
    base = _launch(0, spec, call, "ik_path")
    got = _launch(1, spec, call, "ik_path")
    for k in spec:
        assert got[k].tobytes() == base[k].tobytes(), f"ik_path, cap 1: {k} differs from the uncapped launch"
    assert np.array_equal(got["idx"], ref["idx"])
    for k in ("key", "x", "step", "last"):
        _same(got[k], ref[k], f"ik_path, cap 1: {k} vs the contract")
    _same(got["f"][found], ref["f"][found], "ik_path, cap 1: f vs the contract")


# ---- ik_occupancy.hip and the bake of ik_collision.hip ----------------------------------------------------------------------
GRID_VOXEL = 0.07
GRID_SHAPES = [(13, 9, 17), (2, 2, 2)]  # 1989 nodes: eight trips of one block; 8 nodes: a single partial one


@pytest.fixture(scope="module")
def occupancy(tmp_path_factory):
    return build_occupancy_measure(str(tmp_path_factory.mktemp("stride_occupancy")))


@pytest.mark.parametrize("shape", GRID_SHAPES)
def test_distance_transform_passes(occupancy, shape):
    """edt_pass_kernel<0|1|2> and the kernels around them: occupancy_field of collision_measure.hpp (g++)."""
    hc = _scene("panda", False)["hc"]
    rng = np.random.default_rng(11)
    occ = rng.random(shape) < (0.05 if shape[0] > 2 else 0.5)
    occ.flat[rng.integers(occ.size)] = True
    md = GRID_VOXEL * math.sqrt(sum(s * s for s in shape))
    want = occupancy.field(GRID_VOXEL, occ, md)
    t = _dev(occ.astype(np.uint8))
    _check(dict(field=(shape, F32)),
           lambda o: _lib().optik_hip_world_grid_from_occupancy(hc._h, GRID_VOXEL, *shape, _p(t), md, _p(o["field"]),
                                                                _stream()),
           dict(field=want), f"world_grid_from_occupancy {shape}")


@pytest.mark.parametrize("shape", GRID_SHAPES)
def test_bake_nodes(tmp_path_factory, shape):
    """The bake of the chain's spheres and boxes: primitive_field of collision_measure.hpp (g++)."""
    measure = build_grid_measure(str(tmp_path_factory.mktemp("stride_bake")))
    sc = _scene("panda", False)
    hc = sc["hc"]
    origin = np.array([-0.5, -0.4, 0.0])
    want = measure.bake(origin, GRID_VOXEL, shape, sc["spheres"], sc["boxes"])
    _check(dict(field=(shape, F32)),
           lambda o: _lib().optik_hip_world_grid_bake(hc._h, _dp(origin), GRID_VOXEL, *shape, _p(o["field"]), _stream()),
           dict(field=want), f"world_grid_bake {shape}")


def test_voxelize_points(occupancy):
    """voxelize_kernel: 805 points and 5 exclusion spheres staged in LDS once per block, then read on every trip; NaN
    points, and points of one node that arrive on different trips.  The grid is read and written in place, so it
    starts from zeros and not from a sentinel: a point that is skipped leaves its node at 0, which (a) sees."""
    hc = _scene("panda", False)["hc"]
    shape, origin = (13, 9, 17), np.array([-0.5, -0.25, 0.125])
    rng = np.random.default_rng(805)
    extent = GRID_VOXEL * np.array(shape)
    pts = origin + rng.uniform(-0.1, 1.1, size=(B, 3)) * extent
    pts[300], pts[600], pts[804] = pts[40], pts[40], pts[41]   # one node from three trips of one block
    pts[7, 1] = pts[263, 0] = pts[519, 2] = pts[775, 1] = math.nan
    pts[800] = math.inf
    excl = np.concatenate([origin + rng.uniform(0.2, 0.8, size=(5, 3)) * extent, rng.uniform(0.1, 0.2, size=(5, 1))], 1)
    want = occupancy.voxelize(origin, GRID_VOXEL, shape, pts, excl)
    inside = occupancy.voxelize(origin, GRID_VOXEL, shape, pts, None)
    assert want.sum() >= 100 and (inside & ~want).sum() >= 20  # (points land, and the exclusion spheres remove some)
    p, e = _dev(pts), _dev(excl)
    res = {}
    for cap in [0] + CAPS:
        from optik_amd import _native as nat
        into = torch.zeros(shape, dtype=U8, device="cuda")
        with nat.options(grid_cap=cap):
            nat.check(_lib().optik_hip_occupancy_from_points(hc._h, _dp(origin), GRID_VOXEL, *shape, _p(p), B, _p(e), 5,
                                                             _p(into), _stream()))
            torch.cuda.synchronize()
        res[cap] = into.cpu().numpy()
        assert np.array_equal(res[cap] != 0, want), f"occupancy_from_points, cap {cap}"
        assert np.array_equal(res[cap], res[0]), f"occupancy_from_points, cap {cap} vs the uncapped launch"


# ---- ik_time.hip --------------------------------------------------------------------------------------------------------
def test_trajectory_samples_and_untouched_path_time(tmp_path_factory):
    """trajectory_sample_kernel over 5 * 161 = 805 samples; path_time_kernel takes one block per path and no grid cap:
    its outputs under the cap are pinned as well.  Both against time_measure.hpp (g++)."""
    ref = tu.build_time_ref(str(tmp_path_factory.mktemp("stride_time")))
    hc = _scene("panda", False)["hc"]
    n, L, P, T, dt = 7, 8, 5, 161, 0.01
    rng = np.random.default_rng(161)
    paths = tu.gentle_paths(rng, P, L, n)
    paths[3] = tu.random_walks(rng, 1, L, n)[0]
    vmax, amax = np.linspace(1.5, 2.5, n), np.linspace(4.0, 9.0, n)
    want = ref.time(paths, None, vmax, amax)
    assert (want["status"] == tu.TIMED).sum() >= 3 and want["duration"][want["status"] == tu.TIMED].max() > 0.5 * T * dt / 2
    wq, wv = ref.sample(paths, None, want, dt, T)
    path_d, vd, ad = _dev(tu.to_device_layout(paths)), _dev(vmax), _dev(amax)
    sw = lambda a: np.ascontiguousarray(np.swapaxes(a, 0, 1))  # noqa: E731
    timing = _check(dict(t=((L, P), F64), qd=((L, P, n), F64), qdd=((L, P, n), F64), x=((L, P), F64),
                         duration=((P,), F64), status=((P,), I32)),
                    lambda o: _lib().optik_hip_path_time(hc._h, _p(path_d), None, L, P, _p(vd), _p(ad), _p(o["t"]),
                                                         _p(o["qd"]), _p(o["qdd"]), _p(o["x"]), _p(o["duration"]),
                                                         _p(o["status"]), _stream()),
                    dict(t=sw(want["times"]), qd=sw(want["velocities"]), qdd=sw(want["accelerations"]), x=sw(want["x"]),
                         duration=want["duration"], status=want["status"]), "path_time")
    td, qdd_, sd = _dev(timing["t"]), _dev(timing["qd"]), _dev(timing["status"])
    _check(dict(q=((T, P, n), F64), v=((T, P, n), F64)),
           lambda o: _lib().optik_hip_trajectory_sample(hc._h, _p(path_d), None, L, P, _p(td), _p(qdd_), _p(sd), dt, T,
                                                        _p(o["q"]), _p(o["v"]), _stream()),
           dict(q=sw(wq), v=sw(wv)), "trajectory_sample")


# ---- the host API ---------------------------------------------------------------------------------------------------------
def test_the_cap_reaches_the_host_api(oracle, chains, tmp_path_factory):
    """Robot.collision_clearance_batch_arrays and Robot.optimize_paths under options(grid_cap=1): the option is
    process-wide, so the robot's own chains launch under it, and nothing changes."""
    from optik_amd import _native as nat
    sc = _po_scene("panda")
    robot = _robot("panda")
    robot.set_collision_model(**sc["model"])
    robot.set_world(spheres=sc["spheres"], boxes=sc["boxes"])
    robot.set_world_grid(*sc["grid"])
    xs = _rows(sc["d"])
    po = build_path_optimize(str(tmp_path_factory.mktemp("stride_host_api")))
    paths = _po_paths(oracle, chains["panda"][1], po, sc)
    plain = robot.collision_clearance_batch_arrays(xs), robot.optimize_paths(paths, 20)
    with nat.options(grid_cap=1):
        capped = robot.collision_clearance_batch_arrays(xs), robot.optimize_paths(paths, 20)
    for a, b in zip(plain[0] + tuple(plain[1]), capped[0] + tuple(capped[1])):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert 0 < plain[0][1].sum() < B and plain[1][4].tolist() == [0, 0, 0, 0, 1] + [0] * 6


def test_the_cap_is_back_at_the_devices_own():
    """(last in the file) every test above set the option in a `with` block."""
    from optik_amd import _native as nat
    assert nat.get_option("grid_cap") == 0
