"""-m gpu: shortcutting and resampling under a pose constraint on the device.  path_shortcut_constrained against the
serial reference of csrc/shortcut_constrained_measure.hpp (g++), fed the host header's projections (which
test_gpu_constraint.py shows equal to the device's) and the verdicts the device's own collision_motion_batch and
constraint_motion_batch give on the reference's vertex pairs, bit for bit; the free box against path_shortcut and
path_resample; a path's independence of the batch and of the chunking; path_resample_constrained against the
reference; the invariants on the constrained planner's scene; the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import constraint_util as cu
import shortcut_constrained_util as xu
import shortcut_util as su
from conftest import ROBOT_SPECS

pytestmark = pytest.mark.gpu
PROJ = (xu.PTOL, xu.PITERS, xu.DAMPING, xu.MAX_STEP)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def robots():
    from optik_amd import Robot
    made = {}

    def get(name):
        if name not in made:
            made[name] = Robot.from_urdf_file(*ROBOT_SPECS[name])
        return made[name]
    return get


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return xu.build_shortcut_constrained_ref(str(tmp_path_factory.mktemp("shortcut_constrained_measure")))


@pytest.fixture(scope="module")
def cmlib(tmp_path_factory):
    return xu.build_host_constraint_lib(str(tmp_path_factory.mktemp("constraint_host")))


@pytest.fixture(scope="module")
def scenes(robots, cmlib):
    """name -> the chain, its tables, the home configuration, upright(fk(home), TILT) on the host and the paths
    tests/test_shortcut_constrained_host.py looks at (made once, shared, left unchanged)."""
    from oracle import binding
    made = {}

    def get(name):
        if name not in made:
            robot = robots(name)
            tables = robot.chain_tables()
            lo, hi = np.asarray(tables["lb"]), np.asarray(tables["ub"])
            home = np.clip(0.5 * (lo + hi) + 0.1, lo + 0.2, hi - 0.2)
            ref7 = np.asarray(binding.fk(binding.make_chain(**tables), home)[1])
            c = xu.upright_constraint(ref7, xu.TILT)
            sc = dict(robot=robot, hc=robot.hip_chain(), tables=tables, home=home, ref7=ref7, c=c, paths={})
            for V, Lin in ((8, 8), (64, 64)):
                host = xu.HostConstraint(cmlib, tables, c)
                sc["paths"][(V, Lin)] = xu.scene_paths(host, lo, hi, 11, V, Lin, home)
            made[name] = sc
        return made[name]
    return get


def _t(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all((su.bits(got) == su.bits(want)) | (np.isnan(got) & np.isnan(want))))


def _device(torch, hc, paths, lens, c, V, Lout, tol=xu.TOL, proj=PROJ, h=xu.H, hop=xu.H):
    res = hc.path_shortcut_constrained(_t(torch, su.to_device_layout(paths)),
                                       None if lens is None else _t(torch, np.asarray(lens, dtype=np.int32)), c, tol,
                                       *proj, resolution=h, vertices=V, hop_penalty=hop, max_waypoints=Lout)
    out = {k: v.cpu().numpy() for k, v in res.items()}
    out["path"] = np.ascontiguousarray(np.transpose(out["path"], (1, 0, 2)))
    out["projected"] = np.ascontiguousarray(out["projected"].T)
    return out


def _reference(torch, ref, host, hc, paths, lens, c, V, Lout, tol=xu.TOL, proj=PROJ, h=xu.H, hop=xu.H):
    """The serial reference on the host header's projections and the device's own two verdicts of the reference's
    vertex pairs.  Returns (reference, free [P, pairs], ok [P, pairs])."""
    P = paths.shape[0]
    project = lambda x: host.project(x, *proj)  # noqa: E731
    verts = ref.vertices(paths, lens, V, project)["verts"]
    seg = [su.pair_segments(verts[p], V) for p in range(P)]
    qa, qb = (_t(torch, np.concatenate([s[k] for s in seg]).T) for k in (0, 1))
    free = hc.collision_motion_batch(qa, qb, h, clearance=False)[1].cpu().numpy().reshape(P, -1).astype(bool)
    ok = hc.constraint_motion_batch(qa, qb, h, c, tol)[1].cpu().numpy().reshape(P, -1).astype(bool)
    # the masked kernel on the same pairs: the AND of the two public checks for every pair
    flag = _t(torch, free.reshape(-1).astype(np.uint8))
    hc.constraint_motion_mask(qa, qb, h, c, tol, flag)
    assert np.array_equal(flag.cpu().numpy().astype(bool), (free & ok).reshape(-1)), "the masked verdict is the AND"
    return ref.shortcut(paths, lens, V, project, xu.flags_open(free & ok, V), hop, Lout), free, ok


def _agree(got, want, tag, keys=("cost", "cost_in", "path")):
    for key in ("status", "len", "projected"):
        if key in got and key in want:
            assert np.array_equal(got[key], want[key]), (tag, key, got[key], want[key])
    for key in keys:
        assert _same(got[key], want[key]), (tag, key)


def _set_wall(hc, on):
    if on:
        wall = su.wall_scene()
        hc.set_collision_model(wall["frames"], wall["centers"], wall["radii"], self_pairs=None)
        hc.set_world(boxes=wall["boxes"])
    else:
        hc.clear_collision_model()
        hc.set_world()


@pytest.mark.parametrize("name", ["panda", "arm10"])
@pytest.mark.parametrize("model", [False, True])
def test_device_matches_the_reference(torch_dev, scenes, ref, cmlib, name, model):
    sc = scenes(name)
    hc, c = sc["hc"], sc["c"]
    host = xu.HostConstraint(cmlib, sc["tables"], c)
    _set_wall(hc, model)
    seen, moved, closed, shorter = set(), False, False, False
    try:
        for V, Lin in ((2, 8), (3, 8), (8, 8), (64, 64)):
            paths, lens = sc["paths"][(max(V, 8), Lin)]
            lens = [min(v, Lin) for v in lens]
            runs = [(lens, Lin), (lens, 2)]
            if V == 8:
                runs.append(([1, Lin + 3] + lens[2:], Lin))     # a len outside its range, both ways
            for ln, Lout in runs:
                got = _device(torch_dev, hc, paths, ln, c, V, Lout)
                want, free, ok = _reference(torch_dev, ref, host, hc, paths, ln, c, V, Lout)
                print(f"{name} model={model} V={V} Lin={Lin} Lout={Lout} lens={ln}: status {got['status'].tolist()} len "
                      f"{got['len'].tolist()} projected {got['projected'].tolist()} pairs free {int(free.sum())} ok "
                      f"{int(ok.sum())} closed by the constraint alone {int((free & ~ok).sum())} of {free.size}")
                _agree(got, want, (name, model, V, Lin, Lout))
                seen |= set(got["status"].tolist())
                found = got["status"] == su.FOUND
                assert np.all(got["len"][found] <= Lout)
                assert np.all(got["projected"][:, 1] <= got["projected"][:, 0])
                assert got["status"][4] in (su.PATH_NAN, su.BAD_LENGTH) and got["projected"][4].tolist() == [0, 0]
                moved = moved or not _same(want["verts"], ref.vertices(paths, ln, V, lambda x: (x, 0, 0))["verts"])
                closed = closed or bool((free & ~ok).any())
                shorter = shorter or bool((found & (got["len"] < np.array(ln))).any())
                if Lout == 2 and V >= 8:
                    full = _device(torch_dev, hc, paths, ln, c, V, Lin)
                    long_route = (full["status"] == su.FOUND) & (full["len"] > 2)
                    assert np.all(got["status"][long_route] == su.BAD_LENGTH), "Lout smaller than a found route"
                    assert _same(got["cost"][long_route], full["cost"][long_route]), "which reports its true cost"
        assert {su.FOUND, su.BAD_LENGTH, su.PATH_NAN} <= seen
        if not model:
            assert moved and closed and shorter, "what tests/test_shortcut_constrained_host.py says of the scene"
    finally:
        _set_wall(hc, False)


@pytest.mark.parametrize("name", ["panda", "arm10"])
def test_a_free_box_is_the_unconstrained_stage(torch_dev, scenes, name):
    torch = torch_dev
    sc = scenes(name)
    hc = sc["hc"]
    box = cu.free_constraint(sc["ref7"])
    _set_wall(hc, True)
    try:
        for V, Lin in ((8, 8), (64, 64)):
            paths, lens = sc["paths"][(V, Lin)]
            d_path, d_len = _t(torch, su.to_device_layout(paths)), _t(torch, np.asarray(lens, dtype=np.int32))
            for Lout in (Lin, 2):
                got = hc.path_shortcut_constrained(d_path, d_len, box, 0.0, 0.0, 0, xu.DAMPING, xu.MAX_STEP,
                                                   resolution=xu.H, vertices=V, hop_penalty=xu.H, max_waypoints=Lout)
                want = hc.path_shortcut(d_path, d_len, xu.H, V, xu.H, Lout)
                for key in ("status", "len"):
                    assert torch.equal(got[key], want[key]), (name, V, Lout, key)
                for key in ("cost", "cost_in", "path"):
                    assert _same(got[key].cpu().numpy(), want[key].cpu().numpy()), (name, V, Lout, key)
                assert torch.equal(got["projected"][0], got["projected"][1]), "every projection ends at once"
            for Lout in (2, 3, 64):
                out, st, projected = hc.path_resample_constrained(d_path, d_len, box, Lout, 0.0, 0)
                wout, wst = hc.path_resample(d_path, d_len, Lout)
                assert torch.equal(st, wst) and _same(out.cpu().numpy(), wout.cpu().numpy()), (name, Lin, Lout)
                assert torch.equal(projected[0], projected[1])
    finally:
        _set_wall(hc, False)


def test_a_path_does_not_depend_on_the_batch_or_the_chunking(torch_dev, scenes):
    sc = scenes("panda")
    hc, c, home = sc["hc"], sc["c"], sc["home"]
    _set_wall(hc, False)
    chunk = hc.path_shortcut_constrained_chunk(64)
    assert 1 <= chunk <= 4096, "the test crosses one chunk: a chunk must stay small enough to cross quickly"
    assert chunk <= hc.path_shortcut_chunk(64), "the stored vertices are accounted for"
    P = chunk + 3
    rng = np.random.default_rng(9)
    # T about 0.1 rad at resolution 0.05: at most three samples per pair; the walks start on the constraint
    paths = home + su.random_polylines(rng, P, 3, 7, scale=0.03)
    paths[chunk, 1, 0] = math.nan
    lens = np.full(P, 3, dtype=np.int32)
    lens[chunk - 1] = 2
    many = _device(torch_dev, hc, paths, lens, c, 64, 64)
    print(f"chunk {chunk}, P {P}: statuses {np.bincount(many['status'], minlength=4).tolist()}, projections "
          f"{int(many['projected'][:, 0].sum())} attempted, {int(many['projected'][:, 1].sum())} ended projected")
    assert many["status"][chunk] == su.PATH_NAN and many["projected"][chunk].tolist() == [0, 0]
    assert (np.delete(many["status"], chunk) == su.FOUND).mean() > 0.5 and many["projected"][:, 0].max() > 0
    rows = (0, 1, chunk - 1, chunk, chunk + 1, P - 1)
    few = _device(torch_dev, hc, paths[list(rows)], lens[list(rows)], c, 64, 64)
    _agree(few, {k: v[list(rows)] for k, v in many.items()}, "a batch of six")
    for p in (chunk - 1, chunk, P - 1):
        one = _device(torch_dev, hc, paths[p:p + 1], lens[p:p + 1], c, 64, 64)
        _agree(one, {k: v[p:p + 1] for k, v in many.items()}, p)


@pytest.mark.parametrize("name", ["panda", "arm10"])
def test_resample_matches_the_reference(torch_dev, scenes, ref, cmlib, name):
    torch = torch_dev
    sc = scenes(name)
    hc, c = sc["hc"], sc["c"]
    host = xu.HostConstraint(cmlib, sc["tables"], c)
    paths, lens = sc["paths"][(8, 8)]
    paths, lens = paths.copy(), list(lens)
    lens[1] = 11                                            # outside 2 .. Lin: BAD_LENGTH, resampled all the same
    d_path, d_len = _t(torch, su.to_device_layout(paths)), _t(torch, np.asarray(lens, dtype=np.int32))
    seen = set()
    for Lout in (2, 3, 64):
        # the default budget, and none at all with a ptol the interpolated waypoints violate: status 4
        for proj in (PROJ, (1e-12, 0, xu.DAMPING, xu.MAX_STEP)):
            out, st, projected = hc.path_resample_constrained(d_path, d_len, c, Lout, *proj)
            want, wst, wpr = ref.resample(paths, lens, Lout, lambda x: host.project(x, *proj))
            print(f"{name} resample Lout={Lout} piters={proj[1]}: status {wst.tolist()} projected {wpr.tolist()}")
            assert np.array_equal(st.cpu().numpy(), wst), (name, Lout, proj, st, wst)
            assert np.array_equal(projected.cpu().numpy().T, wpr), (name, Lout, proj)
            assert _same(np.transpose(out.cpu().numpy(), (1, 0, 2)), want), (name, Lout, proj)
            assert wst[4] == su.PATH_NAN and wpr[4].tolist() == [0, 0], "a PATH_NAN row is not projected"
            assert wst[1] == su.BAD_LENGTH
            seen |= set(wst.tolist())
            if Lout > 2 and proj[1] == 0:
                assert wst[0] == xu.UNPROJECTED and wpr[0, 0] == Lout - 2 > wpr[0, 1]
            if Lout == 2:
                assert wpr[:, 0].tolist() == [0] * 5
    assert seen == {0, su.BAD_LENGTH, su.PATH_NAN, xu.UNPROJECTED}
    # lens None: every path has L waypoints
    out, st, projected = hc.path_resample_constrained(_t(torch, su.to_device_layout(paths[:3])), None, c, 17, *PROJ)
    want, wst, wpr = ref.resample(np.ascontiguousarray(paths[:3]), None, 17, lambda x: host.project(x, *PROJ))
    assert np.array_equal(st.cpu().numpy(), wst) and _same(np.transpose(out.cpu().numpy(), (1, 0, 2)), want)


def test_invariants_on_the_planner_scene(torch_dev, robots, tmp_path_factory):
    """Robot.shortcut_paths_constrained / resample_paths_constrained on constraint_util.plan_scene: three-waypoint
    paths through projected configurations.  Every FOUND output passes check_paths_constraint at tol and the
    collision motion check segment by segment, and its vertices that are no input waypoints have violation <= ptol."""
    from oracle import binding
    robot = robots("panda")
    cref = cu.build_constraint(str(tmp_path_factory.mktemp("constraint_measure")))
    tables = robot.chain_tables()
    home7 = np.asarray(binding.fk(binding.make_chain(**tables), np.array(cu.PANDA_HOME))[1])
    scene = cu.plan_scene(cref, tables, home7)
    c, tol, h = scene["c"], cu.PLAN_TOL, cu.PLAN_H
    starts, goals = scene["starts"].T, scene["goals"].T
    paths = np.stack([starts, np.roll(goals, 1, axis=0), goals], axis=1)
    wall = su.wall_scene()
    robot.set_collision_model(wall["frames"], wall["centers"], wall["radii"], self_pairs=None)
    robot.set_world(boxes=wall["boxes"])
    try:
        res = robot.shortcut_paths_constrained(paths, None, c, tol=tol, resolution=h, ptol=cu.PLAN_PROJECT_TOL,
                                               max_waypoints=32)
        found = res["status"] == su.FOUND
        print(f"planner scene: status {res['status'].tolist()} len {res['len'].tolist()} cost {res['cost'].round(3).tolist()} "
              f"cost_in {res['cost_in'].round(3).tolist()} projected {res['projected'].tolist()}")
        assert found.any() and set(res["status"].tolist()) <= {su.FOUND, su.NO_ROUTE}
        assert np.all(res["projected"][:, 0] >= res["projected"][:, 1]) and res["projected"][:, 1].max() > 0
        chk = robot.check_paths_constraint(res["paths"], res["len"], c, tol, h)
        assert chk["ok"][found].all()
        for p in np.nonzero(found)[0]:
            L = int(res["len"][p])
            path = res["paths"][p]
            assert _same(path[0], paths[p, 0]) and _same(path[L - 1], paths[p, 2]), "the ends never move"
            assert robot.collision_motion_batch_arrays(path[:L - 1], path[1:L], h)[1].all()
            assert robot.constraint_motion_batch_arrays(path[:L - 1], path[1:L], h, c, tol)[1].all()
            new = [t for t in range(1, L - 1) if not _same(path[t], paths[p, 1])]
            if new:
                v = robot.constraint_batch_arrays(path[new], c)[1]
                assert np.all(v <= cu.PLAN_PROJECT_TOL), (p, v)
                lo, hi = (np.asarray(a) for a in robot.joint_limits())
                assert np.all(path[new] >= lo) and np.all(path[new] <= hi)
        assert np.all(~found | (res["cost_in"] > 0))
        # unless FOUND the input comes back
        for p in np.nonzero(~found)[0]:
            assert _same(res["paths"][p, :3], paths[p]) and res["len"][p] == 3
        dense, st, projected, free, ok = robot.resample_paths_constrained(res["paths"], res["len"], c, 16, resolution=h,
                                                                          tol=tol, ptol=cu.PLAN_PROJECT_TOL)
        assert dense.shape == (len(paths), 16, 7) and set(st.tolist()) <= {0, xu.UNPROJECTED}
        assert free.shape == ok.shape == (len(paths),)
        assert _same(dense[:, 0], res["paths"][:, 0]) and _same(dense[:, -1], paths[:, 2])
        good = st == 0
        assert good.any() and np.all(projected[good, 0] == 14) and np.all(projected[good, 1] == 14)
        v = robot.constraint_batch_arrays(dense[good][:, 1:-1].reshape(-1, 7), c)[1]
        assert np.all(v <= cu.PLAN_PROJECT_TOL)
        seg_ok = robot.constraint_motion_batch_arrays(dense[:, :-1].reshape(-1, 7), dense[:, 1:].reshape(-1, 7), h, c, tol)[1]
        assert np.array_equal(ok, seg_ok.reshape(len(paths), 15).all(axis=1))
    finally:
        robot.clear_collision_model()
        robot.set_world()


def test_refusals(torch_dev, robots, scenes):
    from optik_amd import _native as nat
    sc = scenes("panda")
    robot, c = sc["robot"], sc["c"]
    paths = np.tile(sc["home"], (2, 4, 1))
    for kw in (dict(vertices=1), dict(vertices=65), dict(max_waypoints=1), dict(max_waypoints=65), dict(resolution=0.0),
               dict(hop_penalty=-1.0), dict(tol=-1.0), dict(tol=math.nan), dict(ptol=-1.0), dict(ptol=math.inf),
               dict(iters=-1), dict(iters=4097), dict(damping=-1.0), dict(max_step=0.0)):
        with pytest.raises(ValueError):
            robot.shortcut_paths_constrained(paths, None, c, **dict(dict(tol=0.05), **kw))
    with pytest.raises(TypeError):
        robot.shortcut_paths_constrained(paths, None, c)    # tol is keyword-only and has no default
    for kw in (dict(waypoints=1), dict(waypoints=65), dict(ptol=-1.0), dict(resolution=0.1), dict(tol=0.05),
               dict(resolution=0.0, tol=0.05)):
        with pytest.raises(ValueError):
            robot.resample_paths_constrained(paths, None, c, **kw)
    # the kernel layer itself, before any device work, each with the message of the check it comes from
    lib, hc = nat.lib(), robot.hip_chain()
    null = C.c_void_p(None)
    dp = C.POINTER(C.c_double)
    ref7, lo, hi = (np.ascontiguousarray(a, dtype=np.float64) for a in (c.ref7, c.lo, c.hi))
    EINVAL, EUNSUPPORTED = -1, -2

    def arr(a):
        return None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(dp)

    def shortcut(V=8, Lin=8, Lout=8, h=0.05, hop=0.0, chain=hc, ref7=ref7, lo=lo, hi=hi, tol=0.05, ptol=1e-6, piters=4,
                 damping=1e-6, max_step=0.5, P=4):
        rc = lib.optik_hip_path_shortcut_constrained(chain._h, None, null, null, Lin, P, V, h, hop, Lout, arr(ref7),
                                                     arr(lo), arr(hi), tol, ptol, piters, damping, max_step, null, null,
                                                     null, null, null, null, null)
        return rc, (lib.optik_hip_last_error() or b"").decode()

    def resample(Lin=8, Lout=8, chain=hc, ref7=ref7, lo=lo, hi=hi, ptol=1e-6, piters=4, damping=1e-6, max_step=0.5, P=4):
        rc = lib.optik_hip_path_resample_constrained(chain._h, None, null, null, Lin, P, Lout, arr(ref7), arr(lo),
                                                     arr(hi), ptol, piters, damping, max_step, null, null, null, null)
        return rc, (lib.optik_hip_last_error() or b"").decode()

    assert shortcut()[0] == 0 and resample()[0] == 0, "nothing to write: a no-op"
    sizes = "the vertices and the waypoints of a path are 2 .. 64"
    skew = ref7.copy()
    skew[3:] *= 1.001
    flipped = lo.copy()
    flipped[4] = hi[4] + 1.0
    for kw, msg in ((dict(V=1), sizes), (dict(V=65), sizes), (dict(Lin=1), sizes), (dict(Lin=65), sizes),
                    (dict(Lout=1), sizes), (dict(Lout=65), sizes), (dict(hop=-1.0), "hop_penalty must be finite"),
                    (dict(h=0.0), "resolution must be finite and > 0"), (dict(P=-1), "bad argument"),
                    (dict(ref7=None), "null reference or bounds"), (dict(lo=None), "null reference or bounds"),
                    (dict(ref7=skew), "unit norm"), (dict(lo=flipped), "lo <= hi"),
                    (dict(tol=-1.0), "tol must be finite and >= 0"), (dict(tol=math.nan), "tol must be finite and >= 0"),
                    (dict(ptol=-1.0), "tol must be finite and >= 0"), (dict(ptol=math.inf), "tol must be finite and >= 0"),
                    (dict(piters=-1), "iters must be 0 .. 4096"), (dict(piters=4097), "iters must be 0 .. 4096"),
                    (dict(damping=-1.0), "damping >= 0 and max_step > 0"), (dict(max_step=0.0), "damping >= 0 and max_step > 0")):
        rc, err = shortcut(**kw)
        assert rc == EINVAL and msg in err, (kw, rc, err)
        rc, err = shortcut(P=0, **{k: v for k, v in kw.items() if k != "P"})
        assert (rc == EINVAL and msg in err) or "P" in kw, ("also when P = 0", kw, rc, err)
    # the order: path_shortcut's refusals come before the constraint's, the constraint's before tol, tol before ptol
    assert sizes in shortcut(V=1, ref7=None)[1]
    assert "null reference" in shortcut(ref7=None, tol=-1.0)[1] and "unit norm" in shortcut(ref7=skew, tol=-1.0)[1]
    rsizes = "a path has 2 .. 64 waypoints"
    for kw, msg in ((dict(Lin=1), rsizes), (dict(Lin=65), rsizes), (dict(Lout=1), rsizes), (dict(Lout=65), rsizes),
                    (dict(P=-1), "bad argument"), (dict(hi=None), "null reference or bounds"), (dict(ref7=skew), "unit norm"),
                    (dict(lo=flipped), "lo <= hi"), (dict(ptol=-1.0), "tol must be finite and >= 0"),
                    (dict(piters=4097), "iters must be 0 .. 4096"), (dict(max_step=math.nan), "damping >= 0 and max_step > 0")):
        rc, err = resample(**kw)
        assert rc == EINVAL and msg in err, (kw, rc, err)
    assert rsizes in resample(Lout=1, ref7=None)[1]
    gantry = robots("gantry").hip_chain()
    for rc, err in (shortcut(chain=gantry), shortcut(chain=gantry, P=0), resample(chain=gantry), resample(chain=gantry, P=0),
                    shortcut(chain=gantry, ref7=None)):
        assert rc == EUNSUPPORTED and "prismatic" in err, (rc, err)
    assert lib.optik_hip_path_shortcut_constrained_chunk(hc._h, 1) == EINVAL
    assert lib.optik_hip_path_shortcut_constrained_chunk(hc._h, 64) >= 1
    assert lib.optik_hip_constraint_motion_mask(hc._h, None, arr(ref7), arr(lo), arr(hi), null, null, 4, 0.05, -1.0, null,
                                                null) == EINVAL
    assert "tol must be finite" in lib.optik_hip_last_error().decode()
