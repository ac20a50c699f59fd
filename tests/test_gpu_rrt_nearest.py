"""-m gpu: rules 1 and 2 of the tree planner (csrc/rrt_measure.hpp: nearest, steer) on trees the test prescribes, through
optik_hip_rrt_nearest_from_nodes -- the hook that runs the step kernel's own wave_nearest and rrt::steer_joint, one wave
per query point.  The planner's parity tests grow their trees from random samples: distances never tie there, and
nothing shows how many nodes a lane's stride loop or the butterfly behind it has seen.  Here the tree sizes sit on the
borders of the 64-lane stride (63, 64, 65, 127, 128, 129, and the cap 4096), distances tie exactly at chosen indices
(same lane in two trips, butterfly partners, a later trip against an earlier lane, the last partial trip), nodes hold
NaN and infinities, and the steer sits on d == step and on the joint limits.

The reference is written here: the Chebyshev distances in float64 with numpy's abs and max, a stable sort on (is NaN,
distance, index), and rrt_util's steer (the g++ build of rrt_measure.hpp).  Every comparison is bit for bit -- a NaN
equals a NaN, +0.0 does not equal -0.0 --, every output is filled with a sentinel before the call, and the columns of
the table past `count` hold the first query point itself: a search that read them would answer distance 0 there."""
import math

import numpy as np
import pytest

import rrt_util as tu
from conftest import ROBOT_SPECS
from gpu_util import _out, _sentinels_left

pytestmark = pytest.mark.gpu

NAMES = ("panda1", "panda", "arm16")
JOINTS = {"panda1": 1, "panda": 7, "arm16": 16}
COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 4096)
STEP = 0.3


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return tu.build_rrt_ref(str(tmp_path_factory.mktemp("rrt_measure")))


@pytest.fixture(scope="module")
def arms(torch_dev):
    from optik_amd import Robot
    out = {}
    for name in NAMES:
        robot = Robot.from_urdf_file(*ROBOT_SPECS[name])
        lo, hi = (np.array(v, dtype=np.float64) for v in robot.joint_limits())
        assert len(lo) == JOINTS[name] and np.isfinite(lo).all() and np.isfinite(hi).all() and (hi - lo > 1.5).all()
        # a point of the grid of quarters near the middle of the range: sums and differences with small multiples of
        # 1/8 are exact
        base = np.round((lo + hi) * 2.0) / 4.0
        out[name] = dict(robot=robot, hc=robot.hip_chain(), lo=lo, hi=hi, n=len(lo), base=base)
    return out


def _device(torch, arm, nodes, M, x, step=STEP):
    """The hook on nodes [count, n] laid out as conf [n][M] and x [X, n]; returns index [X], dist [X], cand [X, n]."""
    from optik_amd import _native as nat
    from optik_amd.device import _ptr, _stream_ptr
    nodes, x = np.atleast_2d(nodes), np.atleast_2d(x)
    (count, n), X = nodes.shape, len(x)
    assert n == arm["n"] and x.shape == (X, n) and count <= M
    conf = np.empty((n, M))
    conf[:, :count] = nodes.T
    conf[:, count:] = x[0][:, None]
    d_conf, d_x = torch.from_numpy(conf).cuda(), torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
    index, dist, cand = _out((X,), torch.int32), _out((X,), torch.float64), _out((n, X), torch.float64)
    nat.check(nat.lib().optik_hip_rrt_nearest_from_nodes(arm["hc"]._h, _ptr(d_conf), M, count, _ptr(d_x), X, step,
                                                         _ptr(index), _ptr(dist), _ptr(cand), _stream_ptr()))
    torch.cuda.synchronize()
    index, dist, cand = index.cpu().numpy(), dist.cpu().numpy(), cand.cpu().numpy()
    for k, v in (("index", index), ("dist", dist), ("cand", cand)):
        assert _sentinels_left(v) == 0, k
    return index, dist, cand.T.copy()


def _reference(ref, arm, nodes, x, step=STEP):
    """Rule 1 as a stable sort on (is NaN, distance, index) over numpy's float64 distances, rule 2 by the header."""
    nodes, x = np.atleast_2d(nodes), np.atleast_2d(x)
    index, dist, cand = [], [], []
    for p in x:
        with np.errstate(invalid="ignore"):
            d = np.max(np.abs(p[None, :] - nodes), axis=1)
        isnan = np.isnan(d)
        j = int(np.lexsort((np.arange(len(d)), np.where(isnan, 0.0, d), isnan))[0])
        c = ref.steer(nodes[j], p, step, arm["lo"], arm["hi"])
        index.append(j)
        dist.append(d[j])
        cand.append(c if c is not None else np.full(arm["n"], math.nan))       # (no candidate: a NaN column)
    return np.array(index, dtype=np.int32), np.array(dist), np.array(cand)


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (what, np.argwhere(~same)[:4].tolist(), got[~same][:4], want[~same][:4])


def _assert_parity(got, want, what):
    print(what, "index", want[0][:8], "dist", want[1][:4])
    assert np.array_equal(got[0], want[0]), (what, "index", got[0], want[0])
    _same_bits(got[1], want[1], f"{what}: dist")
    _same_bits(got[2], want[2], f"{what}: cand")


# ---- tree sizes on the borders of the stride loop --------------------------------------------------------------------

@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", NAMES)
def test_counts_on_the_borders_of_the_stride(torch_dev, ref, arms, name, count):
    arm = arms[name]
    rng = np.random.default_rng(1000 * arm["n"] + count)
    nodes = rng.uniform(arm["lo"], arm["hi"], (count, arm["n"]))
    x = rng.uniform(arm["lo"], arm["hi"], (37, arm["n"]))
    want = _reference(ref, arm, nodes, x)
    if count >= 128:
        # the winners come from every trip of the stride, and from both halves of the wave
        assert len(set((want[0] // 64).tolist())) >= 2
        assert (want[0] % 64 < 32).any() and (want[0] % 64 >= 32).any()
    for M in (count, count + 3):
        if M > tu.MAX_NODES:
            # (a table wider than the cap is refused; the cap with room behind the nodes is the case below)
            from optik_amd._native import OptikHipError
            with pytest.raises(OptikHipError):
                _device(torch_dev, arm, nodes, M, x)
            continue
        _assert_parity(_device(torch_dev, arm, nodes, M, x), want, f"{name} count {count} M {M}")
    if count == tu.MAX_NODES:
        want = _reference(ref, arm, nodes[:-3], x)
        _assert_parity(_device(torch_dev, arm, nodes[:-3], count, x), want, f"{name} count {count - 3} M {count}")


def test_every_node_of_a_large_tree_can_win(torch_dev, ref, arms):
    """129 and 4096 nodes, the query points the nodes themselves moved by less than any two nodes are apart: node j
    wins query j, whatever its lane and trip."""
    arm = arms["panda"]
    for count in (129, 4096):
        # (a grid of 1/64 in joint 0, so every node is at least 1/64 from every other; the move is 1/256)
        nodes = np.tile(arm["base"], (count, 1))
        nodes[:, 0] += (np.arange(count) - count // 2) / 64.0
        nodes[:, 1] += ((np.arange(count) * 7) % 5) / 256.0
        x = nodes.copy()
        x[:, 2] += 1.0 / 256.0
        want = _reference(ref, arm, nodes, x)
        assert np.array_equal(want[0], np.arange(count)) and (want[1] == 1.0 / 256.0).all()
        _assert_parity(_device(torch_dev, arm, nodes, count, x), want, f"count {count}")


# ---- prescribed ties ---------------------------------------------------------------------------------------------------

def _tied(arm, count, ties, nearer=()):
    """A tree of `count` nodes at L-infinity distance 1 or more from arm['base'], but for the nodes `ties` at exactly 1/2
    -- reached in different joints and with different signs, so the tying nodes are not copies of each other -- and
    the nodes `nearer` at exactly 3/8."""
    n = arm["n"]
    nodes = np.tile(arm["base"], (count, 1))
    j = np.arange(count)
    nodes[j, j % n] += np.where(j % 3 == 0, -1.0, 1.0) * (1.0 + 0.125 * (j % 5))
    for k, t in enumerate(ties):
        nodes[t] = arm["base"]
        nodes[t, k % n] += 0.5 if (k // n) % 2 == 0 else -0.5
        if n > 1:
            nodes[t, (k + 1) % n] -= 0.125 * (k % 4)            # (a smaller difference in another joint)
    for k, t in enumerate(nearer):
        nodes[t] = arm["base"]
        nodes[t, (k + 2) % n] -= 0.375
    return nodes


TIES = [
    # (count, the indices that tie at 1/2, what the case is)
    (130, (5, 69), "one lane, two trips"),
    (130, (69, 5), "one lane, two trips, built in the other order"),
    (70, (3, 35), "butterfly partners at offset 32"),
    (70, (0, 63), "the first and the last lane"),
    (64, (0, 63), "the first and the last lane of a full single trip"),
    (130, (64, 1), "a later trip of lane 0 against an earlier trip of lane 1"),
    (130, (1, 64, 129), "three trips, three lanes"),
    (130, (127, 64), "lane 63's second trip against lane 0's second trip"),
    (129, (128, 63), "the lone node of the third trip against the last lane"),
    (70, (6, 69), "the higher index in the last partial trip"),
    (70, (68, 69), "both in the last partial trip"),
    (70, (6, 68, 69), "an early lane against two of the last partial trip"),
    (65, (64, 63), "the one node of the second trip against the last lane of the first"),
    (200, tuple(range(7, 200, 16)), "a tie in every fourth lane of every trip"),
    (64, tuple(range(64)), "every lane"),
    (130, tuple(range(129, -1, -1)), "every node of three trips"),
]


@pytest.mark.parametrize("name", NAMES)
def test_ties_go_to_the_lower_index(torch_dev, ref, arms, name):
    arm = arms[name]
    for count, ties, what in TIES:
        nodes = _tied(arm, count, ties)
        want = _reference(ref, arm, nodes, arm["base"])
        assert want[0][0] == min(ties) and want[1][0] == 0.5, (what, want[0], want[1])
        for M in (count, count + 3):
            _assert_parity(_device(torch_dev, arm, nodes, M, arm["base"]), want, f"{name}: {what}, M {M}")
    # a tie does not hide a nearer node, in whichever lane and trip it sits
    for nearer in (0, 63, 64, 69, 129):
        nodes = _tied(arm, 130, (5, 69, 64, 1), nearer=(nearer,))
        want = _reference(ref, arm, nodes, arm["base"])
        assert want[0][0] == nearer and want[1][0] == 0.375
        _assert_parity(_device(torch_dev, arm, nodes, 130, arm["base"]), want, f"{name}: node {nearer} nearer than a tie")


@pytest.mark.parametrize("name", NAMES)
def test_identical_nodes(torch_dev, ref, arms, name):
    """Every node the same configuration (duplicate goals as roots of tree 1): node 0 wins, at every count."""
    arm = arms[name]
    x = arm["base"] + 0.125
    for count in (1, 2, 63, 64, 65, 129, 4096):
        nodes = np.tile(arm["base"] - 0.25, (count, 1))
        want = _reference(ref, arm, nodes, x)
        assert want[0][0] == 0 and want[1][0] == 0.375
        _assert_parity(_device(torch_dev, arm, nodes, count, x), want, f"{name}: {count} copies")


# ---- NaN, infinities and a query that is a node ------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_nan_and_infinite_nodes(torch_dev, ref, arms, name):
    """Rule 1's order is roadmap::ranks_before: a number before a NaN, +inf a number like any other.  The reference's
    index and distance are checked against the header's own search (rrt_util.nearest, g++) before the device is."""
    arm, n = arms[name], arms[name]["n"]
    rng = np.random.default_rng(77 + n)
    x = rng.uniform(arm["lo"], arm["hi"], (5, n))
    nan, inf = math.nan, math.inf

    def poisoned(count, spec):
        nodes = rng.uniform(arm["lo"], arm["hi"], (count, n))
        for j, v in spec.items():
            if j == "all":
                nodes[:, n // 2] = v
            else:
                nodes[j, (3 * j) % n] = v
        return nodes

    cases = [("NaN and infinite nodes among numbers", poisoned(70, {0: nan, 3: inf, 64: nan, 66: -inf, 69: nan})),
             ("a NaN node before an infinite one", poisoned(2, {0: nan, 1: inf})),
             ("an infinite node before a NaN one", poisoned(2, {0: -inf, 1: nan})),
             ("one NaN node", poisoned(1, {0: nan})),
             ("one infinite node", poisoned(1, {0: inf})),
             ("only NaN nodes", poisoned(70, {"all": nan})),
             ("only infinite nodes", poisoned(130, {"all": inf})),
             ("NaN in both trips of lane 0, an infinite node in lane 1's second", poisoned(66, {"all": nan, 65: inf})),
             ("NaN everywhere but the last node of the last partial trip", poisoned(70, {"all": nan}))]
    cases[7][1][65, n // 2] = 0.0
    cases[7][1][65, (3 * 65) % n] = inf
    cases[8][1][69] = arm["base"]
    expect = {1: (1, inf), 2: (0, inf), 3: (0, nan), 4: (0, inf), 5: (0, nan), 6: (0, inf), 7: (65, inf), 8: (69, None)}
    for k, (what, nodes) in enumerate(cases):
        want = _reference(ref, arm, nodes, x)
        for q in range(len(x)):
            j, d = ref.nearest(nodes, x[q])
            assert j == want[0][q] and (d == want[1][q] or (math.isnan(d) and math.isnan(want[1][q]))), (what, q, j, d)
        if k in expect:
            j, d = expect[k]
            assert (want[0] == j).all(), (what, want[0])
            if d is not None:
                assert np.array_equal(want[1], np.full(5, d), equal_nan=True), (what, want[1])
                assert np.isnan(want[2]).all(), what                # (no steer over a distance that is no number)
        else:
            assert np.isfinite(want[1]).all() and np.isfinite(want[2]).all()
        _assert_parity(_device(torch_dev, arm, nodes, len(nodes) + 3, x), want, f"{name}: {what}")


@pytest.mark.parametrize("name", NAMES)
def test_a_query_that_is_a_node_makes_no_candidate(torch_dev, ref, arms, name):
    """d = 0: rrt::steers is false, the iteration ends there, and the hook's candidate column is NaN (optik_hip.h).  The
    node is in the tree twice: the lower index is the answer."""
    arm, n = arms[name], arms[name]["n"]
    rng = np.random.default_rng(5 + n)
    nodes = rng.uniform(arm["lo"], arm["hi"], (130, n))
    nodes[3] = nodes[67] = nodes[128]
    x = np.stack([nodes[67], nodes[129], nodes[0], rng.uniform(arm["lo"], arm["hi"], n)])
    want = _reference(ref, arm, nodes, x)
    assert want[0][:3].tolist() == [3, 129, 0] and (want[1][:3] == 0.0).all() and want[1][3] > 0.0
    assert np.isnan(want[2][:3]).all() and np.isfinite(want[2][3]).all()
    _assert_parity(_device(torch_dev, arm, nodes, 130, x), want, name)


# ---- the steer's borders -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_steer_at_d_equal_to_the_step(torch_dev, ref, arms, name):
    """d <= step copies the sample, d > step scales: the step is set to d itself and to its two neighbours."""
    arm, n = arms[name], arms[name]["n"]
    rng = np.random.default_rng(9 + n)
    nodes = rng.uniform(arm["lo"], arm["hi"], (5, n))
    for q in range(4):
        x = rng.uniform(arm["lo"], arm["hi"], n)
        j, d, _ = (v[0] for v in _reference(ref, arm, nodes, x))
        assert 0.0 < d < math.inf
        for step, copied in ((d, True), (np.nextafter(d, math.inf), True), (np.nextafter(d, 0.0), False)):
            want = _reference(ref, arm, nodes, x, step)
            assert (d <= step) == copied
            if copied:
                assert np.array_equal(want[2][0], x), (q, step, d)
            _assert_parity(_device(torch_dev, arm, nodes, 8, x, step), want, f"{name}: query {q}, step {step!r}")
    # exact numbers: d = 1/4 = step copies, d = 1/2 halves the difference
    nodes = arm["base"][None, :].copy()
    for shift, cand in ((0.25, 0.25), (-0.25, -0.25), (0.5, 0.25), (-0.5, -0.25)):
        x = arm["base"].copy()
        x[n - 1] += shift
        want = _reference(ref, arm, nodes, x, 0.25)
        assert want[1][0] == abs(shift) and want[2][0][n - 1] == arm["base"][n - 1] + cand
        _assert_parity(_device(torch_dev, arm, nodes, 1, x, 0.25), want, f"{name}: shift {shift}")


@pytest.mark.parametrize("name", NAMES)
def test_steer_clamps_at_the_limits(torch_dev, ref, arms, name):
    """if (c < lo) c = lo; if (c > hi) c = hi, after the scaled step and after the copy alike: nodes just inside the
    limits, query points outside them."""
    arm, n = arms[name], arms[name]["n"]
    lo, hi = arm["lo"], arm["hi"]
    nodes = np.stack([hi - 0.01, lo + 0.01])
    odd = np.arange(n) % 2 == 1
    x = np.stack([hi + 0.5, lo - 0.5, np.where(odd, hi - 0.02, hi + 0.5), np.where(odd, lo + 0.02, lo - 0.5)])
    for step, what in ((0.1, "scaled"), (1.0, "copied")):
        want = _reference(ref, arm, nodes, x, step)
        assert want[0].tolist() == [0, 1, 0, 1]
        assert np.array_equal(want[2][0], hi) and np.array_equal(want[2][1], lo), what
        assert np.array_equal(want[2][2][~odd], hi[~odd]) and np.array_equal(want[2][3][~odd], lo[~odd]), what
        assert (want[2][2][odd] < hi[odd]).all() and (want[2][3][odd] > lo[odd]).all()
        _assert_parity(_device(torch_dev, arm, nodes, 2, x, step), want, f"{name}: {what}")


# ---- the argument rules ------------------------------------------------------------------------------------------------

def test_refusals(torch_dev, arms):
    from optik_amd import _native as nat
    from optik_amd.device import _ptr
    torch = torch_dev
    lib, hc = nat.lib(), arms["panda"]["hc"]
    conf = torch.zeros((7, 8), dtype=torch.float64, device="cuda")
    x = torch.ones((7, 3), dtype=torch.float64, device="cuda")
    index, dist, cand = _out((3,), torch.int32), _out((3,), torch.float64), _out((7, 3), torch.float64)

    def call(h=hc._h, conf=conf, M=8, count=8, x=x, X=3, step=0.3, index=index, dist=dist, cand=cand):
        p = lambda t: _ptr(t) if t is not None else None  # noqa: E731
        return lib.optik_hip_rrt_nearest_from_nodes(h, p(conf), M, count, p(x), X, step, p(index), p(dist), p(cand), None)
    bad = (dict(h=None), dict(count=0), dict(count=-1), dict(count=9), dict(M=0, count=0), dict(M=0, count=1),
           dict(M=tu.MAX_NODES + 1), dict(X=-1), dict(X=(1 << 30) + 1), dict(step=0.0), dict(step=-0.3),
           dict(step=math.nan), dict(step=math.inf), dict(conf=None), dict(x=None), dict(index=None), dict(dist=None),
           dict(cand=None))
    for kw in bad:
        assert call(**kw) == -1, kw                                           # OPTIK_HIP_EINVAL
    assert call(X=0) == 0 and call(X=0, conf=None, x=None, index=None, dist=None, cand=None) == 0
    torch.cuda.synchronize()
    for v in (index, dist, cand):
        assert _sentinels_left(v.cpu().numpy()) == v.numel()
    assert call() == 0 and call(M=8, count=1) == 0
    torch.cuda.synchronize()
    for v in (index, dist, cand):
        assert _sentinels_left(v.cpu().numpy()) == 0
    assert index.cpu().numpy().tolist() == [0, 0, 0] and dist.cpu().numpy().tolist() == [1.0, 1.0, 1.0]
