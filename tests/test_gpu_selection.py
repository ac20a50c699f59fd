"""-m gpu: the selection kernels on prescribed keys -- ties, the borders of their decomposition, boundary comparisons,
"none" outputs.

ik_select.hip, ik_solutions.hip and ik_path.hip are otherwise reached only behind a real solve, whose keys are distinct
real numbers.  Here the three stages run on keys, x and f chosen by the test, through the optik_hip_*_from_keys hooks
(include/optik_hip.h): the product's own launch code with no solve in front.  The reference is tests/selection_util.py,
a sort on (key, index) and a greedy filter in plain Python.

x[i][col] and f[col] encode (i, col) exactly, so a gather from a wrong row or column shows; every output buffer is
filled with a sentinel before the call and none may remain; every comparison is bit for bit -- indices as integers,
key / x / f / step by bit pattern (-0.0 is not +0.0), NaN against NaN."""
import ctypes as C
import functools

import numpy as np
import pytest

import selection_util as su
from gpu_util import _out, _sentinels_left, make_targets

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CHAINS = ["panda", "arm10"]  # n = 7; n = 10: the `threadIdx.x < n` writes above 8
R_ONE_TILE = [1, 63, 64, 65, 255, 256, 257, 4095, 4096]
R_TILES = [4097, 8192, 8193]
R_65_TILES = 64 * 4096 + 1  # the second trip of stage 2, with a single live column in the last tile
BEGINS = [0, 2 ** 32 - 3, 2 ** 53 + 1]  # (the last one does not survive a detour through a double)
# the 65-tile size runs with T = 2 only, once per begin
BIG_CASES = [("panda", 0), ("arm10", 2 ** 32 - 3), ("panda", 2 ** 53 + 1)]
PATH_R = [1, 255, 256, 257, 4096]
F64, I32, I64 = torch.float64, torch.int32, torch.int64
INF_BITS = np.array(np.inf).view(np.uint64)


@pytest.fixture(scope="module")
def hip_chains(chains):
    from optik_amd import device
    return {name: device.HipChain(**chains[name][0]) for name in CHAINS}


# ---- launches ---------------------------------------------------------------------------------------------------------
def _dev(a, dtype=F64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _host(outs, what):
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in outs.items()}
    for k, a in res.items():
        assert _sentinels_left(a) == 0, f"{what}: {_sentinels_left(a)} of {a.size} values of {k} not written"
    if "idx" in res:
        res["idx"] = res["idx"].view(np.uint64)
    return res


@functools.lru_cache(maxsize=4)
def _coded(n, cols):
    """coded_x / coded_f on the host and on the device."""
    x, f = su.coded_x(n, cols), su.coded_f(cols)
    return x, f, _dev(x), _dev(f)


def run_select(hc, keys, d_x, d_f, begin, what=""):
    from optik_amd import _native as nat
    T, R = keys.shape
    outs = dict(x=_out((T, hc.n), F64), f=_out(T, F64), idx=_out(T, I64), key=_out(T, F64))
    o = nat.IkOutputs()
    o.d_win_x, o.d_win_f, o.d_win_idx, o.d_win_key = _p(outs["x"]), _p(outs["f"]), _p(outs["idx"]), _p(outs["key"])
    d_key = _dev(keys)
    nat.check(nat.lib().optik_hip_select_from_keys(hc._h, _p(d_key), _p(d_x), _p(d_f), T, begin, R, C.byref(o),
                                                   _stream()))
    res = _host(outs, what)
    assert d_key.cpu().numpy().tobytes() == np.ascontiguousarray(keys).tobytes(), f"{what}: the keys were written to"
    return res


def run_solutions(hc, keys, d_x, d_f, begin, K, min_dist, what=""):
    from optik_amd import _native as nat
    T, R = keys.shape
    outs = dict(count=_out(T, I32), x=_out((T, K, hc.n), F64), f=_out((T, K), F64), idx=_out((T, K), I64),
                key=_out((T, K), F64))
    o = nat.IkSolutionsOutputs()
    o.d_count, o.d_x, o.d_f, o.d_idx, o.d_key = (_p(outs[k]) for k in ("count", "x", "f", "idx", "key"))
    d_key = _dev(keys)  # (scratch: the multi-tile form sets eliminated keys to +inf)
    nat.check(nat.lib().optik_hip_solutions_from_keys(hc._h, _p(d_key), _p(d_x), _p(d_f), T, begin, R, K,
                                                      float(min_dist), C.byref(o), _stream()))
    return _host(outs, what)


def run_path(hc, keys, d_x, d_f, seed, begin, max_step, alias, what=""):
    """One waypoint; alias: `carry` is the seed buffer itself.  Returns the outputs, `carry` among them."""
    from optik_amd import _native as nat
    P, R = keys.shape
    n = hc.n
    outs = dict(x=_out((P, n), F64), f=_out(P, F64), idx=_out(P, I64), key=_out(P, F64), step=_out(P, F64),
                last=_out((P, n), F64))
    o = nat.IkPathOutputs()
    o.d_x, o.d_f, o.d_idx, o.d_key, o.d_step, o.d_last = (_p(outs[k]) for k in ("x", "f", "idx", "key", "step", "last"))
    d_seed = _dev(seed)
    carry = d_seed if alias else _out((P, n), F64)
    d_key = _dev(keys)
    nat.check(nat.lib().optik_hip_path_select_from_keys(hc._h, _p(d_key), _p(d_x), _p(d_f), _p(d_seed), P, begin, R,
                                                        float(max_step), C.byref(o), _p(carry), _stream()))
    outs["carry"] = carry
    res = _host(outs, what)
    if not alias:
        assert d_seed.cpu().numpy().tobytes() == np.ascontiguousarray(seed).tobytes(), f"{what}: the seed was written to"
    return res


# ---- comparisons ------------------------------------------------------------------------------------------------------
def assert_bits(got, want, what):
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), f"{what}: {(~same).sum()} of {got.size} differ; first at {tuple(np.argwhere(~same)[0])}: " \
                       f"gpu={got[tuple(np.argwhere(~same)[0])]!r} want={want[tuple(np.argwhere(~same)[0])]!r}"


def assert_idx(got, want, what):
    want = np.array(want, dtype=np.uint64).reshape(got.shape)
    assert np.array_equal(got, want), f"{what}: idx gpu={got.tolist()} want={want.tolist()}"


def check_select(hc, keys, x, f, d_x, d_f, begin, what):
    """One launch of T targets against select_ref; none: idx ~0, key +inf, x and f NaN."""
    T, R = keys.shape
    got = run_select(hc, keys, d_x, d_f, begin, what)
    w_idx, w_key, w_x, w_f = [], [], [], []
    for t in range(T):
        ref = su.select_ref(keys[t], begin)
        if ref is None:
            w_idx.append(su.NONE), w_key.append(np.inf), w_x.append(np.full(hc.n, np.nan)), w_f.append(np.nan)
        else:
            c = t * R + (ref[0] - begin)
            w_idx.append(ref[0]), w_key.append(ref[1]), w_x.append(x[:, c]), w_f.append(f[c])
    assert_idx(got["idx"], w_idx, what)
    assert_bits(got["key"], w_key, what + " key")
    assert_bits(got["x"], w_x, what + " x")
    assert_bits(got["f"], w_f, what + " f")
    return got


def solutions_want(n, keys, x, f, begin, K, min_dist):
    T, R = keys.shape
    want = dict(count=np.zeros(T, dtype=np.int32), idx=np.full((T, K), su.NONE, dtype=np.uint64),
                key=np.full((T, K), np.inf), x=np.full((T, K, n), np.nan), f=np.full((T, K), np.nan))
    for t in range(T):
        acc = su.solutions_ref(keys[t], x[:, t * R:(t + 1) * R], begin, K, min_dist)
        want["count"][t] = len(acc)
        for k, (i, key, r) in enumerate(acc):
            want["idx"][t, k], want["key"][t, k] = i, key
            want["x"][t, k], want["f"][t, k] = x[:, t * R + r], f[t * R + r]
    return want


def check_solutions(hc, keys, x, f, d_x, d_f, begin, K, min_dist, what):
    """One launch against solutions_ref; the slots past count: x and f NaN, idx ~0, key +inf."""
    got = run_solutions(hc, keys, d_x, d_f, begin, K, min_dist, what)
    want = solutions_want(hc.n, keys, x, f, begin, K, min_dist)
    assert got["count"].tolist() == want["count"].tolist(), f"{what}: count"
    assert_idx(got["idx"], want["idx"], what)
    for k in ("key", "x", "f"):
        assert_bits(got[k], want[k], f"{what} {k}")
    return got, want


def check_path(hc, keys, x, f, d_x, d_f, seed, begin, max_step, alias, what):
    """One waypoint against path_ref; none: x, f and step NaN, idx ~0, key +inf, carry and last the seed's bits."""
    P, R = keys.shape
    got = run_path(hc, keys, d_x, d_f, seed, begin, max_step, alias, what)
    w = dict(idx=[], key=[], x=[], f=[], step=[], carry=[])
    for p in range(P):
        i, key, r, step, nxt = su.path_ref(keys[p], x[:, p * R:(p + 1) * R], seed[p], begin, max_step)
        found = i is not None
        w["idx"].append(i if found else su.NONE), w["key"].append(key if found else np.inf)
        w["x"].append(x[:, p * R + r] if found else np.full(hc.n, np.nan))
        w["f"].append(f[p * R + r] if found else np.nan)
        w["step"].append(step if found else np.nan), w["carry"].append(nxt)
    assert_idx(got["idx"], w["idx"], what)
    for k in ("key", "x", "f", "step", "carry"):
        assert_bits(got[k], w[k], f"{what} {k}")
    assert_bits(got["last"], w["carry"], what + " last")
    return got


def chunks(rows, sizes=(3, 4, 5)):
    """The rows in groups of 3, 4, 5, 3, ... targets (a short last group is filled up from the front), each with the
    next `begin`: (names, keys [T, R], begin)."""
    i = j = 0
    while i < len(rows):
        T = sizes[j % len(sizes)]
        group = rows[i:i + T]
        group += [rows[m % len(rows)] for m in range(T - len(group))]
        yield [g[0] for g in group], np.array([g[1] for g in group]), BEGINS[(j + j // len(BEGINS)) % len(BEGINS)]
        i, j = i + T, j + 1


# ---- the selection of optik_hip_ik_batch ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("R", R_ONE_TILE + R_TILES)
@pytest.mark.parametrize("begin", BEGINS)
def test_select_on_prescribed_keys(hip_chains, name, R, begin):
    hc = hip_chains[name]
    for names, keys, _ in chunks(su.key_patterns(R)):
        x, f, d_x, d_f = _coded(hc.n, keys.size)
        check_select(hc, keys, x, f, d_x, d_f, begin, f"{name} R={R} begin={begin} {names}")


@pytest.mark.parametrize("name,begin", BIG_CASES)
def test_select_on_prescribed_keys_over_65_tiles(hip_chains, name, begin):
    hc = hip_chains[name]
    R = R_65_TILES
    x, f, d_x, d_f = _coded(hc.n, 2 * R)
    for names, keys, _ in chunks(su.key_patterns(R), sizes=(2,)):
        check_select(hc, keys, x, f, d_x, d_f, begin, f"{name} R={R} begin={begin} {names}")


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("R", R_ONE_TILE + R_TILES + [R_65_TILES])
def test_select_fuzz(hip_chains, name, R):
    """Keys drawn from 4 values, half of them +inf, a few NaN: ties everywhere.  20 seeds."""
    hc = hip_chains[name]
    for seed in range(20):
        rng = np.random.default_rng(R * 100 + seed)
        T = 2 if R == R_65_TILES else 3 + seed % 3
        keys = np.array([su.fuzz_keys(rng, R) for _ in range(T)])
        x, f, d_x, d_f = _coded(hc.n, T * R)
        check_select(hc, keys, x, f, d_x, d_f, BEGINS[seed % 3], f"{name} R={R} seed={seed}")


def test_select_none_writes_inf_key_and_nan(hip_chains):
    """The rule of d_win_key (optik_hip.h) for a target without a finite key: +inf, with idx UINT64_MAX and NaN x, f --
    between two targets that have a winner, in the one-kernel and in the two-kernel form."""
    hc = hip_chains["arm10"]
    for R in (300, 4097):
        keys = np.full((3, R), np.inf)
        keys[0, R - 1], keys[2, 0] = -0.0, 7.0
        keys[1, ::7] = np.nan
        x, f, d_x, d_f = _coded(hc.n, 3 * R)
        got = check_select(hc, keys, x, f, d_x, d_f, 5, f"R={R}")
        assert got["idx"].tolist() == [5 + R - 1, su.NONE, 5]
        assert got["key"].view(np.uint64)[1] == INF_BITS and np.signbit(got["key"][0])
        assert np.isnan(got["x"][1]).all() and np.isnan(got["f"][1]) and not np.isnan(got["x"][[0, 2]]).any()


# ---- the solution sets of optik_hip_ik_solutions -------------------------------------------------------------------------
SPACING = 1.5 * 2.0 ** -24  # of coded_x: a column eliminates its two neighbours


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("R", R_ONE_TILE + R_TILES)
def test_solutions_on_prescribed_keys(hip_chains, name, R):
    """Round 0 on every key pattern; rounds 1 and 2 on what the first acceptances leave."""
    hc = hip_chains[name]
    for names, keys, begin in chunks(su.key_patterns(R)):
        x, f, d_x, d_f = _coded(hc.n, keys.size)
        check_solutions(hc, keys, x, f, d_x, d_f, begin, 3, SPACING, f"{name} R={R} begin={begin} {names}")


@pytest.mark.parametrize("name,begin", BIG_CASES)
def test_solutions_on_prescribed_keys_over_65_tiles(hip_chains, name, begin):
    hc = hip_chains[name]
    R = R_65_TILES
    x, f, d_x, d_f = _coded(hc.n, 2 * R)
    for j, (names, keys, _) in enumerate(chunks(su.key_patterns(R), sizes=(2,))):
        check_solutions(hc, keys, x, f, d_x, d_f, begin, 1 + j % 3, SPACING, f"{name} R={R} begin={begin} {names}")


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("R", [63, 257, 4096, 4097, 8193])
def test_solutions_fuzz(hip_chains, name, R):
    """Tied keys over lattice points 0.25 apart: distances on both sides of and next to min_dist, every K."""
    hc = hip_chains[name]
    for seed in range(4):
        rng = np.random.default_rng(R * 100 + seed)
        T = 3 + seed % 3
        keys = np.array([su.fuzz_keys(rng, R) for _ in range(T)])
        x, f = su.lattice_x(rng, hc.n, T * R, levels=2 + seed % 2), su.coded_f(T * R)
        d_x, d_f = _dev(x), _dev(f)
        for K, min_dist in ((1, 0.25), (2, 0.0), (5, 0.25), (256, 0.25), (256, 0.5), (7, 2.0 ** -11)):
            check_solutions(hc, keys, x, f, d_x, d_f, BEGINS[seed % 3], K, min_dist,
                            f"{name} R={R} seed={seed} K={K} min_dist={min_dist}")


def test_solutions_fuzz_over_65_tiles(hip_chains):
    hc = hip_chains["panda"]
    R = R_65_TILES
    rng = np.random.default_rng(65)
    keys = np.array([su.fuzz_keys(rng, R) for _ in range(2)])
    x, f = su.lattice_x(rng, hc.n, 2 * R, levels=2), su.coded_f(2 * R)
    d_x, d_f = _dev(x), _dev(f)
    for K, min_dist in ((3, 0.0), (3, 0.25)):
        check_solutions(hc, keys, x, f, d_x, d_f, BEGINS[2], K, min_dist, f"K={K} min_dist={min_dist}")


def _sparse(n, T, R, cands):
    """keys [T, R] all +inf and x [n, T*R] coded, but for cands = [(t, column, key, x [n])]."""
    keys = np.full((T, R), np.inf)
    x = su.coded_x(n, T * R) + 64.0  # (far from every candidate below)
    for t, r, key, v in cands:
        keys[t, r] = key
        x[:, t * R + r] = v
    return keys, x, su.coded_f(T * R)


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("R", [257, 4096, 4097, 8193])
def test_solutions_duplicates_equality_and_nan(hip_chains, name, R):
    """min_dist = 0 merges bit-identical x and keeps x one ulp away; a candidate at exactly min_dist = 0.25 is eliminated,
    one at 0.25 + 2^-50 kept; NaN components of x are skipped by the distance.  The differing joint is the last one."""
    hc = hip_chains[name]
    n = hc.n
    v = np.arange(1, n + 1) / 8.0
    last = R - 1

    def at(j, val):
        u = v.copy()
        u[j] = val
        return u

    ulp = at(n - 1, np.nextafter(v[n - 1], 9.0))
    nan_same, nan_far = at(2, np.nan), at(1, np.nan)
    nan_far[0] += 1.0
    # target 0: duplicates (min_dist = 0); target 1: NaN components (min_dist = 0); target 2: the same as 0, mirrored
    keys, x, f = _sparse(n, 3, R, [(0, 5, 1.0, v), (0, last, 2.0, v), (0, 130, 3.0, ulp), (0, 131, 3.0, ulp),
                                   (1, 0, 1.0, v), (1, 70, 2.0, nan_same), (1, last, 3.0, nan_far),
                                   (2, last, 1.0, v), (2, 5, 2.0, v), (2, 1, 3.0, ulp)])
    got, _ = check_solutions(hc, keys, x, f, _dev(x), _dev(f), 0, 4, 0.0, f"{name} R={R} duplicates")
    assert got["idx"].tolist() == [[5, 130, su.NONE, su.NONE], [0, last, su.NONE, su.NONE], [last, 1, su.NONE, su.NONE]]
    assert got["count"].tolist() == [2, 2, 2] and np.isnan(got["x"][1, 1, 1])
    # exactly min_dist away: eliminated; 2^-50 further: kept
    a, b, c = at(n - 1, 0.5), at(n - 1, 0.75), at(n - 1, 0.75 + 2.0 ** -50)
    keys, x, f = _sparse(n, 3, R, [(0, 9, 1.0, a), (0, last, 1.0, b), (1, 9, 1.0, a), (1, last, 1.0, c),
                                   (2, last, 0.5, a), (2, 0, 1.0, b), (2, 64, 1.0, c)])
    got, _ = check_solutions(hc, keys, x, f, _dev(x), _dev(f), 3, 2, 0.25, f"{name} R={R} equality")
    assert got["idx"].tolist() == [[12, su.NONE], [12, 3 + last], [3 + last, 3 + 64]]


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("R", [300, 4097])
def test_solutions_k_and_padding(hip_chains, name, R):
    """K = 1, 2, 256 over 5 candidates and over 300 mutually distant ones: counts and the padding past them."""
    hc = hip_chains[name]
    n = hc.n
    rng = np.random.default_rng(R)
    cols = rng.permutation(R)[:300]
    # target 0: 300 candidates 1.0 apart with distinct keys; target 1: 5 of them; target 2: 300 with one key (index order)
    cands = [(0, int(c), float(k), np.full(n, float(c))) for k, c in enumerate(cols)]
    cands += [(1, int(c), 1.0, np.full(n, float(c))) for c in cols[:5]]
    cands += [(2, int(c), -2.5, np.full(n, float(c))) for c in cols]
    keys, x, f = _sparse(n, 3, R, cands)
    d_x, d_f = _dev(x), _dev(f)
    for K in (1, 2, 256):
        got, _ = check_solutions(hc, keys, x, f, d_x, d_f, BEGINS[1], K, 0.5, f"{name} R={R} K={K}")
        assert got["count"].tolist() == [min(K, 300), min(K, 5), min(K, 300)]
        assert got["idx"][0].tolist() == [BEGINS[1] + int(c) for c in cols[:K]]
        assert got["idx"][2].tolist() == [BEGINS[1] + int(c) for c in np.sort(cols)[:K]]
        assert (got["idx"][1, 5:] == su.NONE).all() and (got["key"][1, 5:].view(np.uint64) == INF_BITS).all()
        assert np.isnan(got["x"][1, 5:]).all() and np.isnan(got["f"][1, 5:]).all()


@pytest.mark.parametrize("name", CHAINS)
def test_solutions_later_rounds_across_tiles(hip_chains, name):
    """Ties in the rounds after the first, between tiles; a target that runs dry at round 1 (its tile kernel returns
    early, its slots are padded, its count stays) beside neighbours that fill all K rounds."""
    hc = hip_chains[name]
    n, R, K = hc.n, 8193, 4
    spread = [10, 4095, 4096, 5000, 8191, 8192]

    def far(c):
        return np.full(n, float(c))

    cands = [(0, c, 1.0, far(c)) for c in spread]
    cands += [(1, 4096, 1.0, far(0)), (1, 8192, 1.0, far(0)), (1, 7, 2.0, far(0))]  # three at one point: one solution
    cands += [(2, c, 1.0, far(c)) for c in reversed(spread)]
    keys, x, f = _sparse(n, 3, R, cands)
    got, _ = check_solutions(hc, keys, x, f, _dev(x), _dev(f), BEGINS[2], K, 0.5, name)
    b = BEGINS[2]
    assert got["idx"].tolist() == [[b + c for c in spread[:K]], [b + 4096] + [su.NONE] * 3, [b + c for c in spread[:K]]]
    assert got["count"].tolist() == [4, 1, 4]
    # a target with no candidate at all between them, and K larger than what the others hold
    keys[1] = np.inf
    got, _ = check_solutions(hc, keys, x, f, _dev(x), _dev(f), b, 8, 0.5, name + " dry at round 0")
    assert got["count"].tolist() == [6, 0, 6]


@pytest.mark.parametrize("name", CHAINS)
def test_solutions_small_and_tiled_forms_agree(hip_chains, name):
    """The same candidates as R = 4096 (one kernel) and, padded with one +inf key per target, as R = 4097 (tile and
    pick kernels): identical outputs."""
    hc = hip_chains[name]
    n, T, R = hc.n, 3, 4096
    rng = np.random.default_rng(4096)
    keys = np.array([su.fuzz_keys(rng, R) for _ in range(T)])
    x, f = su.lattice_x(rng, n, T * R, levels=2), su.coded_f(T * R)
    keys2 = np.concatenate([keys, np.full((T, 1), np.inf)], axis=1)
    x2 = np.concatenate([x.reshape(n, T, R), np.full((n, T, 1), 0.125)], axis=2).reshape(n, T * (R + 1))
    f2 = np.concatenate([f.reshape(T, R), np.full((T, 1), -1.0)], axis=1).reshape(-1)
    for K, min_dist in ((1, 0.0), (6, 0.25), (256, 0.25)):
        a, _ = check_solutions(hc, keys, x, f, _dev(x), _dev(f), 11, K, min_dist, f"{name} small K={K}")
        b, _ = check_solutions(hc, keys2, x2, f2, _dev(x2), _dev(f2), 11, K, min_dist, f"{name} tiled K={K}")
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), f"{name} K={K} min_dist={min_dist}: {k} differs between the forms"


# ---- one waypoint of optik_hip_ik_path -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("R", PATH_R)
def test_path_select_on_prescribed_keys(hip_chains, name, R):
    """Every key pattern without a filter and with one that admits the columns up to R // 2 (the last of them at a
    distance of exactly max_step); carry aliasing the seed buffer and not."""
    hc = hip_chains[name]
    for j, (names, keys, begin) in enumerate(chunks(su.key_patterns(R))):
        P = keys.shape[0]
        x, f, d_x, d_f = _coded(hc.n, P * R)
        seed = np.array([x[:, p * R] for p in range(P)])  # (column c of a path is c * 2^-24 away from it)
        for max_step in (np.inf, (R // 2) * 2.0 ** -24):
            check_path(hc, keys, x, f, d_x, d_f, seed, begin, max_step, alias=bool(j % 2),
                       what=f"{name} R={R} begin={begin} max_step={max_step} {names}")


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("R", PATH_R)
def test_path_select_fuzz(hip_chains, name, R):
    hc = hip_chains[name]
    for seed_no in range(8):
        rng = np.random.default_rng(R * 100 + seed_no)
        P = 3 + seed_no % 3
        keys = np.array([su.fuzz_keys(rng, R) for _ in range(P)])
        x, f = su.lattice_x(rng, hc.n, P * R, levels=2 + seed_no % 2), su.coded_f(P * R)
        d_x, d_f = _dev(x), _dev(f)
        seed = rng.integers(0, 2, size=(P, hc.n)) * 0.25 + 2.0 ** -5
        for max_step in (0.0, 0.25, 0.5, np.inf):
            check_path(hc, keys, x, f, d_x, d_f, seed, BEGINS[seed_no % 3], max_step, alias=bool(seed_no % 2),
                       what=f"{name} R={R} seed={seed_no} max_step={max_step}")


@pytest.mark.parametrize("name", CHAINS)
@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("R", [1, 257, 4096])
def test_path_filter_boundary_and_none(hip_chains, name, alias, R):
    """A distance of exactly max_step is admitted, one ulp above it refused; max_step = +inf switches the filter off;
    with nothing admitted x, f and step are NaN, idx ~0, key +inf, and carry and last hold the seed's bits."""
    hc = hip_chains[name]
    n, P = hc.n, 4
    last = R - 1
    seed = np.zeros((P, n))
    seed[:, 0] = [-0.0, 0.0, 5e-324, -1.5]  # (bits that only a copy preserves)
    exact, above = np.zeros(n), np.zeros(n)
    exact[n - 1], above[n - 1] = 0.25, np.nextafter(0.25, 1.0)
    far = np.full(n, 9.0)
    far[3] = np.nan
    # path 0: the better key is one ulp too far; path 1: only that one; path 2: +inf keys and a NaN; path 3: far away
    cands = [(0, last, 2.0, exact), (0, 0, 1.0, above)] if R > 1 else [(0, 0, 2.0, exact)]
    cands += [(1, last, 1.0, above), (3, last // 2, -1.0, far)]
    keys, x, f = _sparse(n, P, R, cands)
    keys[2, 0] = np.nan
    d_x, d_f = _dev(x), _dev(f)
    got = check_path(hc, keys, x, f, d_x, d_f, seed, 7, 0.25, alias, f"{name} R={R} max_step=0.25")
    assert got["idx"].tolist() == [7 + last, su.NONE, su.NONE, su.NONE]
    assert got["step"][0] == 0.25 and np.isnan(got["step"][1:]).all() and np.isnan(got["x"][1:]).all()
    assert np.isnan(got["f"][1:]).all() and (got["key"][1:].view(np.uint64) == INF_BITS).all()
    for k in ("carry", "last"):
        assert got[k][1:].tobytes() == seed[1:].tobytes(), f"{k} is not the seed, bit for bit"
        assert got[k][0].tobytes() == exact.tobytes()
    got = check_path(hc, keys, x, f, d_x, d_f, seed, 7, np.inf, alias, f"{name} R={R} no filter")
    assert got["idx"].tolist() == [7 if R > 1 else 7 + last, 7 + last, su.NONE, 7 + last // 2]
    assert got["step"][3] == 10.5 and np.isnan(got["x"][3, 3]) and got["carry"][2].tobytes() == seed[2].tobytes()


# ---- the hooks leave the chain as it was --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CHAINS)
def test_no_state_leaks_into_the_product(oracle, chains, hip_chains, name):
    """ik_batch on the same chain, before and after a series of hook calls: byte-identical (Quality: every output;
    Speed with early exit, whose launch relies on the work-item counter and first-success words being clean: the
    winners -- what an abandoned restart leaves behind depends on timing)."""
    from optik_amd import _native as nat
    hc = hip_chains[name]
    d, ch = chains[name]
    tg, x0 = make_targets(oracle, d, ch, np.random.default_rng(3), 5)
    tg[2] = [5.0, 5.0, 5.0, 0.0, 0.0, 0.0, 1.0]  # (no winner)
    tg, x0 = _dev(tg), _dev(x0)
    R = 32

    def product():
        res = {}
        for mode, flags, per_restart in (("speed", nat.IK_EARLY_EXIT, False), ("quality", 0, True),
                                         ("speed", nat.IK_EARLY_EXIT | nat.IK_RESTART_MAJOR, False)):
            out = hc.ik_batch(nat.make_config(solution_mode=mode), tg, x0, 0, R, flags=flags, per_restart=per_restart)
            torch.cuda.synchronize()
            res.update({(mode, flags, k): v.cpu().numpy().tobytes() for k, v in out.items()})
        return res

    before = product()
    rng = np.random.default_rng(9)
    for Rh in (300, 4097):
        keys = np.array([su.fuzz_keys(rng, Rh) for _ in range(7)])  # (more targets than the product calls have)
        x, f, d_x, d_f = _coded(hc.n, keys.size)
        check_select(hc, keys, x, f, d_x, d_f, 3, "select")
        check_solutions(hc, keys, x, f, d_x, d_f, 3, 4, SPACING, "solutions")
    keys = np.array([su.fuzz_keys(rng, 300) for _ in range(7)])
    x, f, d_x, d_f = _coded(hc.n, keys.size)
    check_path(hc, keys, x, f, d_x, d_f, np.zeros((7, hc.n)), 3, np.inf, True, "path")
    after = product()
    assert before.keys() == after.keys()
    for k in before:
        assert before[k] == after[k], f"{name}: {k} differs after the hook calls"
    idx = np.frombuffer(after[("quality", 0, "win_idx")], dtype=np.int64)
    key = np.frombuffer(after[("quality", 0, "win_key")], dtype=np.float64)
    assert idx[2] == -1 and (idx[[0, 1, 3, 4]] >= 0).any()
    assert (key[idx < 0].view(np.uint64) == INF_BITS).all()  # (the product's own launch: +inf where none)
