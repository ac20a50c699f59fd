"""CPU checks for the selection tests: the Python reference of tests/selection_util.py agrees with the greedy rule that
tests/test_gpu_ik_solutions.py writes out (expected_set), its builders are exact, and the optik_hip_*_from_keys hooks
are exported and refuse bad arguments before any device work (these run on a machine without a GPU)."""
import ctypes as C
import math

import numpy as np
import pytest

import selection_util as su


@pytest.fixture(scope="module")
def built():
    from optik_amd import build
    build.build()
    from optik_amd import _native
    return _native.lib()


@pytest.mark.parametrize("quality", [True, False])
@pytest.mark.parametrize("seed", range(6))
def test_solutions_ref_agrees_with_expected_set(quality, seed):
    from test_gpu_ik_solutions import expected_set
    rng = np.random.default_rng(1000 + seed)
    n, R, begin = 6, 200, 17
    # few lattice points per joint: many candidates within min_dist of each other, some exact duplicates
    xs = rng.integers(0, 3, size=(R, n)) * 0.25 + rng.integers(0, 2, size=(R, n)) * 2.0 ** -20
    x0 = rng.integers(0, 3, size=n) * 0.25
    success = rng.random(R) < 0.6
    ref = dict(success=success, xs=xs, fs=rng.random(R))
    keys = np.full(R, np.inf)
    for r in np.nonzero(success)[0]:
        if quality:
            s = 0.0
            for u, v in zip(xs[r], x0):
                d = float(u) - float(v)
                s += d * d
            keys[r] = math.sqrt(s)
        else:
            keys[r] = float(begin + int(r))
    for K in (1, 5, 256):
        for min_dist in (0.0, 2.0 ** -20, 0.25, 0.3):
            want = expected_set(ref, x0, quality, K, min_dist, begin)
            got = su.solutions_ref(keys, xs.T, begin, K, min_dist)
            assert [(i, k) for i, k, _ in got] == [(w[0], w[1]) for w in want], (K, min_dist)
            for (i, k, r), w in zip(got, want):
                assert xs[r].tobytes() == np.asarray(w[2]).tobytes() and ref["fs"][r] == w[3]


def test_the_reference_on_cases_worked_by_hand():
    inf, nan = np.inf, np.nan
    assert su.select_ref([inf, nan, inf], 5) is None
    assert su.select_ref([2.0, 1.0, nan, 1.0], 5) == (6, 1.0)
    i, k = su.select_ref([0.5, -0.0, 0.0], 0)
    assert i == 1 and math.copysign(1.0, k) == -1.0
    i, k = su.select_ref([0.5, 0.0, -0.0], 0)
    assert i == 1 and math.copysign(1.0, k) == 1.0
    # distance exactly min_dist: eliminated; a little more: kept; NaN terms skipped
    x = np.array([[0.5, 0.75, 0.75 + 2.0 ** -50, nan]])
    keys = [0.0, 1.0, 2.0, 3.0]
    assert [a[0] for a in su.solutions_ref(keys, x, 0, 4, 0.25)] == [0, 2]
    assert [a[0] for a in su.solutions_ref(keys, x, 0, 4, 0.0)] == [0, 1, 2]  # (the all-NaN column is 0 away from all)
    assert [a[0] for a in su.solutions_ref(keys, x, 0, 2, 0.0)] == [0, 1]
    # the path filter admits a distance of exactly max_step
    seed = np.array([0.5])
    assert su.path_ref([1.0, 0.5, inf], np.array([[0.75, 0.75 + 2.0 ** -50, 0.5]]), seed, 3, 0.25)[:4] == (3, 1.0, 0, 0.25)
    assert su.path_ref([1.0, 0.5, inf], np.array([[0.75, 0.75 + 2.0 ** -50, 0.5]]), seed, 3, np.inf)[0] == 4
    none = su.path_ref([1.0, 0.5, inf], np.array([[0.75, 0.75, 0.5]]), seed, 3, 0.125)
    assert none[:4] == (None, None, None, None) and none[4].tobytes() == seed.tobytes()


def test_the_builders_are_exact():
    x = su.coded_x(10, 2 * 262145)
    i, c = 9, 2 * 262145 - 1
    assert x[i, c] == (i + 1) / 16 + c * 2.0 ** -24 and (x[i, c] - (i + 1) / 16) * 2.0 ** 24 == c
    assert len(np.unique(x)) == x.size
    lat = su.lattice_x(np.random.default_rng(0), 10, 5 * 8193)
    col = (lat - np.floor(lat * 4.0) / 4.0 - (np.arange(1, 11) * 2.0 ** -7)[:, None]) * 2.0 ** 30
    assert (col == np.arange(5 * 8193)[None, :]).all()
    for R in (1, 63, 257, 4097, 64 * 4096 + 1):
        names = [name for name, _ in su.key_patterns(R)]
        assert len(set(names)) == len(names) and all(len(k) == R for _, k in su.key_patterns(R))
    assert sum(n.startswith("two minima") for n, _ in su.key_patterns(64 * 4096 + 1)) >= 40
    assert any(n.startswith("two minima") for n, _ in su.key_patterns(63))


HOOKS = ("optik_hip_select_from_keys", "optik_hip_solutions_from_keys", "optik_hip_path_select_from_keys")


def test_hook_symbols_are_exported(built):
    for s in HOOKS:
        assert hasattr(built, s), f"{s} is not exported by liboptik_amd.so"


def test_hooks_refuse_before_any_device_work(built):
    """Every argument rule is checked before the chain is looked at: with no chain at all (and pointers that are never
    followed) each bad argument gets its own message, and good arguments end at the missing chain."""
    from optik_amd import _native as nat
    L = built
    buf = np.zeros(16)
    p = buf.ctypes.data  # (host memory: nothing may read or write it)
    o1, o2, o3 = nat.IkOutputs(), nat.IkSolutionsOutputs(), nat.IkPathOutputs()
    full = 1 << 24

    def err():
        return L.optik_hip_last_error().decode()

    def select(key=p, T=3, begin=0, R=64, out=C.byref(o1)):
        return L.optik_hip_select_from_keys(None, key, p, p, T, begin, R, out, None)

    def solutions(key=p, T=3, begin=0, R=64, K=4, min_dist=0.1, out=C.byref(o2)):
        return L.optik_hip_solutions_from_keys(None, key, p, p, T, begin, R, K, min_dist, out, None)

    def path(key=p, P=3, begin=0, R=64, max_step=0.5, out=C.byref(o3), carry=p):
        return L.optik_hip_path_select_from_keys(None, key, p, p, p, P, begin, R, max_step, out, carry, None)

    for call in (select, solutions, path):
        for kw, words in (({"key": None}, "bad argument"), ({"out": None}, "bad argument"),
                          ({"R": 0}, "empty restart range"), ({"begin": nat.UINT64_MAX - 63}, "empty restart range"),
                          ({"begin": nat.UINT64_MAX}, "empty restart range"), ({}, "bad argument")):
            assert call(**kw) != 0, (call.__name__, kw)
            assert words in err(), (call.__name__, kw, err())
    for kw in ({"T": 0}, {"T": -1}):
        assert select(**kw) != 0 and "bad argument" in err()
        assert solutions(**kw) != 0 and "bad argument" in err()
    assert path(P=0) != 0 and "bad argument" in err()
    for call in (select, solutions):
        for kw in ({"T": 1, "R": (full - 1) * 4096 + 1}, {"T": 4096, "R": 4096 * 4096 - 4095},
                   {"T": 1, "R": nat.UINT64_MAX - 1}, {"T": 3, "R": 1 << 62}):
            assert call(**kw) != 0 and "selection tiles" in err(), (call.__name__, kw, err())
        assert call(T=1, R=(full - 1) * 4096) != 0 and "bad argument" in err()  # (planned: it ends at the chain)
    for K in (0, -1, 257):
        assert solutions(K=K) != 0 and "K must be" in err()
    for md in (-0.5, float("nan"), float("inf"), -1e-300):
        assert solutions(min_dist=md) != 0 and "min_dist" in err()
    for R in (4097, 1 << 40):
        assert path(R=R) != 0 and "4096 restarts" in err()
    for ms in (-0.5, float("nan"), float("-inf")):
        assert path(max_step=ms) != 0 and "max_step" in err()
    assert path(max_step=float("inf")) != 0 and "bad argument" in err()  # (+inf: no limit; it ends at the chain)
    assert (buf == 0.0).all()
