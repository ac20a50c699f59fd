"""The selection stages (csrc/ik_select.hip, ik_solutions.hip, ik_path.hip) written out in plain Python / numpy, and
inputs for them: the reference of tests/test_gpu_selection.py, which feeds prescribed keys to the kernels through the
optik_hip_*_from_keys hooks.  Nothing here is compiled from csrc.

The order is (key, index): the smaller key first, ties to the smaller index, -0.0 == +0.0 a tie.  A key that is not
< +inf (+inf, NaN) is no candidate.  Distances are max_i |x_i - a_i| with NaN terms skipped (0 if every term is NaN);
they are differences of doubles and exact for the dyadic inputs built below."""
import numpy as np

NONE = 0xFFFFFFFFFFFFFFFF  # UINT64_MAX: no entry
TILE = 4096                # restarts per selection tile (SEL_TILE of csrc/ik_launch_plan.hpp)


def _ordered_candidates(keys):
    """Columns with a key < +inf in (key, column) order (a stable sort on the key: equal keys, the two zeros among
    them, stay in column order)."""
    k = np.asarray(keys, dtype=np.float64)
    cand = np.nonzero(k < np.inf)[0]
    return cand[np.argsort(k[cand], kind="stable")]


def linf(a, b):
    """max_i |a_i - b_i|, NaN terms skipped."""
    e = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    return float(np.where(np.isnan(e), 0.0, e).max(initial=0.0))


def select_ref(keys, begin):
    """keys [R] of one target -> (index, key) minimising (key, index) over the keys < +inf, or None.  The key is the
    winner's own (its sign bit too)."""
    k = np.asarray(keys, dtype=np.float64)
    order = _ordered_candidates(k)
    if not len(order):
        return None
    r = int(order[0])
    return begin + r, k[r]


def solutions_ref(keys, x, begin, K, min_dist):
    """The greedy set of ik_solutions.hip's header for one target: keys [R], x [n, R].  Candidates in (key, index) order;
    one is accepted if its distance to every earlier acceptance is > min_dist; at most K.  [(index, key, column)] in
    acceptance order."""
    k = np.asarray(keys, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    acc = []
    kept = np.empty((x.shape[0], 0))  # the accepted columns of x, side by side
    for r in _ordered_candidates(k):
        r = int(r)
        e = np.abs(x[:, r:r + 1] - kept)  # (one candidate against every acceptance at once)
        if (np.where(np.isnan(e), 0.0, e).max(axis=0, initial=0.0) > min_dist).all():
            acc.append((begin + r, k[r], r))
            kept = np.concatenate([kept, x[:, r:r + 1]], axis=1)
            if len(acc) == K:
                break
    return acc


def path_ref(keys, x, seed, begin, max_step):
    """One waypoint of one path (ik_path.hip): keys [R], x [n, R], seed [n].  The candidates are the keys < +inf whose
    distance to the seed is <= max_step (+inf: no filter).  Returns (index, key, column, step, next_seed); without a
    candidate (None, None, None, None, seed)."""
    k = np.asarray(keys, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    seed = np.asarray(seed, dtype=np.float64)
    for r in _ordered_candidates(k):
        r = int(r)
        if max_step == np.inf or linf(x[:, r], seed) <= max_step:
            return begin + r, k[r], r, linf(x[:, r], seed), x[:, r].copy()
    return None, None, None, None, seed.copy()


# ---- inputs -----------------------------------------------------------------------------------------------------------
def coded_x(n, cols):
    """x [n, cols] with x[i, c] = (i + 1) / 16 + c * 2^-24: row and column can be read off every value exactly (cols <=
    2^20), so a gather from a wrong row or column shows bit for bit.  Two columns c, d are |c - d| * 2^-24 apart."""
    assert n <= 16 and cols <= 1 << 20
    return (np.arange(1, n + 1, dtype=np.float64) / 16.0)[:, None] + np.arange(cols, dtype=np.float64)[None, :] * 2.0 ** -24


def coded_f(cols):
    """f [cols] = c + 0.5."""
    return np.arange(cols, dtype=np.float64) + 0.5


def lattice_x(rng, n, cols, levels=3):
    """x [n, cols] on a lattice of step 0.25 (`levels` steps per joint) plus the column's code c * 2^-30 and the row's
    (i + 1) * 2^-7: columns on the same lattice point are less than 2^-10 apart, columns on different ones 0.25 * m -+
    a multiple of 2^-30 -- distances on both sides of, and next to, min_dist = 0.25 * m.  All exact."""
    assert n <= 16 and cols <= 1 << 20
    g = rng.integers(0, levels, size=(n, cols)).astype(np.float64)
    return (g * 0.25 + (np.arange(1, n + 1, dtype=np.float64) * 2.0 ** -7)[:, None]
            + np.arange(cols, dtype=np.float64)[None, :] * 2.0 ** -30)


def fuzz_keys(rng, R):
    """keys [R] drawn from 4 values, about half of them +inf, a few NaN."""
    vals = np.array([-1.5, -0.0, 0.0, 2.0])
    k = vals[rng.integers(0, 4, size=R)]
    k[rng.random(R) < 0.5] = np.inf
    k[rng.random(R) < 0.02] = np.nan
    return k


def key_patterns(R):
    """The prescribed key rows of length R, [(name, keys [R])]: none, one, all equal, exactly two equal minima, signed
    zeros, extreme values."""
    inf = np.inf
    rows = []
    rows.append(("all +inf", np.full(R, inf)))
    k = np.full(R, inf)
    k[[0, R // 2, R - 1]] = np.nan
    rows.append(("+inf and NaN", k))
    rows.append(("all NaN", np.full(R, np.nan)))
    for p in sorted({0, 63, 64, 255, 256, 257, R - 1, 4095, 4096} & set(range(R))):
        k = np.full(R, inf)
        k[p] = 3.25
        rows.append((f"one finite key at {p}", k))
        k = np.full(R, np.nan)  # (and among NaNs)
        k[p] = -3.25
        rows.append((f"one finite key at {p} among NaN", k))
    rows.append(("all equal", np.full(R, 1.5)))
    rows.append(("all zero", np.zeros(R)))
    # (d) exactly two equal minima at p < q, a larger key everywhere else (at the lower indices too): lanes 0 and off
    # of the second wave for every butterfly offset, two waves, a thread's first and second stride, two tiles, tiles 0
    # and 64, the last column
    pairs = [(64, 64 + off) for off in (1, 2, 4, 8, 16, 32)]
    pairs += [(1, 2), (63, 64), (70, 130), (5, 192 + 5), (255, 256), (3, 3 + 256), (257, 257 + 15 * 256), (1, R - 1),
              (4095, 4096), (100, 4096 + 100), (4100, 8192), (4097, 2 * 4096 + 1), (7, 64 * 4096), (64 * 4096 - 1, 64 * 4096),
              (63 * 4096 + 9, 64 * 4096)]
    for p, q in pairs:
        if 0 < p < q < R:
            k = np.full(R, 2.0)
            k[[p, q]] = 1.0
            rows.append((f"two minima at {p} and {q}", k))
            k = np.full(R, inf)  # (and with nothing else alive above the lower index)
            k[:p] = 2.0
            k[[p, q]] = 1.0
            rows.append((f"two minima at {p} and {q}, the rest +inf", k))
    # (e) the two zeros: a tie, the lower index wins with its own sign
    for p, q in [(0, 1), (1, 64), (2, 256 + 2), (3, R - 1), (10, 4096), (4096, 64 * 4096)]:
        if p < q < R:
            for lo, hi in ((0.0, -0.0), (-0.0, 0.0)):
                k = np.full(R, 0.5)
                k[p], k[q] = lo, hi
                rows.append((f"zeros {lo!r} at {p}, {hi!r} at {q}", k))
    # (f) negative keys, a subnormal, DBL_MAX
    big = np.finfo(np.float64).max
    k = np.full(R, big)
    k[R // 2] = np.nextafter(big, 0.0)
    rows.append(("DBL_MAX and one key below it", k))
    rows.append(("all DBL_MAX", np.full(R, big)))
    k = np.full(R, 5e-324)
    k[R - 1] = 0.0
    rows.append(("subnormals and a zero at the end", k))
    k = np.full(R, -5e-324)
    k[R // 3] = -1e-310
    rows.append(("negative subnormals", k))
    k = -np.arange(R, dtype=np.float64)  # strictly decreasing: the last column wins
    rows.append(("negative, decreasing", k))
    k = np.full(R, -big)
    k[0] = inf
    rows.append(("all -DBL_MAX but the first", k))
    return rows
