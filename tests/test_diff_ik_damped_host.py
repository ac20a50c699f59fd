"""CPU-only: the damped LP of collision-avoiding diff_ik (optik_amd/csrc/diff_ik_lp.hpp: diff_ik_lp_damped, built with
g++ as plain C++).  Without damper rows it is diff_ik_lp bit for bit; with 1 .. 4 rows G v >= h it solves random LPs
as scipy's HiGHS does, infeasible ones included."""
import numpy as np
import pytest

from avoid_util import MAXM, build_avoid
from test_diff_ik_batch_host import _random_cases, _rot


@pytest.fixture(scope="module")
def avoid(tmp_path_factory):
    return build_avoid(str(tmp_path_factory.mktemp("avoid_lp")))


def test_without_rows_it_is_diff_ik_lp_bit_for_bit(avoid):
    rng = np.random.default_rng(2024)  # (the seed and generator of test_diff_ik_batch_host's HiGHS comparison)
    cases = [c + (np.zeros((0, c[0])), np.zeros(0)) for c in _random_cases(rng, 400)]
    # and the refusals: a negative and a NaN limit
    for bad in (-1e-3, np.nan):
        n, quat, J, V, vmax, G, h = cases[len(cases) // 2]
        vm = vmax.copy()
        vm[0] = bad
        cases.append((n, quat, J, V, vm, G, h))
    plain = avoid.lp(cases, damped=False)
    damped = avoid.lp(cases, damped=True)
    assert plain[:400, 0].max() == 0 and (plain[400:, 0] == 1).all()
    assert np.array_equal(plain.view(np.uint64), damped.view(np.uint64))


def _highs(JW, V, vmax, G, h):
    from scipy.optimize import linprog
    n = len(vmax)
    c = np.zeros(n + 1)
    c[n] = -1.0
    return linprog(c, A_ub=np.hstack([-G, np.zeros((len(h), 1))]), b_ub=-h, A_eq=np.hstack([JW, -V[:, None]]),
                   b_eq=np.zeros(6), bounds=[(-m, m) for m in vmax] + [(0.0, 1.0)], method="highs")


def test_damped_lp_matches_highs_on_random_lps(avoid):
    rng = np.random.default_rng(77)
    base = _random_cases(rng, 320)
    cases = []
    for t, (n, quat, J, V, vmax) in enumerate(base):
        m = 1 + t % MAXM
        G = rng.normal(size=(m, n))
        # h <= 0: z = 0 stays feasible; h > 0: the row asks for motion, feasible or not
        h = rng.uniform(-1.0, 0.0, size=m) if t % 3 == 0 else rng.uniform(-0.6, 0.6, size=m)
        # (below 6 joints z = 0 is the only point: h = 0 would sit on the edge of feasibility)
        if t % 7 == 0 and n >= 6:
            h[0] = 0.0
        cases.append((n, quat, J, V, vmax, G, h))
    out = avoid.lp(cases)
    skipped = solved = refused = 0
    for (n, quat, J, V, vmax, G, h), res in zip(cases, out):
        JW = np.vstack([_rot(quat) @ J[:3], _rot(quat) @ J[3:]])
        ref = _highs(JW, V, vmax, G, h)
        assert ref.status in (0, 2), ref.message
        status, alpha, v = int(res[0]), res[1], res[2:2 + n]
        # a status that a shift of h by 1e-6 changes is not compared (at most 5 % of the cases)
        if not all(_highs(JW, V, vmax, G, h + s).status == ref.status for s in (1e-6, -1e-6)):
            skipped += 1
            continue
        assert status == (0 if ref.status == 0 else 1), (n, status, ref.status, h)
        if status:
            refused += 1
            assert (res[1:] == 0.0).all()  # nothing written
            continue
        solved += 1
        assert abs(alpha - ref.x[n]) <= 1e-7, (n, len(h), alpha, ref.x[n])
        assert 0.0 <= alpha <= 1.0
        assert np.all(np.abs(v) <= vmax + 1e-9), (n, v, vmax)
        assert np.allclose(JW @ v, alpha * V, rtol=0, atol=1e-8), (n, JW @ v - alpha * V)
        assert np.all(G @ v >= h - 1e-9), (n, G @ v - h)
    assert skipped <= 0.05 * len(cases), skipped
    assert solved >= 100 and refused >= 20, (solved, refused)


def test_the_full_four_rows_are_accepted(avoid):
    n = 3
    case = (n, np.array([0.0, 0.0, 0.0, 1.0]), np.eye(6)[:, :n], np.zeros(6), np.ones(n), np.zeros((MAXM, n)),
            np.zeros(MAXM))
    assert avoid.lp([case])[0, 0] == 0
