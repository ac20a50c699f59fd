"""CPU checks of the manipulability / condition solution modes: the measure that the device kernels run
(optik_amd/csrc/manip_measure.hpp) -- compiled here as plain C++ with g++, no HIP runtime -- against numpy's singular
values, exact zeros where the Jacobian is exactly rank-deficient, the exported symbols, the mode names, and the
argument errors of the new entry points (these run on a machine without a GPU)."""
import os

import numpy as np
import pytest

from conftest import REF_GOLDEN
from manip_util import build_measure

MAXN = 16


@pytest.fixture(scope="module")
def built():
    from optik_amd import build
    build.build()
    from optik_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def measure(tmp_path_factory):
    """jacobians (list of 6 x n arrays) -> (w [B], c [B]) from the g++-built header."""
    return build_measure(str(tmp_path_factory.mktemp("manip_measure")))


def _random_jacobians(rng, count):
    """6 x n, n = 1 .. 16: U diag(s) V^T with singular values spread over two orders of magnitude (and the whole
    matrix scaled by 0.1 .. 10), plus plain Gaussian ones of moderate condition."""
    jacs = []
    for t in range(count):
        n = 1 + t % MAXN
        m = min(n, 6)
        if t % 3 == 2:
            while True:
                J = rng.normal(size=(6, n))
                sv = np.linalg.svd(J, compute_uv=False)
                if sv[0] / sv[-1] < 30.0:
                    break
        else:
            U, _ = np.linalg.qr(rng.normal(size=(6, 6)))
            V, _ = np.linalg.qr(rng.normal(size=(n, n)))
            S = np.zeros((6, n))
            S[range(m), range(m)] = rng.uniform(0.05, 2.0, size=m) * 10.0 ** rng.uniform(-1.0, 1.0)
            J = U @ S @ V.T
        jacs.append(J)
    return jacs


def test_measures_match_singular_values(measure):
    rng = np.random.default_rng(11)
    jacs = _random_jacobians(rng, 3000)
    w, c = measure(jacs)
    for J, wi, ci in zip(jacs, w, c):
        sv = np.linalg.svd(J, compute_uv=False)[:min(J.shape[1], 6)]
        prod = float(np.prod(sv))
        assert abs(wi - prod) <= 1e-12 * prod, (J.shape, wi, prod)
        assert abs(ci - sv[-1] / sv[0]) <= 1e-12, (J.shape, ci, sv[-1] / sv[0])
        assert 0.0 < ci <= 1.0


def test_frame_does_not_change_the_measures(measure):
    """diag(R, R) J (the world-frame Jacobian) has the singular values of J."""
    rng = np.random.default_rng(5)
    jacs = _random_jacobians(rng, 64)
    rot = []
    for J in jacs:
        R, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        rot.append(np.vstack([R @ J[:3], R @ J[3:]]))
    w0, c0 = measure(jacs)
    w1, c1 = measure(rot)
    np.testing.assert_allclose(w1, w0, rtol=1e-12)
    np.testing.assert_allclose(c1, c0, atol=1e-12)


def test_rank_deficient_jacobians_give_exact_zeros(measure):
    rng = np.random.default_rng(7)
    jacs = []
    for t in range(600):
        n = 1 + t % MAXN
        J = rng.normal(size=(6, n))
        kind = t % 3
        if n <= 6:
            if kind == 0 and n >= 2:        # two equal columns
                i, j = rng.choice(n, size=2, replace=False)
                J[:, j] = J[:, i]
            else:                           # a zero column
                J[:, rng.integers(n)] = 0.0
        else:
            if kind == 0:                   # two equal rows: J J^T has two equal rows
                i, j = rng.choice(6, size=2, replace=False)
                J[j] = J[i]
            else:                           # a zero row (a planar arm's Jacobian has three)
                J[rng.integers(6)] = 0.0
        jacs.append(J)
    w, c = measure(jacs)
    assert (w == 0.0).all() and (c == 0.0).all()
    assert not np.signbit(w).any() and not np.signbit(c).any()


def test_singular_configurations_of_real_chains_give_exact_zeros(measure, oracle, chains):
    """The Panda at q = 0 (joint axes 1, 3, 5 on one vertical line) and its sub-chains: Jacobians from the CPU oracle
    whose Gram matrix has an exactly zero pivot."""
    jacs = []
    for name in ("panda", "panda_hand", "panda3", "panda4", "panda5"):
        d, ch = chains[name]
        jacs.append(oracle.joint_jacobian(ch, np.zeros(len(d["lb"]))))
    w, c = measure(jacs)
    assert (w == 0.0).all() and (c == 0.0).all()
    # and a regular configuration of the same chains is not
    rng = np.random.default_rng(3)
    regular = [oracle.joint_jacobian(chains[name][1], rng.uniform(chains[name][0]["lb"], chains[name][0]["ub"]))
               for name in ("panda", "panda3")]
    w, c = measure(regular)
    assert (w > 0.0).all() and (c > 0.0).all()


def test_manip_symbols_are_exported(built):
    for s in ("optik_hip_manip_batch", "optik_robot_manipulability_batch"):
        assert hasattr(built, s), f"{s} is not exported by liboptik_amd.so"


def test_mode_names():
    from optik_amd import SolverConfig
    from optik_amd import _native as nat
    for name, code in (("quality", 1), ("speed", 2), ("manipulability", 3), ("condition", 4)):
        assert SolverConfig(solution_mode=name).to_c().solution_mode == code
        assert nat.make_config(solution_mode=name).solution_mode == code
    for bad in ("fast", "Manipulability", "manip", "", None, 3):
        with pytest.raises(ValueError):
            SolverConfig(solution_mode=bad)
        with pytest.raises(ValueError):
            nat.make_config(solution_mode=bad)


@pytest.fixture(scope="module")
def ur3e(built):
    from optik_amd import Robot
    return Robot.from_urdf_file(os.path.join(REF_GOLDEN, "ur3e.urdf"), "ur_base_link", "ur_ee_link")


def test_manipulability_arguments_are_validated_before_any_device_call(ur3e):
    n = ur3e.num_positions()
    for bad in (np.zeros(n), np.zeros((4, n + 1)), np.zeros((2, 3, n))):
        with pytest.raises(ValueError, match="xs"):
            ur3e.manipulability_batch_arrays(bad)
    with pytest.raises(ValueError, match="incorrect length"):
        ur3e.manipulability(np.zeros(n - 1))
    ee = np.eye(4)
    ee[0, 0] = 2.0
    with pytest.raises(ValueError, match="invalid target transform"):
        ur3e.manipulability(np.zeros(n), ee_offset=ee)
    with pytest.raises(ValueError):
        ur3e.manipulability_batch_arrays(np.zeros((2, n)), ee_offset=np.eye(3))
