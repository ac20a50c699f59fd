"""-m gpu: the refill of the lane-per-restart form (ik_lane64.hpp) -- work item -> (target, restart index), the target
pose and the seed of a lane's next restart, the publish of the one that ended -- on launch shapes around its branches,
forced onto that form at the test's size.  Every restart's x, f, status and evaluation count equal the oracle's, bit
for bit, as tests/test_gpu_parity.py checks them."""
import numpy as np
import pytest

from gpu_util import assert_bit_equal, make_targets

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KW = dict(solution_mode="speed", tol_f=1e-6)


@pytest.fixture(scope="module")
def panda(chains):
    from optik_amd import device
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    d, ch = chains["panda"]
    return d, ch, device.HipChain(**d)


# (targets, restarts per target, first restart index, restart-major hand-out)
CASES = {
    "2x96: a refill's items cross a target boundary": (2, 96, 0, False),
    "3x40: fewer restarts per target than lanes": (3, 40, 0, False),
    "5x64 restart-major": (5, 64, 0, True),
    "restart indices across 2^32": (1, 64, 2**32 - 32, False),
}


@pytest.mark.parametrize("case", list(CASES))
def test_every_restart_of_the_launch_bit_exact(oracle, panda, case):
    from optik_amd import _native as nat
    T, R, begin, restart_major = CASES[case]
    d, ch, hc = panda
    rng = np.random.default_rng(31)
    tg, x0 = make_targets(oracle, d, ch, rng, T)
    with nat.options(solve_kernel="lane64"):
        out = hc.ik_batch(nat.make_config(**KW), torch.tensor(tg, device="cuda"), torch.tensor(x0, device="cuda"),
                          begin, begin + R, flags=nat.IK_RESTART_MAJOR if restart_major else 0)
        torch.cuda.synchronize()
    assert hc.last_launch()["lds_bytes"] > 30000, "the launch did not take the lane-per-restart form"
    status = out["status"].cpu().numpy().reshape(T, R)
    evals = out["evals"].cpu().numpy().reshape(T, R)
    f = out["f"].cpu().numpy().reshape(T, R)
    x = out["x"].cpu().numpy()
    cfg = oracle.make_config(**KW)
    for t in range(T):
        ref = oracle.ik(ch, cfg, tg[t], x0[t], begin, begin + R, n_threads=4, early_exit=False, per_restart=True)
        assert np.array_equal(status[t], ref["status"]), (t, np.argwhere(status[t] != ref["status"])[:10])
        assert np.array_equal(evals[t], ref["evals"]), t
        assert_bit_equal(f[t], ref["fs"], f"per-restart f, target {t}")
        assert_bit_equal(x[:, t * R:(t + 1) * R], ref["xs"].T, f"per-restart x, target {t}")
