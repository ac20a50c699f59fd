"""bench.py's rank accounting, without a GPU: `--gpus N` must either BE N ranks or refuse.  (The
runs themselves are -m gpu: tests/test_gpu_bench_ranks.py.)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra)
    return env


def test_gpus_flag_disagreeing_with_the_launcher_is_refused():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2"], cwd=ROOT, capture_output=True, text=True,
                       env=_clean_env(WORLD_SIZE="3", RANK="0", LOCAL_RANK="0"), timeout=300)
    assert r.returncode != 0
    assert "refusing" in r.stderr and "WORLD_SIZE=3" in r.stderr
    assert '{"metric"' not in r.stdout


def test_gpus_flag_without_a_launcher_spawns_that_many_ranks():
    """No GPU here: every spawned rank must stop at 'needs a GPU' -- two of them, from one command."""
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU box: the spawned two-rank run itself is tests/test_gpu_bench_ranks.py")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "1", "--warmup", "0"], cwd=ROOT,
                       capture_output=True, text=True, env=_clean_env(), timeout=600)
    assert r.returncode != 0
    assert r.stderr.count("bench.py needs a GPU") >= 2, r.stderr[-3000:]
    assert '{"metric"' not in r.stdout


def test_inprocess_refuses_a_multi_rank_launcher():
    r = subprocess.run([sys.executable, "bench.py", "--inprocess", "--gpus", "2"], cwd=ROOT, capture_output=True,
                       text=True, env=_clean_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), timeout=300)
    assert r.returncode != 0 and "one process" in r.stderr


def test_pmc_record_of_the_default_command_has_the_shape_bench_reads():
    """bench.py takes roofline.traffic and the f64 VALU scalars of the driver's command from profiles/: the record must sit
    under its command key as {"kernel_path": {...}} with the fields the line quotes (written flat once, the line said null)."""
    import json
    import bench
    with open(next(f for f in bench.PMC_FILES if os.path.exists(f))) as fh:  # (the newest round that has one)
        recs = json.load(fh)["commands"]
    key = "robot=panda,restarts=65536,steps=20,warmup=5,mode=speed,scaling=weak,targets=0,path=kernel,gpus=1"
    assert key in recs and "kernel_path" in recs[key]
    kp = recs[key]["kernel_path"]
    for f in ("hbm_bytes_per_restart", "f64_flops_per_restart", "launches", "valu_busy", "valu_active_lane_frac"):
        assert f in kp, f


def test_ranks_sharing_a_gpu_are_refused():
    """A line that says N GPUs needs N physical GPUs: distinct device indices; repeated UUIDs on distinct indices are
    reported, not fatal (a runtime that gives every device one placeholder must not cost the node its scaling run)."""
    import pytest
    import bench
    ok = [{"rank": r, "device": r, "uuid": f"GPU-{r:04x}"} for r in range(8)]
    assert bench.check_distinct_devices(ok, False) is None
    assert bench.check_distinct_devices([{"rank": 0, "device": 0, "uuid": None}, {"rank": 1, "device": 1, "uuid": None}], False) is None
    same_uuid = [dict(ok[0]), dict(ok[1], uuid=ok[0]["uuid"])]
    assert "repeated UUIDs" in bench.check_distinct_devices(same_uuid, False)
    shared = [dict(ok[0]), dict(ok[1], device=0)]
    with pytest.raises(SystemExit, match="share a physical GPU"):
        bench.check_distinct_devices(shared, False)
    assert bench.check_distinct_devices(shared, True) is None  # OPTIK_BENCH_ONE_DEVICE=1: the one-GPU test box


def test_a_plain_run_times_its_steps_once():
    """`--steps K` is the number of timed steps of a plain run; --full keeps the ~2 s repetition, --reps sets any count."""
    import argparse
    import bench
    assert bench.default_reps(argparse.Namespace(reps=None, full=False)) == 1
    assert bench.default_reps(argparse.Namespace(reps=None, full=True)) is None
    assert bench.default_reps(argparse.Namespace(reps=7, full=False)) == 7


def test_dump_outputs_stays_within_its_budget(tmp_path):
    """--dump-outputs: float64 .npy files, at most 64 MB in all; per-restart arrays beyond the budget are cut to the same
    seeded sample of rows on every run, restart_index.npy naming them."""
    import numpy as np
    import bench
    rows, n = 1 << 20, 7
    rng = np.random.default_rng(1)
    arrays = {"x": rng.standard_normal((rows, n)), "f": rng.standard_normal(rows),
              "status": rng.integers(-5, 5, rows).astype(np.int32), "evals": rng.integers(0, 99, rows).astype(np.int32),
              "restart_index": np.arange(1000, 1000 + rows, dtype=np.int64),
              "win_x": np.ones((1, n)), "win_f": np.zeros(1), "win_idx": np.array([1234], dtype=np.int64)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    total = 0
    for name in arrays:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, b), name
        total += os.path.getsize(tmp_path / "a" / f"{name}.npy")
    assert total <= 64_000_000
    idx = np.load(tmp_path / "a" / "restart_index.npy").astype(np.int64)
    assert 0 < len(idx) < rows and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "x.npy"), arrays["x"][idx - 1000])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "status.npy"), arrays["status"][idx - 1000])
    assert np.load(tmp_path / "a" / "win_idx.npy").tolist() == [1234.0]
    # a dump that fits is written whole
    small = {k: (v[:4096] if k in bench.PER_RESTART else v) for k, v in arrays.items()}
    bench.dump_outputs(str(tmp_path / "c"), small)
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "x.npy"), arrays["x"][:4096])
