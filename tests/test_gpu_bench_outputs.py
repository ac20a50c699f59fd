"""-m gpu: what a plain `bench.py` run does and writes.  It times its --steps once and runs none of the --full legs; with
--dump-outputs it writes what the timed path computed in its last step, the same arrays on every run of the same
command (seeded inputs, a deterministic solver)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, out_dir):
    r = subprocess.run([sys.executable, "bench.py", *args, "--dump-outputs", str(out_dir)], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(rows) == 1, r.stdout[-2000:]
    return json.loads(rows[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--restarts", "4096"]
    a, b = _run(args, tmp_path / "a"), _run(args, tmp_path / "b")
    for line in (a, b):
        assert line["steps"] == 3 and line["config"]["reps"] == 1 and line["ms_per_step"] > 0
        assert line["cpu_baseline"] is None and line["config"]["other_configs"] is None
        assert line["config"]["collective_us"] is None
    da, db = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(da) == {"x", "f", "status", "evals", "restart_index", "win_x", "win_f", "win_idx"}
    for k in da:
        assert da[k].dtype == np.float64 and np.array_equal(da[k], db[k], equal_nan=True), k
    assert da["x"].shape == (4096, 7) and np.array_equal(da["restart_index"], np.arange(4096))
    w = int(da["win_idx"][0])
    assert w == a["config"]["winner_index_per_step"][-1]
    if w >= 0:  # the winner's row of the per-restart outputs is what the step handed back
        assert np.array_equal(da["win_x"][0], da["x"][w]) and da["win_f"][0] == da["f"][w] < 1e-6


def test_targets_run_dumps_every_targets_winner(tmp_path):
    line = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--targets", "16", "--restarts", "128"], tmp_path)
    d = _load(tmp_path)
    assert set(d) == {"win_x", "win_f", "win_idx"} and d["win_x"].shape == (16, 7)
    # (the line's per-step winner is the step's first target; I64_MAX there = no solution = -1 here)
    first = line["config"]["winner_index_per_step"][-1]
    assert int(d["win_idx"][0]) == (first if 0 <= first < 2 ** 63 - 1 else -1)
    solved = d["win_idx"] >= 0
    assert solved.sum() >= 12 and np.all(d["win_f"][solved] < 1e-6) and np.all(d["win_x"][~solved] == 0)
