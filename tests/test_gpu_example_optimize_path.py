"""-m gpu: examples/optimize_path.py runs as a user would run it."""
import os
import subprocess
import sys

import pytest

from conftest import ROBOTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANDA = [os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"]


def test_optimize_path_example():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "optimize_path.py"), *PANDA], env=env,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    assert "straight path: blocked" in res.stdout and "optimised path: free" in res.stdout, res.stdout
    clearance = float(res.stdout.split("optimised path: free, clearance ")[1].split(" m")[0])
    assert clearance >= 0.05, res.stdout  # (the example's safety distance)
