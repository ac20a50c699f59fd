"""-m gpu: examples/time_path_tool.py runs as a user would run it."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROBOTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANDA = [os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"]


def test_time_path_tool_example():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "time_path_tool.py"), *PANDA], env=env,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    print(res.stdout)
    free = re.search(r"^joint limits alone: duration ([0-9.]+) s, peak tool speed ([0-9.]+) m/s", res.stdout, re.M)
    capped = re.search(r"^tool capped at 0.25 m/s: duration ([0-9.]+) s, peak tool speed ([0-9.]+) m/s", res.stdout,
                       re.M)
    assert free and capped, res.stdout
    assert float(capped[2]) <= 0.25 * (1.0 + 1e-9), res.stdout
    assert float(free[2]) > 0.25 and float(capped[1]) > float(free[1]) > 0.0, res.stdout
    assert "ends at the goal" in res.stdout, res.stdout
