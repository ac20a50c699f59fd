"""-m gpu: examples/time_path.py runs as a user would run it."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROBOTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANDA = [os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"]


def test_time_path_example():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "time_path.py"), *PANDA], env=env,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    print(res.stdout)
    duration = re.search(r"^timed: duration ([0-9.]+) s", res.stdout, re.M)
    assert duration and 0.0 < float(duration[1]) < 60.0, res.stdout
    peaks = re.search(r"^waypoints: peak \|qd\| / v_max ([0-9.]+), peak \|qdd\| / a_max ([0-9.]+)", res.stdout, re.M)
    assert peaks, res.stdout
    assert float(peaks[1]) <= 1.0 + 1e-9 and float(peaks[2]) <= 1.0 + 1e-9, res.stdout
    assert re.search(r"^samples: \d+ at 1000 Hz", res.stdout, re.M) and "ends at the goal" in res.stdout, res.stdout
