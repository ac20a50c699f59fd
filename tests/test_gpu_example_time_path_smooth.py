"""-m gpu: examples/time_path_smooth.py runs as a user would run it."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROBOTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANDA = [os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"]


def test_time_path_smooth_example():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "time_path_smooth.py"), *PANDA], env=env,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    print(res.stdout)
    timed = re.search(r"^time_paths: duration ([0-9.]+) s", res.stdout, re.M)
    smooth = re.search(r"^smooth_timing: duration ([0-9.]+) s, factor ([0-9.]+), peak / limit along the curve: "
                       r"velocity ([0-9.]+), acceleration ([0-9.]+), jerk ([0-9.]+)", res.stdout, re.M)
    sampled = re.search(r"^smooth_timing sampled: \d+ samples at 1000 Hz, peak \|acceleration\| ([0-9.]+) rad/s\^2, "
                        r"peak \|jerk\| ([0-9.]+) rad/s\^3, ends at the goal", res.stdout, re.M)
    assert timed and smooth and sampled, res.stdout
    assert float(smooth[2]) >= 1.0 and float(smooth[1]) >= float(timed[1]) > 0.0
    assert max(float(smooth[3]), float(smooth[4]), float(smooth[5])) <= 1.0
    # differences of a C2 curve's velocity are means of its acceleration and of its jerk: within the limits, up to the
    # printed digits
    assert float(sampled[1]) <= 7.5 + 1e-4 and float(sampled[2]) <= 500.0 + 0.1
