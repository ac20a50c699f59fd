"""-m gpu: examples/shortcut_path.py runs as a user would run it."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROBOTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANDA = [os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"]


def test_shortcut_path_example():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "shortcut_path.py"), *PANDA], env=env,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    stages = {m[0]: (int(m[1]), float(m[2])) for m in
              re.findall(r"^(plan|shortcut|resampled|optimised): (\d+) waypoints, length ([0-9.]+) rad", res.stdout, re.M)}
    assert set(stages) == {"plan", "shortcut", "resampled", "optimised"}, res.stdout
    assert stages["shortcut"][0] <= stages["plan"][0] and stages["shortcut"][1] <= stages["plan"][1] + 1e-9, res.stdout
    assert stages["resampled"][0] == 32 and stages["optimised"][0] == 32, res.stdout
    assert "segments free" in res.stdout, res.stdout
