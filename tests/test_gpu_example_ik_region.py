"""-m gpu: examples/ik_region.py runs as a user would run it."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROBOTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANDA = [os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"]


def test_ik_region_example():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ik_region.py"), *PANDA], env=env,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    # the story: each region gives several configurations that satisfy it, and the planner ends inside the shelf
    for what in ("position_only", "axis_free z", "shelf, upright"):
        m = re.search(rf"^{what}: (\d+) configurations, largest violation ([\d.e+-]+), closest pair ([\d.]+|inf) rad "
                      r"apart$", res.stdout, re.M)
        assert m and 1 <= int(m.group(1)) <= 8 and float(m.group(2)) <= 1e-6 and float(m.group(3)) > 0.3, res.stdout
    p = re.search(r"^plan_rrt_to_region: status 0, goal (\d+) of (\d+), (\d+) waypoints, length [\d.]+ rad$",
                  res.stdout, re.M)
    assert p and 0 <= int(p.group(1)) < int(p.group(2)) <= 8 and 2 <= int(p.group(3)) <= 64, res.stdout
    v = re.search(r"^the last waypoint violates the shelf region by ([\d.e+-]+)$", res.stdout, re.M)
    assert v and float(v.group(1)) <= 1e-6, res.stdout
