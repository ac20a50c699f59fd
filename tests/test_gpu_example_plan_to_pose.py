"""-m gpu: examples/plan_to_pose.py runs as a user would run it."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROBOTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANDA = [os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"]


def test_plan_to_pose_example():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "plan_to_pose.py"), *PANDA], env=env,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    m = re.search(r"^plan: reached IK solution (\d+) of (\d+), (\d+) waypoints, length ([0-9.]+) rad, segments free$",
                  res.stdout, re.M)
    assert m and int(m.group(1)) < int(m.group(2)) <= 8, res.stdout
    alone = re.search(r"^planning to IK solution 0 alone \(the one nearest the start\): (length ([0-9.]+) rad|status \d)$",
                      res.stdout, re.M)
    assert alone, res.stdout
    if alone.group(2):
        assert float(m.group(4)) <= float(alone.group(2)), res.stdout
