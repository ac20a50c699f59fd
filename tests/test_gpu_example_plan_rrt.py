"""-m gpu: examples/plan_rrt.py runs as a user would run it."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROBOTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANDA = [os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"]


def test_plan_rrt_example():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "plan_rrt.py"), *PANDA], env=env,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    # the story: the small roadmap has no route for the pair, the trees find one, and its shortcut is certified
    assert re.search(r"^roadmap of 8 nodes, \d+ free edges: status 1$", res.stdout, re.M), res.stdout
    m = re.search(r"^plan_rrt: status 0, (\d+) waypoints, length [\d.]+ rad, (\d+) iterations, trees of (\d+) and "
                  r"(\d+) nodes$", res.stdout, re.M)
    assert m and 3 <= int(m.group(1)) <= 64 and 1 <= int(m.group(2)) <= 256, res.stdout
    assert max(int(m.group(3)), int(m.group(4))) <= 256, res.stdout
    s = re.search(r"^shortcut: status 0, (\d+) waypoints, length [\d.]+ rad; certified (free|blocked)$", res.stdout, re.M)
    assert s and int(s.group(1)) <= int(m.group(1)), res.stdout
