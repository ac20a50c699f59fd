"""-m gpu: examples/plan_rrt_to_pose.py runs as a user would run it."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROBOTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANDA = [os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"]


def test_plan_rrt_to_pose_example():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "plan_rrt_to_pose.py"), *PANDA], env=env,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    # the story: the small roadmap has no route to any IK solution of the pose, the trees find one, and it shortcuts
    r = re.search(r"^roadmap of 8 nodes, \d+ free edges: plan_to_poses status 1 with (\d+) IK solutions$", res.stdout,
                  re.M)
    assert r and 1 <= int(r.group(1)) <= 8, res.stdout
    m = re.search(r"^plan_rrt_to_poses: status 0, reached IK solution (\d+) of (\d+), (\d+) waypoints, length [\d.]+ "
                  r"rad, (\d+) iterations, trees of (\d+) and (\d+) nodes$", res.stdout, re.M)
    assert m and 0 <= int(m.group(1)) < int(m.group(2)) == int(r.group(1)), res.stdout
    assert 2 <= int(m.group(3)) <= 64 and 0 <= int(m.group(4)) <= 256, res.stdout
    assert max(int(m.group(5)), int(m.group(6))) <= 256, res.stdout
    s = re.search(r"^shortcut: status 0, (\d+) waypoints, length [\d.]+ rad$", res.stdout, re.M)
    assert s and int(s.group(1)) <= int(m.group(3)), res.stdout
