"""-m gpu: examples/plan_to_pose_lazy.py runs as a user would run it."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROBOTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANDA = [os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"]


def test_plan_to_pose_lazy_example():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "plan_to_pose_lazy.py"), *PANDA], env=env,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    assert "lazy roadmap: 512 nodes" in res.stdout, res.stdout
    plans = re.findall(r"^(wall in place|wall moved away): (\d+) IK solutions, status 0, goal (\d+), (\d+) waypoints, .* "
                       r"segments free; rounds (\d+), checked (\d+) of 4096 edges$", res.stdout, re.M)
    assert [p[0] for p in plans] == ["wall in place", "wall moved away"], res.stdout
    assert all(int(p[1]) >= 1 and int(p[2]) < int(p[1]) and int(p[5]) < 4096 for p in plans), res.stdout
    assert "the same plan again: rounds 0, checked 0" in res.stdout, res.stdout
