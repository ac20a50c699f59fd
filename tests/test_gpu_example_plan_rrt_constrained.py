"""-m gpu: examples/plan_rrt_constrained.py runs as a user would run it."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROBOTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANDA = [os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"]
TREE = (r"^%s: status 0, (\d+) waypoints, length [\d.]+ rad, (\d+) iterations, trees of (\d+) and (\d+) nodes; "
        r"constraint (kept|broken) \(violation [\d.]+\)$")


def test_plan_rrt_constrained_example():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "plan_rrt_constrained.py"), *PANDA], env=env,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    # the story: the constrained roadmap has no route, plan_rrt's path breaks the constraint, plan_rrt_constrained's
    # keeps it, and certify_paths and time_paths take that path
    assert re.search(r"^constrained roadmap of 8 nodes \(\d+ projected\): status 1$", res.stdout, re.M), res.stdout
    m = re.search(TREE % "plan_rrt", res.stdout, re.M)
    assert m and m.group(5) == "broken" and 3 <= int(m.group(1)) <= 64, res.stdout
    m = re.search(TREE % "plan_rrt_constrained", res.stdout, re.M)
    assert m and m.group(5) == "kept" and 3 <= int(m.group(1)) <= 64 and 1 <= int(m.group(2)) <= 128, res.stdout
    assert max(int(m.group(3)), int(m.group(4))) <= 64, res.stdout
    p = re.search(r"^projections: (\d+) attempted, (\d+) ended on the constraint$", res.stdout, re.M)
    assert p and int(p.group(1)) >= int(p.group(2)) >= int(m.group(3)) + int(m.group(4)) - 2, res.stdout
    t = re.search(r"^certified free; timed: status 0, ([\d.]+) s$", res.stdout, re.M)
    assert t and float(t.group(1)) > 0.0, res.stdout
